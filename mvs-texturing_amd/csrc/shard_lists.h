// shard_lists.h -- the arithmetic of the sharded driver's lists: the key a list is sorted by, the per (phase, peer) offsets of a sorted
// list and the byte ranges of a phase's chunk.  The device writes the keys (shard_plan.hip, shard_table.hip), the host decodes them
// here: one layout for both.  Plain host C++, no HIP (the key functions are constexpr, which the device compiler takes as they are):
// tests/cpp/test_shard_lists.cpp runs it on its own, the counts past 2^32 and the edges of the bit fields included.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdexcept>
#include <vector>

namespace mvs {

constexpr int MAX_PARTS = 64;   // ranks of a communicator = parts of a partition

// key = phase << 40 | peer << 32 | index: PHASE-major, so everything a colour phase puts on the wire is one contiguous range
// of a list (one pack and one unpack launch per phase, whatever the number of neighbours), inside it one contiguous chunk per
// peer, ascending in the global directed-edge index / node id -- the order BOTH ends of a pair derive independently
constexpr unsigned long long plan_key(int peer, uint32_t phase, uint32_t index) { return ((unsigned long long)phase << 40) | ((unsigned long long)peer << 32) | index; }
constexpr uint32_t plan_key_phase(unsigned long long key) { return (uint32_t)(key >> 40); }
constexpr int plan_key_peer(unsigned long long key) { return (int)((key >> 32) & 0xFFu); }
constexpr uint32_t plan_key_index(unsigned long long key) { return (uint32_t)(key & 0xFFFFFFFFull); }
static_assert(MAX_PARTS <= 256, "a peer is 8 bits of a key");

// per (phase, peer) offsets of a sorted key list whose records have the given lengths (null: 1 each).  The list is sorted
// by (phase, peer, index) and the exchange buffers use the same order: off[phase * P + peer].
inline void segment(const std::vector<unsigned long long>& keys, const std::vector<uint32_t>* lens, int P, uint32_t phases, std::vector<uint64_t>& off, uint64_t& total) {
    off.assign((size_t)P * phases + 1, 0);
    std::vector<uint64_t> cnt((size_t)P * phases, 0);
    for (size_t k = 0; k < keys.size(); ++k) {
        const uint32_t ph = plan_key_phase(keys[k]); const int peer = plan_key_peer(keys[k]);
        if (peer >= P || ph >= phases) throw std::out_of_range("halo plan: key out of range");
        cnt[(size_t)ph * P + peer] += lens ? (*lens)[k] : 1u;
    }
    for (size_t c = 0; c < cnt.size(); ++c) off[c + 1] = off[c] + cnt[c];
    total = off.back();
}

// per-peer byte offsets of every phase's chunk of a list, relative to the start of the phase (elem = bytes per element): a phase's
// chunk is contiguous, peer after peer.  off: segment's; bytes[phase * (P + 1) + peer], the closing entry [P] = the phase's byte total
inline void phase_offsets(const std::vector<uint64_t>& off, int P, uint32_t elem, std::vector<uint64_t>& bytes) {
    const size_t phases = (off.size() - 1) / P;
    bytes.assign(phases * (P + 1), 0);
    for (size_t ph = 0; ph < phases; ++ph)
        for (int q = 0; q <= P; ++q) bytes[ph * (P + 1) + q] = (off[ph * P + q] - off[ph * P]) * elem;
}

}  // namespace mvs
