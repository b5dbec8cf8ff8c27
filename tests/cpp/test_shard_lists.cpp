// The host arithmetic of the sharded driver's lists (csrc/shard_lists.h) on its own: the key layout phase << 40 | peer << 32 | index at
// the edges of its bit fields, the per (phase, peer) offsets of a sorted key list -- record lengths past 2^32 included -- and the byte
// ranges of a phase's chunk.  Built with -fsanitize=address,undefined by tests/test_shard_lists_host.py; prints "ok" and exits 0, or
// says which check failed.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <stdexcept>
#include <string>
#include <vector>

#include "shard_lists.h"

using namespace mvs;

#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) { fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); exit(1); } \
    } while (0)

typedef std::vector<unsigned long long> Keys;
typedef std::vector<uint64_t> Offs;

// true: segment refused the list, with the text a caller of the library sees
static bool refused(const Keys& keys, int P, uint32_t phases) {
    Offs off; uint64_t total = 0;
    try { segment(keys, nullptr, P, phases, off, total); } catch (const std::out_of_range& e) { return std::string(e.what()) == "halo plan: key out of range"; }
    return false;
}

int main() {
    static_assert(MAX_PARTS == 64, "the cases below name rank 63 as the last one");
    // ---- the key: every field at both ends of its bits, none bleeds into its neighbour ----
    {
        static_assert(plan_key(0, 0, 0) == 0ull && plan_key(1, 0, 0) == 1ull << 32 && plan_key(0, 1, 0) == 1ull << 40, "the layout");
        CHECK(plan_key(0, 0, 0xFFFFFFFFu) == 0xFFFFFFFFull);                        // a full index leaves the peer field alone
        CHECK(plan_key_peer(plan_key(0, 0, 0xFFFFFFFFu)) == 0 && plan_key_phase(plan_key(0, 0, 0xFFFFFFFFu)) == 0);
        CHECK(plan_key(63, 0, 0) == 63ull << 32 && plan_key_index(plan_key(63, 0, 0)) == 0 && plan_key_phase(plan_key(63, 0, 0)) == 0);
        CHECK(plan_key(0, 255, 0) == 255ull << 40 && plan_key_peer(plan_key(0, 255, 0)) == 0);
        CHECK(plan_key(255, 254, 0) < plan_key(0, 255, 0));                        // phase-major: any peer of phase 254 sorts in front of phase 255
        CHECK(plan_key(0, 7, 0xFFFFFFFFu) < plan_key(1, 7, 0));                    // ... and inside a phase any index of peer 0 in front of peer 1
        const uint32_t phases[] = {0u, 1u, 254u, 255u}, indices[] = {0u, 1u, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFFFu};
        const int peers[] = {0, 1, 63, 255};
        for (uint32_t ph : phases) for (int peer : peers) for (uint32_t index : indices) {   // encode -> decode
            const unsigned long long key = plan_key(peer, ph, index);
            CHECK(plan_key_phase(key) == ph && plan_key_peer(key) == peer && plan_key_index(key) == index && key >> 48 == 0);
        }
    }
    // ---- empty lists ----
    {
        Offs off{7, 7}, bytes{7}; uint64_t total = 7;
        segment(Keys(), nullptr, 4, 0, off, total);                                // no phase at all: the closing entry alone
        CHECK(off == Offs({0}) && total == 0);
        phase_offsets(off, 4, 1, bytes);
        CHECK(bytes.empty());
        segment(Keys(), nullptr, 1, 3, off, total);                                // one rank: no peer, three phases
        CHECK(off == Offs(4, 0) && total == 0);
        phase_offsets(off, 1, 4, bytes);
        CHECK(bytes == Offs(6, 0));
        CHECK(refused(Keys{plan_key(0, 0, 0)}, 4, 0));                             // no phase holds a key
    }
    // ---- P == 1 with entries (a rank's own id as the peer: the layout does not care) ----
    {
        Offs off, bytes; uint64_t total = 0;
        segment(Keys{plan_key(0, 0, 5), plan_key(0, 2, 1), plan_key(0, 2, 9)}, nullptr, 1, 3, off, total);
        CHECK(off == Offs({0, 1, 1, 3}) && total == 3);
        phase_offsets(off, 1, 4, bytes);
        CHECK(bytes == Offs({0, 4, 0, 0, 0, 8}));
    }
    // ---- P == MAX_PARTS, the last rank as the peer; phases 0, 254 and 255 ----
    {
        const int P = MAX_PARTS;
        const Keys keys{plan_key(0, 0, 0), plan_key(63, 0, 0xFFFFFFFFu), plan_key(63, 254, 3), plan_key(0, 255, 0), plan_key(63, 255, 0xFFFFFFFFu)};
        Offs off; uint64_t total = 0;
        segment(keys, nullptr, P, 256, off, total);
        CHECK(off.size() == (size_t)P * 256 + 1 && total == 5 && off.back() == 5);
        CHECK(off[0] == 0 && off[1] == 1 && off[63] == 1 && off[64] == 2);         // phase 0: peer 0, nobody, peer 63
        CHECK(off[(size_t)254 * P + 63] == 2 && off[(size_t)254 * P + 64] == 3);
        CHECK(off[(size_t)255 * P] == 3 && off[(size_t)255 * P + 1] == 4 && off[(size_t)255 * P + 63] == 4 && off[(size_t)255 * P + 64] == 5);
        // 255 phases (the most a plan takes): phase 254 is the last one in range, phase 255 is refused; so is a peer that is no rank
        CHECK(!refused(Keys{plan_key(63, 254, 3)}, P, 255) && refused(Keys{plan_key(0, 255, 0)}, P, 255));
        CHECK(refused(Keys{plan_key(64, 0, 0)}, P, 255) && refused(Keys{plan_key(255, 0, 0)}, P, 255));
        CHECK(refused(Keys{plan_key(2, 0, 0)}, 2, 1) && !refused(Keys{plan_key(1, 0, 0xFFFFFFFFu)}, 2, 1));   // a full index is still peer 1
        CHECK(refused(Keys{plan_key(0, 1, 0)}, 2, 1));
    }
    // ---- record lengths whose sum passes 2^32: the offsets stay 64 bits wide ----
    {
        const Keys keys{plan_key(0, 0, 1), plan_key(1, 0, 2), plan_key(1, 0, 3), plan_key(0, 1, 4)};
        const std::vector<uint32_t> lens{0xFFFFFFFFu, 0xFFFFFFFFu, 2u, 0xFFFFFFFFu};
        Offs off, bytes; uint64_t total = 0;
        segment(keys, &lens, 2, 2, off, total);
        CHECK(off == Offs({0, 0xFFFFFFFFull, 0x200000000ull, 0x2FFFFFFFFull, 0x2FFFFFFFFull}) && total == 0x2FFFFFFFFull);
        phase_offsets(off, 2, 4, bytes);                                           // ... and so do the byte ranges of the words
        CHECK(bytes == Offs({0, 0x3FFFFFFFCull, 0x800000000ull, 0, 0x3FFFFFFFCull, 0x3FFFFFFFCull}));
    }
    // ---- byte ranges: relative to each phase's start, peer after peer, the closing entry = the phase's total ----
    {
        const int P = 3;
        const Keys keys{plan_key(1, 0, 0), plan_key(2, 0, 0), plan_key(2, 0, 1), plan_key(0, 1, 0), plan_key(0, 1, 1), plan_key(2, 1, 0), plan_key(1, 2, 7)};
        Offs off, b1, b4; uint64_t total = 0;
        segment(keys, nullptr, P, 3, off, total);
        CHECK(off == Offs({0, 0, 1, 3, 5, 5, 6, 6, 7, 7}) && total == 7);
        phase_offsets(off, P, 1, b1); phase_offsets(off, P, 4, b4);
        CHECK(b1 == Offs({0, 0, 1, 3, /**/ 0, 2, 2, 3, /**/ 0, 0, 1, 1}));
        CHECK(b1.size() == b4.size());
        for (size_t k = 0; k < b1.size(); ++k) CHECK(b4[k] == 4 * b1[k]);
        for (size_t ph = 0; ph < 3; ++ph) {
            CHECK(b1[ph * (P + 1)] == 0 && b1[ph * (P + 1) + P] == off[(ph + 1) * P] - off[ph * P]);
            for (int q = 0; q < P; ++q) CHECK(b1[ph * (P + 1) + q + 1] - b1[ph * (P + 1) + q] == off[ph * P + q + 1] - off[ph * P + q]);
        }
    }
    printf("ok\n");
    return 0;
}
