// view_batches.h -- the arithmetic every view input shares in front of its launches (view_input.h): the cut of a list of items into batches
// whose bytes fit max_scratch_bytes, where an item lies inside its batch, and the prefix array and block count of a span launch.  Plain
// host C++, no HIP: tests/cpp/test_view_batches.cpp runs it on its own, the counts near 2^32 and the grid bound included.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <vector>

namespace mvs {

constexpr uint64_t VIEW_SCRATCH_DEFAULT = 1ull << 30;   // max_scratch_bytes where the caller names none (mvs_jpegdec_default_params)
constexpr size_t VIEW_FILES_PER_BATCH = 32768;          // files get an image per grid row: at most 65535

inline uint64_t align16(uint64_t v) { return (v + 15u) & ~15ull; }

// the first item that does not fit alone (need > cap), or n: the caller refuses it with its view number and its own text
inline size_t first_over_cap(const uint64_t* need, size_t n, uint64_t cap) { size_t k = 0; while (k < n && need[k] <= cap) ++k; return k; }

// The batch cut: items [cut[k], cut[k + 1]) are batch k.  A batch always takes its first item, then grows while the sum with the next
// one stays <= cap and it holds fewer than max_items (0: no bound).  No item: cut == {0}.
inline std::vector<size_t> cut_batches(const uint64_t* need, size_t n, uint64_t cap, size_t max_items = 0) {
    std::vector<size_t> cut{0};
    for (size_t a = 0; a < n;) {
        size_t b = a; uint64_t sum = 0;
        while (b < n && (!max_items || b - a < max_items) && (b == a || sum + need[b] <= cap)) sum += need[b++];
        cut.push_back(b);
        a = b;
    }
    return cut;
}

// Where the items' bytes lie: every batch starts at 0 of one buffer, its items follow each other at multiples of 16: off[k] is the
// running sum of align16(bytes) inside k's batch, and `most`, the largest batch sum, the buffer every batch fits.
struct BatchLayout { std::vector<uint64_t> off; uint64_t most = 0; };
inline BatchLayout batch_layout(const uint64_t* bytes, size_t n, const std::vector<size_t>& cut) {
    BatchLayout L;
    L.off.assign(n, 0);
    for (size_t b = 0; b + 1 < cut.size(); ++b) {
        uint64_t sum = 0;
        for (size_t k = cut[b]; k < cut[b + 1]; ++k) { L.off[k] = sum; sum += align16(bytes[k]); }
        if (sum > L.most) L.most = sum;
    }
    return L;
}

// A span launch numbers the work of all items of a batch through: item k owns [ptr[k], ptr[k + 1]) -- 64 bits wide, one item may bring 2^32.
inline std::vector<unsigned long long> span_prefix(const std::vector<uint64_t>& count) {
    std::vector<unsigned long long> ptr(count.size() + 1, 0);
    for (size_t k = 0; k < count.size(); ++k) ptr[k + 1] = ptr[k] + count[k];
    return ptr;
}
// the blocks of `threads` lanes that `lanes` lanes need; false: more than a grid holds, the caller refuses with its own text.  The mask
// kernels' launchers refuse blocks >= 0x7FFFFFFF, those of lens_kernel and colour_kernel lanes >= 0x7FFFFFFF * threads (one block more).
inline bool span_blocks(uint64_t lanes, uint32_t threads, bool bound_on_lanes, uint64_t& blocks) {
    blocks = (lanes + threads - 1u) / threads;
    return bound_on_lanes ? lanes < 0x7FFFFFFFull * threads : blocks < 0x7FFFFFFFull;
}

}  // namespace mvs
