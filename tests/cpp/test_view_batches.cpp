// The arithmetic in front of the view inputs' launches (csrc/view_batches.h) on its own: the batch cut on hand-written cases and on
// properties of seeded random inputs (never against a second copy of its loop), where an item lies in its batch, and the prefix array and
// grid bound of a span launch at counts around 2^32.  Built with -fsanitize=address,undefined by tests/test_view_batches_host.py; prints
// "ok" and exits 0, or says which check failed.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>

#include "view_batches.h"

using namespace mvs;

#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) { fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); exit(1); } \
    } while (0)

typedef std::vector<uint64_t> Needs;
typedef std::vector<size_t> Cut;

static Cut cut_of(const Needs& need, uint64_t cap, size_t max_items = 0) { return cut_batches(need.data(), need.size(), cap, max_items); }

static uint64_t next_random(uint64_t& s) { s = s * 6364136223846793005ull + 1442695040888963407ull; return s >> 33; }

int main() {
    CHECK(align16(0) == 0 && align16(1) == 16 && align16(16) == 16 && align16(17) == 32 && align16((1ull << 32) + 1) == (1ull << 32) + 16);
    // ---- hand-written cases ----
    {
        CHECK(cut_of({}, 100) == Cut({0}));                                        // empty input
        CHECK(first_over_cap(nullptr, 0, 100) == 0);
        CHECK(cut_of({100}, 100) == Cut({0, 1}));                                  // one item equal to cap
        const Needs over{101};                                                     // one item of cap + 1: reported as item 0
        CHECK(first_over_cap(over.data(), 1, 100) == 0);
        const Needs third{100, 7, 101, 300};                                       // ... and the FIRST of several
        CHECK(first_over_cap(third.data(), 4, 100) == 2 && first_over_cap(third.data(), 2, 100) == 2);
        // eight items, a cap that is the sum of a run of them, three batches (tests/test_gpu_jpeg_decode.py test_three_batches)
        CHECK(cut_of({5, 3, 4, 6, 2, 7, 1, 4}, 12) == Cut({0, 3, 5, 8}));
        CHECK(cut_of({30, 30, 40}, 100) == Cut({0, 3}));                           // needs that sum to exactly cap
        CHECK(cut_of({30, 30, 41}, 100) == Cut({0, 2, 3}));
        CHECK(cut_of(Needs(32769, 1), 1ull << 30, 32768) == Cut({0, 32768, 32769}));   // max_items reached before cap
        CHECK(cut_of(Needs(32769, 1), 1ull << 30) == Cut({0, 32769}));             // ... and no bound without it
        CHECK(cut_of({60, 0, 40, 0, 1}, 100) == Cut({0, 4, 5}));                   // a need of 0 joins its neighbour
        CHECK(cut_of({0, 0}, 0) == Cut({0, 2}));
        // (the caller refuses an item above cap first; the cut itself still gives it a batch of its own: a batch always takes its first item)
        CHECK(cut_of({5, 200, 5}, 100) == Cut({0, 1, 2, 3}));
    }
    // ---- properties, a few hundred seeded random inputs: n <= 40, needs <= cap, cap drawn per case ----
    uint64_t seed = 20240607;
    for (int it = 0; it < 400; ++it) {
        const size_t n = (size_t)(next_random(seed) % 41);
        const uint64_t cap = 1 + next_random(seed) % (it % 3 == 0 ? 64 : 100000);
        const size_t max_items = it % 4 == 0 ? 1 + (size_t)(next_random(seed) % 5) : 0;
        Needs bytes(n), need(n);
        for (size_t k = 0; k < n; ++k) {
            bytes[k] = next_random(seed) % (cap + 1);
            if (it % 5 == 0 && next_random(seed) % 4 == 0) bytes[k] = 0;
            if (align16(bytes[k]) > cap) bytes[k] = cap / 16 * 16;   // the staged callers' needs are align16(bytes): keep them <= cap
            need[k] = it % 2 ? align16(bytes[k]) : bytes[k];         // ... and the files' are plain byte counts
        }
        CHECK(first_over_cap(need.data(), n, cap) == n);
        const Cut cut = cut_of(need, cap, max_items);
        // the batches tile [0, n) in order, none is empty
        CHECK(cut.front() == 0 && cut.back() == n && (n == 0) == (cut.size() == 1));
        for (size_t b = 0; b + 1 < cut.size(); ++b) {
            CHECK(cut[b] < cut[b + 1]);
            uint64_t sum = 0;
            for (size_t k = cut[b]; k < cut[b + 1]; ++k) sum += need[k];
            CHECK(sum <= cap);                                                    // every batch fits
            if (max_items) CHECK(cut[b + 1] - cut[b] <= max_items);
            // ... and is maximal: the next item would not have fitted, or the item bound stopped it
            if (cut[b + 1] < n) CHECK(sum + need[cut[b + 1]] > cap || (max_items && cut[b + 1] - cut[b] == max_items));
        }
        // where the items lie: the running align16 sums inside a batch; most: the largest batch sum
        const BatchLayout L = batch_layout(bytes.data(), n, cut);
        CHECK(L.off.size() == n);
        uint64_t most = 0;
        for (size_t b = 0; b + 1 < cut.size(); ++b) {
            CHECK(L.off[cut[b]] == 0);
            for (size_t k = cut[b]; k + 1 < cut[b + 1]; ++k) CHECK(L.off[k + 1] == L.off[k] + align16(bytes[k]) && L.off[k + 1] % 16 == 0);
            const uint64_t sum = L.off[cut[b + 1] - 1] + align16(bytes[cut[b + 1] - 1]);
            if (sum > most) most = sum;
        }
        CHECK(L.most == most && (n != 0 || most == 0));
        if (it % 2) CHECK(L.most <= cap);                                         // (cut by the aligned needs: the staging never exceeds the cap)
    }
    // ---- prefix arrays: 64 bits wide ----
    {
        CHECK(span_prefix({}) == std::vector<unsigned long long>({0ull}));
        const std::vector<unsigned long long> p = span_prefix({0xFFFFFFFFull, 1, 0, 0xFFFFFFFFull});   // the counts reach 2^32 without wrapping
        CHECK(p.size() == 5 && p[1] == 0xFFFFFFFFull && p[2] == 1ull << 32 && p[3] == 1ull << 32 && p[4] == (1ull << 33) - 1);
        const std::vector<unsigned long long> q = span_prefix({1ull << 32, 5});   // a total above 2^32 from two items
        CHECK(q[1] == 1ull << 32 && q[2] == (1ull << 32) + 5);
    }
    // ---- the grid bound, exactly where the launchers had it ----
    {
        const uint64_t G = 0x7FFFFFFFull;
        uint64_t blocks = 1;
        CHECK(span_blocks(0, 256, false, blocks) && blocks == 0);
        CHECK(span_blocks(1, 256, false, blocks) && blocks == 1);
        CHECK(span_blocks(257, 256, true, blocks) && blocks == 2);
        // mask_pack_kernel (a lane per word) and lens_mask_kernel (32 lanes per word): blocks >= 0x7FFFFFFF is refused
        CHECK(span_blocks((G - 1) * 256, 256, false, blocks) && blocks == G - 1);
        CHECK(!span_blocks((G - 1) * 256 + 1, 256, false, blocks) && blocks == G);
        CHECK(span_blocks((G - 1) * 8 * 32, 256, false, blocks) && !span_blocks(((G - 1) * 8 + 1) * 32, 256, false, blocks));
        // lens_kernel and colour_kernel (a lane per chunk): n_chunks >= 0x7FFFFFFF * 256 is refused, one block later
        CHECK(span_blocks(G * 256 - 1, 256, true, blocks) && blocks == G);
        CHECK(!span_blocks(G * 256, 256, true, blocks));
    }
    printf("ok\n");
    return 0;
}
