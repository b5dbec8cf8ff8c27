// The planner and the 64-bit accounting of the ranged data-cost pass (csrc/dc_ranges.h) on their own: the cases of 2^32 (face, view)
// pairs and 2^32 kept entries, which no test scene reaches, run here and nowhere else.  Built with -fsanitize=address,undefined by
// tests/test_dc_ranges_host.py; prints "ok" and exits 0, or says which check failed.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "dc_ranges.h"

using namespace mvs;

#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) { fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); exit(1); } \
    } while (0)

// consecutive, covers [begin, end) exactly, never empty except for an empty input; every range but the last holds `per` faces.
// Walks every range up to `walk_limit` of them, and the first and last thousand of a longer plan.
static void check_cover(const DcPlan& p, uint32_t begin, uint32_t end, uint32_t walk_limit = 1u << 20) {
    CHECK(p.n >= 1 && p.begin == begin && p.end == end);
    if (begin == end) { CHECK(p.n == 1 && p.range(0).begin == begin && p.range(0).end == begin && p.first_faces() == 0); return; }
    CHECK(p.range(0).begin == begin && p.range(p.n - 1).end == end);
    CHECK(p.first_faces() == p.range(0).end - p.range(0).begin);
    auto one = [&](uint32_t r) {
        const DcRange g = p.range(r);
        CHECK(g.begin < g.end && g.end <= end && g.begin >= begin);
        if (r + 1 < p.n) { CHECK(g.end - g.begin == p.per); CHECK(p.range(r + 1).begin == g.end); }
        else CHECK(g.end - g.begin <= p.per);
    };
    if (p.n <= walk_limit) { for (uint32_t r = 0; r < p.n; ++r) one(r); }
    else { for (uint32_t r = 0; r < 1000; ++r) { one(r); one(p.n - 1 - r); } }
    // the lengths add up (64-bit: per x n may pass 2^32)
    const uint64_t nf = (uint64_t)end - begin;
    CHECK((uint64_t)p.per * (p.n - 1) < nf && nf <= (uint64_t)p.per * p.n);
}

int main() {
    // ---- the rule for B > 0: exactly max(1, floor(B / V)) faces per range, the last range holds the rest ----
    {
        const uint32_t V = 12, begin = 37, end = 37 + 9680, nf = end - begin;
        const uint64_t Bs[] = {1, V - 1, V, V + 1, 64ull * V, 12ull * 1000, 12ull * 9680, 12ull * 9681, 1ull << 62, ~0ull};
        for (uint64_t B : Bs) {
            const DcPlan p = dc_plan(begin, end, V, B);
            uint64_t per = B / V; if (per < 1) per = 1; if (per > nf) per = nf;
            CHECK(p.per == per && p.n == (nf + per - 1) / per);
            check_cover(p, begin, end);
        }
        CHECK(dc_plan(0, 9680, 12, 12 * 1000).n == 10 && dc_plan(0, 9680, 12, 12 * 1000).range(9).end - dc_plan(0, 9680, 12, 12 * 1000).range(9).begin == 680);
        CHECK(dc_plan(100, 164, 8, 8).n == 64 && dc_plan(100, 164, 8, 8).per == 1);
        // one range per face of the largest mesh: nothing is materialised, nothing wraps
        const DcPlan big = dc_plan(0, 0xFFFFFFFFu, 7, 1);
        CHECK(big.n == 0xFFFFFFFFu && big.per == 1);
        check_cover(big, 0, 0xFFFFFFFFu);
    }
    // ---- empty inputs: one empty range; no views: one range (nothing to bound) ----
    for (uint64_t B : {0ull, 1ull, 400ull, ~0ull}) {
        check_cover(dc_plan(5, 5, 12, B), 5, 5);
        check_cover(dc_plan(0, 0, 0, B), 0, 0);
        const DcPlan p = dc_plan(0, 1280, 0, B);
        CHECK(p.n == 1 && p.per == 1280);
        check_cover(p, 0, 1280);
    }
    // ---- the automatic rule (B = 0) ----
    {
        const DcPlan p = dc_plan(0, 9680, 12, 0);
        CHECK(p.n == 1 && p.per == 9680);
        // the last scene of one range and the first of two
        const uint32_t V = 65535;
        const uint32_t f1 = (uint32_t)((DC_LIMIT_32 - 1) / V);                   // f1 x V < limit <= (f1 + 1) x V
        CHECK((uint64_t)f1 * V < DC_LIMIT_32 && (uint64_t)(f1 + 1) * V >= DC_LIMIT_32);
        CHECK(dc_plan(0, f1, V, 0).n == 1 && dc_plan(0, f1 + 1, V, 0).n == 2);
        const struct { uint32_t F, V; } cases[] = {{9996980u, 1000u}, {65537u, 65535u}, {0xFFFFFFFFu, 65535u}, {0xFFFFFFFFu, 1u}, {0xFFFFFFF0u, 1u}, {0xFFFFFFEFu, 1u}, {3000000000u, 3u}};
        for (const auto& c : cases) {
            for (uint32_t begin : {0u, 11u}) {
                if (begin > c.F) continue;
                const DcPlan q = dc_plan(begin, c.F, c.V, 0);
                const uint64_t nf = (uint64_t)c.F - begin;
                check_cover(q, begin, c.F);
                CHECK((uint64_t)q.per * c.V < DC_LIMIT_32);                       // every range stays below the limit ...
                if (nf * c.V < DC_LIMIT_32) { CHECK(q.n == 1); continue; }
                CHECK(q.n >= 2);
                const uint64_t fewer = (nf + (q.n - 1) - 1) / (q.n - 1);          // ... and one range fewer would not: its largest range
                CHECK(fewer * c.V >= DC_LIMIT_32);
                // equal ranges: the last one is at most one `per` short of the others by less than n faces
                CHECK((uint64_t)q.per * q.n - nf < q.n);
            }
        }
        CHECK(dc_plan(0, 9996980u, 1000u, 0).n == 3);                             // 9 996 980 000 pairs: three ranges of 3 332 327 faces
        CHECK(dc_plan(0, 0xFFFFFFFFu, 65535u, 0).n == 65536u);
    }
    // ---- accounting: bases of ranges whose entries sum past 2^32 do not wrap ----
    {
        DcKept k;
        CHECK(k.ranges() == 0 && k.total() == 0);
        const uint32_t big = 0xFFFFFFEFu;                                        // the most one range can hold
        uint64_t want = 0, want_ptr = 0;
        for (int r = 0; r < 40; ++r) {
            const uint32_t faces = 1000000u + (uint32_t)r, entries = r % 3 == 2 ? 0u : big;
            CHECK(k.base[r] == want && k.ptr_base[r] == want_ptr);
            k.push(faces, entries);
            want += entries; want_ptr += (uint64_t)faces + 1;
            CHECK(k.entries(r) == entries);
        }
        CHECK(k.ranges() == 40 && k.total() == want && want > (1ull << 36) && k.ptr_base.back() == want_ptr);
        for (size_t r = 0; r + 1 < k.base.size(); ++r) CHECK(k.base[r] <= k.base[r + 1]);
        // kept col_ptr words of 2^32 - 1 one-face ranges: 2 words each
        DcKept p;
        p.push(0xFFFFFFFFu, 0); p.push(0xFFFFFFFFu, 7);
        CHECK(p.ptr_base[2] == 2ull * 0x100000000ull && p.total() == 7);
        k.clear();
        CHECK(k.ranges() == 0 && k.total() == 0 && k.ptr_base.back() == 0);
    }
    // ---- the final table: 32-bit column pointers ----
    CHECK(dc_final_fits(0) && dc_final_fits(0xFFFFFFEFull));
    CHECK(!dc_final_fits(0xFFFFFFF0ull) && !dc_final_fits(0xFFFFFFFFull) && !dc_final_fits(0x100000000ull) && !dc_final_fits(45ull << 30));
    {
        DcKept k;   // two ranges that fit one by one and not together
        k.push(10, 0x80000000u); k.push(10, 0x7FFFFFEFu);
        CHECK(dc_final_fits(k.total()));
        k.push(10, 1);
        CHECK(!dc_final_fits(k.total()));
    }
    printf("ok\n");
    return 0;
}
