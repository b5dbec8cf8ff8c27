// dc_ranges.h -- planner and 64-bit accounting of the ranged data-cost pass (k_dc.hip dc_ranged).  Plain host C++, no HIP: the
// branches that only a scene of 2^32 (face, view) pairs reaches are exercised by tests/cpp/test_dc_ranges.cpp, nowhere else.
#pragma once
#include <stdint.h>
#include <vector>

namespace mvs {

// ranks of passing pairs, column pointers and nnz of ONE table are 32 bits wide: every such count stays below this
constexpr uint64_t DC_LIMIT_32 = 0xFFFFFFF0ull;

struct DcRange { uint32_t begin, end; };   // positions [begin, end) of the library's face order

// The walk over the context's faces [begin, end): n consecutive ranges of `per` faces, the last one holds the rest.  No list is
// materialised (B = 1 on a large mesh is one range per face).  n >= 1 always: an empty input is ONE empty range, and that is the
// only empty range a plan ever has.
struct DcPlan {
    uint32_t begin = 0, end = 0, per = 0, n = 1;
    DcRange range(uint32_t r) const {
        const uint64_t b = (uint64_t)begin + (uint64_t)r * per, e = b + per;
        return DcRange{(uint32_t)b, (uint32_t)(e < end ? e : end)};
    }
    uint32_t first_faces() const { const DcRange g = range(0); return g.end - g.begin; }   // what mvs_ctx_dc_ranges reports
};

// option "dc_range_pairs" = B:
//   B > 0: a range holds exactly max(1, floor(B / n_views)) faces (no rounding to the 64-face words of the bit matrices);
//   B = 0: one range, unless faces x views >= DC_LIMIT_32 -- then the fewest equal ranges whose faces x views stay below it.
// Without views there is nothing to bound: one range.
inline DcPlan dc_plan(uint32_t face_begin, uint32_t face_end, uint32_t n_views, uint64_t B) {
    DcPlan p;
    p.begin = face_begin; p.end = face_end < face_begin ? face_begin : face_end;
    const uint64_t nf = (uint64_t)p.end - p.begin;
    p.per = (uint32_t)nf; p.n = 1;
    if (nf == 0 || n_views == 0) return p;
    uint64_t per = nf;
    if (B > 0) {
        per = B / n_views;
        if (per < 1) per = 1;
    } else if (nf * n_views >= DC_LIMIT_32) {
        const uint64_t per_max = (DC_LIMIT_32 - 1) / n_views;   // the most faces with faces x views < DC_LIMIT_32 (>= 65536: n_views <= 65535)
        const uint64_t n = (nf + per_max - 1) / per_max;        // fewer ranges would need more than per_max faces in one of them
        per = (nf + n - 1) / n;                                 // equal ranges; ceil(nf / per) == n because per <= per_max
    }
    if (per > nf) per = nf;
    p.per = (uint32_t)per;
    p.n = (uint32_t)((nf + per - 1) / per);
    return p;
}

// The (view_id, quality) entries every range leaves behind are kept back to back; range r starts at base[r] of them.  A range's own
// col_ptr stays 32-bit and local (one range never holds DC_LIMIT_32 entries), the bases are 64-bit and live on the host: their sum
// may pass 2^32.  The kept col_ptr arrays (faces + 1 words per range) are back to back as well: ptr_base.
struct DcKept {
    std::vector<uint64_t> base{0}, ptr_base{0};
    void clear() { base.assign(1, 0); ptr_base.assign(1, 0); }
    void push(uint32_t faces, uint32_t entries) { base.push_back(base.back() + entries); ptr_base.push_back(ptr_base.back() + (uint64_t)faces + 1); }
    size_t ranges() const { return base.size() - 1; }
    uint64_t entries(size_t r) const { return base[r + 1] - base[r]; }
    uint64_t total() const { return base.back(); }
};

// only the FINAL table has to fit 32-bit column pointers: its exact 64-bit total is taken first
inline bool dc_final_fits(uint64_t total_entries) { return total_entries < DC_LIMIT_32; }

}  // namespace mvs
