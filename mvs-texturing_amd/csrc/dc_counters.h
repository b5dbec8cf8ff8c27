// dc_counters.h -- the slots of ctx->counters (64 words of 64 bits, cleared at the start of every data-cost pass) by name, and the host
// function that turns a block of them into mvs_dc_stats.  Plain constants and plain host C++, no HIP: k_dc.hip / k_bvh.hip index the
// block with the names, k_prep.hip borrows a word of it, tests/cpp/test_dc_counters.cpp compiles this header on its own.
#pragma once
#include <stdint.h>
#include <string.h>

#include "../../include/mvs_viewsel.h"

namespace mvs {

enum {
    // why a (face, view) pair left, counted per pair with the option "stats" (cull_kernel, info_kernel and the two kernels behind it)
    C_BACK = 0, C_ANGLE = 1, C_OUTSIDE = 2, C_OCCL = 3, C_ZEROQ = 4, C_SURV = 5,
    C_RAYS = 6,              // (vertex, view) rays needed (need_kernel)
    C_PASS = 7,              // pairs that pass the culls
    // the packet ray kernel of k_bvh.hip: node visits, leaf visits (16 triangles each), packets, packets under the generic slab test
    C_RNODES = 8, C_RTRIS = 9, C_RPACKETS = 10, C_RGENERIC = 11,
    C_REWALK = 12,           // footprints left to rewalk_info_kernel: the device-side length of its list, counted with or without "stats"
    C_RLEAF_ROUNDS = 13,     // rounds of 4 candidate rays x 16 triangles at the leaves
    C_N_SUMMED = 14,         // [0, C_N_SUMMED): counts per pair or per ray -- a ranged pass sums them over its ranges
    C_MAX_Q_BITS = 14, C_PCTL_BITS = 15,   // percentile_kernel's report: the bits of the maximum quality and of the percentile
    C_N_STATS = 16,          // [0, C_N_STATS) is what mvs_dc_stats is made of: one read-back
    C_PREP = 32,             // k_prep.hip: two 32-bit words ("changed", "any seed") of the flood fill, on the second stream
    C_KMAX = 48,             // launch_outlier: the longest column, one 32-bit word
    C_N_SLOTS = 64           // what mvs_ctx_create allocates and a pass clears
};
static_assert(C_RLEAF_ROUNDS < C_N_SUMMED && C_N_SUMMED == C_MAX_Q_BITS && C_PCTL_BITS == C_MAX_Q_BITS + 1 && C_PCTL_BITS < C_N_STATS,
              "the summed counters, then the two report words, are the block that is read back");
static_assert(C_N_STATS <= C_PREP && C_PREP < C_KMAX && C_KMAX < C_N_SLOTS, "borrowed words lie behind the statistics, apart from each other, inside the block");

// sum[k] += block[k] for the counters a ranged pass adds up (64 bits: the pairs of all ranges together pass 2^32)
inline void dc_counters_add(unsigned long long* sum, const unsigned long long* block) {
    for (int k = 0; k < C_N_SUMMED; ++k) sum[k] += block[k];
}

// The fields of mvs_dc_stats that come from the C_N_STATS words `c` (one pass's block, or dc_counters_add's sums with the report words
// of the final percentile), from the deferred footprints and from the table's nnz.  pairs and nnz_pre are not the counters' business.
inline void dc_stats_from_counters(const unsigned long long* c, uint64_t deferred, uint64_t nnz, mvs_dc_stats* S) {
    S->cull_backface = c[C_BACK]; S->cull_angle = c[C_ANGLE]; S->cull_outside = c[C_OUTSIDE]; S->cull_occluded = c[C_OCCL];
    S->cull_zero_quality = c[C_ZEROQ]; S->rays = c[C_RAYS]; S->ray_nodes = c[C_RNODES];
    S->ray_tris = c[C_RTRIS] * 16ull;   // leaf visits -> triangles: 16 per leaf (k_bvh.hip MVS_LEAF_T)
    S->ray_leaf_rounds = c[C_RLEAF_ROUNDS]; S->ray_packets = c[C_RPACKETS]; S->ray_packets_generic = c[C_RGENERIC];
    S->footprints_lane_group = deferred; S->footprints_rewalked = c[C_REWALK];
    S->nnz = nnz;
    const uint32_t mq = (uint32_t)c[C_MAX_Q_BITS], pc = (uint32_t)c[C_PCTL_BITS];
    memcpy(&S->max_quality, &mq, 4); memcpy(&S->percentile, &pc, 4);
}

}  // namespace mvs
