// k_mrf_sweep.hip -- tex::view_selection on the GPU, part 2 of 3 (k_mrf_setup.hip has the overview): the colour-phased sweeps, which
// dominate a solve, and their launch logic.
//
// Work mapping: G lanes per node (G = 8 / 16 / 32 / 64 from the largest column), 4
// consecutive labels per lane; messages are 8-bit fixed point in HBM (four per 4-byte
// word), damped on odd sweeps only; per-edge cavity vectors go through an LDS tile for
// the label re-alignment gather; min / argmin are fused DPP butterflies.
#include "mrf.h"
#include <atomic>

namespace mvs {

namespace {

struct MsgQ { float scale, step; };      // 255 / lam and lam / 255, fp32, the oracle computes them the same way
__device__ __forceinline__ MsgQ msg_q(float lam) { return MsgQ{255.0f / lam, lam / 255.0f}; }
// 32-bit byte offsets from a wave-uniform base: the load takes the base from SGPRs and the offset from one VGPR
// (global_load ... v_off, s[base]) instead of a 64-bit address built with v_lshl_add_u64 per load
template <class T> __device__ __forceinline__ T ld_off(const void* base, uint32_t byte_off) { return *reinterpret_cast<const T*>(reinterpret_cast<const char*>(base) + byte_off); }
template <class T> __device__ __forceinline__ void st_off(void* base, uint32_t byte_off, T v) { *reinterpret_cast<T*>(reinterpret_cast<char*>(base) + byte_off) = v; }
// v_min_f32 without the canonicalising v_max_f32 x, x, x the compiler puts in front of fminf() on values it loaded from
// memory (no NaN can reach these operands: +inf and finite values only)
__device__ __forceinline__ float min_raw(float a, float b) { float r; asm("v_min_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
// the code a message value `raw` in [0, lam] is stored as, damped against the old code (oracle.cpp msg_code):
// rne(fma(old, alpha, raw * oms)), oms = (1 - alpha) * scale, saturated at 255 -- v_cvt_pk_u8_f32 IS a saturating
// round-to-nearest-even conversion on gfx950 (scripts/probe/cvt_probe.hip), and it drops the byte into place
template <bool DAMP>
__device__ __forceinline__ uint32_t msg_pack_s(float raw_s, float alpha, float old_code, uint32_t byte, uint32_t word) {
    return __builtin_amdgcn_cvt_pk_u8_f32(DAMP ? __builtin_fmaf(old_code, alpha, raw_s) : raw_s, byte, word);
}

// Butterfly partner exchange inside a lane group with DPP (VALU latency) instead of ds_bpermute (LDS
// latency): the pairings xor 1, xor 2 (quad_perm), i <-> 7-i (row_half_mirror) and i <-> 15-i (row_mirror)
// are involutions that merge groups of 2, 4, 8 and 16 lanes, which is all an all-reduce needs (min and
// argmin are exact in any order); only the 32- and 64-lane steps go through a shuffle.
// Fused forms for the hot sweep: v_min_f32 / v_min_u32 with the DPP modifier on src0, i.e. ONE VALU instruction per
// butterfly step where the compiler's v_mov_dpp + canonicalise + min takes three (plus the exec-mask branches it
// builds for a short-circuit argmin).  s_nop 1 = the two wait states a DPP read needs after a VALU write of the
// same register (the hazard recogniser does not look inside inline asm).  All lanes are active where these run.
#define MVS_DPP_OP(op, ctrl) asm("s_nop 1\n\t" op " %0, %1, %1 " ctrl " row_mask:0xf bank_mask:0xf" : "=v"(r) : "v"(v))
template <int STEP, int G>
__device__ __forceinline__ float min_step_f(float v) {
    float r;
    if (STEP == 1) MVS_DPP_OP("v_min_f32_dpp", "quad_perm:[1,0,3,2]");
    else if (STEP == 2) MVS_DPP_OP("v_min_f32_dpp", "quad_perm:[2,3,0,1]");
    else if (STEP == 4) MVS_DPP_OP("v_min_f32_dpp", "row_half_mirror");
    else if (STEP == 8) MVS_DPP_OP("v_min_f32_dpp", "row_mirror");
    else r = fminf(v, __shfl_xor(v, STEP, G));
    return r;
}
template <int STEP, int G>
__device__ __forceinline__ uint32_t min_step_u(uint32_t v) {
    uint32_t r;
    if (STEP == 1) MVS_DPP_OP("v_min_u32_dpp", "quad_perm:[1,0,3,2]");
    else if (STEP == 2) MVS_DPP_OP("v_min_u32_dpp", "quad_perm:[2,3,0,1]");
    else if (STEP == 4) MVS_DPP_OP("v_min_u32_dpp", "row_half_mirror");
    else if (STEP == 8) MVS_DPP_OP("v_min_u32_dpp", "row_mirror");
    else r = min(v, (uint32_t)__shfl_xor(v, STEP, G));
    return r;
}
#undef MVS_DPP_OP
template <int G>
__device__ __forceinline__ float group_min_fused(float v) {
    v = min_step_f<1, G>(v); v = min_step_f<2, G>(v); v = min_step_f<4, G>(v);
    if (G >= 16) v = min_step_f<8, G>(v);
    if (G >= 32) v = min_step_f<16, G>(v);
    if (G >= 64) v = min_step_f<32, G>(v);
    return v;
}
// Four group minima at once: the DPP steps of the four chains are interleaved, so a step's operand was written three
// instructions earlier and only the first block needs the DPP read-after-write wait states (one chain at a time costs
// `s_nop 1` plus the compiler's own padding in front of each of its 4 steps).
#define MVS_DPP4(nop, ctrl) asm(nop "v_min_f32_dpp %0, %4, %4 " ctrl " row_mask:0xf bank_mask:0xf\n\tv_min_f32_dpp %1, %5, %5 " ctrl " row_mask:0xf bank_mask:0xf\n\t" \
                                    "v_min_f32_dpp %2, %6, %6 " ctrl " row_mask:0xf bank_mask:0xf\n\tv_min_f32_dpp %3, %7, %7 " ctrl " row_mask:0xf bank_mask:0xf"          \
                                : "=&v"(ra), "=&v"(rb), "=&v"(rc), "=&v"(rd) : "v"(a), "v"(b), "v"(c), "v"(d)); a = ra; b = rb; c = rc; d = rd
template <int G>
__device__ __forceinline__ void group_min_fused4(float& a, float& b, float& c, float& d) {
    if (G == 8) {
        float ra, rb, rc, rd;
        MVS_DPP4("s_nop 1\n\t", "quad_perm:[1,0,3,2]");
        MVS_DPP4("", "quad_perm:[2,3,0,1]");
        MVS_DPP4("", "row_half_mirror");
    } else { a = group_min_fused<G>(a); b = group_min_fused<G>(b); c = group_min_fused<G>(c); d = group_min_fused<G>(d); }
}
#undef MVS_DPP4
template <int G>
__device__ __forceinline__ uint32_t group_min_fused(uint32_t v) {
    v = min_step_u<1, G>(v); v = min_step_u<2, G>(v); v = min_step_u<4, G>(v);
    if (G >= 16) v = min_step_u<8, G>(v);
    if (G >= 32) v = min_step_u<16, G>(v);
    if (G >= 64) v = min_step_u<32, G>(v);
    return v;
}

// own share of every (sub-class, zone): positions of the ids in [nb, ne) inside perm[sb[k], sb[k + 1]) (ids ascending inside a key)
__global__ void mrf_sub_range_kernel(const uint32_t* __restrict__ perm, const uint32_t* __restrict__ sub_begin,
                                     uint32_t nb, uint32_t ne, uint32_t* __restrict__ out) {
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= N_KEY) return;
    const uint32_t cb = sub_begin[c], ce = sub_begin[c + 1];
    uint32_t lo = cb, hi = ce;
    while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (perm[mid] < nb) lo = mid + 1; else hi = mid; }
    out[2 * c] = lo;
    hi = ce;
    while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (perm[mid] < ne) lo = mid + 1; else hi = mid; }
    out[2 * c + 1] = lo;
}

// ---- one colour phase of a sweep; fast path: degree <= 3, K <= 255 (and K <= 4 * G) ----
// 4 labels per lane: lane gl owns labels 4*gl .. 4*gl+3 (one 16-byte load = four label words, one 4-byte access = four
// 8-bit messages or four map bytes), so a 64-lane wave sweeps 64/G nodes per iteration at roughly the instruction count
// of one.  The layout is arranged so that NO per-label masking of the loads is needed:
//   * elements [0, MSG_BASE) of the message buffer are zero for ever: an absent edge (degree < 3, or an empty
//     neighbour column) and every lane beyond the node's labels read their "incoming message" there; words
//     [0, REC_BASE) of the record array are zero as well (label / map words of masked lanes);
//   * an edge whose two label lists are identical (flag in the descriptor; 3/4 of the edges on the synthetic scenes)
//     has no map at all: the identity bytes 4*gl .. 4*gl+3 are a per-lane constant;
//   * the re-alignment gather c[p] goes through a per-group LDS tile with one extra slot holding +inf: 0xFF ("label
//     absent at the sender") is steered onto that slot, so it needs no compare -- fmin(inf - cmin, 1/rho) = 1/rho;
//   * message runs are padded to multiples of 4 elements, so a lane stores all four of its values or none.
// Values a lane computes for label slots beyond the column are garbage that never reaches a valid label: they are
// excluded from min / argmin by the ok[] mask (the only per-label selects left) and land in run padding.
// LDS operations of a wave execute in order and a lane group never spans waves, so the tile needs no barrier.
//
// Decode: the lane that owns the winning label writes the node's sel / label / unary into decode buffer st->w.
// Energy: E = sum_i D_i(l_i) + sum_(i,j) [l_i != l_j] is accumulated HERE, in 32.32 fixed point: the node adds its unary
// and one cut per model edge to a neighbour of a LOWER colour whose label differs -- that neighbour was swept in an
// earlier phase of this sweep, so its label is final, and every edge has exactly one higher-coloured end.  Integer sums:
// the per-block partials (partial[2 * block]) add up to the oracle's energy of the sweep whatever the launch geometry.
// (The access-pattern probes of rounds 4 and 5 -- scripts/sweep_probe.py: all accesses inside a 64 KB window, arithmetic removed, one stream
// dropped at a time, an edge-pair message layout, wider map loads -- are a PATCH on this kernel, scripts/probe/sweep4_probes.patch, which
// scripts/build_variant.py --patch applies to a copy of this file; the product source carries none of them.)
template <int G, bool DAMP, bool XCD>
__global__ void __launch_bounds__(256) mrf_sweep4_kernel(const NodeDesc* __restrict__ desc, const uint32_t* __restrict__ rec, msg_t* msg,
                                                         const mvs_mrf_progress* __restrict__ st, uint32_t* lab2, uint32_t buf_stride,
                                                         uint32_t node_begin /* positions in the (colour, id) order */, uint32_t node_end, float rho, float alpha,
                                                         unsigned long long* __restrict__ partial) {
    // in place: the nodes of one launch share a colour (an independent set), so no run is read by one node and
    // written by another; a node reads its old outgoing run before it overwrites it
    const msg_t* mo = msg; msg_t* mn = msg;
    constexpr int NPB = 256 / G;
    // Tile of a lane group: the 4G cavity values ROW-major over r = label mod 4 (label 4 * gl + r at slot r * G + gl) + the +inf slot 4G.
    // A ds_read_b32 / ds_write_b32 serves lanes 0-31 and 32-63 in one LDS cycle each when they hit 32 different banks (bank = word
    // address mod 32): with this layout the lanes of a group touch consecutive banks (exactly for identical label lists, 3/4 of the
    // edges), and the stride puts the 32 / G groups of a half-wave on disjoint banks (TS = G mod 32 for G < 32).  The label-major tile
    // (slot = label, one float4 write) made every gather a 4-way bank conflict: PMC SQ_LDS_BANK_CONFLICT = 56 % of the LDS cycles.
    // (One tile per group, reused by the three out-edges.  A variant with three tiles -- all writes first, then all twelve gathers, one
    // LDS round trip per node and 9 VGPRs fewer -- measured the same at C3 and 28 % slower where a quarter of the nodes take the
    // 64-lane class: profiles/EXPERIMENTS.md.)
    constexpr int TS = G == 8 ? 40 : 4 * G + 4;
    __shared__ float s_c[NPB * TS];
    __shared__ unsigned long long s_e[8];
    const int grp = threadIdx.x / G, gl = threadIdx.x % G;
    float* __restrict__ tile = s_c + grp * TS;
    // The stop rule runs on the device (mrf_step_kernel) while the host queues sweeps ahead of the reports it reads: a sweep queued
    // after the rule fired changes nothing anybody reads (the best labeling is frozen, the step kernel ignores its energy) -- it ends here
    if (st->stopped) return;
    if (gl == 0) tile[4 * G] = INFINITY;
    __syncthreads();
    const uint32_t wofs = st->w * buf_stride;                // decode buffer of this sweep (flipped by the step kernel when a sweep improves the best energy)
    uint32_t* lab = lab2 + wofs;
    const float lam = 1.0f / rho;
    const MsgQ mq = msg_q(lam);
    const float kappa = rho * mq.step, nstep = -mq.step, oms = (1.0f - alpha) * mq.scale, lam_s = lam * oms;   // the oracle's constants, fp32
    constexpr float HUGE_COST = 1e30f;                       // unary of the label slots beyond the column: never a minimum
    const uint32_t stride = gridDim.x * NPB;
    uint32_t vb = blockIdx.x;
    if (XCD && (gridDim.x & 7u) == 0u) vb = (blockIdx.x & 7u) * (gridDim.x >> 3) + (blockIdx.x >> 3);
    uint32_t i = node_begin + vb * NPB + grp;
    const uint32_t last = node_end - 1;
    const uint32_t n_iter = (node_end - node_begin + stride - 1) / stride;
    const uint32_t t0 = 4u * gl;
    const uint32_t ident_word = 0x03020100u * (uint32_t)G + 0x01010101u * (uint32_t)gl;   // map bytes of an identical-list edge: the slots r * G + gl of the lane's own labels
    // Software pipeline, two nodes deep: while a lane group computes node `it`, the loads of node `it + 1` (label words,
    // three incoming runs, three map words, three neighbour labels and -- damped sweeps -- the three old outgoing runs)
    // and the descriptor of node `it + 2` are in flight.  The kernel had been latency bound: waves parked on memory 65 %
    // of their time with the vector unit 60 % busy and HBM at 3.5 TB/s (PMC, profiles/).  Same-colour nodes never touch
    // each other's runs or labels, so reading a node's inputs one iteration early cannot observe a write of this launch.
    // No address needs a select: a lane beyond the column / the neighbour's column reads whatever follows the run or
    // the record (valid memory -- both arrays carry slack -- and lines its neighbours fetch anyway) and its values never
    // reach a valid label; an absent edge has offsets 0 in the descriptor, i.e. the reserved zero run.
    struct Raw { uint4 lw; uint32_t in[3], map[3], nl[3], old[3]; };
    const uint32_t t0b = 4u * t0, glb = 4u * (uint32_t)gl;   // byte offsets of the lane's label words / map word inside a record
    auto issue = [&](const NodeDesc& d, Raw& r) {
        const uint32_t K = d.kk & 0xFFu, recb = 4u * d.rec;
        r.lw = ld_off<uint4>(rec, recb + t0b);
        uint32_t mposb = recb + 4u * ((K + 3u) & ~3u) + glb;
#pragma unroll
        for (int e = 0; e < 3; ++e) {
            r.in[e] = ld_off<uint32_t>(mo, (d.in_off[e] & ~3u) + t0);
            r.map[e] = ld_off<uint32_t>(rec, mposb);
            if (!(d.out_off[e] & 1u)) mposb += (((d.kk >> (8 + 8 * e)) & 0xFFu) + 3u) & ~3u;   // 4 bytes per 4 map entries
            r.nl[e] = ld_off<uint32_t>(lab, 4u * d.nbr[e]);     // an absent neighbour is recorded as the node itself
            if (DAMP) r.old[e] = ld_off<uint32_t>(mo, (d.out_off[e] & ~3u) + t0); else r.old[e] = d.out_off[e];
        }
    };
    NodeDesc cur = ld_off<NodeDesc>(desc, (uint32_t)sizeof(NodeDesc) * min(i, last));
    Raw rw; issue(cur, rw);
    NodeDesc nxt = ld_off<NodeDesc>(desc, (uint32_t)sizeof(NodeDesc) * min(i + stride, last));
    uint32_t acc_e = 0u, acc_c = 0u;                         // sum of the decoded labels' cost codes (< 2^32 per thread: <= 65535 per node) and cut edges
    for (uint32_t it = 0; it < n_iter; ++it, i += stride) {
        const bool node_ok = i < node_end;
        Raw rn; issue(nxt, rn);                                // node it + 1 (clamped to the last descriptor past the end: harmless reads)
        const NodeDesc nn = ld_off<NodeDesc>(desc, (uint32_t)sizeof(NodeDesc) * min(i + 2u * stride, last));  // node it + 2
        const uint32_t K = node_ok ? (cur.kk & 0xFFu) : 0u;
        bool ok[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) ok[r] = t0 + r < K;
        uint32_t kj3[3], o_out[3]; bool ident[3], low[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            kj3[d] = node_ok ? ((cur.kk >> (8 + 8 * d)) & 0xFFu) : 0u;
            ident[d] = (cur.out_off[d] & 1u) != 0u; low[d] = (cur.in_off[d] & 1u) != 0u && kj3[d] != 0u;
            o_out[d] = cur.out_off[d] & ~3u;
        }
        const uint32_t lw[4] = {rw.lw.x, rw.lw.y, rw.lw.z, rw.lw.w};
        const uint32_t* r_in = rw.in; const uint32_t* r_map = rw.map; const uint32_t* nl = rw.nl; const uint32_t* r_old = rw.old;
        // The update on the 8-bit codes (oracle.cpp mrf_sweep is the definition): Sc = sum of the incoming codes (exact),
        // b = fma(rho * step, Sc, D), cs_e = fma(-step, code_e, b) * oms -- the reweighted cavity D + rho * sum_all - m_e in
        // damped code units, oms = (1 - alpha) * scale -- code' = rne(fma(old, alpha, min(cs[p] - cmin, lam * oms))).
        float cf[3][4], b[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
#pragma unroll
            for (int d = 0; d < 3; ++d) cf[d][r] = (float)((r_in[d] >> (8 * r)) & 0xFFu);   // v_cvt_f32_ubyte<r>
            const float D = ok[r] ? cost_value(lw[r] >> 16) : HUGE_COST;
            b[r] = __builtin_fmaf(kappa, (cf[0][r] + cf[1][r]) + cf[2][r], D);
        }
        // the three cavities and the four group minima (of b and of each cavity) in one interleaved reduction
        float cv[3][4];
#pragma unroll
        for (int d = 0; d < 3; ++d)
#pragma unroll
            for (int r = 0; r < 4; ++r) cv[d][r] = __builtin_fmaf(nstep, cf[d][r], b[r]) * oms;
        float gm = fminf(fminf(b[0], b[1]), fminf(b[2], b[3]));
        float cm0 = fminf(fminf(cv[0][0], cv[0][1]), fminf(cv[0][2], cv[0][3])), cm1 = fminf(fminf(cv[1][0], cv[1][1]), fminf(cv[1][2], cv[1][3])),
              cm2 = fminf(fminf(cv[2][0], cv[2][1]), fminf(cv[2][2], cv[2][3]));
        group_min_fused4<G>(gm, cm0, cm1, cm2);
        const float cmin3[3] = {cm0, cm1, cm2};
        // decode: first argmin_t b[t] -- the group minimum, then the smallest label attaining it (== the sequential
        // "first minimum": comparisons are exact)
        uint32_t bt = (b[3] == gm) ? t0 + 3u : 0xFFFFFFFFu;
        bt = (b[2] == gm) ? t0 + 2u : bt; bt = (b[1] == gm) ? t0 + 1u : bt; bt = (b[0] == gm) ? t0 : bt;
        bt = group_min_fused<G>(bt);                          // every lane of the group holds the winner
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            // the tile holds cs - cmin of edge d (the same subtraction the oracle performs after its gather); the extra slot stays +inf
#pragma unroll
            for (int r = 0; r < 4; ++r) tile[r * G + gl] = cv[d][r] - cmin3[d];
            const uint32_t mw = ident[d] ? ident_word : r_map[d];
            uint32_t w = 0u;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const uint32_t mp = (mw >> (8 * r)) & 0xFFu;
                const uint32_t slot = (G < 64) ? mp : ((mp == 0xFFu) ? (uint32_t)(4 * G) : mp);   // "absent at the sender" -> the +inf slot (G < 64: the records hold 4 * G)
                w = msg_pack_s<DAMP>(min_raw(tile[slot], lam_s), alpha, (float)((r_old[d] >> (8 * r)) & 0xFFu), (uint32_t)r, w);
            }
            if (t0 < kj3[d]) st_off<uint32_t>(mn, o_out[d] + t0, w);      // one 4-byte store (runs are padded)
        }
        // the lane that owns the winning label publishes the decode (K == 0: lane 0 publishes the single label 0 with
        // unary 1, view_selection.cpp:50-51,70-71) and accounts the node's share of the tracking energy (integer:
        // cost codes + 65535 per cut edge, oracle.cpp mrf_energy_sel)
        const bool owner = node_ok && ((K > 0u) ? ((bt >> 2) == (uint32_t)gl) : (gl == 0));
        if (owner) {
            const uint32_t r = bt & 3u;
            const uint32_t wsel = (r == 0u) ? lw[0] : (r == 1u) ? lw[1] : (r == 2u) ? lw[2] : lw[3];
            const uint32_t my_lab = (K > 0u) ? (wsel & 0xFFFFu) + 1u : 0u;
            const uint32_t my_code = (K > 0u) ? (wsel >> 16) : 65535u;
            const uint32_t idb = 4u * cur.id;
            // ONE store: the label.  The position in the column and the unary of the decoded label are not kept per sweep: whoever
            // needs them -- the polish, the reported energy -- derives them from the label once, after the sweeps (mrf_exact_cost_kernel)
            st_off<uint32_t>(lab, idb, my_lab);
            acc_e += my_code;
            acc_c += (low[0] && nl[0] != my_lab) + (low[1] && nl[1] != my_lab) + (low[2] && nl[2] != my_lab);
        }
        cur = nxt; rw = rn; nxt = nn;
    }
    // one partial pair per block (no atomics: same-address atomics serialise at ~12 ns each)
    unsigned long long e = acc_e, c = acc_c;
    for (int o = 32; o > 0; o >>= 1) { e += __shfl_xor(e, o, 64); c += __shfl_xor(c, o, 64); }
    if ((threadIdx.x & 63) == 0) { s_e[threadIdx.x >> 6] = e; s_e[4 + (threadIdx.x >> 6)] = c; }
    __syncthreads();
    if (threadIdx.x == 0) {
        e = s_e[0] + s_e[1] + s_e[2] + s_e[3]; c = s_e[4] + s_e[5] + s_e[6] + s_e[7];
        partial[2 * blockIdx.x] = e + 65535ull * c; partial[2 * blockIdx.x + 1] = c;
    }
}


// ---- the same update with EIGHT labels per lane (class 1: neighbourhood columns of 33 .. 64 labels) ----
// mrf_sweep4_kernel spends one memory instruction on 4 bytes of a run per lane: a 64-lane wave sweeps 4 nodes of this class per iteration
// and issues 20 loads / stores for them.  The probes of rounds 4 and 5 (EXPERIMENTS.md) say the kernel is bound by the NUMBER of memory
// instructions and requests per node, not by their bytes.  Here a node takes 8 lanes and a lane 8 consecutive labels: the three incoming
// runs, the three old outgoing runs, the three map words and the three stores are 8-byte accesses, the label words two 16-byte loads, and
// a wave sweeps 8 nodes per iteration with 21 memory instructions -- half the instructions per node, the same bytes, the same lines.
// Arithmetic, reduction results (min / first argmin are exact in any order), sums (adjacency order per label) and the message / record /
// decode layouts are those of mrf_sweep4_kernel: bit-identical results; only the map BYTES differ (a byte is the slot of THIS kernel's
// LDS tile: row-major over label mod 8, slot = (at & 7) * 8 + (at >> 3), "absent" = slot 64 -- mrf_record_kernel writes them per class).
template <bool DAMP, bool XCD>
__global__ void __launch_bounds__(256) mrf_sweep8_kernel(const NodeDesc* __restrict__ desc, const uint32_t* __restrict__ rec, msg_t* msg,
                                                         const mvs_mrf_progress* __restrict__ st, uint32_t* lab2, uint32_t buf_stride,
                                                         uint32_t node_begin, uint32_t node_end, float rho, float alpha,
                                                         unsigned long long* __restrict__ partial) {
    const msg_t* mo = msg; msg_t* mn = msg;                    // in place: one colour per launch (see mrf_sweep4_kernel)
    constexpr int G = 8, L = 8, NPB = 256 / G;
    constexpr int TS = 72;                                     // 8 x 8 slots + the +inf slot; 72 mod 32 = 8: the 4 groups of a half-wave sit on disjoint banks
    __shared__ float s_c[NPB * TS];
    __shared__ unsigned long long s_e[8];
    const int grp = threadIdx.x / G, gl = threadIdx.x % G;
    float* __restrict__ tile = s_c + grp * TS;
    if (st->stopped) return;
    if (gl == 0) tile[L * G] = INFINITY;
    __syncthreads();
    const uint32_t wofs = st->w * buf_stride;
    uint32_t* lab = lab2 + wofs;
    const float lam = 1.0f / rho;
    const MsgQ mq = msg_q(lam);
    const float kappa = rho * mq.step, nstep = -mq.step, oms = (1.0f - alpha) * mq.scale, lam_s = lam * oms;
    constexpr float HUGE_COST = 1e30f;
    const uint32_t stride = gridDim.x * NPB;
    uint32_t vb = blockIdx.x;
    if (XCD && (gridDim.x & 7u) == 0u) vb = (blockIdx.x & 7u) * (gridDim.x >> 3) + (blockIdx.x >> 3);
    uint32_t i = node_begin + vb * NPB + grp;
    const uint32_t last = node_end - 1;
    const uint32_t n_iter = (node_end - node_begin + stride - 1) / stride;
    const uint32_t t0 = (uint32_t)L * gl;
    // map bytes of an identical-list edge: the slots r * G + gl of the lane's own labels r = 0 .. 7
    const uint32_t ident_lo = 0x18100800u + 0x01010101u * (uint32_t)gl, ident_hi = 0x38302820u + 0x01010101u * (uint32_t)gl;
    struct Raw { uint4 lw0, lw1; uint2 in[3], map[3], old[3]; uint32_t nl[3]; };
    auto issue = [&](const NodeDesc& d, Raw& r) {
        const uint32_t K = d.kk & 0xFFu, recb = 4u * d.rec;
        r.lw0 = ld_off<uint4>(rec, recb + 32u * (uint32_t)gl);
        r.lw1 = ld_off<uint4>(rec, recb + 32u * (uint32_t)gl + 16u);
        uint32_t mposb = recb + 4u * ((K + 3u) & ~3u) + 8u * (uint32_t)gl;
#pragma unroll
        for (int e = 0; e < 3; ++e) {
            r.in[e] = ld_off<uint2>(mo, (d.in_off[e] & ~3u) + t0);
            r.map[e] = ld_off<uint2>(rec, mposb);
            if (!(d.out_off[e] & 1u)) mposb += (((d.kk >> (8 + 8 * e)) & 0xFFu) + 7u) & ~7u;   // (a wide node's map sections are padded to 8 bytes)
            r.nl[e] = ld_off<uint32_t>(lab, 4u * d.nbr[e]);
            if (DAMP) r.old[e] = ld_off<uint2>(mo, (d.out_off[e] & ~3u) + t0); else r.old[e] = make_uint2(0u, 0u);
        }
    };
    NodeDesc cur = ld_off<NodeDesc>(desc, (uint32_t)sizeof(NodeDesc) * min(i, last));
    Raw rw; issue(cur, rw);
    NodeDesc nxt = ld_off<NodeDesc>(desc, (uint32_t)sizeof(NodeDesc) * min(i + stride, last));
    uint32_t acc_e = 0u, acc_c = 0u;
    for (uint32_t it = 0; it < n_iter; ++it, i += stride) {
        const bool node_ok = i < node_end;
        Raw rn; issue(nxt, rn);
        const NodeDesc nn = ld_off<NodeDesc>(desc, (uint32_t)sizeof(NodeDesc) * min(i + 2u * stride, last));
        const uint32_t K = node_ok ? (cur.kk & 0xFFu) : 0u;
        uint32_t kj3[3], o_out[3]; bool ident[3], low[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            kj3[d] = node_ok ? ((cur.kk >> (8 + 8 * d)) & 0xFFu) : 0u;
            ident[d] = (cur.out_off[d] & 1u) != 0u; low[d] = (cur.in_off[d] & 1u) != 0u && kj3[d] != 0u;
            o_out[d] = cur.out_off[d] & ~3u;
        }
        const uint32_t lw[8] = {rw.lw0.x, rw.lw0.y, rw.lw0.z, rw.lw0.w, rw.lw1.x, rw.lw1.y, rw.lw1.z, rw.lw1.w};
        // (the update on the 8-bit codes: see mrf_sweep4_kernel; oracle.cpp mrf_sweep is the definition)
        float b[8], cv[3][8];
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            float cf[3];
#pragma unroll
            for (int d = 0; d < 3; ++d) cf[d] = (float)((((r < 4) ? rw.in[d].x : rw.in[d].y) >> (8 * (r & 3))) & 0xFFu);
            const float D = (t0 + r < K) ? cost_value(lw[r] >> 16) : HUGE_COST;
            b[r] = __builtin_fmaf(kappa, (cf[0] + cf[1]) + cf[2], D);
#pragma unroll
            for (int d = 0; d < 3; ++d) cv[d][r] = __builtin_fmaf(nstep, cf[d], b[r]) * oms;
        }
        float gm = fminf(fminf(fminf(b[0], b[1]), fminf(b[2], b[3])), fminf(fminf(b[4], b[5]), fminf(b[6], b[7])));
        float cm[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) cm[d] = fminf(fminf(fminf(cv[d][0], cv[d][1]), fminf(cv[d][2], cv[d][3])), fminf(fminf(cv[d][4], cv[d][5]), fminf(cv[d][6], cv[d][7])));
        group_min_fused4<G>(gm, cm[0], cm[1], cm[2]);
        // decode: first argmin_t b[t] (the group minimum, then the smallest label attaining it)
        uint32_t bt = 0xFFFFFFFFu;
#pragma unroll
        for (int r = 7; r >= 0; --r) bt = (b[r] == gm) ? t0 + (uint32_t)r : bt;
        bt = group_min_fused<G>(bt);
#pragma unroll
        for (int d = 0; d < 3; ++d) {
#pragma unroll
            for (int r = 0; r < 8; ++r) tile[r * G + gl] = cv[d][r] - cm[d];
            const uint32_t mlo = ident[d] ? ident_lo : rw.map[d].x, mhi = ident[d] ? ident_hi : rw.map[d].y;
            uint32_t w0 = 0u, w1 = 0u;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const uint32_t s0 = (mlo >> (8 * r)) & 0xFFu, s1 = (mhi >> (8 * r)) & 0xFFu;   // slots (64 = the +inf slot: "absent at the sender")
                w0 = msg_pack_s<DAMP>(min_raw(tile[s0], lam_s), alpha, (float)((rw.old[d].x >> (8 * r)) & 0xFFu), (uint32_t)r, w0);
                w1 = msg_pack_s<DAMP>(min_raw(tile[s1], lam_s), alpha, (float)((rw.old[d].y >> (8 * r)) & 0xFFu), (uint32_t)r, w1);
            }
            if (t0 < kj3[d]) st_off<uint2>(mn, o_out[d] + t0, make_uint2(w0, w1));   // one 8-byte store: the runs are padded to 8 elements

        }
        const bool owner = node_ok && ((K > 0u) ? ((bt >> 3) == (uint32_t)gl) : (gl == 0));
        if (owner) {
            const uint32_t r = bt & 7u;
            uint32_t wsel = lw[0];
#pragma unroll
            for (int k = 1; k < 8; ++k) wsel = (r == (uint32_t)k) ? lw[k] : wsel;
            const uint32_t my_lab = (K > 0u) ? (wsel & 0xFFFFu) + 1u : 0u;
            const uint32_t my_code = (K > 0u) ? (wsel >> 16) : 65535u;
            st_off<uint32_t>(lab, 4u * cur.id, my_lab);
            acc_e += my_code;
            acc_c += (low[0] && rw.nl[0] != my_lab) + (low[1] && rw.nl[1] != my_lab) + (low[2] && rw.nl[2] != my_lab);
        }
        cur = nxt; rw = rn; nxt = nn;
    }
    unsigned long long e = acc_e, c = acc_c;
    for (int o = 32; o > 0; o >>= 1) { e += __shfl_xor(e, o, 64); c += __shfl_xor(c, o, 64); }
    if ((threadIdx.x & 63) == 0) { s_e[threadIdx.x >> 6] = e; s_e[4 + (threadIdx.x >> 6)] = c; }
    __syncthreads();
    if (threadIdx.x == 0) {
        e = s_e[0] + s_e[1] + s_e[2] + s_e[3]; c = s_e[4] + s_e[5] + s_e[6] + s_e[7];
        partial[2 * blockIdx.x] = e + 65535ull * c; partial[2 * blockIdx.x + 1] = c;
    }
}

// generic nodes: any degree, any K.  One BLOCK per node (persistent blocks striding over the range): the four waves split the
// labels for the belief vector b (which goes through a global scratch row: K is unbounded here) and then take the out-edges in
// turn, one edge per wave at a time -- a generic node is a chain of dependent gathers (edge record -> run -> map -> run), and
// with a handful of generic nodes per colour phase (one non-manifold edge, one long column) the launch lasts as long as ONE
// node's chain, so the chain is what is parallelised.  Same arithmetic as the fast kernel / the oracle; the node's share of the
// sweep's tracking energy (cost code of the decoded label + one cut per model edge to a lower-coloured neighbour whose label
// differs) goes into per-block partials like the fast kernel's.
template <bool DAMP>
__global__ void __launch_bounds__(256) mrf_sweep_generic_kernel(const uint32_t* __restrict__ col_ptr, const uint16_t* __restrict__ view_id, const float* __restrict__ cost,
                                                                const uint32_t* __restrict__ adj_ptr, const uint32_t* __restrict__ adj, const MrfEdge* __restrict__ edge,
                                                                const uint16_t* __restrict__ map, const uint32_t* __restrict__ colour,
                                                                msg_t* msg, const uint32_t* __restrict__ perm, const mvs_mrf_progress* __restrict__ st,
                                                                uint32_t* lab2, uint32_t buf_stride,
                                                                float* scratch, uint32_t node_begin, uint32_t node_end, float rho, float alpha,
                                                                unsigned long long* __restrict__ partial) {
    const msg_t* mo = msg; msg_t* mn = msg;                  // in place (one colour per launch)
    __shared__ float s_b[4]; __shared__ uint32_t s_t[4]; __shared__ uint32_t s_cuts[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (st->stopped) return;                                 // a sweep queued after the stop rule fired (see mrf_sweep4_kernel)
    const uint32_t wofs = st->w * buf_stride;
    uint32_t* lab = lab2 + wofs;
    const float lam = 1.0f / rho;
    const MsgQ mq = msg_q(lam);
    const float kappa = rho * mq.step, nstep = -mq.step, oms = (1.0f - alpha) * mq.scale, lam_s = lam * oms;
    unsigned long long acc_e = 0ull, acc_c = 0ull;           // thread 0 accumulates
    for (uint32_t q = node_begin + blockIdx.x; q < node_end; q += gridDim.x) {   // block-uniform
        const uint32_t i = perm[q];
        const uint32_t p0 = col_ptr[i], K = col_ptr[i + 1] - p0;
        if (K == 0) {   // the single label 0 with unary 1 (view_selection.cpp:50-51,70-71): cost code 65535, no model edge
            if (threadIdx.x == 0) { lab[i] = 0u; acc_e += 65535ull; }
            continue;
        }
        const uint32_t e0 = adj_ptr[i], e1 = adj_ptr[i + 1];
        float bb = INFINITY; uint32_t bt = 0xFFFFFFFFu;
        for (uint32_t t = threadIdx.x; t < K; t += 256) {
            float Sc = 0.0f;
            for (uint32_t e = e0; e < e1; ++e) { const MrfEdge m = edge[e]; if (m.kj) Sc = Sc + (float)mo[m.in_off + t]; }   // adjacency order, like the oracle
            const float b = __builtin_fmaf(kappa, Sc, cost_value(cost_code(cost[p0 + t])));   // the unaries as the sweeps see them: 16-bit fixed point
            scratch[p0 + t] = b;
            if (b < bb) { bb = b; bt = t; }
        }
        for (int o = 32; o > 0; o >>= 1) {
            const float ob = __shfl_xor(bb, o, 64); const uint32_t ot = __shfl_xor(bt, o, 64);
            if (ob < bb || (ob == bb && ot < bt)) { bb = ob; bt = ot; }
        }
        if (lane == 0) { s_b[wave] = bb; s_t[wave] = bt; }
        __syncthreads();                                     // also orders the scratch row: written above, read below by other threads of the block
#pragma unroll
        for (int w = 0; w < 4; ++w) { const float ob = s_b[w]; const uint32_t ot = s_t[w]; if (w == 0 || ob < bb || (ob == bb && ot < bt)) { bb = ob; bt = ot; } }
        const uint32_t my_lab = (uint32_t)view_id[p0 + bt] + 1u, my_code = cost_code(cost[p0 + bt]);
        // cut edges to lower-coloured neighbours (their labels of this sweep are final): one edge per thread
        {
            const uint32_t ci = colour[i];
            uint32_t cuts = 0;
            for (uint32_t e = e0 + threadIdx.x; e < e1; e += 256) {
                const uint32_t j = adj[e];
                if (edge[e].kj != 0u && colour[j] < ci && lab[j] != my_lab) ++cuts;
            }
            for (int o = 32; o > 0; o >>= 1) cuts += __shfl_xor(cuts, o, 64);
            if (lane == 0) s_cuts[wave] = cuts;
        }
        // the out-edges, one per wave at a time
        for (uint32_t e = e0 + (uint32_t)wave; e < e1; e += 4) {
            const MrfEdge m = edge[e];
            if (!m.kj) continue;  // wave-uniform
            float cmin = INFINITY;
            for (uint32_t t = lane; t < K; t += 64) cmin = fminf(cmin, __builtin_fmaf(nstep, (float)mo[m.in_off + t], scratch[p0 + t]) * oms);
            for (int o = 32; o > 0; o >>= 1) cmin = fminf(cmin, __shfl_xor(cmin, o, 64));
            for (uint32_t t2 = lane; t2 < m.kj; t2 += 64) {
                const uint16_t p = map[m.out_off + t2];
                const float raw = (p == MAP_NONE) ? lam_s : fminf(__builtin_fmaf(nstep, (float)mo[m.in_off + p], scratch[p0 + p]) * oms - cmin, lam_s);
                mn[m.out_off + t2] = (msg_t)msg_pack_s<DAMP>(raw, alpha, (float)mo[m.out_off + t2], 0u, 0u);
            }
        }
        __syncthreads();                                     // s_cuts complete; s_b / s_t free for the next node
        if (threadIdx.x == 0) {
            lab[i] = my_lab;   // (position and unary of the label: derived after the sweeps, see mrf_sweep4_kernel)
            acc_e += my_code; acc_c += (unsigned long long)s_cuts[0] + s_cuts[1] + s_cuts[2] + s_cuts[3];
        }
    }
    if (threadIdx.x == 0) { partial[2 * blockIdx.x] = acc_e + 65535ull * acc_c; partial[2 * blockIdx.x + 1] = acc_c; }
}

}  // namespace

// Damping schedule (part of the solver's definition, restated in oracle/oracle.cpp): messages are damped with
// alpha = params.damping on ODD sweeps (1st, 3rd, ...) and written undamped on even sweeps.  Undamped sweeps oscillate
// (C3: 0.9 % higher final energy), but damping every second sweep suppresses that just as well as damping every sweep
// (C3: 44 sweeps to E = 1 111 890 with 0.2 on odd sweeps vs 47 to 1 110 970 with 0.1 on all) -- and an undamped sweep
// does not re-read its previous outgoing messages.
// Round 6 re-scored the schedule in milliseconds (scripts/schedule_score.py, retired after commit 1bd22ac; profiles/r06_schedule_score_*.json):
// an undamped launch is 14 % cheaper than a damped one, and damping every FOURTH sweep (1st, 5th, ...) holds the oscillation as well:
// the definition is period 4 (MRF_DAMP_PERIOD).
static float sweep_alpha(const mvs_ctx* ctx) {
    return ctx->m_sweep_no % MRF_DAMP_PERIOD == 1u ? ctx->m_params.damping : 0.0f;
}

// the fast sweep kernels' signature; k[DAMP][XCD] are a kernel's four instantiations
using FastSweep = void (*)(const NodeDesc*, const uint32_t*, msg_t*, const mvs_mrf_progress*, uint32_t*, uint32_t, uint32_t, uint32_t, float, float, unsigned long long*);
// one launch of a fast kernel (npb nodes per block) over positions [qb, qe) (one (colour, class) range of the schedule order); its per-block
// energy partials go to slots [slot, slot + blocks) of the phase's region.  Returns the number of blocks (= slots) used.
// Persistent lane groups: at most as many blocks as are resident at once (a partial second wave of blocks would double the tail);
// mrf_blocks_per_cu > 0 overrides.  `resident_once` caches the resident count of k[1][1] (the same value on every device of a node;
// in-process ranks race for it: atomic, idempotent).
static unsigned launch_fast(mvs_ctx* ctx, const FastSweep (&k)[2][2], unsigned npb, std::atomic<int>& resident_once,
                            uint32_t phase, uint32_t qb, uint32_t qe, unsigned slot, unsigned slot_cap) {
    const unsigned need = (qe - qb + npb - 1) / npb;
    const float alpha = sweep_alpha(ctx);
    int resident = resident_once.load(std::memory_order_relaxed);
    if (resident == 0) {
        int per_cu = 0; hipDeviceProp_t prop;
        MVS_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k[1][1], 256, 0));
        MVS_HIP(hipGetDeviceProperties(&prop, ctx->device));
        resident = std::max(1, per_cu) * prop.multiProcessorCount;
        resident_once.store(resident, std::memory_order_relaxed);
    }
    unsigned blocks = ctx->mrf_blocks_per_cu > 0 ? 256u * (unsigned)ctx->mrf_blocks_per_cu : (unsigned)resident;
    blocks = std::max(1u, std::min(std::min(need, blocks), slot_cap));
    if (blocks > 8) blocks &= ~7u;   // multiple of the 8 XCDs
    msg_t* msg = reinterpret_cast<msg_t*>(ctx->m_msg_a.p);
    unsigned long long* partial = ctx->m_energy.p + 4 + 2 * ((size_t)EPART_BLOCKS * phase + slot);
    hipLaunchKernelGGL(k[alpha != 0.0f][ctx->mrf_xcd != 0], dim3(blocks), dim3(256), 0, ctx->stream, ctx->m_desc.p, ctx->m_rec.p, msg, ctx->m_state.p,
                       ctx->m_lab.p, ctx->m_stride, qb, qe, ctx->m_params.rho, alpha, partial);
    MVS_LAUNCH_CHECK();
    return blocks;
}
template <int G>
static unsigned launch_sweep4_g(mvs_ctx* ctx, uint32_t phase, uint32_t qb, uint32_t qe, unsigned slot, unsigned slot_cap) {
    static const FastSweep k[2][2] = {{mrf_sweep4_kernel<G, false, false>, mrf_sweep4_kernel<G, false, true>}, {mrf_sweep4_kernel<G, true, false>, mrf_sweep4_kernel<G, true, true>}};
    static std::atomic<int> resident{0};
    return launch_fast(ctx, k, 256 / G, resident, phase, qb, qe, slot, slot_cap);
}
// class 1 through mrf_sweep8_kernel: 8 lanes per node, 32 nodes per block
static unsigned launch_sweep8(mvs_ctx* ctx, uint32_t phase, uint32_t qb, uint32_t qe, unsigned slot, unsigned slot_cap) {
    static const FastSweep k[2][2] = {{mrf_sweep8_kernel<false, false>, mrf_sweep8_kernel<false, true>}, {mrf_sweep8_kernel<true, false>, mrf_sweep8_kernel<true, true>}};
    static std::atomic<int> resident{0};
    return launch_fast(ctx, k, 256 / 8, resident, phase, qb, qe, slot, slot_cap);
}
static unsigned launch_sweep_generic(mvs_ctx* ctx, uint32_t phase, uint32_t qb, uint32_t qe, unsigned slot, unsigned slot_cap) {
    const unsigned need = qe - qb;   // one block per node
    const unsigned blocks = std::max(1u, std::min(std::min(need, 256u * 4u), slot_cap));
    const float rho = ctx->m_params.rho, alpha = sweep_alpha(ctx);
    msg_t* msg = reinterpret_cast<msg_t*>(ctx->m_msg_a.p);
    unsigned long long* partial = ctx->m_energy.p + 4 + 2 * ((size_t)EPART_BLOCKS * phase + slot);
    hipLaunchKernelGGL(alpha != 0.0f ? mrf_sweep_generic_kernel<true> : mrf_sweep_generic_kernel<false>, dim3(blocks), dim3(256), 0, ctx->stream,
                       ctx->r_ptr, ctx->r_view, ctx->r_cost, ctx->r_adj_ptr, ctx->r_adj, ctx->m_edge.p, ctx->m_map.p, ctx->m_colour.p, msg, ctx->m_perm.p,
                       ctx->m_state.p, ctx->m_lab.p, ctx->m_stride, ctx->pq.p, qb, qe, rho, alpha, partial);
    MVS_LAUNCH_CHECK();
    return blocks;
}

// positions [qb, qe) in the schedule order of the nodes of (sub-class `sub`, zone) whose id lies in [nb0, ne0)
static void sub_range(mvs_ctx* ctx, uint32_t sub, uint32_t zone, uint32_t nb0, uint32_t ne0, uint32_t* qb, uint32_t* qe) {
    const uint32_t key = 2u * sub + zone;
    const uint32_t cb = ctx->m_sub_begin[key], ce = ctx->m_sub_begin[key + 1];
    if (ce <= cb || (nb0 == 0 && ne0 >= ctx->csr_faces)) { *qb = cb; *qe = ce; return; }
    if (ctx->m_range_nb != nb0 || ctx->m_range_ne != ne0 || ctx->m_range_q.size() != 2 * (size_t)N_KEY) {
        // a rank's own share of every (sub-class, zone): one small kernel + read-back per (range, setup), then cached
        uint32_t* d = ctx->m_sub.p + N_KEY + 2;   // (allocated by mrf_setup: ensure() here would drop sub_begin)
        hipLaunchKernelGGL(mrf_sub_range_kernel, dim3((N_KEY + 255) / 256), dim3(256), 0, ctx->stream, ctx->m_perm.p, ctx->m_sub.p, nb0, ne0, d);
        MVS_LAUNCH_CHECK();
        ctx->m_range_q.assign(2 * (size_t)N_KEY, 0);
        MVS_HIP(hipMemcpyAsync(ctx->m_range_q.data(), d, 2 * N_KEY * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
        MVS_HIP(hipStreamSynchronize(ctx->stream));
        ctx->m_range_nb = nb0; ctx->m_range_ne = ne0;
    }
    *qb = ctx->m_range_q[2 * key]; *qe = ctx->m_range_q[2 * key + 1];
}

// one colour phase of a sweep over the nodes of that colour with id in [nb0, ne0): in place.  Up to five launches per zone, one per node
// class present in the colour (a uniform mesh has one); their energy partials share the phase's EPART_BLOCKS slots: the boundary zone's
// launches take slots [0, EPART_BOUNDARY), the interior's the rest (a slot nobody writes stays zero; the geometry of a phase's launches
// is the same in every sweep, so every slot that is ever written is rewritten by every sweep).
// part: MRF_PART_ALL = both zones, slots from 0 (one launch where the zones are adjacent in the schedule),
//       MRF_PART_BOUNDARY / MRF_PART_INTERIOR = one zone -- a sharded caller runs BOUNDARY, hands over, then INTERIOR.
// A solve keeps to one of the two modes (the slots of a launch differ between them).
void mrf_sweep_phase(mvs_ctx* ctx, uint32_t phase, uint32_t nb0, uint32_t ne0, int part) {
    // A sweep starts when the phase number falls back (or with the first call after the set-up).  Callers run the phases in ascending
    // order, a split phase boundary first; consecutive calls of one phase -- a phase cut into several node ranges -- belong to one sweep.
    // A graph of one colour has no edge, hence no message a damping factor could reach: there every call counts.
    if (part != MRF_PART_INTERIOR && (phase < ctx->m_last_phase || ctx->m_last_phase == 0xFFFFFFFFu || ctx->m_colours <= 1u)) ++ctx->m_sweep_no;
    ctx->m_last_phase = phase;
    if (phase >= ctx->m_colours || ne0 <= nb0) return;
    constexpr unsigned EPART_BOUNDARY = 256;
    struct Launch { uint32_t g, qb, qe; } L[10]; int n = 0;
    for (uint32_t g = 0; g < 5; ++g) {
        const uint32_t sub = g < 4 ? 4 * phase + g : SUB_GENERIC + phase;
        uint32_t b0 = 0, b1 = 0, i0 = 0, i1 = 0;
        if (part != MRF_PART_INTERIOR) sub_range(ctx, sub, 0, nb0, ne0, &b0, &b1);
        if (part != MRF_PART_BOUNDARY) sub_range(ctx, sub, 1, nb0, ne0, &i0, &i1);
        if (b1 > b0 && i1 > i0 && b1 == i0) { L[n++] = {g, b0, i1}; continue; }   // both zones, adjacent in the schedule (a single context's marks): one launch
        if (b1 > b0) L[n++] = {g, b0, b1};
        if (i1 > i0) L[n++] = {g, i0, i1};
    }
    unsigned slot = part == MRF_PART_INTERIOR ? EPART_BOUNDARY : 0u;
    const unsigned slot_end = part == MRF_PART_BOUNDARY ? EPART_BOUNDARY : EPART_BLOCKS;
    for (int k = 0; k < n; ++k) {
        const unsigned cap = slot_end - slot - (unsigned)(n - 1 - k);   // leaves at least one slot for every launch still to come
        const uint32_t qb = L[k].qb, qe = L[k].qe;
        switch (L[k].g) {
            case 0: slot += launch_sweep4_g<8>(ctx, phase, qb, qe, slot, cap); break;
            case 1: slot += launch_sweep8(ctx, phase, qb, qe, slot, cap); break;
            case 2: slot += launch_sweep4_g<32>(ctx, phase, qb, qe, slot, cap); break;
            case 3: slot += launch_sweep4_g<64>(ctx, phase, qb, qe, slot, cap); break;      // one node per wave: several hundred views per face
            default: slot += launch_sweep_generic(ctx, phase, qb, qe, slot, cap);
        }
    }
}
// one sweep = every colour phase in turn (callers that shard the nodes exchange halos between the phases themselves)
void mrf_sweep(mvs_ctx* ctx, uint32_t nb0, uint32_t ne0) {
    for (uint32_t ph = 0; ph < ctx->m_colours; ++ph) mrf_sweep_phase(ctx, ph, nb0, ne0, MRF_PART_ALL);
    // the sweep kernels leave the sweep's energy behind as per-block partials (valid when the range is the whole graph)
    ctx->m_energy_from_sweep = nb0 == 0 && ne0 >= ctx->csr_faces && ctx->m_colours > 0;
}

}  // namespace mvs
