// k_mrf_polish.hip -- tex::view_selection on the GPU, part 3 of 3 (k_mrf_setup.hip has the overview): everything that works on a labeling
// after a sweep -- the energies (tracking and exact), the device-side stop rule and its reports, "keep the best labeling", the exact
// costs of the best labeling, the monotone ICM polish, and the labels on their way out.
#include "mrf.h"

namespace mvs {

namespace {

__device__ __forceinline__ unsigned long long fix32(float d) { return (unsigned long long)((double)d * 4294967296.0); }
// position of label `l` (> 0: view id l - 1) in the ascending view list of a column (calculate_data_costs.cpp:272); a labeling only ever
// holds labels of the node's own column, so the search finds it
__device__ __forceinline__ uint32_t label_position(const uint16_t* __restrict__ view_id, uint32_t p0, uint32_t K, uint32_t l) {
    uint32_t lo = 0, hi = K;
    const uint32_t key = l - 1u;
    while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if ((uint32_t)view_id[p0 + mid] < key) lo = mid + 1; else hi = mid; }
    return lo < K ? lo : K - 1u;
}

// ---- exact energy of a labeling (32.32 fixed point) over nodes [node_begin, node_end) ----
// needs only the labels and selected unary costs: an edge is in the model iff both labels are
// non-zero (both columns non-empty, view_selection.cpp:29-42)
__global__ void __launch_bounds__(256) mrf_energy_kernel(const uint32_t* __restrict__ col_ptr, const uint16_t* __restrict__ view_id, const float* __restrict__ cost,
                                                         const uint32_t* __restrict__ adj_ptr, const uint32_t* __restrict__ adj,
                                                         const uint32_t* __restrict__ lab, const float* __restrict__ selcost,
                                                         const mvs_mrf_progress* __restrict__ st /* non-null: the decode buffer st->w of lab / selcost */, uint32_t buf_stride,
                                                         uint32_t node_begin, uint32_t node_end, unsigned long long* __restrict__ out /* [0] energy, [1] cuts */) {
    // st != null: the TRACKING energy of the current decode (its unaries are dequantised 16-bit codes: integer units of
    // 1 / 65535, 65535 per cut edge); else the exact 32.32 fixed-point energy of the labeling given
    // (the sweeps keep only labels: the tracking energy looks the label's unary up in the table -- the 16-bit code the records hold)
    if (st) { const uint32_t wofs = st->w * buf_stride; lab += wofs; }
    unsigned long long unary = 0, cuts = 0;
    for (uint32_t i = node_begin + blockIdx.x * blockDim.x + threadIdx.x; i < node_end; i += gridDim.x * blockDim.x) {
        const uint32_t li = lab[i];
        if (st) { const uint32_t p0 = col_ptr[i], K = col_ptr[i + 1] - p0; unary += (K && li) ? (unsigned long long)cost_code(cost[p0 + label_position(view_id, p0, K, li)]) : 65535ull; }
        else unary += fix32(selcost[i]);
        if (li == 0u) continue;
        for (uint32_t e = adj_ptr[i]; e < adj_ptr[i + 1]; ++e) {
            const uint32_t j = adj[e];
            if (j <= i) continue;                          /* :38 uni directional */
            const uint32_t lj = lab[j];
            cuts += (lj != 0u && lj != li);
        }
    }
    // no atomics (same-address atomics serialise at ~12 ns each): one partial pair per block, summed by
    // mrf_energy_reduce_kernel; integer sums, so the result does not depend on the launch geometry
    __shared__ unsigned long long su[4], sc[4];
    for (int o = 32; o > 0; o >>= 1) { unary += __shfl_xor(unary, o, 64); cuts += __shfl_xor(cuts, o, 64); }
    if ((threadIdx.x & 63) == 0) { su[threadIdx.x >> 6] = unary; sc[threadIdx.x >> 6] = cuts; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned long long u = su[0] + su[1] + su[2] + su[3], c = sc[0] + sc[1] + sc[2] + sc[3];
        out[2 * blockIdx.x] = st ? u + 65535ull * c : u + (c << 32); out[2 * blockIdx.x + 1] = c;
    }
}
__global__ void __launch_bounds__(1024) mrf_energy_reduce_kernel(const unsigned long long* __restrict__ partial, uint32_t n_blocks,
                                                                 unsigned long long* __restrict__ out /* [0] energy, [1] cuts */,
                                                                 unsigned long long* __restrict__ out2 = nullptr /* a second copy (sharded solves: the slot the peers read) */) {
    unsigned long long e = 0, c = 0;
    const ulonglong2* pp = reinterpret_cast<const ulonglong2*>(partial);
#pragma unroll 8
    for (uint32_t b = threadIdx.x; b < n_blocks; b += 1024u) { const ulonglong2 v = pp[b]; e += v.x; c += v.y; }
    __shared__ unsigned long long su[16], sc[16];
    for (int o = 32; o > 0; o >>= 1) { e += __shfl_xor(e, o, 64); c += __shfl_xor(c, o, 64); }
    if ((threadIdx.x & 63) == 0) { su[threadIdx.x >> 6] = e; sc[threadIdx.x >> 6] = c; }
    __syncthreads();
    if (threadIdx.x == 0) { e = 0; c = 0; for (int k = 0; k < 16; ++k) { e += su[k]; c += sc[k]; } out[0] = e; out[1] = c; if (out2) { out2[0] = e; out2[1] = c; } }
}

// ---- ICM polish: G lanes per node over its labels ----
template <int G>
__global__ void __launch_bounds__(256) mrf_icm_gain_kernel(const uint32_t* __restrict__ col_ptr, const uint16_t* __restrict__ view_id, const float* __restrict__ cost,
                                                           const uint32_t* __restrict__ adj_ptr, const uint32_t* __restrict__ adj,
                                                           const uint32_t* __restrict__ sel, const uint32_t* __restrict__ lab,
                                                           uint32_t node_begin, uint32_t node_end, float* __restrict__ gain, uint32_t* __restrict__ cand,
                                                           const uint32_t* __restrict__ list /* null: nodes [node_begin, node_end); else node ids list[node_begin .. node_end) */,
                                                           const uint32_t* __restrict__ list_count /* non-null: node_end = node_begin + *list_count */) {
    constexpr int NPB = 256 / G;
    const int grp = threadIdx.x / G, gl = threadIdx.x % G;
    if (list_count) node_end = node_begin + *list_count;   // the active list's length stays on the device: no read-back between the ICM rounds
    for (uint32_t pos = node_begin + blockIdx.x * NPB + grp; pos < node_end; pos += gridDim.x * NPB) {   // trip counts are uniform within a lane group
        const uint32_t i = list ? list[pos] : pos;
        const uint32_t p0 = col_ptr[i];
        const uint32_t K = col_ptr[i + 1] - p0;
        const uint32_t e0 = adj_ptr[i], e1 = adj_ptr[i + 1];
        const uint32_t cur_l = (K > 0) ? lab[i] : 0u;   // the node's current label (labels of a column are distinct: it names one position)
        float best = INFINITY, cur = 0.0f; uint32_t bt = 0xFFFFFFFFu;
        // neighbour labels: the first three once (the manifold case), any further ones inside the loop
        uint32_t nl[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) nl[d] = (K > 0 && e0 + d < e1) ? lab[adj[e0 + d]] : 0u;
        for (uint32_t t = gl; t < K; t += G) {
            const uint32_t l = (uint32_t)view_id[p0 + t] + 1u;
            uint32_t diff = (nl[0] != 0u && nl[0] != l) + (nl[1] != 0u && nl[1] != l) + (nl[2] != 0u && nl[2] != l);
            for (uint32_t e = e0 + 3; e < e1; ++e) { const uint32_t lj = lab[adj[e]]; diff += (lj != 0u && lj != l); }
            const float en = cost[p0 + t] + (float)diff;
            if (en < best) { best = en; bt = t; }
            if (l == cur_l) cur = en;
        }
#pragma unroll
        for (int o = G / 2; o > 0; o >>= 1) {
            const float ob = __shfl_xor(best, o, G); const uint32_t ot = __shfl_xor(bt, o, G);
            if (ob < best || (ob == best && ot < bt)) { best = ob; bt = ot; }
            cur += __shfl_xor(cur, o, G);   // exactly one lane holds a non-zero term (or none: 0)
        }
        if (gl == 0) { gain[i] = (K > 0) ? (cur - best) : 0.0f; cand[i] = (K > 0) ? bt : 0u; }
    }
}

// fast path (degree <= 3): persistent lane groups over the node descriptors, next descriptor prefetched
template <int G>
__global__ void __launch_bounds__(256) mrf_icm_gain_desc_kernel(const NodeDesc* __restrict__ desc, const uint32_t* __restrict__ col_ptr, const uint16_t* __restrict__ view_id, const float* __restrict__ cost,
                                                                const uint32_t* __restrict__ sel, const uint32_t* __restrict__ lab,
                                                                uint32_t node_begin, uint32_t node_end, float* __restrict__ gain, uint32_t* __restrict__ cand) {
    // node_begin / node_end are positions in the descriptor array ((colour, id) order); the node itself is cur.id
    constexpr int NPB = 256 / G;
    const int grp = threadIdx.x / G, gl = threadIdx.x % G;
    const uint32_t stride = gridDim.x * NPB;
    uint32_t i = node_begin + blockIdx.x * NPB + grp;
    NodeDesc nd = {};
    if (i < node_end) nd = desc[i];
    const uint32_t n_iter = (node_end - node_begin + stride - 1) / stride;
    for (uint32_t it = 0; it < n_iter; ++it, i += stride) {
        const bool node_ok = i < node_end;
        const NodeDesc cur = nd;
        if (i + stride < node_end) nd = desc[i + stride];
        const uint32_t K = node_ok ? (cur.kk & 0xFFu) : 0u;
        const uint32_t id = cur.id;
        const uint32_t p0 = (K > 0) ? col_ptr[id] : 0u;
        const uint32_t cur_l = (K > 0) ? lab[id] : 0u;
        uint32_t nl[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) nl[d] = (K > 0 && ((cur.kk >> (8 + 8 * d)) & 0xFFu)) ? lab[cur.nbr[d]] : 0u;
        float best = INFINITY, cur_e = 0.0f; uint32_t bt = 0xFFFFFFFFu;
        for (uint32_t t = gl; t < K; t += G) {
            const uint32_t l = (uint32_t)view_id[p0 + t] + 1u;
            const uint32_t diff = (nl[0] != 0u && nl[0] != l) + (nl[1] != 0u && nl[1] != l) + (nl[2] != 0u && nl[2] != l);
            const float en = cost[p0 + t] + (float)diff;
            if (en < best) { best = en; bt = t; }
            if (l == cur_l) cur_e = en;
        }
#pragma unroll
        for (int o = G / 2; o > 0; o >>= 1) {
            const float ob = __shfl_xor(best, o, G); const uint32_t ot = __shfl_xor(bt, o, G);
            if (ob < best || (ob == best && ot < bt)) { best = ob; bt = ot; }
            cur_e += __shfl_xor(cur_e, o, G);   // exactly one lane holds a non-zero term (or none: 0)
        }
        if (gl == 0 && node_ok) { gain[id] = (K > 0) ? (cur_e - best) : 0.0f; cand[id] = (K > 0) ? bt : 0u; }
    }
}

__global__ void __launch_bounds__(256) mrf_icm_apply_kernel(const uint32_t* __restrict__ col_ptr, const uint16_t* __restrict__ view_id, const float* __restrict__ cost,
                                                            const uint32_t* __restrict__ adj_ptr, const uint32_t* __restrict__ adj,
                                                            const float* __restrict__ gain, const uint32_t* __restrict__ cand,
                                                            uint32_t* sel, uint32_t* lab, float* selcost,
                                                            uint32_t node_begin, uint32_t node_end, uint32_t* __restrict__ moved /* [0] nodes moved, [1] list length */,
                                                            uint32_t* __restrict__ alist /* null, or: nodes whose gain has to be re-evaluated */,
                                                            const uint32_t* __restrict__ orig /* null: identity; ties between equal gains go to the smaller id of the CALLER's numbering */) {
    const uint32_t i = node_begin + blockIdx.x * blockDim.x + threadIdx.x;
    bool mv = false;
    if (i < node_end) {
        const float gi = gain[i];
        if (gi > 0.0f) {   // only nodes with a non-empty column have a positive gain
            bool win = true;
            for (uint32_t e = adj_ptr[i]; e < adj_ptr[i + 1] && win; ++e) {
                const uint32_t j = adj[e];
                if (lab[j] == 0u) continue;               // edge not in the model (gain[j] is 0 anyway)
                const float gj = gain[j];
                if (gj > gi || (gj == gi && (orig ? orig[j] < orig[i] : j < i))) win = false;
            }
            if (win) mv = true;
        }
    }
    // all reads of neighbours' labels happen before any write: a winner's neighbours never win in the same
    // iteration (independent set), and lab[j] == 0 never changes
    if (mv) {
        const uint32_t p0 = col_ptr[i], t = cand[i];
        sel[i] = t; lab[i] = (uint32_t)view_id[p0 + t] + 1u; selcost[i] = cost[p0 + t];
        if (alist) {   // a node's gain depends on its column, its own label and its neighbours' labels only (duplicates in the list are harmless)
            const uint32_t e0 = adj_ptr[i], e1 = adj_ptr[i + 1];
            uint32_t w = atomicAdd(&moved[1], 1u + (e1 - e0));
            alist[w++] = i;
            for (uint32_t e = e0; e < e1; ++e) alist[w++] = adj[e];
        }
    }
    const unsigned long long b = __ballot(mv);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(moved, (uint32_t)__popcll(b));
}

/* label extraction (view_selection.cpp:120-132): labels are already decoded; range check + unseen count */
__global__ void mrf_labels_kernel(const uint32_t* __restrict__ lab, uint32_t node_begin, uint32_t node_end, uint32_t n_views,
                                  uint32_t* __restrict__ labels, uint32_t* __restrict__ bad_unseen /* [0] bad, [1] unseen */,
                                  const uint32_t* __restrict__ orig /* non-null: labels[orig[i]] = label of node i (the caller's numbering) */,
                                  const uint32_t* __restrict__ foreign /* may be null: labels outside their column, counted by mrf_exact_cost_kernel over the same range */) {
    const uint32_t i = node_begin + blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= node_end) return;
    if (foreign && i == node_begin && *foreign) atomicAdd(&bad_unseen[0], *foreign);
    const uint32_t label = lab[i];
    if (label > n_views) atomicAdd(&bad_unseen[0], 1u);       /* :126-128 "Incorrect labeling" */
    if (label == 0u) atomicAdd(&bad_unseen[1], 1u);            /* :129 */
    labels[orig ? orig[i] : i - node_begin] = label;
}


// ---- device-side solver bookkeeping: one block.  Same decisions, in the same arithmetic, as the host loop it
// replaces: best = min(best, e); stop iff sweep >= min_sweeps, sweep > window and
// double(hist[sweep - window] - best) < double(min_improvement) * double(hist[sweep - window]).
// With `partial` (single-GPU loop) the block first sums the per-block energy pairs the sweep kernels (fast path) or the
// energy kernel left behind and publishes them in energy_out; sharded callers pass the all-reduced pair in `energy`.
// "Keep the best labeling" is a flip of two indices: the sweep that improved the best energy wrote decode buffer w, which
// becomes best_w, and the next sweeps write the other buffer -- nothing is copied.  The report goes straight into the
// pinned ring slot (host memory), so a step is ONE launch.
// The step's number (which ring slot its report goes to, which sequence number announces it) is device state too -- ctl[0] counts
// the steps of the solve, ctl[1] is the solve's sequence base -- so a step's launch has the SAME arguments every time and the
// sweep loop can be replayed from a hipGraph.
__global__ void __launch_bounds__(1024) mrf_step_kernel(mvs_mrf_progress* __restrict__ st, unsigned long long* __restrict__ hist,
                                const unsigned long long* __restrict__ energy, const unsigned long long* __restrict__ partial, uint32_t n_partial,
                                unsigned long long* __restrict__ energy_out, mvs_mrf_progress* __restrict__ ring, uint32_t* __restrict__ ring_seq, uint32_t ring_slots,
                                uint32_t* __restrict__ ctl, int max_sweeps, int min_sweeps, int window, float min_improvement,
                                const unsigned long long* const* __restrict__ peer_tab = nullptr, uint32_t n_peer = 0, uint32_t peer_off = 0) {
    // peer_tab (sharded solves, peer-push transport): the energy pair of the sweep = the sum over the ranks' published pairs
    // peer_tab[q][peer_off], [peer_off + 1] -- read here, so that summing them is no launch of its own
    __shared__ unsigned long long su[16], sc[16];
    unsigned long long e_sum = 0, c_sum = 0;
    if (partial) {
        // up to 8192 pairs: 1024 threads, the loads of a thread independent of each other (a serial 256-thread loop was
        // a chain of 32 dependent round trips: 15 us per sweep)
        const ulonglong2* pp = reinterpret_cast<const ulonglong2*>(partial);
#pragma unroll 8
        for (uint32_t b = threadIdx.x; b < n_partial; b += 1024u) { const ulonglong2 v = pp[b]; e_sum += v.x; c_sum += v.y; }
        for (int o = 32; o > 0; o >>= 1) { e_sum += __shfl_xor(e_sum, o, 64); c_sum += __shfl_xor(c_sum, o, 64); }
        if ((threadIdx.x & 63) == 0) { su[threadIdx.x >> 6] = e_sum; sc[threadIdx.x >> 6] = c_sum; }
        __syncthreads();
    }
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (partial) {
        e_sum = 0; c_sum = 0;
        for (int k = 0; k < 16; ++k) { e_sum += su[k]; c_sum += sc[k]; }
        energy_out[0] = e_sum; energy_out[1] = c_sum;
    } else if (peer_tab) {
        e_sum = 0; c_sum = 0;
        for (uint32_t q = 0; q < n_peer; ++q) { e_sum += peer_tab[q][peer_off]; c_sum += peer_tab[q][peer_off + 1u]; }
        energy_out[0] = e_sum; energy_out[1] = c_sum;
    }
    mvs_mrf_progress p = *st;
    if (p.stopped) { p.improved = 0u; }
    else {
        const uint32_t sw = p.sweep + 1u;
        const unsigned long long e0 = (partial || peer_tab) ? e_sum : energy[0];
        const bool imp = e0 < p.best;
        if (imp) { p.best = e0; p.best_w = p.w; p.w ^= 1u; }
        p.sweep = sw; p.improved = imp ? 1u : 0u; p.energy = e0;
        hist[sw] = p.best;
        bool stop = false;
        if ((int)sw >= min_sweeps && (int)sw > window) {
            const unsigned long long prev = hist[sw - (uint32_t)window];
            stop = (double)(prev - p.best) < (double)min_improvement * (double)prev;
        }
        if ((int)sw >= max_sweeps) stop = true;
        if (stop) { p.stopped = 1u; p.stop_sweep = sw; }
    }
    *st = p;
    const uint32_t n = ctl[0] + 1u; ctl[0] = n;
    if (ring) {   // pinned host memory: the report, a system-scope fence, then its sequence number -- the host polls the number
        const uint32_t slot = n % ring_slots;
        ring[slot] = p;
        __threadfence_system();
        __hip_atomic_store(ring_seq + slot, ctl[1] + n, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}
// best labeling := the current decode buffer (mvs_ctx_mrf_keep_best): the same index flip, unconditionally
__global__ void mrf_flip_kernel(mvs_mrf_progress* __restrict__ st) { st->best_w = st->w; st->w ^= 1u; }

}  // namespace

// the best labeling's buffer, once the host needs it (ICM, final energy, labels): one read-back of the solver state
void resolve_best(mvs_ctx* ctx) {
    if (ctx->best_resolved) return;
    if (!ctx->m_state.p) throw StatusError(MVS_ERR_STATE, "mrf setup first");
    mvs_mrf_progress p;
    static_assert(sizeof(p) % 4 == 0 && sizeof(p) <= 64, "mvs_mrf_progress travels through read_words");
    read_words(ctx, ctx->m_state.p, &p, (uint32_t)(sizeof(p) / 4));
    const size_t o = (size_t)(p.best_w & 1u) * ctx->m_stride;
    ctx->b_sel = ctx->m_sel.p + o; ctx->b_lab = ctx->m_lab.p + o; ctx->b_cost = ctx->m_cost.p + o;
    ctx->best_resolved = true;
}

// One bookkeeping step (see mrf_step_kernel); energy = device pointer to the (all-reduced) energy pair, or null: the pair is
// still in per-block partials -- the sweep kernels' (fast path) or mrf_energy(..., reduce = false)'s -- summed by the step kernel.
void mrf_step(mvs_ctx* ctx, const unsigned long long* energy, const unsigned long long* const* peer_tab, uint32_t n_peer, uint32_t peer_off) {
    hipStream_t s = ctx->stream;
    const mvs_mrf_params& P = ctx->m_params;
    if (!ctx->h_ring) throw StatusError(MVS_ERR_STATE, "mrf step before mrf setup");
    ++ctx->steps_issued;   // the kernel derives the ring slot and the sequence number from its own step counter (ctl), which mirrors this one
    const unsigned long long* partial = nullptr; uint32_t n_partial = 0;
    if (!energy && !peer_tab) { partial = ctx->m_energy.p + 4; n_partial = ctx->m_energy_from_sweep ? EPART_BLOCKS * std::max<uint32_t>(ctx->m_colours, 1u) : ctx->m_energy_blocks; }
    hipLaunchKernelGGL(mrf_step_kernel, dim3(1), dim3(1024), 0, s, ctx->m_state.p, ctx->m_hist.p, energy, partial, n_partial, ctx->m_energy.p,
                       ctx->d_ring, ctx->d_seq, (uint32_t)mvs_ctx::RING, ctx->m_ctl.p, P.max_sweeps, P.min_sweeps, P.window, P.min_improvement, peer_tab, n_peer, peer_off);
    MVS_LAUNCH_CHECK();
    best_labeling_may_have_changed(ctx);
}
void mrf_poll(mvs_ctx* ctx, uint32_t step, mvs_mrf_progress* out) {
    if (step == 0 || step > ctx->steps_issued || step + mvs_ctx::RING <= ctx->steps_issued)
        throw StatusError(MVS_ERR_INVALID, "mrf poll: step not among the last 16 issued");
    const uint32_t slot = step % mvs_ctx::RING;
    wait_report(ctx, slot, ctx->seq_base + step);
    *out = ctx->h_ring[slot];
}

// The "moved" counts come back through the pinned ring of ICM_RING slots, LAG rounds late: the host queues round k + LAG before it reads
// round k's count, so the GPU never idles on a round trip; a round queued after the one that moved nothing changes nothing.
int icm_rounds(mvs_ctx* ctx, int max_rounds, const uint32_t* d_moved, const std::function<void(int)>& round) {
    constexpr int R = (int)mvs_ctx::ICM_RING, LAG = 2;
    ensure_report_ring(ctx);
    int issued = 0, polled = 0, stop = -1;
    const uint32_t seq0 = ctx->icm_seq;
    auto poll = [&]() { const int k = polled++; wait_report(ctx, mvs_ctx::RING + (uint32_t)(k % R), seq0 + (uint32_t)k + 1u); if (stop < 0 && ctx->h_icm[k % R] == 0u) stop = k; };
    ProfChain pc(ctx);
    while (issued < max_rounds && stop < 0) {
        pc.begin();
        round(issued);
        report_u32(ctx, d_moved, ctx->d_icm + issued % R, mvs_ctx::RING + (uint32_t)(issued % R), seq0 + (uint32_t)issued + 1u);
        pc.mark("mrf_icm");
        ++issued;
        if (issued - polled > LAG) poll();
    }
    while (polled < issued) poll();
    ctx->icm_seq = seq0 + (uint32_t)issued;
    return stop >= 0 ? stop : max_rounds;
}

// The solver tracks energies of the 16-bit unaries the sweeps see; the polish and everything reported use the exact costs:
// best_cost[i] := cost[col_ptr[i] + best_sel[i]] (1.0 for an empty column)
// The sweeps keep ONE word per node, its label.  Whatever works on the best labeling afterwards (polish, region moves, reported energy)
// needs the label's position in the column and its EXACT unary as well: derived here, once, from the label (idempotent).
__global__ void mrf_exact_cost_kernel(const uint32_t* __restrict__ col_ptr, const uint16_t* __restrict__ view_id, const float* __restrict__ cost,
                                      const uint32_t* __restrict__ lab, uint32_t node_begin, uint32_t node_end, uint32_t* __restrict__ sel, float* __restrict__ selcost,
                                      uint32_t* __restrict__ foreign /* labels that are NOT entries of their node's column (counted into "Incorrect labeling") */) {
    const uint32_t i = node_begin + blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= node_end) return;
    const uint32_t p0 = col_ptr[i], K = col_ptr[i + 1] - p0, l = lab[i];
    const uint32_t t = (K && l) ? label_position(view_id, p0, K, l) : 0u;
    // label_position clamps: a stale or foreign label (a scatter through the building blocks, a table pruned behind the labeling) would
    // silently take a neighbour's position and unary -- it is counted instead
    if ((K != 0u) != (l != 0u) || (K && l && (uint32_t)view_id[p0 + t] + 1u != l)) atomicAdd(foreign, 1u);
    sel[i] = t;
    selcost[i] = K ? cost[p0 + t] : 1.0f;
}
void mrf_exact_costs(mvs_ctx* ctx, uint32_t nb0, uint32_t ne0) {
    resolve_best(ctx);
    if (ne0 <= nb0) return;
    // the polish and the region moves keep position / label / unary of the best labeling consistent: derived once per labeling and range
    if (ctx->exact_valid && ctx->exact_nb == nb0 && ctx->exact_ne == ne0) return;
    ctx->exact_valid = true; ctx->exact_nb = nb0; ctx->exact_ne = ne0;
    MVS_HIP(hipMemsetAsync(&ctx->words->exact_foreign, 0, sizeof(uint32_t), ctx->stream));
    hipLaunchKernelGGL(mrf_exact_cost_kernel, dim3((ne0 - nb0 + 255) / 256), dim3(256), 0, ctx->stream, ctx->r_ptr, ctx->r_view, ctx->r_cost, (const uint32_t*)ctx->b_lab, nb0, ne0, ctx->b_sel, ctx->b_cost, &ctx->words->exact_foreign);
    MVS_LAUNCH_CHECK();
}

// energy of the current decode (best == false) or of the best labeling over nodes [nb0, ne0)
// -> ctx->m_energy (device, 2 x u64), asynchronous
void mrf_energy(mvs_ctx* ctx, bool best, uint32_t nb0, uint32_t ne0, bool reduce) {
    const unsigned blocks = ne0 > nb0 ? std::min<unsigned>((ne0 - nb0 + 255) / 256, 2048u) : 0u;
    ctx->m_energy_blocks = blocks; ctx->m_energy_from_sweep = false;
    unsigned long long* partial = ctx->m_energy.p + 4;
    if (best) mrf_exact_costs(ctx, nb0, ne0);   // idempotent: whatever is reported about the best labeling uses the exact costs
    if (blocks) {
        if (best) hipLaunchKernelGGL(mrf_energy_kernel, dim3(blocks), dim3(256), 0, ctx->stream, ctx->r_ptr, ctx->r_view, ctx->r_cost, ctx->r_adj_ptr, ctx->r_adj, ctx->b_lab, ctx->b_cost, (const mvs_mrf_progress*)nullptr, 0u, nb0, ne0, partial);
        else hipLaunchKernelGGL(mrf_energy_kernel, dim3(blocks), dim3(256), 0, ctx->stream, ctx->r_ptr, ctx->r_view, ctx->r_cost, ctx->r_adj_ptr, ctx->r_adj, ctx->m_lab.p, ctx->m_cost.p, ctx->m_state.p, ctx->m_stride, nb0, ne0, partial);
        MVS_LAUNCH_CHECK();
    }
    if (!reduce) return;   // the caller's mrf_step sums the partials
    hipLaunchKernelGGL(mrf_energy_reduce_kernel, dim3(1), dim3(1024), 0, ctx->stream, partial, blocks, ctx->m_energy.p, (unsigned long long*)nullptr);
    MVS_LAUNCH_CHECK();
}
// the energy pair the fast-path sweep kernels of the last sweep left behind as per-block partials (own node range of a
// sharded caller, or the whole graph) -> ctx->m_energy (device), asynchronous
// (here and not beside mrf_sweep: it shares mrf_energy_reduce_kernel with mrf_energy, and a kernel is launched from the file that defines it)
void mrf_sweep_energy_reduce(mvs_ctx* ctx, unsigned long long* out2) {
    const uint32_t n = EPART_BLOCKS * std::max<uint32_t>(ctx->m_colours, 1u);
    hipLaunchKernelGGL(mrf_energy_reduce_kernel, dim3(1), dim3(1024), 0, ctx->stream, ctx->m_energy.p + 4, n, ctx->m_energy.p, out2);
    MVS_LAUNCH_CHECK();
}

// best labeling := the current decode (an index flip on the device)
void mrf_keep_best(mvs_ctx* ctx) {
    best_labeling_may_have_changed(ctx);
    if (!ctx->m_state.p) throw StatusError(MVS_ERR_STATE, "mrf setup first");
    hipLaunchKernelGGL(mrf_flip_kernel, dim3(1), dim3(1), 0, ctx->stream, ctx->m_state.p);
    MVS_LAUNCH_CHECK();
}

// blocks of 256 / G nodes that cover n nodes, one lane group of G lanes per node
static unsigned icm_blocks(uint32_t n, uint32_t G) { return (n + (256u / G) - 1u) / (256u / G); }
// gains of nodes [b, e), or of the node ids list[b .. e) -- with `count`, of list[b .. b + *count) -- G lanes per node
static void launch_icm_gain(mvs_ctx* ctx, uint32_t G, unsigned blocks, uint32_t b, uint32_t e, const uint32_t* list, const uint32_t* count) {
    const auto k = G == 8 ? mrf_icm_gain_kernel<8> : G == 16 ? mrf_icm_gain_kernel<16> : G == 32 ? mrf_icm_gain_kernel<32> : mrf_icm_gain_kernel<64>;
    hipLaunchKernelGGL(k, dim3(blocks), dim3(256), 0, ctx->stream, ctx->r_ptr, ctx->r_view, ctx->r_cost, ctx->r_adj_ptr, ctx->r_adj,
                       ctx->b_sel, ctx->b_lab, b, e, ctx->m_gain.p, ctx->m_cand.p, list, count);
    MVS_LAUNCH_CHECK();
}
// gains of the fast nodes through their descriptors, schedule positions [0, nf)
static void launch_icm_gain_desc(mvs_ctx* ctx, uint32_t G, uint32_t nf) {
    const auto k = G == 8 ? mrf_icm_gain_desc_kernel<8> : G == 16 ? mrf_icm_gain_desc_kernel<16> : mrf_icm_gain_desc_kernel<32>;
    hipLaunchKernelGGL(k, dim3(std::max(1u, std::min(icm_blocks(nf, G), 256u * 8u))), dim3(256), 0, ctx->stream,
                       ctx->m_desc.p, ctx->r_ptr, ctx->r_view, ctx->r_cost, ctx->b_sel, ctx->b_lab, 0u, nf, ctx->m_gain.p, ctx->m_cand.p);
    MVS_LAUNCH_CHECK();
}

// ICM on the best labeling (in place): gains of nodes [nb0, ne0)
void mrf_icm_gain(mvs_ctx* ctx, uint32_t nb0, uint32_t ne0) {
    if (ne0 <= nb0) return;
    resolve_best(ctx);
    const uint32_t K = ctx->m_kmax, n = ne0 - nb0;
    const bool whole = nb0 == 0 && ne0 == ctx->csr_faces;
    // active set (unsharded calls only): after one full evaluation, only the nodes the last apply listed -- the nodes that
    // moved and their neighbours -- are re-evaluated; everybody else's stored gain / candidate are still the values a
    // full pass would compute.  Sharded callers exchange labels behind the library's back, so they evaluate all.
    // The list's length is read on the device (fixed grid, grid-stride loop): no host round trip between the rounds.
    if (whole && ctx->icm_dirty_valid) {
        const uint32_t G = K <= 8 ? 8 : K <= 16 ? 16 : K <= 32 ? 32 : 64;
        launch_icm_gain(ctx, G, std::max(1u, std::min(icm_blocks(n, G), 1024u)), 0u, 0u, ctx->m_alist.p, &ctx->words->icm_cursor);
        return;
    }
    if (whole) {   // whole-graph calls: the fast nodes through their descriptors (schedule positions [0, n_fast)), the generic nodes as a list
        const uint32_t nf = ctx->m_n_fast;
        if (nf) launch_icm_gain_desc(ctx, K <= 8 ? 8 : K <= 64 ? 16 : 32, nf);   // 16 lanes up to 64 labels: 0.74 -> 0.62 ms of polish at C3 (K = 50)
        if (nf < n) launch_icm_gain(ctx, 64, icm_blocks(n - nf, 64), nf, n, ctx->m_perm.p, nullptr);
    } else {
        // lanes per node: the label loop strides by the group size, so any size is exact; 16 lanes keep four nodes per wave busy up to
        // 64 labels (a 64-lane group would idle most of its lanes on the usual 40 - 50 candidates)
        const uint32_t G = K <= 8 ? 8 : K <= 64 ? 16 : K <= 128 ? 32 : 64;
        launch_icm_gain(ctx, G, icm_blocks(n, G), nb0, ne0, nullptr, nullptr);
    }
    ctx->icm_dirty_valid = whole;   // every gain is current: the next apply starts the list
}
void mrf_icm_apply(mvs_ctx* ctx, uint32_t nb0, uint32_t ne0) {
    MVS_HIP(hipMemsetAsync(&ctx->words->icm_n_moved, 0, 2 * sizeof(uint32_t), ctx->stream));   // moved count and list cursor
    if (ne0 <= nb0) return;
    resolve_best(ctx);
    const bool whole = nb0 == 0 && ne0 == ctx->csr_faces;
    if (!whole) ctx->icm_dirty_valid = false;
    uint32_t* alist = nullptr;
    if (ctx->icm_dirty_valid) {   // winners form an independent set: at most (nodes + directed edges) entries
        ctx->m_alist.ensure((size_t)ctx->csr_faces + (size_t)ctx->m_n_adj + 16);
        alist = ctx->m_alist.p;
    }
    hipLaunchKernelGGL(mrf_icm_apply_kernel, dim3((ne0 - nb0 + 255) / 256), dim3(256), 0, ctx->stream, ctx->r_ptr, ctx->r_view, ctx->r_cost, ctx->r_adj_ptr, ctx->r_adj,
                       ctx->m_gain.p, ctx->m_cand.p, ctx->b_sel, ctx->b_lab, ctx->b_cost, nb0, ne0, &ctx->words->icm_n_moved, alist, ctx->t_perm);
    MVS_LAUNCH_CHECK();
}
// labels of nodes [nb0, ne0) of the best labeling into d_labels[0 .. ne0 - nb0); out = {bad, unseen}
// (caller_order: the whole graph's labels at the caller's face ids -- ctx->t_perm; otherwise positions nb0 .. of the table's order)
void mrf_labels(mvs_ctx* ctx, uint32_t nb0, uint32_t ne0, uint32_t* d_labels, uint32_t out[2], bool caller_order) {
    uint32_t* bu = &ctx->words->labels_bad;   // [0] bad, [1] unseen
    resolve_best(ctx);
    MVS_HIP(hipMemsetAsync(bu, 0, 2 * sizeof(uint32_t), ctx->stream));
    if (ne0 > nb0) {
        const uint32_t* foreign = (ctx->exact_valid && ctx->exact_nb == nb0 && ctx->exact_ne == ne0) ? &ctx->words->exact_foreign : (const uint32_t*)nullptr;
        hipLaunchKernelGGL(mrf_labels_kernel, dim3((ne0 - nb0 + 255) / 256), dim3(256), 0, ctx->stream, ctx->b_lab, nb0, ne0, ctx->csr_views, d_labels, bu, caller_order ? ctx->t_perm : (const uint32_t*)nullptr, foreign);
        MVS_LAUNCH_CHECK();
    }
    read_words(ctx, bu, out, 2);
}

}  // namespace mvs
