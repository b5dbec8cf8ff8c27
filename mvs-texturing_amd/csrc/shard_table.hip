// shard_table.hip -- the sharded cost table (shard.hip's scheme: global shape, only the own columns and the halo columns filled) and the
// steps of mvs_shard_data_costs that make it.  Every rank takes the steps in the same order: the communicator calls inside them
// (all-reduce MAX, all-reduce SUM, all-gather, exchange) are collective.
#include "shard.h"

using namespace mvs;

namespace {

__global__ void counts_kernel(const uint32_t* __restrict__ col_ptr, uint32_t n, uint32_t* __restrict__ counts) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) counts[i] = col_ptr[i + 1] - col_ptr[i];
}
// all-gathered padded blocks -> one array of F column lengths
__global__ void unpad_counts_kernel(const uint32_t* __restrict__ padded, uint32_t pad, Parts parts, uint32_t F, uint32_t* __restrict__ counts_g) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= F) return;
    const int q = part_of(parts, i);
    counts_g[i] = padded[(size_t)q * pad + (i - parts.b[q])];
}
// keep[i] = 1 for own faces and for halo faces (faces of other parts adjacent to an own face); one thread per own face
__global__ void keep_own_kernel(uint32_t nb, uint32_t ne, uint32_t* __restrict__ keep) {
    const uint32_t i = nb + blockIdx.x * blockDim.x + threadIdx.x;
    if (i < ne) keep[i] = 1u;
}
__global__ void halo_mark_kernel(const uint32_t* __restrict__ adj_ptr, const uint32_t* __restrict__ adj, Parts parts, int me, uint32_t nb, uint32_t ne,
                                 uint32_t* __restrict__ keep, unsigned long long* __restrict__ k_send, unsigned long long* __restrict__ k_recv, uint32_t* __restrict__ counters) {
    const uint32_t i = nb + blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ne) return;
    for (uint32_t e = adj_ptr[i]; e < adj_ptr[i + 1]; ++e) {
        const uint32_t j = adj[e];
        const int q = part_of(parts, j);
        if (q == me) continue;
        keep[j] = 1u;                                                     // racing stores of the same value
        k_send[atomicAdd(&counters[0], 1u)] = plan_key(q, 0u, i);          // my column i goes to q
        k_recv[atomicAdd(&counters[1], 1u)] = plan_key(q, 0u, j);          // column j comes from q
    }
}
__global__ void masked_counts_kernel(const uint32_t* __restrict__ counts_g, const uint32_t* __restrict__ keep, uint32_t F, uint32_t* __restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i <= F) out[i] = (i < F && keep[i]) ? counts_g[i] : 0u;
}
// column records of a face list: {view id, cost} pairs, 8 bytes each, at rec[pos[k] ..]
__global__ void pack_columns_kernel(const uint32_t* __restrict__ faces, const uint32_t* __restrict__ pos, uint32_t n, uint32_t face_base, const uint32_t* __restrict__ col_ptr,
                                    const uint16_t* __restrict__ view_id, const float* __restrict__ cost, uint2* __restrict__ rec) {
    const uint32_t k = (blockIdx.x * blockDim.x + threadIdx.x) >> 4, lane = threadIdx.x & 15;
    if (k >= n) return;
    const uint32_t f = faces[k] - face_base, p0 = col_ptr[f], K = col_ptr[f + 1] - p0, o = pos[k];
    for (uint32_t t = lane; t < K; t += 16) rec[o + t] = make_uint2((uint32_t)view_id[p0 + t], __float_as_uint(cost[p0 + t]));
}
__global__ void unpack_columns_kernel(const uint32_t* __restrict__ faces, const uint32_t* __restrict__ pos, uint32_t n, const uint32_t* __restrict__ col_ptr_l,
                                      const uint2* __restrict__ rec, uint16_t* __restrict__ view_id, float* __restrict__ cost) {
    const uint32_t k = (blockIdx.x * blockDim.x + threadIdx.x) >> 4, lane = threadIdx.x & 15;
    if (k >= n) return;
    const uint32_t f = faces[k], p0 = col_ptr_l[f], K = col_ptr_l[f + 1] - p0, o = pos[k];
    for (uint32_t t = lane; t < K; t += 16) { const uint2 r = rec[o + t]; view_id[p0 + t] = (uint16_t)r.x; cost[p0 + t] = __uint_as_float(r.y); }
}
// *changed = 1 iff a != b somewhere (racing stores of the same value)
__global__ void differ_kernel(const uint32_t* __restrict__ a, const uint32_t* __restrict__ b, uint32_t n, uint32_t* __restrict__ changed) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && a[i] != b[i]) *changed = 1u;
}
__global__ void face_len_kernel(const uint32_t* __restrict__ faces, uint32_t n, const uint32_t* __restrict__ counts_g, uint32_t* __restrict__ len) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k <= n) len[k] = k < n ? counts_g[faces[k]] : 0u;
}

// halo faces and the boundary faces that go to each neighbour, both ascending by (peer, face)
void rebuild_face_lists(mvs_shard* S) {
    hipStream_t s = S->ctx->stream;
    const uint32_t F = S->F, nb = S->nb, ne = S->ne, nf = ne - nb; const int me = S->me;
    const uint32_t own_edges = own_directed_edges(S);
    S->k0.ensure((size_t)own_edges + 8); S->k1.ensure((size_t)own_edges + 8);
    MVS_HIP(hipMemsetAsync(S->counters.p, 0, 8 * sizeof(uint32_t), s));
    MVS_HIP(hipMemsetAsync(S->keep.p, 0, ((size_t)F + 1) * sizeof(uint32_t), s));
    if (nf) {
        hipLaunchKernelGGL(keep_own_kernel, dim3((nf + 255) / 256), dim3(256), 0, s, nb, ne, S->keep.p); MVS_LAUNCH_CHECK();
        hipLaunchKernelGGL(halo_mark_kernel, dim3((nf + 255) / 256), dim3(256), 0, s, S->d_adj_ptr, S->d_adj, S->parts, me, nb, ne, S->keep.p, S->k0.p, S->k1.p, S->counters.p); MVS_LAUNCH_CHECK();
    }
    uint32_t n[2];
    MVS_HIP(hipMemcpyAsync(n, S->counters.p, sizeof(n), hipMemcpyDeviceToHost, s));
    MVS_HIP(hipStreamSynchronize(s));
    sort_pairs(S, S->k0, nullptr, n[0], s); sort_pairs(S, S->k1, nullptr, n[1], s);
    const uint32_t ns = unique_keys(S, S->k0, n[0], s), nr = unique_keys(S, S->k1, n[1], s);
    finish_node_list(S, S->fs, S->k0, ns, 1, s); finish_node_list(S, S->fr, S->k1, nr, 1, s);
}
// the local table: own + halo columns at their global positions
void rebuild_table_shape(mvs_shard* S) {
    mvs_ctx* ctx = S->ctx; hipStream_t s = ctx->stream;
    const uint32_t F = S->F;
    S->t_ptr.ensure((size_t)F + 2); S->tmp_c.ensure((size_t)F + 2);
    hipLaunchKernelGGL(masked_counts_kernel, dim3((F + 256) / 256), dim3(256), 0, s, S->counts_g.p, S->keep.p, F, S->tmp_c.p); MVS_LAUNCH_CHECK();
    exclusive_scan_u32(ctx, S->tmp_c.p, S->t_ptr.p, (size_t)F + 1, nullptr);
    const uint64_t nnz_bound = sum_u32(ctx, S->tmp_c.p, F);
    if (nnz_bound >= 0xFFFFFFF0ull) throw StatusError(MVS_ERR_UNSUPPORTED, "local cost table exceeds 2^32 entries: use more parts");
    S->nnz_l = (uint32_t)nnz_bound;
    MVS_HIP(hipMemcpyAsync(&S->own_start, S->t_ptr.p + S->nb, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    MVS_HIP(hipStreamSynchronize(s));
}
// where the records of the columns of a face list sit in an exchange buffer: pos per face, byte offsets per peer; returns the records
uint64_t positions(mvs_shard* S, mvs_shard::Lists& L, DBuf<uint32_t>& pos, std::vector<uint64_t>& off_bytes) {
    mvs_ctx* ctx = S->ctx; hipStream_t s = ctx->stream; const int P = S->P;
    const uint32_t m = (uint32_t)L.total;
    S->tmp_a.ensure((size_t)m + 2); pos.ensure((size_t)m + 2);
    hipLaunchKernelGGL(face_len_kernel, dim3((m + 256) / 256), dim3(256), 0, s, L.idx.p, m, S->counts_g.p, S->tmp_a.p); MVS_LAUNCH_CHECK();
    exclusive_scan_u32(ctx, S->tmp_a.p, pos.p, (size_t)m + 1, nullptr);
    std::vector<uint32_t> hp((size_t)m + 1);
    MVS_HIP(hipMemcpyAsync(hp.data(), pos.p, ((size_t)m + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    MVS_HIP(hipStreamSynchronize(s));
    off_bytes.assign((size_t)P + 1, 0);
    for (int q = 0; q <= P; ++q) off_bytes[q] = (uint64_t)hp[L.off[std::min(q, P)]] * sizeof(uint2);
    return hp[m];
}

}  // namespace

namespace mvs {

// data costs over the ranks: the global barrier of postprocess_face_infos is one all-reduce MAX and one all-reduce SUM of the histogram
uint64_t shard_costs_over_ranks(mvs_shard* S, const mvs_settings* settings, mvs_dc_stats* stats) {
    mvs_ctx* ctx = S->ctx; hipStream_t s = ctx->stream; mvs_comm* comm = S->comm;
    ctx->face_begin = S->nb; ctx->face_end = S->ne; ctx->have_costs = false; ctx->dc_phase = 0;
    dc_phase1(ctx, settings);
    comm->allreduce(ctx->max_q.p, 1, mvs_comm::F32, mvs_comm::MAX, s);                 /* :278-281 */
    dc_phase2(ctx);
    comm->allreduce(ctx->hist.p, MVS_HIST_WORDS, mvs_comm::U32, mvs_comm::SUM, s);     /* :283-286 */
    mvs_dc_stats st; dc_phase3(ctx, &st);
    if (stats) *stats = st;
    return ctx->csr_nnz;
}

// column lengths of every face: one padded all-gather
void shard_gather_lengths(mvs_shard* S) {
    mvs_ctx* ctx = S->ctx; hipStream_t s = ctx->stream;
    const uint32_t F = S->F, nf = S->ne - S->nb; const int P = S->P;
    uint32_t pad = 0; for (int q = 0; q < P; ++q) pad = std::max(pad, S->parts.b[q + 1] - S->parts.b[q]);
    S->tmp_a.ensure((size_t)pad + 2); S->tmp_b.ensure((size_t)pad * P + 2); S->counts_g.ensure((size_t)F + 2); S->keep.ensure((size_t)F + 2);
    MVS_HIP(hipMemsetAsync(S->tmp_a.p, 0, ((size_t)pad + 1) * sizeof(uint32_t), s));
    if (nf) { hipLaunchKernelGGL(counts_kernel, dim3((nf + 255) / 256), dim3(256), 0, s, ctx->r_ptr, nf, S->tmp_a.p); MVS_LAUNCH_CHECK(); }
    S->comm->allgather(S->tmp_a.p, S->tmp_b.p, (size_t)pad * sizeof(uint32_t), s);
    hipLaunchKernelGGL(unpad_counts_kernel, dim3((F + 255) / 256), dim3(256), 0, s, S->tmp_b.p, pad, S->parts, F, S->counts_g.p); MVS_LAUNCH_CHECK();
}

// are the column lengths those of the previous step?  Then the table's shape, the boundary / halo lists and the solver's
// halo plan are still valid.  The global entry count and the comparison come back in ONE read-back.
bool shard_lengths_unchanged(mvs_shard* S, uint64_t* nnz_global) {
    mvs_ctx* ctx = S->ctx; hipStream_t s = ctx->stream; const uint32_t F = S->F;
    S->counts_prev.ensure((size_t)F + 2); S->counters.ensure(8);
    MVS_HIP(hipMemsetAsync(S->counters.p, 0, 8 * sizeof(uint32_t), s));
    bool same = S->have_prev && S->tables_valid;
    if (same && F) { hipLaunchKernelGGL(differ_kernel, dim3((F + 255) / 256), dim3(256), 0, s, (const uint32_t*)S->counts_g.p, (const uint32_t*)S->counts_prev.p, F, S->counters.p + 4); MVS_LAUNCH_CHECK(); }
    S->nnz_global = sum_u32(ctx, S->counts_g.p, F);               // (blocking: the stream is drained here)
    if (nnz_global) *nnz_global = S->nnz_global;
    if (same) { uint32_t ch = 0; MVS_HIP(hipMemcpyAsync(&ch, S->counters.p + 4, sizeof(uint32_t), hipMemcpyDeviceToHost, s)); MVS_HIP(hipStreamSynchronize(s)); same = ch == 0; }
    return same;
}

void shard_rebuild_tables(mvs_shard* S) {
    hipStream_t s = S->ctx->stream;
    S->tables_valid = false; S->plan_valid = false;
    MVS_HIP(hipMemcpyAsync(S->counts_prev.p, S->counts_g.p, (size_t)S->F * sizeof(uint32_t), hipMemcpyDeviceToDevice, s)); S->have_prev = true;
    rebuild_face_lists(S);
    rebuild_table_shape(S);
    // where the records of the boundary columns (out) and of the halo columns (in) sit in the exchange buffers
    S->rec_s = positions(S, S->fs, S->pos_s, S->col_so); S->rec_r = positions(S, S->fr, S->pos_r, S->col_ro);
    S->tables_valid = true;
}

void shard_fill_table(mvs_shard* S, uint64_t nnz_own) {
    mvs_ctx* ctx = S->ctx; hipStream_t s = ctx->stream;
    const uint32_t nnz_l = S->nnz_l, own_start = S->own_start;
    mvs_shard::Lists& fs = S->fs; mvs_shard::Lists& fr = S->fr;
    S->t_view.ensure((size_t)nnz_l + 8); S->t_cost.ensure((size_t)nnz_l + 16);
    if (nnz_own) {   // the own columns are one contiguous block
        MVS_HIP(hipMemcpyAsync(S->t_view.p + own_start, ctx->r_view, nnz_own * sizeof(uint16_t), hipMemcpyDeviceToDevice, s));
        MVS_HIP(hipMemcpyAsync(S->t_cost.p + own_start, ctx->r_cost, nnz_own * sizeof(float), hipMemcpyDeviceToDevice, s));
    }
    // halo columns: {view, cost} records, the boundary columns out, the halo columns in
    S->sbuf_col.ensure(S->rec_s + 4); S->rbuf_col.ensure(S->rec_r + 4);
    if (fs.total) { hipLaunchKernelGGL(pack_columns_kernel, dim3((unsigned)((fs.total * 16 + 255) / 256)), dim3(256), 0, s, fs.idx.p, S->pos_s.p, (uint32_t)fs.total, S->nb, ctx->r_ptr, ctx->r_view, ctx->r_cost, S->sbuf_col.p); MVS_LAUNCH_CHECK(); }
    S->comm->exchange((const uint8_t*)S->sbuf_col.p, S->col_so.data(), (uint8_t*)S->rbuf_col.p, S->col_ro.data(), s);
    if (fr.total) { hipLaunchKernelGGL(unpack_columns_kernel, dim3((unsigned)((fr.total * 16 + 255) / 256)), dim3(256), 0, s, fr.idx.p, S->pos_r.p, (uint32_t)fr.total, S->t_ptr.p, S->rbuf_col.p, S->t_view.p, S->t_cost.p); MVS_LAUNCH_CHECK(); }
    MVS_HIP(hipMemsetAsync(S->t_cost.p + nnz_l, 0, 8 * sizeof(float), s));
    MVS_HIP(hipStreamSynchronize(s));
}

// the context's active table := the sharded one (its own buffers keep the own columns for the next step's reuse)
void shard_activate_table(mvs_shard* S) {
    mvs_ctx* ctx = S->ctx;
    ctx->r_ptr = S->t_ptr.p; ctx->r_view = S->t_view.p; ctx->r_cost = S->t_cost.p;
    ctx->csr_faces = S->F; ctx->csr_views = ctx->n_views; ctx->csr_nnz = S->nnz_l; ctx->have_costs = true; ctx->csr_q_valid = false;
    // the table has the global shape, in the library's face order
    ctx->u_valid = false;
    if (ctx->mesh_ordered) { ctx->t_perm = ctx->f_perm.p; ctx->t_pos = ctx->f_pos.p; } else { ctx->t_perm = nullptr; ctx->t_pos = nullptr; }
}

}  // namespace mvs
