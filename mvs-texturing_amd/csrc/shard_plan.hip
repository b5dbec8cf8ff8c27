// shard_plan.hip -- the halo plan of the sharded solver (shard.hip's scheme: which runs, which nodes, in which order), built ON THE
// DEVICE from the adjacency, the partition, the colouring and the rank's own message layout; and the sorted key lists it is made of,
// which the sharded table's face lists (shard_table.hip) use as well.  The key layout and the offsets' arithmetic are shard_lists.h.
#include "shard.h"
#include "sort_scan.h"

using namespace mvs;

namespace {

// One thread per own face: the cut edges around it.  For the in-edge e = (i <- j) with j on another rank q:
//   RECV  the run of e (K_i bytes at in_off[e] of MY layout), written by q in phase colour[j];
//   SEND  the run of the reverse edge r = (j <- i) (K_j bytes at MY in_off[r] = out_off of e), written here in phase colour[i];
//   node j is a halo node (its label arrives after phase colour[j]), node i a boundary node (its label leaves after phase colour[i]).
__global__ void plan_emit_kernel(const uint32_t* __restrict__ col_ptr, const uint32_t* __restrict__ adj_ptr, const uint32_t* __restrict__ adj,
                                 const MrfEdge* __restrict__ edge, const uint32_t* __restrict__ colour, Parts parts, int me, uint32_t nb, uint32_t ne,
                                 unsigned long long* __restrict__ k_msg_send, unsigned long long* __restrict__ v_msg_send,
                                 unsigned long long* __restrict__ k_msg_recv, unsigned long long* __restrict__ v_msg_recv,
                                 unsigned long long* __restrict__ k_node_send, unsigned long long* __restrict__ k_node_recv, uint32_t* __restrict__ counters) {
    const uint32_t i = nb + blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ne) return;
    const uint32_t Ki = col_ptr[i + 1] - col_ptr[i], ci = colour[i];
    for (uint32_t e = adj_ptr[i]; e < adj_ptr[i + 1]; ++e) {
        const uint32_t j = adj[e];
        const int q = part_of(parts, j);
        if (q == me) continue;
        const uint32_t cj = colour[j];
        k_node_send[atomicAdd(&counters[2], 1u)] = plan_key(q, ci, i);     // duplicates (several neighbours on q) are removed after the sort
        k_node_recv[atomicAdd(&counters[3], 1u)] = plan_key(q, cj, j);
        const MrfEdge m = edge[e];
        if (m.kj == 0) continue;                                           // edge not in the model
        uint32_t r = adj_ptr[j]; while (adj[r] != i) ++r;                  // global index of the reverse directed edge (j <- i); m.kj != 0 => it exists
        uint32_t w = atomicAdd(&counters[1], 1u);
        k_msg_recv[w] = plan_key(q, cj, e); v_msg_recv[w] = ((unsigned long long)m.in_off << 32) | Ki;
        w = atomicAdd(&counters[0], 1u);
        k_msg_send[w] = plan_key(q, ci, r); v_msg_send[w] = ((unsigned long long)m.out_off << 32) | m.kj;
    }
}
// flag[k] = 1 iff key[k] differs from key[k - 1] (first of its run)
__global__ void plan_first_kernel(const unsigned long long* __restrict__ key, uint32_t n, uint32_t* __restrict__ flag) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k <= n) flag[k] = (k < n && (k == 0 || key[k] != key[k - 1])) ? 1u : 0u;
}
__global__ void plan_compact_kernel(const unsigned long long* __restrict__ key, const uint32_t* __restrict__ flag, const uint32_t* __restrict__ pos, uint32_t n,
                                    unsigned long long* __restrict__ out) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n && flag[k]) out[pos[k]] = key[k];
}
__global__ void plan_len_kernel(const unsigned long long* __restrict__ val, uint32_t n, uint32_t* __restrict__ len) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k <= n) len[k] = k < n ? (uint32_t)(val[k] & 0xFFFFFFFFull) : 0u;
}
// element offsets of record k: off .. off + len - 1 at idx[pos[k] ..]; one wave per record
__global__ void plan_expand_kernel(const unsigned long long* __restrict__ val, const uint32_t* __restrict__ pos, uint32_t n, uint32_t* __restrict__ idx) {
    const uint32_t k = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63;
    if (k >= n) return;
    const uint32_t off = (uint32_t)(val[k] >> 32), len = (uint32_t)(val[k] & 0xFFFFFFFFull), p = pos[k];
    for (uint32_t t = lane; t < len; t += 64) idx[p + t] = off + t;
}
// (phase, peer, id) -> (0, peer, id)
__global__ void plan_rekey_kernel(unsigned long long* __restrict__ key, uint32_t n) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) key[k] &= 0xFFFFFFFFFFull;
}
__global__ void plan_node_kernel(const unsigned long long* __restrict__ key, uint32_t n, uint32_t* __restrict__ node) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) node[k] = (uint32_t)(key[k] & 0xFFFFFFFFull);
}

// builds one message list (records -> expanded element indices) from sorted device keys
void finish_msg_list(mvs_shard* S, mvs_shard::Lists& L, DBuf<unsigned long long>& k, DBuf<unsigned long long>& v, uint32_t n, hipStream_t s) {
    std::vector<unsigned long long> hk(n), hv(n);
    if (n) {
        MVS_HIP(hipMemcpyAsync(hk.data(), k.p, (size_t)n * 8, hipMemcpyDeviceToHost, s));
        MVS_HIP(hipMemcpyAsync(hv.data(), v.p, (size_t)n * 8, hipMemcpyDeviceToHost, s));
        MVS_HIP(hipStreamSynchronize(s));
    }
    std::vector<uint32_t> lens(n);
    for (uint32_t i = 0; i < n; ++i) lens[i] = (uint32_t)(hv[i] & 0xFFFFFFFFull);
    segment(hk, &lens, S->P, S->phases, L.off, L.total);
    L.idx.ensure(L.total + 4);
    if (n) {
        S->tmp_a.ensure((size_t)n + 2); S->tmp_b.ensure((size_t)n + 2);
        hipLaunchKernelGGL(plan_len_kernel, dim3((n + 256) / 256), dim3(256), 0, s, v.p, n, S->tmp_a.p); MVS_LAUNCH_CHECK();
        exclusive_scan_u32(S->ctx, S->tmp_a.p, S->tmp_b.p, (size_t)n + 1, nullptr);
        hipLaunchKernelGGL(plan_expand_kernel, dim3((unsigned)(((size_t)n * 64 + 255) / 256)), dim3(256), 0, s, v.p, S->tmp_b.p, n, L.idx.p); MVS_LAUNCH_CHECK();
    }
}

}  // namespace

namespace mvs {

uint32_t own_directed_edges(mvs_shard* S) {
    hipStream_t s = S->ctx->stream;
    uint32_t h[2] = {0, 0};
    MVS_HIP(hipMemcpyAsync(&h[0], S->d_adj_ptr + S->nb, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    MVS_HIP(hipMemcpyAsync(&h[1], S->d_adj_ptr + S->ne, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    MVS_HIP(hipStreamSynchronize(s));
    return h[1] - h[0];
}

void sort_pairs(mvs_shard* S, DBuf<unsigned long long>& k, DBuf<unsigned long long>* v, uint32_t n, hipStream_t s) {
    if (n == 0) return;
    S->ks.ensure(n + 1); if (v) S->vs.ensure(n + 1);
    if (v) {
        dev_sort_pairs(S->sort_tmp, s, k.p, S->ks.p, v->p, S->vs.p, n, 0, 48);
        MVS_HIP(hipMemcpyAsync(v->p, S->vs.p, (size_t)n * 8, hipMemcpyDeviceToDevice, s));
    } else {
        dev_sort_keys(S->sort_tmp, s, k.p, S->ks.p, n, 0, 48);
    }
    MVS_HIP(hipMemcpyAsync(k.p, S->ks.p, (size_t)n * 8, hipMemcpyDeviceToDevice, s));
}
// sorted keys with duplicates -> unique keys (in place), returns the new count
uint32_t unique_keys(mvs_shard* S, DBuf<unsigned long long>& k, uint32_t n, hipStream_t s) {
    if (n == 0) return 0;
    S->tmp_a.ensure((size_t)n + 2); S->tmp_b.ensure((size_t)n + 2); S->ks.ensure((size_t)n + 1);
    hipLaunchKernelGGL(plan_first_kernel, dim3((n + 256) / 256), dim3(256), 0, s, k.p, n, S->tmp_a.p); MVS_LAUNCH_CHECK();
    exclusive_scan_u32(S->ctx, S->tmp_a.p, S->tmp_b.p, (size_t)n + 1, nullptr);
    hipLaunchKernelGGL(plan_compact_kernel, dim3((n + 255) / 256), dim3(256), 0, s, k.p, S->tmp_a.p, S->tmp_b.p, n, S->ks.p); MVS_LAUNCH_CHECK();
    uint32_t m = 0;
    MVS_HIP(hipMemcpyAsync(&m, S->tmp_b.p + n, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    MVS_HIP(hipStreamSynchronize(s));
    MVS_HIP(hipMemcpyAsync(k.p, S->ks.p, (size_t)m * 8, hipMemcpyDeviceToDevice, s));
    return m;
}
// builds one node list from sorted, unique device keys
void finish_node_list(mvs_shard* S, mvs_shard::Lists& L, DBuf<unsigned long long>& k, uint32_t n, uint32_t phases, hipStream_t s) {
    std::vector<unsigned long long> hk(n);
    if (n) { MVS_HIP(hipMemcpyAsync(hk.data(), k.p, (size_t)n * 8, hipMemcpyDeviceToHost, s)); MVS_HIP(hipStreamSynchronize(s)); }
    segment(hk, nullptr, S->P, phases, L.off, L.total);
    L.idx.ensure(L.total + 4);
    if (n) { hipLaunchKernelGGL(plan_node_kernel, dim3((n + 255) / 256), dim3(256), 0, s, k.p, n, L.idx.p); MVS_LAUNCH_CHECK(); }
}

void build_plan(mvs_shard* S) {
    mvs_ctx* ctx = S->ctx; hipStream_t s = ctx->stream;
    const uint32_t nf = S->ne - S->nb;
    const uint32_t own_edges = own_directed_edges(S);
    const size_t cap = (size_t)own_edges + 8;
    S->k0.ensure(cap); S->k1.ensure(cap); S->k2.ensure(cap); S->k3.ensure(cap); S->v0.ensure(cap); S->v1.ensure(cap); S->counters.ensure(8);
    MVS_HIP(hipMemsetAsync(S->counters.p, 0, 8 * sizeof(uint32_t), s));
    S->phases = ctx->m_colours;
    if (S->phases > 255) throw StatusError(MVS_ERR_UNSUPPORTED, "more than 255 colour phases");
    if (nf) {
        hipLaunchKernelGGL(plan_emit_kernel, dim3((nf + 255) / 256), dim3(256), 0, s, ctx->r_ptr, S->d_adj_ptr, S->d_adj, ctx->m_edge.p, ctx->m_colour.p, S->parts, S->me, S->nb, S->ne,
                           S->k0.p, S->v0.p, S->k1.p, S->v1.p, S->k2.p, S->k3.p, S->counters.p);
        MVS_LAUNCH_CHECK();
    }
    uint32_t n[4];
    MVS_HIP(hipMemcpyAsync(n, S->counters.p, sizeof(n), hipMemcpyDeviceToHost, s));
    MVS_HIP(hipStreamSynchronize(s));
    sort_pairs(S, S->k0, &S->v0, n[0], s); sort_pairs(S, S->k1, &S->v1, n[1], s);
    sort_pairs(S, S->k2, nullptr, n[2], s); sort_pairs(S, S->k3, nullptr, n[3], s);
    const uint32_t ns = unique_keys(S, S->k2, n[2], s), nr = unique_keys(S, S->k3, n[3], s);
    finish_msg_list(S, S->msg_send, S->k0, S->v0, n[0], s);
    finish_msg_list(S, S->msg_recv, S->k1, S->v1, n[1], s);
    finish_node_list(S, S->node_send, S->k2, ns, S->phases, s);
    finish_node_list(S, S->node_recv, S->k3, nr, S->phases, s);
    // the same nodes peer-major over all phases (key = peer << 32 | id): the ICM exchanges send one range per peer
    if (ns) { hipLaunchKernelGGL(plan_rekey_kernel, dim3((ns + 255) / 256), dim3(256), 0, s, S->k2.p, ns); MVS_LAUNCH_CHECK(); }
    if (nr) { hipLaunchKernelGGL(plan_rekey_kernel, dim3((nr + 255) / 256), dim3(256), 0, s, S->k3.p, nr); MVS_LAUNCH_CHECK(); }
    sort_pairs(S, S->k2, nullptr, ns, s); sort_pairs(S, S->k3, nullptr, nr, s);
    finish_node_list(S, S->all_send, S->k2, ns, 1, s);
    finish_node_list(S, S->all_recv, S->k3, nr, 1, s);
    auto offsets = [&](mvs_shard::Lists& L, uint32_t elem) { phase_offsets(L.off, S->P, elem, L.bytes); };
    offsets(S->msg_send, 1); offsets(S->msg_recv, 1);
    offsets(S->node_send, 4); offsets(S->node_recv, 4);
    offsets(S->all_send, 4); offsets(S->all_recv, 4);
}

}  // namespace mvs
