// shard_transport.hip -- the two halo transports of the sharded solver's sweep loop (shard.hip's scheme; the Transport interface of
// shard.h): Exchange packs, sends and receives through the communicator and unpacks -- RCCL ranks --, PeerPush stores straight into
// the neighbours' arrays -- ranks that can address each other's device memory (comm.h PeerHub).  Each with its kernels.
#include "shard.h"

#include <chrono>
#include <thread>

using namespace mvs;

namespace {

// pack / unpack of one exchange of node words: labels (or gains) by node id
__global__ void pack_words_kernel(const uint32_t* __restrict__ src, const mvs_mrf_progress* __restrict__ st, uint32_t buf_stride, const uint32_t* __restrict__ idx, uint64_t n, uint32_t* __restrict__ dst) {
    if (st) src += (size_t)st->w * buf_stride;      // the current decode buffer
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (uint64_t)gridDim.x * blockDim.x) dst[k] = src[idx[k]];
}
__global__ void unpack_words_kernel(uint32_t* __restrict__ dst, const mvs_mrf_progress* __restrict__ st, uint32_t buf_stride, const uint32_t* __restrict__ idx, uint64_t n, const uint32_t* __restrict__ src) {
    if (st) dst += (size_t)st->w * buf_stride;
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (uint64_t)gridDim.x * blockDim.x) dst[idx[k]] = src[k];
}

// one launch per phase: the message bytes and the labels of everything this phase sends (all peers) / received
__global__ void pack_phase_kernel(const uint8_t* __restrict__ msg, const uint32_t* __restrict__ midx, uint64_t nm, uint8_t* __restrict__ mdst,
                                  const uint32_t* __restrict__ lab, const mvs_mrf_progress* __restrict__ st, uint32_t buf_stride,
                                  const uint32_t* __restrict__ nidx, uint64_t nn, uint32_t* __restrict__ ndst) {
    lab += (size_t)st->w * buf_stride;              // the current decode buffer
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < nm || k < nn; k += (uint64_t)gridDim.x * blockDim.x) {
        if (k < nm) mdst[k] = msg[midx[k]];
        if (k < nn) ndst[k] = lab[nidx[k]];
    }
}
__global__ void unpack_phase_kernel(uint8_t* __restrict__ msg, const uint32_t* __restrict__ midx, uint64_t nm, const uint8_t* __restrict__ msrc,
                                    uint32_t* __restrict__ lab, const mvs_mrf_progress* __restrict__ st, uint32_t buf_stride,
                                    const uint32_t* __restrict__ nidx, uint64_t nn, const uint32_t* __restrict__ nsrc) {
    lab += (size_t)st->w * buf_stride;
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < nm || k < nn; k += (uint64_t)gridDim.x * blockDim.x) {
        if (k < nm) msg[midx[k]] = msrc[k];
        if (k < nn) lab[nidx[k]] = nsrc[k];
    }
}

// ---- peer push (see PeerHub): one launch per colour phase; blockIdx.y = the peer's segment ----
constexpr int PUSH_SEGS = 8;
struct PushSeg {
    const uint32_t* sidx; const uint32_t* didx; uint8_t* dmsg; uint32_t nm;        // message bytes: dmsg[didx[k]] = msg[sidx[k]]
    const uint32_t* nsidx; const uint32_t* ndidx; uint32_t* dlab; uint32_t nn;     // labels:        dlab[w * dstride + ndidx[k]] = lab[w * stride + nsidx[k]]
    uint32_t dstride;
};
struct PushArgs { PushSeg seg[PUSH_SEGS]; };
__global__ void push_phase_kernel(const uint8_t* __restrict__ msg, const uint32_t* __restrict__ lab, const mvs_mrf_progress* __restrict__ st, uint32_t stride, PushArgs a) {
    const PushSeg& g = a.seg[blockIdx.y];
    const uint32_t w = st->w;                          // the current decode buffer: the same index on every rank (identical decisions)
    const uint32_t* src = lab + (size_t)w * stride; uint32_t* dst = g.dlab + (size_t)w * g.dstride;
    const uint32_t n = g.nm > g.nn ? g.nm : g.nn;
    for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < n; k += gridDim.x * blockDim.x) {
        if (k < g.nm) g.dmsg[g.didx[k]] = msg[g.sidx[k]];
        if (k < g.nn) dst[g.ndidx[k]] = src[g.nsidx[k]];
    }
}
struct PushWSeg { const uint32_t* sidx; const uint32_t* didx; uint32_t* dst; uint32_t n; };
struct PushWArgs { PushWSeg seg[PUSH_SEGS]; };
__global__ void push_words_kernel(const uint32_t* __restrict__ src, PushWArgs a) {   // dst[didx[k]] = src[sidx[k]]: gains / labels of boundary nodes (ICM)
    const PushWSeg& g = a.seg[blockIdx.y];
    for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < g.n; k += gridDim.x * blockDim.x) g.dst[g.didx[k]] = src[g.sidx[k]];
}
struct WordPtrs { const uint32_t* p[MAX_PARTS]; int n; };
__global__ void publish_word_kernel(const uint32_t* __restrict__ v, uint32_t* __restrict__ pub, uint32_t parity) { if (threadIdx.x == 0) pub[parity] = v[0]; }
__global__ void sum_words_kernel(WordPtrs e, uint32_t parity, uint32_t* __restrict__ out) {
    if (threadIdx.x == 0) { uint32_t a = 0u; for (int q = 0; q < e.n; ++q) a += e.p[q][parity]; out[0] = a; }
}

// Pack, grouped send / recv through the communicator, unpack; a phase's hand-over runs on a second stream beside its interior launch
struct Exchange : Transport {
    hipStream_t stream = nullptr; hipEvent_t ev_main = nullptr, ev_comm = nullptr;
    bool busy = false;                                          // the last phase's unpack is queued behind ev_comm
    DBuf<uint8_t> sbuf_msg, rbuf_msg; DBuf<uint32_t> sbuf_node, rbuf_node;   // staging (made to the plan's size by reserve)
    ~Exchange() override { if (ev_main) (void)hipEventDestroy(ev_main); if (ev_comm) (void)hipEventDestroy(ev_comm); if (stream) (void)hipStreamDestroy(stream); }
    // the staging buffers at the size of the plan just built (the node exchange serves the peer-push route's argmin-unary start too)
    void reserve(mvs_shard* S) {
        sbuf_msg.ensure(S->msg_send.total + 64); rbuf_msg.ensure(S->msg_recv.total + 64); sbuf_node.ensure(S->node_send.total + 16); rbuf_node.ensure(S->node_recv.total + 16);
    }
    void before_phase(mvs_shard* S, uint32_t) override {
        if (busy) { MVS_HIP(hipStreamWaitEvent(S->ctx->stream, ev_comm, 0)); busy = false; }
    }
    // the runs written in phase `ph` over cut edges and the labels of its boundary nodes: pack, grouped send / recv and unpack on the
    // second stream, beside the interior launch
    void after_boundary(mvs_shard* S, uint32_t ph) override {
        mvs_ctx* ctx = S->ctx;
        const int P = S->P; const size_t b = (size_t)ph * (P + 1);
        const uint64_t* so_m = S->msg_send.bytes.data() + b; const uint64_t* ro_m = S->msg_recv.bytes.data() + b;
        const uint64_t* so_n = S->node_send.bytes.data() + b; const uint64_t* ro_n = S->node_recv.bytes.data() + b;
        // a rank with no boundary or halo node of this colour (or an empty part) skips the call only on a point-to-point communicator:
        // a collective one is a rendezvous of all ranks, and a rank that stayed away would pair its NEXT operation with this one
        if (so_m[P] + ro_m[P] + so_n[P] + ro_n[P] == 0 && !S->comm->exchange_is_collective()) return;
        if (!stream) {
            MVS_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
            MVS_HIP(hipEventCreateWithFlags(&ev_main, hipEventDisableTiming));
            MVS_HIP(hipEventCreateWithFlags(&ev_comm, hipEventDisableTiming));
        }
        MVS_HIP(hipEventRecord(ev_main, ctx->stream));
        MVS_HIP(hipStreamWaitEvent(stream, ev_main, 0));
        // ONE pack launch (message bytes and labels of the whole phase, all peers), one grouped exchange, ONE unpack launch
        const uint64_t ms0 = S->msg_send.off[(size_t)ph * P], nms = S->msg_send.off[(size_t)(ph + 1) * P] - ms0;
        const uint64_t ns0 = S->node_send.off[(size_t)ph * P], nns = S->node_send.off[(size_t)(ph + 1) * P] - ns0;
        const uint64_t mr0 = S->msg_recv.off[(size_t)ph * P], nmr = S->msg_recv.off[(size_t)(ph + 1) * P] - mr0;
        const uint64_t nr0 = S->node_recv.off[(size_t)ph * P], nnr = S->node_recv.off[(size_t)(ph + 1) * P] - nr0;
        if (nms + nns) {
            hipLaunchKernelGGL(pack_phase_kernel, dim3(grid_for(std::max(nms, nns))), dim3(256), 0, stream, ctx->m_msg_a.p, S->msg_send.idx.p + ms0, nms, sbuf_msg.p,
                               ctx->m_lab.p, ctx->m_state.p, ctx->m_stride, S->node_send.idx.p + ns0, nns, sbuf_node.p);
            MVS_LAUNCH_CHECK();
        }
        S->comm->exchange2(sbuf_msg.p, so_m, rbuf_msg.p, ro_m, (const uint8_t*)sbuf_node.p, so_n, (uint8_t*)rbuf_node.p, ro_n, stream);
        if (nmr + nnr) {
            hipLaunchKernelGGL(unpack_phase_kernel, dim3(grid_for(std::max(nmr, nnr))), dim3(256), 0, stream, ctx->m_msg_a.p, S->msg_recv.idx.p + mr0, nmr, rbuf_msg.p,
                               ctx->m_lab.p, ctx->m_state.p, ctx->m_stride, S->node_recv.idx.p + nr0, nnr, rbuf_node.p);
            MVS_LAUNCH_CHECK();
        }
        MVS_HIP(hipEventRecord(ev_comm, stream));
        busy = true;
    }
    void sweep_energy(mvs_shard* S, int) override {
        mvs_ctx* ctx = S->ctx;
        before_phase(S, 0);   // the last phase's unpack is in (the all-reduce below runs on the main stream: one communicator, one order)
        Prof pr(ctx, "mrf_energy");
        mrf_sweep_energy_reduce(ctx, S->d_energy.p);
        if (S->P > 1) S->comm->allreduce(S->d_energy.p, 2, mvs_comm::U64, mvs_comm::SUM, ctx->stream);
        mrf_step(ctx, S->d_energy.p);
    }
    void icm_round(mvs_shard* S, int) override {
        mvs_ctx* ctx = S->ctx;
        mrf_icm_gain(ctx, S->nb, S->ne);
        if (S->P > 1) nodes(S, (uint32_t*)ctx->m_gain.p);
        mrf_icm_apply(ctx, S->nb, S->ne);
        MVS_HIP(hipMemcpyAsync(S->d_moved.p, &ctx->words->icm_n_moved, sizeof(uint32_t), hipMemcpyDeviceToDevice, ctx->stream));
        if (S->P > 1) { S->comm->allreduce(S->d_moved.p, 1, mvs_comm::U32, mvs_comm::SUM, ctx->stream); nodes(S, ctx->b_lab); }
    }
    // gains, or labels of the best labeling (ICM; the halo labels of the argmin-unary start)
    void nodes(mvs_shard* S, uint32_t* arr) {
        hipStream_t s = S->ctx->stream;
        const int P = S->P;
        const uint64_t* so = S->all_send.bytes.data(); const uint64_t* ro = S->all_recv.bytes.data();   // peer-major lists over all phases
        if (so[P] + ro[P] == 0 && !S->comm->exchange_is_collective()) return;
        const uint64_t ns = S->all_send.total, nr = S->all_recv.total;
        if (ns) { hipLaunchKernelGGL(pack_words_kernel, dim3(grid_for(ns)), dim3(256), 0, s, arr, (const mvs_mrf_progress*)nullptr, 0u, S->all_send.idx.p, ns, sbuf_node.p); MVS_LAUNCH_CHECK(); }
        S->comm->exchange((const uint8_t*)sbuf_node.p, so, (uint8_t*)rbuf_node.p, ro, s);
        if (nr) { hipLaunchKernelGGL(unpack_words_kernel, dim3(grid_for(nr)), dim3(256), 0, s, arr, (const mvs_mrf_progress*)nullptr, 0u, S->all_recv.idx.p, nr, rbuf_node.p); MVS_LAUNCH_CHECK(); }
    }
};

// Stores straight into the neighbours' arrays, ordered by stream events (see PeerHub)
struct PeerPush : Transport {
    DBuf<const unsigned long long*> e_tab;   // device table of the ranks' published energy pairs (read by the step kernel)
    DBuf<unsigned long long> e_pub;          // [parity][2] this rank's share of a sweep's energy pair
    DBuf<uint32_t> m_pub;                    // [parity] this rank's ICM "moved" count
    uint64_t n_ev = 0; uint32_t ev_ring = 0; // events recorded in this solve, size of the rank's event ring
    std::vector<int> nbr;                    // the ranks this one shares a cut with
    uint64_t phases_pushed = 0;              // over all solves
    // start of a solve: every rank publishes where its halo lives (after mrf_setup and the plan, so the pointers are final), learns its
    // neighbours (ranks it shares any cut edge with) and checks that both ends of every (phase, pair) chunk agree on its size
    void start(mvs_shard* S) override {
        mvs_ctx* ctx = S->ctx; mvs_comm* comm = S->comm; PeerHub& H = *comm->peers();
        const int P = S->P, me = S->me; const uint32_t C = S->phases;
        e_pub.ensure(4);
        MVS_HIP(hipMemsetAsync(e_pub.p, 0, 4 * sizeof(unsigned long long), ctx->stream));
        MVS_HIP(hipStreamSynchronize(ctx->stream));     // set-up, plan and the zeroed messages are in place before any peer may store into them
        comm->barrier();                                // nobody still uses the previous solve's slots or events
        PeerSlot& mine = H.slot[me];
        mine.msg = ctx->m_msg_a.p; mine.lab = ctx->m_lab.p; mine.stride = ctx->m_stride; mine.phases = C;
        mine.msg_recv_idx = S->msg_recv.idx.p; mine.node_recv_idx = S->node_recv.idx.p;
        mine.msg_recv_off = S->msg_recv.off.data(); mine.node_recv_off = S->node_recv.off.data(); mine.msg_send_off = S->msg_send.off.data();
        mine.energy = e_pub.p;
        const uint32_t ring = 2u * std::max<uint32_t>(C, 1u) + 2u;     // a rank is never more than one sweep ahead of a rank that waits for it
        while (mine.ev.size() < ring) { hipEvent_t e; MVS_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming)); mine.ev.push_back(e); }
        ev_ring = ring; n_ev = 0;
        H.recorded[me].store(0, std::memory_order_release);
        comm->barrier();
        nbr.clear();
        for (int q = 0; q < P; ++q) {
            if (q == me) continue;
            const PeerSlot& o = H.slot[q];
            if (o.phases != C) throw HipError("peer push: the ranks disagree on the number of colour phases");
            uint64_t traffic = 0;
            for (uint32_t ph = 0; ph < C; ++ph) {
                const size_t a = (size_t)ph * P;
                const uint64_t sm = S->msg_send.off[a + q + 1] - S->msg_send.off[a + q], rm = o.msg_recv_off[a + me + 1] - o.msg_recv_off[a + me];
                const uint64_t sn = S->node_send.off[a + q + 1] - S->node_send.off[a + q], rn = o.node_recv_off[a + me + 1] - o.node_recv_off[a + me];
                if (sm != rm || sn != rn) throw HipError("peer push: send / receive sizes disagree");
                traffic += sm + sn + (o.msg_send_off[a + me + 1] - o.msg_send_off[a + me]);
            }
            if (traffic) nbr.push_back(q);
        }
        std::vector<const unsigned long long*> tab((size_t)P);
        for (int q = 0; q < P; ++q) tab[q] = H.slot[q].energy;
        e_tab.ensure((size_t)P + 1);
        MVS_HIP(hipMemcpyAsync(e_tab.p, tab.data(), (size_t)P * sizeof(tab[0]), hipMemcpyHostToDevice, ctx->stream));
        MVS_HIP(hipStreamSynchronize(ctx->stream));
    }
    void before_phase(mvs_shard* S, uint32_t ph) override {
        if (ph == 0) return;   // (phase 0: the all-rank wait of the last sweep's energy)
        Prof pr(S->ctx, "mrf_halo");
        for (int q : nbr) wait(S, q, n_ev - 1);   // the neighbours' runs of the previous phase are in place
    }
    // this rank's boundary runs and labels of the phase, stored at their places in the neighbours' arrays
    void after_boundary(mvs_shard* S, uint32_t ph) override {
        mvs_ctx* ctx = S->ctx; hipStream_t s = ctx->stream; PeerHub& H = *S->comm->peers();
        Prof pr(ctx, "mrf_halo");
        const int P = S->P, me = S->me; const size_t a = (size_t)ph * P;
        PushArgs args; int n = 0; uint64_t longest = 0;
        auto flush = [&]() {
            if (!n) return;
            const unsigned gx = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((longest + 255) / 256, 256));
            hipLaunchKernelGGL(push_phase_kernel, dim3(gx, (unsigned)n), dim3(256), 0, s, ctx->m_msg_a.p, ctx->m_lab.p, ctx->m_state.p, ctx->m_stride, args);
            MVS_LAUNCH_CHECK();
            n = 0; longest = 0;
        };
        for (int q : nbr) {
            const uint64_t sm = S->msg_send.off[a + q + 1] - S->msg_send.off[a + q], sn = S->node_send.off[a + q + 1] - S->node_send.off[a + q];
            if (sm + sn == 0) continue;
            const PeerSlot& o = H.slot[q];
            PushSeg& g = args.seg[n++];
            g.sidx = S->msg_send.idx.p + S->msg_send.off[a + q]; g.didx = o.msg_recv_idx + o.msg_recv_off[a + me]; g.dmsg = o.msg; g.nm = (uint32_t)sm;
            g.nsidx = S->node_send.idx.p + S->node_send.off[a + q]; g.ndidx = o.node_recv_idx + o.node_recv_off[a + me]; g.dlab = o.lab; g.nn = (uint32_t)sn; g.dstride = o.stride;
            longest = std::max(longest, std::max(sm, sn));
            if (n == PUSH_SEGS) flush();
        }
        flush();
        if (ph + 1 < S->phases) record(S);
    }
    // the rank's pair next to its peers' (written by the reduction itself), one event behind the last phase's push AND the pair; the step
    // kernel of every rank sums all of them: TWO launches per sweep.  The wait for ALL ranks is also what lets the next sweep's first phase
    // start (and store into its neighbours)
    void sweep_energy(mvs_shard* S, int sweep) override {
        mvs_ctx* ctx = S->ctx;
        Prof pr(ctx, "mrf_energy");
        const uint32_t parity = (uint32_t)(sweep & 1);
        mrf_sweep_energy_reduce(ctx, e_pub.p + 2 * parity);
        const uint64_t idx = record(S);
        for (int q = 0; q < S->P; ++q) if (q != S->me) wait(S, q, idx);
        mrf_step(ctx, nullptr, e_tab.p, (uint32_t)S->P, 2u * parity);
    }
    // gains of the boundary nodes into the neighbours' arrays; the winners move once the neighbours' gains are in; labels of the boundary
    // nodes and the rank's "moved" count behind ONE event that every rank waits for (apply only tests halo labels against 0, which no move
    // changes: a neighbour's label store may overlap it); the counts are summed on the device
    void icm_round(mvs_shard* S, int k) override {
        mvs_ctx* ctx = S->ctx; hipStream_t s = ctx->stream; PeerHub& H = *S->comm->peers();
        if (k == 0) {   // where this rank's halo gains / labels live (the best labeling's buffer is known only after the sweeps)
            m_pub.ensure(4);
            MVS_HIP(hipMemsetAsync(m_pub.p, 0, 4 * sizeof(uint32_t), s));
            MVS_HIP(hipStreamSynchronize(s));
            PeerSlot& mine = H.slot[S->me];
            mine.gain = (uint32_t*)ctx->m_gain.p; mine.blab = ctx->b_lab; mine.moved = m_pub.p;
            mine.all_recv_idx = S->all_recv.idx.p; mine.all_recv_off = S->all_recv.off.data();
            S->comm->barrier();
            for (int q : nbr) {
                const PeerSlot& o = H.slot[q];
                if (S->all_send.off[q + 1] - S->all_send.off[q] != o.all_recv_off[S->me + 1] - o.all_recv_off[S->me]) throw HipError("peer push: send / receive sizes disagree (ICM)");
            }
        }
        mrf_icm_gain(ctx, S->nb, S->ne);
        push_nodes(S, (const uint32_t*)ctx->m_gain.p, false);
        const uint64_t ig = record(S);
        for (int q : nbr) wait(S, q, ig);
        mrf_icm_apply(ctx, S->nb, S->ne);
        push_nodes(S, ctx->b_lab, true);
        const uint32_t parity = (uint32_t)(k & 1);
        hipLaunchKernelGGL(publish_word_kernel, dim3(1), dim3(64), 0, s, (const uint32_t*)&ctx->words->icm_n_moved, m_pub.p, parity); MVS_LAUNCH_CHECK();
        const uint64_t im = record(S);
        WordPtrs wp; wp.n = S->P;
        for (int q = 0; q < S->P; ++q) { if (q != S->me) wait(S, q, im); wp.p[q] = H.slot[q].moved; }
        hipLaunchKernelGGL(sum_words_kernel, dim3(1), dim3(64), 0, s, wp, parity, S->d_moved.p); MVS_LAUNCH_CHECK();
    }
    void finish(mvs_shard* S, int sweeps) override {
        MVS_HIP(hipStreamSynchronize(S->ctx->stream)); S->comm->barrier();   // every rank's stores into this rank have landed
        phases_pushed += (uint64_t)sweeps * S->phases;
    }
    // every boundary node's word of `src` (this rank's gains, or its labels of the best labeling) to its place in the neighbours' arrays
    void push_nodes(mvs_shard* S, const uint32_t* src, bool labels) {
        hipStream_t s = S->ctx->stream; PeerHub& H = *S->comm->peers();
        PushWArgs args; int n = 0; uint64_t longest = 0;
        auto flush = [&]() {
            if (!n) return;
            const unsigned gx = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((longest + 255) / 256, 256));
            hipLaunchKernelGGL(push_words_kernel, dim3(gx, (unsigned)n), dim3(256), 0, s, src, args); MVS_LAUNCH_CHECK();
            n = 0; longest = 0;
        };
        for (int q : nbr) {
            const uint64_t cnt = S->all_send.off[q + 1] - S->all_send.off[q];
            if (!cnt) continue;
            const PeerSlot& o = H.slot[q];
            PushWSeg& g = args.seg[n++];
            g.sidx = S->all_send.idx.p + S->all_send.off[q]; g.didx = o.all_recv_idx + o.all_recv_off[S->me]; g.dst = labels ? o.blab : o.gain; g.n = (uint32_t)cnt;
            longest = std::max(longest, cnt);
            if (n == PUSH_SEGS) flush();
        }
        flush();
    }
    // one event behind everything this rank queued so far; its index (the same on every rank: one event per colour phase) is returned
    uint64_t record(mvs_shard* S) {
        PeerHub& H = *S->comm->peers();
        const uint64_t idx = n_ev++;
        MVS_HIP(hipEventRecord(H.slot[S->me].ev[idx % ev_ring], S->ctx->stream));
        H.recorded[S->me].store(idx + 1, std::memory_order_release);
        return idx;
    }
    // this rank's stream waits for event `idx` of rank q; the host only waits until q has RECORDED it (so that the stream wait refers to that record)
    void wait(mvs_shard* S, int q, uint64_t idx) {
        PeerHub& H = *S->comm->peers();
        const auto t0 = std::chrono::steady_clock::now();
        for (uint32_t spin = 0; H.recorded[q].load(std::memory_order_acquire) <= idx; ++spin) {
            if ((spin & 255u) == 255u) {
                if (S->comm->aborted()) throw HipError("peer push: another rank failed");
                if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(120)) throw HipError("peer push: a rank did not reach its next colour phase within 120 s");
                if ((spin & 4095u) == 4095u) std::this_thread::yield();
            }
        }
        MVS_HIP(hipStreamWaitEvent(S->ctx->stream, H.slot[q].ev[idx % ev_ring], 0));
    }
};

}  // namespace

namespace mvs {

std::unique_ptr<Transport> make_exchange() { return std::unique_ptr<Transport>(new Exchange); }
std::unique_ptr<Transport> make_peer_push() { return std::unique_ptr<Transport>(new PeerPush); }
void exchange_reserve(mvs_shard* S) { static_cast<Exchange&>(*S->xch).reserve(S); }
void exchange_nodes(mvs_shard* S, uint32_t* arr) { static_cast<Exchange&>(*S->xch).nodes(S, arr); }
void peer_push_info(const mvs_shard* S, uint64_t* phases_pushed, int* neighbours) {
    const PeerPush& push = static_cast<const PeerPush&>(*S->push);
    if (phases_pushed) *phases_pushed = push.phases_pushed;
    if (neighbours) *neighbours = (int)push.nbr.size();
}

}  // namespace mvs
