// shard.hip -- the sharded view-selection path in the product's host language (C++): one rank per GPU, RCCL over
// xGMI for the halo exchange.  tex::calculate_data_costs + tex::view_selection over a face partition:
//
//   * faces are cut into `world` contiguous parts (the caller renumbers them along a space-filling curve); rank r evaluates
//     the (face, view) pairs of its part against the replicated scene, the global barrier of postprocess_face_infos
//     (calculate_data_costs.cpp:278-288) is one all-reduce MAX of a float and one all-reduce SUM of the 10001 histogram words;
//   * the cost table stays sharded: global shape, only the own columns and the halo columns (faces of other parts adjacent to
//     own faces) filled -- column lengths travel by all-gather, halo columns by a neighbour exchange;
//   * MRF: every rank sweeps its own nodes, colour phase by colour phase; after phase c the runs written in that phase
//     over cut edges (as BYTES: the messages are 8-bit codes) and the labels of the boundary nodes of colour c go to the
//     neighbouring ranks -- grouped ncclSend / ncclRecv to actual neighbours only, one group per phase; per sweep one
//     all-reduce of the energy pair feeds the device-side stop rule, so no rank ever waits on the host for a sweep's energy;
//   * the halo plan (which runs, which nodes, in which order) is built ON THE DEVICE from the adjacency, the partition, the
//     colouring and the rank's own message layout: both ends of a pair enumerate a (peer, phase) chunk by ascending global
//     directed-edge index / node id, so no index ever travels.
//
// A phase's nodes read only nodes of other colours, which were exchanged before: labels are bit-identical for any number of parts.
//
// Two communicators behind one interface: RCCL (resolved with dlopen at run time, so the library carries no link-time
// dependency and shares whatever RCCL the process already loaded, e.g. PyTorch's) and an in-process one for `world` host threads
// whose devices address each other's memory.  It decides the sweep loop's halo transport: in-process ranks push, RCCL ranks exchange.
//
// This file holds the shard object's life and the two entry points as sequences of steps -- every rank makes the same communicator
// calls in the same order, and here is where that order reads top to bottom.  The rest by concern: comm.h / comm.hip (the
// communicators), shard_table.hip (the sharded table: the steps of mvs_shard_data_costs), shard_plan.hip (the halo plan),
// shard_transport.hip (the two transports), shard_lists.h (the lists' host arithmetic); shard.h is what they share.
#include "shard.h"

using namespace mvs;

namespace {

// bnd[i] = 1 for an own node with an edge into another rank's part (a BOUNDARY node: its runs / label travel); everybody else 0
__global__ void boundary_mark_kernel(const uint32_t* __restrict__ adj_ptr, const uint32_t* __restrict__ adj, Parts parts, int me, uint32_t nb, uint32_t ne, uint8_t* __restrict__ bnd) {
    const uint32_t i = nb + blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ne) return;
    uint8_t b = 0;
    for (uint32_t e = adj_ptr[i]; e < adj_ptr[i + 1]; ++e) if (part_of(parts, adj[e]) != me) b = 1;
    bnd[i] = b;
}
__global__ void iota_from_kernel(uint32_t* __restrict__ v, uint32_t first, uint32_t n) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) v[k] = first + k;
}

// ---- the steps of mvs_shard_view_selection ----
// the solver's tables, with the boundary marks and -- from the second solve on -- the kept colouring
void setup_with_marks(mvs_shard* S, const mvs_mrf_params& P) {
    mvs_ctx* ctx = S->ctx; hipStream_t s = ctx->stream;
    set_adjacency(ctx, S->d_adj_ptr, S->d_adj, 1, /*table_order=*/true);
    Prof pr(ctx, "mrf_setup");
    struct Marks { mvs_ctx* c; ~Marks() { c->m_bnd = nullptr; c->m_colour_in = nullptr; } } marks{ctx};   // the set-up is the only reader: no pointer into this shard stays behind
    ctx->m_bnd = S->P > 1 ? S->bnd.p : nullptr;
    ctx->m_colour_in = S->colours_valid ? S->colours.p : nullptr;
    mrf_setup(ctx, &P);
    if (!S->colours_valid && S->F) {
        S->colours.ensure((size_t)S->F + 2);
        MVS_HIP(hipMemcpyAsync(S->colours.p, ctx->m_colour.p, (size_t)S->F * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
        S->colours_valid = true;
    }
}
// the halo plan follows from adjacency, partition, colouring and the message layout, i.e. from the column lengths: kept while
// mvs_shard_data_costs found them unchanged (the layout's size is checked as well)
void plan_or_reuse(mvs_shard* S) {
    mvs_ctx* ctx = S->ctx; hipStream_t s = ctx->stream;
    if (!S->plan_valid || S->plan_colours != ctx->m_colours || S->plan_total != ctx->m_total) {
        Prof pr(ctx, "mrf_plan");
        hipEvent_t e0, e1; MVS_HIP(hipEventCreate(&e0)); MVS_HIP(hipEventCreate(&e1)); MVS_HIP(hipEventRecord(e0, s));
        build_plan(S);
        exchange_reserve(S);
        S->d_energy.ensure(4); S->d_moved.ensure(4);
        MVS_HIP(hipEventRecord(e1, s)); MVS_HIP(hipEventSynchronize(e1));
        float ms = 0.0f; MVS_HIP(hipEventElapsedTime(&ms, e0, e1)); S->plan_ms = ms;
        (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
        S->plan_valid = S->tables_valid; S->plan_colours = ctx->m_colours; S->plan_total = ctx->m_total; ++S->plans_built;
    } else { S->plan_ms = 0.0; ++S->plans_reused; }
}
// The transport follows from the communicator: ranks that can address each other's memory (the in-process communicator) store
// into each other's arrays, RCCL ranks exchange.  Every rank takes the same route: the colour phases are those of one global colouring.
Transport& choose_transport(mvs_shard* S) {
    Transport& T = S->P > 1 && S->comm->peers() && S->phases > 0 ? *S->push : *S->xch;
    S->route = &T;
    return T;
}
// the sweeps, until the device-side stop rule says so or max_sweeps are queued; returns the sweeps issued, pg = the last report
int sweep_loop(mvs_shard* S, Transport& T, int max_sweeps, mvs_mrf_progress& pg) {
    mvs_ctx* ctx = S->ctx; const uint32_t nb = S->nb, ne = S->ne;
    const int lag = std::max(0, std::min(std::max(ctx->mrf_lag, 2), (int)mvs_ctx::RING - 2));
    memset(&pg, 0, sizeof(pg));
    int issued = 0, polled = 0;
    // A colour phase: BOUNDARY nodes first, their runs and labels leave, then the INTERIOR -- whose nodes have no neighbour on another rank,
    // so their launch neither waits for a peer nor reads anything a peer stores; the hand-over of phase c has the whole interior launch of
    // phase c to land before this rank's boundary nodes of colour c + 1 need it.  (A colour class is an independent set: same values.)
    const bool split = S->P > 1;
    while (issued < max_sweeps && !pg.stopped) {
        for (uint32_t ph = 0; ph < S->phases; ++ph) {
            T.before_phase(S, ph);
            if (!split) { Prof pr(ctx, "mrf_sweep"); mrf_sweep_phase(ctx, ph, nb, ne, MRF_PART_ALL); continue; }
            { Prof pr(ctx, "mrf_sweep_boundary"); mrf_sweep_phase(ctx, ph, nb, ne, MRF_PART_BOUNDARY); }
            T.after_boundary(S, ph);
            { Prof pr(ctx, "mrf_sweep"); mrf_sweep_phase(ctx, ph, nb, ne, MRF_PART_INTERIOR); }
        }
        // the sweep's energy: own share (accumulated by the sweep kernels), summed over the ranks, fed to the device-side stop rule --
        // the host polls the report of `lag` sweeps ago
        T.sweep_energy(S, issued);
        ++issued;
        if (issued - lag > polled) mrf_poll(ctx, (uint32_t)++polled, &pg);
    }
    while (polled < issued && !pg.stopped) mrf_poll(ctx, (uint32_t)++polled, &pg);
    if (issued > 0) mrf_poll(ctx, (uint32_t)issued, &pg);
    T.finish(S, issued);
    return issued;
}
// the best labeling's buffers; without a sweep it is the argmin-unary start, whose halo labels no phase has carried yet
void best_labeling(mvs_shard* S, int issued) {
    resolve_best(S->ctx);
    if (S->P > 1 && issued == 0) exchange_nodes(S, S->ctx->b_lab);
}
// ICM rounds: gains of the own nodes, gains of the boundary nodes to the neighbours, winners move, labels of the boundary nodes
// to the neighbours; the all-reduced "moved" count of a round reaches the host through the pinned ring two rounds late (as in
// the single-context polish: icm_rounds), so no round waits for a read-back.  Every rank reads the same counts at the same
// round indices, hence takes the same decisions; a round queued after the one that moved nothing finds no positive gain anywhere.
int polish(mvs_shard* S, Transport& T, int icm_iters) {
    mvs_ctx* ctx = S->ctx;
    mrf_exact_costs(ctx, S->nb, S->ne);
    return icm_rounds(ctx, icm_iters, S->d_moved.p, [&](int k) { T.icm_round(S, k); });
}
// two words of this rank summed over the ranks, on the host: copy, all-reduce where there are peers, read back
template <class W>
void sum_pair_over_ranks(mvs_shard* S, const W* d_src, W* d_buf, W out[2]) {
    hipStream_t s = S->ctx->stream;
    MVS_HIP(hipMemcpyAsync(d_buf, d_src, 2 * sizeof(W), hipMemcpyDeviceToDevice, s));
    if (S->P > 1) S->comm->allreduce(d_buf, 2, sizeof(W) == 8 ? mvs_comm::U64 : mvs_comm::U32, mvs_comm::SUM, s);
    MVS_HIP(hipMemcpyAsync(out, d_buf, 2 * sizeof(W), hipMemcpyDeviceToHost, s));
    MVS_HIP(hipStreamSynchronize(s));
}

}  // namespace

extern "C" {

mvs_status mvs_shard_create(mvs_ctx* ctx, mvs_comm* comm, const uint32_t* part_begin, const uint32_t* adj_ptr_device, const uint32_t* adj_device, mvs_shard** out) {
    if (!ctx || !comm || !adj_ptr_device || !adj_device || !out) return api_fail(MVS_ERR_INVALID, "null argument");
    *out = nullptr;
    MVS_API_BEGIN
    MVS_HIP(hipSetDevice(ctx->device));
    if (!ctx->d_verts || !ctx->d_faces) throw StatusError(MVS_ERR_STATE, "the context needs the full mesh (mvs_scene_set_mesh) before a shard is made of it");
    // peers store into this rank's arrays through the peer access the communicator set up between ITS devices
    if (comm->device() >= 0 && comm->device() != ctx->device)
        throw StatusError(MVS_ERR_INVALID, "rank " + std::to_string(comm->rank) + " of this communicator drives device " + std::to_string(comm->device()) + ", the context lives on device " + std::to_string(ctx->device));
    std::unique_ptr<mvs_shard> S(new mvs_shard); S->ctx = ctx; S->comm = comm; S->me = comm->rank; S->P = comm->world;
    S->xch = make_exchange(); S->push = make_peer_push();
    S->parts.n = S->P;
    S->F = ctx->n_faces;
    // The parts are contiguous ranges of the LIBRARY's face order (k_bvh.hip build_scene_order: a Hilbert curve over the face
    // centroids, derived identically by every rank from the replicated mesh): compact patches, short cuts -- whatever order the
    // caller's mesh file has.  part_begin == null: `world` equal parts.
    for (int q = 0; q <= S->P; ++q) {
        S->parts.b[q] = part_begin ? part_begin[q] : (uint32_t)(((uint64_t)S->F * (uint64_t)q) / (uint64_t)S->P);
        if (q && S->parts.b[q] < S->parts.b[q - 1]) throw StatusError(MVS_ERR_INVALID, "part_begin must ascend");
    }
    if (S->parts.b[0] != 0 || S->parts.b[S->P] != S->F) throw StatusError(MVS_ERR_INVALID, "the partition must cover the mesh of the context");
    S->nb = S->parts.b[S->me]; S->ne = S->parts.b[S->me + 1];
    MVS_HIP(hipMemcpyAsync(&S->E, adj_ptr_device + S->F, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    MVS_HIP(hipStreamSynchronize(ctx->stream));
    // the caller's adjacency lists (its own face numbering) once into the library's order, list order kept
    build_scene_order(ctx); (void)scene_order_commit(ctx);
    if (ctx->mesh_ordered) {
        renumber_adjacency(ctx, S->F, ctx->f_perm.p, ctx->f_pos.p, adj_ptr_device, adj_device, S->E, S->own_adj_ptr, S->own_adj);
        MVS_HIP(hipStreamSynchronize(ctx->stream));
        S->d_adj_ptr = S->own_adj_ptr.p; S->d_adj = S->own_adj.p;
    } else { S->d_adj_ptr = adj_ptr_device; S->d_adj = adj_device; }   // option "face_order" = 0: the caller's numbering is the order
    // The shard IS this layout (parts, renumbered lists, later the halo plan): the context keeps it for the shard's data-cost passes
    // instead of deriving the same order from the same mesh in every step; mvs_scene_set_mesh (another mesh) un-pins it.
    ctx->order_pinned = true;
    S->bnd.ensure((size_t)S->F + 4);
    MVS_HIP(hipMemsetAsync(S->bnd.p, 0, (size_t)S->F + 4, ctx->stream));
    if (S->ne > S->nb && S->P > 1) {
        hipLaunchKernelGGL(boundary_mark_kernel, dim3((S->ne - S->nb + 255) / 256), dim3(256), 0, ctx->stream, S->d_adj_ptr, S->d_adj, S->parts, S->me, S->nb, S->ne, S->bnd.p);
        MVS_LAUNCH_CHECK();
    }
    MVS_HIP(hipStreamSynchronize(ctx->stream));
    *out = S.release();
    MVS_API_END
}

/* the caller's ids of the faces this rank owns (positions part_begin[rank] .. of the library's order), in the order of the labels
 * mvs_shard_view_selection returns */
mvs_status mvs_shard_own_faces(mvs_shard* S, uint32_t* ids_device, uint32_t* n_own) {
    if (!S) return api_fail(MVS_ERR_INVALID, "null argument");
    if (n_own) *n_own = S->ne - S->nb;
    if (!ids_device) return MVS_OK;
    MVS_API_BEGIN
    mvs_ctx* ctx = S->ctx;
    MVS_HIP(hipSetDevice(ctx->device));
    const uint32_t n = S->ne - S->nb;
    if (n) {
        if (ctx->mesh_ordered) MVS_HIP(hipMemcpyAsync(ids_device, ctx->f_perm.p + S->nb, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToDevice, ctx->stream));
        else { hipLaunchKernelGGL(iota_from_kernel, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, ids_device, S->nb, n); MVS_LAUNCH_CHECK(); }
        MVS_HIP(hipStreamSynchronize(ctx->stream));
    }
    MVS_API_END
}

void mvs_shard_destroy(mvs_shard* shard) {
    if (!shard) return;
    // the context's active table may point into this shard's buffers (mvs_shard_data_costs): no dangling pointers behind
    mvs_ctx* ctx = shard->ctx;
    if (ctx) ctx->order_pinned = false;
    if (ctx && (ctx->r_ptr == shard->t_ptr.p || ctx->r_view == shard->t_view.p || ctx->r_cost == shard->t_cost.p)) {
        (void)hipStreamSynchronize(ctx->stream);
        ctx->have_costs = false; ctx->dc_phase = 0; ctx->csr_q_valid = false;
        ctx->r_ptr = ctx->csr_ptr.p; ctx->r_view = ctx->csr_view.p; ctx->r_cost = ctx->csr_cost.p;
    }
    delete shard;
}

/* tex::calculate_data_costs over all ranks (calculate_data_costs.cpp:308-323): afterwards the context holds the cost table
 * of the GLOBAL shape with the own and the halo columns filled */
mvs_status mvs_shard_data_costs(mvs_shard* S, const mvs_settings* settings, mvs_dc_stats* stats, uint64_t* nnz_global) {
    if (!S) return api_fail(MVS_ERR_INVALID, "null argument");
    MVS_API_BEGIN
    S->comm->begin_call();   // every call is numbered on every rank -- also one that fails its own argument checks below
    try {   // (a failure on this rank ends the other ranks' host-side waits of this call: mvs_comm::fail)
    if (!settings) throw StatusError(MVS_ERR_INVALID, "null argument");
    MVS_HIP(hipSetDevice(S->ctx->device));
    RoctxRange range("Calculating data costs");   /* texrecon.cpp:118 */
    const uint64_t nnz_own = shard_costs_over_ranks(S, settings, stats);
    shard_gather_lengths(S);
    if (!shard_lengths_unchanged(S, nnz_global)) shard_rebuild_tables(S);
    shard_fill_table(S, nnz_own);
    shard_activate_table(S);
    } catch (...) { S->comm->fail(); throw; }
    MVS_API_END
}

/* tex::view_selection over all ranks (view_selection.cpp:18-133): labels of the own nodes into labels_own_device */
mvs_status mvs_shard_view_selection(mvs_shard* S, const mvs_mrf_params* params, uint32_t* labels_own_device, mvs_mrf_stats* stats) {
    if (!S) return api_fail(MVS_ERR_INVALID, "null argument");
    MVS_API_BEGIN
    S->comm->begin_call();
    try {
    if (!labels_own_device) throw StatusError(MVS_ERR_INVALID, "null argument");
    if (!S->ctx->have_costs) throw StatusError(MVS_ERR_STATE, "view selection needs data costs (mvs_shard_data_costs)");   // (e.g. this rank's data costs failed: its peers are released)
    mvs_ctx* ctx = S->ctx;
    MVS_HIP(hipSetDevice(ctx->device));
    RoctxRange range("Running MRF optimization");   /* texrecon.cpp:126 */
    mvs_mrf_params P; if (params) P = *params; else mvs_mrf_default_params(&P);
    if (P.region_rounds > 0) throw StatusError(MVS_ERR_UNSUPPORTED, "region moves (region_rounds > 0) are a single-context option");
    mvs_mrf_stats R; memset(&R, 0, sizeof(R));
    setup_with_marks(S, P);
    plan_or_reuse(S);
    Transport& T = choose_transport(S);
    T.start(S);
    mvs_mrf_progress pg;
    const int issued = sweep_loop(S, T, P.max_sweeps, pg);
    R.sweeps = issued > 0 ? pg.stop_sweep : 0u;
    best_labeling(S, issued);
    R.icm_iters = (uint32_t)polish(S, T, P.icm_iters);
    mrf_energy(ctx, true, S->nb, S->ne, true);
    unsigned long long e[2];
    sum_pair_over_ranks(S, ctx->m_energy.p, S->d_energy.p, e);
    R.energy_fixed = e[0]; R.energy = (double)e[0] / 4294967296.0; R.cut_edges = e[1];
    uint32_t bu[2];
    mrf_labels(ctx, S->nb, S->ne, labels_own_device, bu);
    sum_pair_over_ranks(S, &ctx->words->labels_bad, S->d_moved.p, bu);
    R.unseen = bu[1];
    if (stats) *stats = R;
    if (bu[0]) throw StatusError(MVS_ERR_LABELING, "Incorrect labeling");  /* view_selection.cpp:126-128 */
    } catch (...) { S->comm->fail(); throw; }
    MVS_API_END
}

mvs_status mvs_shard_plan_info(mvs_shard* S, uint64_t* msg_bytes_per_sweep, uint64_t* boundary_nodes, double* plan_ms) {
    if (!S) return api_fail(MVS_ERR_INVALID, "null argument");
    if (msg_bytes_per_sweep) *msg_bytes_per_sweep = S->msg_send.total;
    if (boundary_nodes) *boundary_nodes = S->node_send.total;
    if (plan_ms) *plan_ms = S->plan_ms;
    return MVS_OK;
}

mvs_status mvs_shard_transport_info(mvs_shard* S, int* peer_push, uint64_t* phases_pushed, int* neighbours, uint32_t* colour_phases) {
    if (!S) return api_fail(MVS_ERR_INVALID, "null argument");
    if (peer_push) *peer_push = S->route == S->push.get() ? 1 : 0;
    peer_push_info(S, phases_pushed, neighbours);
    if (colour_phases) *colour_phases = S->phases;
    return MVS_OK;
}

}  // extern "C"
