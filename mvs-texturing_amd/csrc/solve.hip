// solve.hip -- the solver's host loop on one context (mvs_ctx_view_selection): sweeps with the device-side stop rule, replayed from a
// hipGraph after the first damping period, exact costs, ICM polish, region moves, labels; and the solver's diagnostics.  (The sharded
// loop is shard.hip sweep_loop: it differs in transport, lag and graph use.)
#include "ctx.h"

#include <algorithm>
#include <cstdio>
#include <cstring>

using namespace mvs;

// the executable graph of the sweep loop and its capture stream (mvs_ctx_destroy)
namespace mvs { void sweep_graph_release(mvs_ctx* ctx) { if (ctx->sweep_exec) (void)hipGraphExecDestroy(ctx->sweep_exec); if (ctx->cap_stream) (void)hipStreamDestroy(ctx->cap_stream); } }

// Captures n_sweeps sweeps + steps (whatever `one_sweep` launches) on the context's private capture stream and makes ctx->sweep_exec
// launch exactly that.  The capture executes nothing; host-side counters the launches advance are restored.  The graph is
// re-captured for every solve (a dozen launches into a capturing stream) and pushed into the existing executable graph with
// hipGraphExecUpdate; only a changed topology (another number of node classes per colour) instantiates a new one.
// Returns false -- the caller then keeps launching directly -- if the runtime refuses any step.
template <class Sweep>
static bool prepare_sweep_graph(mvs_ctx* ctx, Sweep&& one_sweep, int n_sweeps) {
    if (!ctx->cap_stream && hipStreamCreateWithFlags(&ctx->cap_stream, hipStreamNonBlocking) != hipSuccess) { (void)hipGetLastError(); ctx->mrf_graph = 0; return false; }
    const uint32_t steps0 = ctx->steps_issued, sweep0 = ctx->m_sweep_no, phase0 = ctx->m_last_phase;
    hipStream_t user = ctx->stream;
    hipGraph_t graph = nullptr;
    bool ok = hipStreamBeginCapture(ctx->cap_stream, hipStreamCaptureModeThreadLocal) == hipSuccess;
    if (ok) {
        ctx->stream = ctx->cap_stream;
        try { for (int k = 0; k < n_sweeps; ++k) one_sweep(); } catch (...) { ok = false; }
        ctx->stream = user;
        if (hipStreamEndCapture(ctx->cap_stream, &graph) != hipSuccess || !graph) ok = false;
    }
    ctx->steps_issued = steps0; ctx->m_sweep_no = sweep0; ctx->m_last_phase = phase0;
    if (ok && ctx->sweep_exec) {
        hipGraphNode_t bad = nullptr; hipGraphExecUpdateResult res = hipGraphExecUpdateError;
        if (hipGraphExecUpdate(ctx->sweep_exec, graph, &bad, &res) == hipSuccess && res == hipGraphExecUpdateSuccess) ++ctx->graph_updates;
        else { (void)hipGetLastError(); (void)hipGraphExecDestroy(ctx->sweep_exec); ctx->sweep_exec = nullptr; }
    }
    if (ok && !ctx->sweep_exec) {
        if (hipGraphInstantiate(&ctx->sweep_exec, graph, nullptr, nullptr, 0) == hipSuccess) ++ctx->graph_instantiations;
        else { ctx->sweep_exec = nullptr; ok = false; }
    }
    if (graph) (void)hipGraphDestroy(graph);
    if (!ok) { (void)hipGetLastError(); ctx->mrf_graph = 0; if (ctx->verbose) fprintf(stderr, "[mvs] hipGraph capture of the sweep loop failed: launching directly\n"); }
    return ok;
}

static void read_energy(mvs_ctx* ctx, uint64_t out[2]) {
    unsigned long long h[2];
    read_words(ctx, ctx->m_energy.p, h, 4);
    out[0] = h[0]; out[1] = h[1];
}

// The solver's host loop (single GPU): sweeps with exact-energy tracking, the
// stop rule mirroring StopWhenReturnsDiminish (view_selection.cpp:84), ICM polish.
// ICM polish of the best labeling (whole graph): rounds of gain + apply (see icm_rounds)
static int icm_polish(mvs_ctx* ctx, uint32_t F, int max_iters) {
    return icm_rounds(ctx, max_iters, &ctx->words->icm_n_moved, [&](int) {
        mrf_icm_gain(ctx, 0, F);
        mrf_icm_apply(ctx, 0, F);   // in place: winners form an independent set
    });
}

extern "C" {

mvs_status mvs_ctx_view_selection(mvs_ctx* ctx, const uint32_t* adj_ptr, const uint32_t* adj, int adj_on_device,
                                  const mvs_mrf_params* params, uint32_t* labels_out, int labels_on_device, mvs_mrf_stats* stats) {
    if (!ctx || !adj_ptr || !adj || !labels_out) return api_fail(MVS_ERR_INVALID, "null argument");
    if (!ctx->have_costs) return api_fail(MVS_ERR_STATE, "view selection needs data costs (mvs_ctx_data_costs or mvs_ctx_costs_upload)");
    MVS_CTX_API_BEGIN
    RoctxRange range("Running MRF optimization");   /* texrecon.cpp:126 */
    mvs_mrf_params P; if (params) P = *params; else mvs_mrf_default_params(&P);
    const uint32_t F = ctx->csr_faces;
    { Prof pr(ctx, "mrf_setup"); set_adjacency(ctx, adj_ptr, adj, adj_on_device, false); mrf_setup(ctx, &P); }
    hipStream_t s = ctx->stream;
    mvs_mrf_stats S; memset(&S, 0, sizeof(S));
    // The stop rule runs on the device (mrf_step); the host only polls the report of `lag` sweeps ago, so the next
    // sweep is already queued when a sweep's energy becomes known.  Sweeps issued after the rule fired are no-ops
    // for the result (the best labeling is frozen on the device).
    // reports outstanding at any time: lag + 2 with direct launches, up to lag + 2 GS under graph replay (a graph issues GS steps before
    // the host polls, and one more graph stays queued behind it): the ring of RING slots must hold them all
    // sweeps per graph = one period of the damping schedule (a damped sweep and three undamped ones)
    constexpr int GS = (int)MRF_DAMP_PERIOD;
    const int lag = std::max(0, std::min(ctx->mrf_lag, (int)mvs_ctx::RING - 2 * GS - 1));
    mvs_mrf_progress pg; memset(&pg, 0, sizeof(pg));
    auto report = [&](uint32_t n) {
        mrf_poll(ctx, n, &pg);
        if (ctx->verbose) fprintf(stderr, "[mvs] sweep %u tracking energy %.3f best %.3f%s\n", n, (double)pg.energy / 65535.0, (double)pg.best / 65535.0, pg.stopped ? " (stopped)" : "");
    };
    int issued = 0, polled = 0;
    ProfChain pc(ctx);
    auto one_sweep = [&]() {
        pc.begin();
        mrf_sweep(ctx, 0, F);
        pc.mark("mrf_sweep");
        // the sweep kernels accumulate the sweep's energy themselves; the step kernel sums their partials and applies the stop rule
        if (!ctx->m_energy_from_sweep) mrf_energy(ctx, false, 0, F, /*reduce=*/false);
        mrf_step(ctx, nullptr);
        pc.mark("mrf_energy");
    };
    // Sweeps 1 .. 4 are launched directly.  From sweep 5 on the loop replays a hipGraph of one damping period, FOUR sweeps (a damped
    // one, three undamped ones), with their steps: a small problem's sweep is a handful of 3 - 10 us kernels, and launching them one by one is bound by
    // the host's ~3.5 us per launch (MI355X_MICROARCH.md "graph-replay-floor"), not by the GPU.  Every launch of the loop has
    // the same arguments each time (the step kernel numbers its reports itself), sweeps queued after the device-side stop rule fired
    // end at their first instruction, so replaying past the stop costs microseconds.  Not while profiling (stage marks are events).
    bool graphs = ctx->mrf_graph != 0 && !ctx->profile && P.max_sweeps >= 3 * GS && F > 0;
    while (issued < std::min(GS, P.max_sweeps) && !pg.stopped) {
        one_sweep(); ++issued;
        if (issued - lag > polled) report((uint32_t)++polled);
    }
    if (graphs && issued == GS && !pg.stopped) graphs = prepare_sweep_graph(ctx, one_sweep, GS);
    while (issued < P.max_sweeps && !pg.stopped) {
        if (graphs && issued + GS <= P.max_sweeps) {
            MVS_HIP(hipGraphLaunch(ctx->sweep_exec, s));
            ctx->steps_issued += (uint32_t)GS; ctx->m_sweep_no += (uint32_t)GS; issued += GS; ++ctx->graph_launches;
            best_labeling_may_have_changed(ctx);
            // one whole graph stays queued behind the one whose reports are read
            while (issued - lag - GS > polled && !pg.stopped) report((uint32_t)++polled);
        } else {
            one_sweep(); ++issued;
            if (issued - lag > polled) report((uint32_t)++polled);
        }
    }
    while (polled < issued && !pg.stopped) report((uint32_t)++polled);
    if (issued > 0) mrf_poll(ctx, (uint32_t)issued, &pg);   // final state (drains the stream)
    S.sweeps = issued > 0 ? pg.stop_sweep : 0u;   // max_sweeps <= 0: best labeling = the argmin-unary start state of mrf_setup
    // the sweeps track energies of the 16-bit unaries they stream; from here on (polish, reported energy) the exact costs count
    mrf_exact_costs(ctx, 0, F);
    int it = icm_polish(ctx, F, P.icm_iters);
    S.icm_iters = (uint32_t)it;
    /* region moves (off by default), each round followed by a fresh polish -- the control flow the oracle defines */
    for (int r = 0; r < P.region_rounds; ++r) {
        const uint32_t m = mrf_region_round(ctx);
        if (m == 0) break;
        S.region_rounds++; S.region_moves += m;
        it = icm_polish(ctx, F, P.icm_iters);
        S.icm_iters += (uint32_t)std::min(it + 1, P.icm_iters);   // rounds run, including the one that found nothing to move
    }
    mrf_energy(ctx, true, 0, F);
    uint64_t e[2]; read_energy(ctx, e);
    S.energy_fixed = e[0]; S.energy = (double)e[0] / 4294967296.0; S.cut_edges = e[1];
    uint32_t* d_labels = labels_on_device ? labels_out : ctx->m_cand.p;
    uint32_t bu[2];
    mrf_labels(ctx, 0, F, d_labels, bu, /*caller_order=*/true);
    S.unseen = bu[1];
    if (bu[0]) throw StatusError(MVS_ERR_LABELING, "Incorrect labeling");  /* view_selection.cpp:126-128 */
    if (!labels_on_device && F) {
        MVS_HIP(hipMemcpyAsync(labels_out, d_labels, (size_t)F * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        MVS_HIP(hipStreamSynchronize(s));
    }
    if (stats) *stats = S;
    MVS_API_END
}

/* colour phases of the solver's schedule / diagnostics of the last solves of this context (mvs_viewsel.h) */
mvs_status mvs_ctx_mrf_num_phases(mvs_ctx* ctx, uint32_t* n_phases) {
    if (!ctx || !n_phases) return api_fail(MVS_ERR_INVALID, "null argument");
    *n_phases = ctx->m_colours;
    return MVS_OK;
}
mvs_status mvs_ctx_mrf_diagnostics(mvs_ctx* ctx, uint32_t out[4]) {
    if (!ctx || !out) return api_fail(MVS_ERR_INVALID, "null argument");
    out[0] = ctx->graph_launches; out[1] = ctx->graph_updates; out[2] = ctx->graph_instantiations; out[3] = ctx->csr_faces - ctx->m_n_fast;
    return MVS_OK;
}

}  // extern "C"
