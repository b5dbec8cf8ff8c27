// oneshot.hip -- the entry points that make, borrow or park a context of their own: the host-pointer drop-ins for
// tex::calculate_data_costs / tex::view_selection (mvs_data_costs, its streamed forms, mvs_view_selection, mvs_view_selection_cached)
// with the stash that keeps the table on the device between them (stash.h) and the table's fingerprint, and the two calls that work
// on a temporary context (mvs_undistort_image, mvs_postprocess_face_infos).
#include "ctx.h"
#include "stash.h"

#include <chrono>
#include <cstdio>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

using namespace mvs;

namespace {
Stash<mvs_ctx> g_stash(mvs_ctx_destroy);
TableShape shape_of(const mvs_ctx* c) { return TableShape{c->csr_faces, c->csr_views, c->csr_nnz}; }
// where a solve leaves its context: the next one-shot call starts from its buffers
void park_spare_or_destroy(mvs_ctx* ctx, bool park) { if (park) g_stash.park_spare(ctx); else mvs_ctx_destroy(ctx); }

thread_local std::string g_call_profile = "{}";
double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
inline uint64_t fp_mix(uint64_t k, uint64_t v) { return mvs_fp_mix(k, v); }   // (mvs_viewsel.h: the adapter sums the same terms over the caller's container)
// the entry / column terms of the fingerprint of a DEVICE table: per-block sums, one 64-bit atomic each (wrap-around sums: any order)
__device__ __forceinline__ unsigned long long fp_mix_dev(unsigned long long k, unsigned long long v) {   // == mvs_fp_mix (a host inline in the C header)
    unsigned long long x = (k * 0x9E3779B97F4A7C15ull) ^ (v + 0x7F4A7C15D6E8FEB8ull); x ^= x >> 29; x *= 0xBF58476D1CE4E5B9ull; x ^= x >> 32; return x;
}
__global__ void __launch_bounds__(256) fingerprint_kernel(const uint32_t* __restrict__ col_ptr, const uint16_t* __restrict__ view_id, const float* __restrict__ cost,
                                                          uint32_t F, uint64_t n, unsigned long long* __restrict__ out) {
    unsigned long long h = 0ull;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x, t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (uint64_t i = t; i < F; i += stride) h += fp_mix_dev(i, col_ptr[i + 1]);
    for (uint64_t k = t; k < n; k += stride) h += fp_mix_dev((1ull << 40) + k, ((unsigned long long)view_id[k] << 32) | __float_as_uint(cost[k]));
    for (int o = 32; o > 0; o >>= 1) h += __shfl_xor(h, o, 64);
    __shared__ unsigned long long sh[4];
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = h;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(out, sh[0] + sh[1] + sh[2] + sh[3]);
}
// order-independent 64-bit sum of per-element mixes of (position, value) over col_ptr, view ids and cost bits: chunks add up, so it threads
uint64_t csr_fingerprint(const mvs_csr* c) {
    const size_t F = c->n_faces, n = c->nnz;
    const unsigned T = (unsigned)std::max<size_t>(1, std::min<size_t>(std::min<unsigned>(16u, std::max(1u, std::thread::hardware_concurrency())), n / (1u << 20) + 1));
    std::vector<uint64_t> part(T, 0);
    auto work = [&](unsigned t) {
        uint64_t h = 0;
        for (size_t i = F * t / T; i < F * (t + 1) / T; ++i) h += fp_mix(i, c->col_ptr[i + 1]);
        const uint32_t* cb = reinterpret_cast<const uint32_t*>(c->cost);
        for (size_t k = n * t / T; k < n * (t + 1) / T; ++k) h += fp_mix((1ull << 40) + k, ((uint64_t)c->view_id[k] << 32) | cb[k]);
        part[t] = h;
    };
    std::vector<std::thread> th;
    for (unsigned t = 1; t < T; ++t) th.emplace_back(work, t);
    work(0);
    for (auto& x : th) x.join();
    uint64_t h = fp_mix(F, c->n_views) + fp_mix(n, 1);
    for (uint64_t v : part) h += v;
    return h;
}

// What the two forms of the data-cost drop-in share: the working context (from the stash, or a new one), the scene, the data costs;
// `leave(ctx)` then hands the table to the caller and says how that went (TableLeft); the context is parked with the fingerprint of what
// was handed over (stash enabled, all went well) or destroyed: a failed call leaves nothing behind, not even the older table its
// context may have been parked with.  report(c) writes the profile.
struct TableLeft { mvs_status st; uint64_t fp; double t_ready, t_done, first_chunk_ms; };   // status, fingerprint of the table handed over, when it was ready / handed over
struct DcCall { double t[4], t_parked; TableLeft left; uint32_t n_ranges; bool kept; };    // t: start, context, mesh, images
template <class Leave, class Report>
mvs_status data_costs_call(const mvs_mesh* mesh, const mvs_view* views, uint32_t n_views, const mvs_image_source* images, const mvs_settings* settings, mvs_dc_stats* stats,
                           Leave&& leave, Report&& report) {
    DcCall c; c.t[0] = now_ms();
    mvs_ctx* ctx = stash_enabled() ? g_stash.take_working() : nullptr;
    mvs_status st = MVS_OK;
    if (!ctx) st = mvs_ctx_create(default_device(), &ctx);
    if (st != MVS_OK) return st;
    c.t[1] = now_ms();
    st = mvs_scene_set_mesh(ctx, mesh, 0);
    c.t[2] = now_ms();
    if (st == MVS_OK) st = images ? mvs_scene_set_views_from(ctx, views, n_views, images) : mvs_scene_set_views(ctx, views, n_views, 0);
    c.t[3] = now_ms();
    ctx->dc_range_pairs = env_dc_range_pairs();   // (a parked context was made under whatever the variable said then)
    if (st == MVS_OK) st = mvs_ctx_data_costs(ctx, settings, stats);
    c.n_ranges = st == MVS_OK ? ctx->dc_n_ranges : 0u;
    c.left = st == MVS_OK ? leave(ctx) : TableLeft{st, 0, now_ms(), now_ms(), 0.0};
    st = c.left.st;
    c.kept = st == MVS_OK && stash_enabled();
    if (c.kept) g_stash.park_table(ctx, c.left.fp, shape_of(ctx));   // for the mvs_view_selection that follows
    c.t_parked = now_ms();
    if (!c.kept) mvs_ctx_destroy(ctx);
    report(c);
    return st;
}

// the table leaves in chunks of faces through pinned staging; its fingerprint is summed on the device
TableLeft stream_table_out(mvs_ctx* ctx, mvs_csr_chunk_fn fn, void* user, mvs_csr* shape_out) {
    TableLeft L{MVS_OK, 0, now_ms(), 0.0, 0.0};
    try {
        hipStream_t s = ctx->stream;
        const uint32_t F = ctx->csr_faces; const uint64_t nnz = ctx->csr_nnz;
        const bool reordered = table_to_caller_order(ctx, false);
        const uint32_t* d_ptr = reordered ? ctx->u_ptr.p : ctx->r_ptr; const uint16_t* d_view = reordered ? ctx->u_view.p : ctx->r_view;
        const float* d_cost = reordered ? ctx->u_cost.p : ctx->r_cost;
        // fingerprint of the table as it leaves, on the device
        ctx->fp_acc.ensure(2);
        MVS_HIP(hipMemsetAsync(ctx->fp_acc.p, 0, sizeof(unsigned long long), s));
        hipLaunchKernelGGL(fingerprint_kernel, dim3(2048), dim3(256), 0, s, d_ptr, d_view, d_cost, F, nnz, ctx->fp_acc.p); MVS_LAUNCH_CHECK();
        // pinned staging: the column offsets whole, the entries in two buffers of one chunk each
        ctx->stage_ptr.ensure((size_t)F + 2);
        unsigned long long h_fp = 0;
        MVS_HIP(hipMemcpyAsync(ctx->stage_ptr.p, d_ptr, ((size_t)F + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        MVS_HIP(hipMemcpyAsync(&h_fp, ctx->fp_acc.p, sizeof(h_fp), hipMemcpyDeviceToHost, s));
        MVS_HIP(hipStreamSynchronize(s));
        L.t_ready = now_ms();
        L.fp = fp_mix(F, ctx->csr_views) + fp_mix(nnz, 1) + (uint64_t)h_fp;
        const uint32_t* hp = ctx->stage_ptr.p;
        constexpr uint32_t CHUNK = 1u << 16;   // faces per chunk
        uint64_t max_entries = 1;
        for (uint32_t f0 = 0; f0 < F; f0 += CHUNK) max_entries = std::max<uint64_t>(max_entries, (uint64_t)hp[std::min(F, f0 + CHUNK)] - hp[f0]);
        for (int b = 0; b < 2; ++b) { ctx->stage_view[b].ensure(max_entries + 8); ctx->stage_cost[b].ensure(max_entries + 8); }
        hipEvent_t ev[2] = {nullptr, nullptr};
        for (int b = 0; b < 2; ++b) MVS_HIP(hipEventCreateWithFlags(&ev[b], hipEventDisableTiming));
        auto issue = [&](uint32_t f0, int b) {
            const uint32_t f1 = std::min(F, f0 + CHUNK); const uint64_t e0 = hp[f0], ne = (uint64_t)hp[f1] - e0;
            if (ne) {
                MVS_HIP(hipMemcpyAsync(ctx->stage_view[b].p, d_view + e0, ne * sizeof(uint16_t), hipMemcpyDeviceToHost, s));
                MVS_HIP(hipMemcpyAsync(ctx->stage_cost[b].p, d_cost + e0, ne * sizeof(float), hipMemcpyDeviceToHost, s));
            }
            MVS_HIP(hipEventRecord(ev[b], s));
        };
        try {
            if (F) issue(0, 0);
            int b = 0;
            for (uint32_t f0 = 0; f0 < F; f0 += CHUNK, b ^= 1) {
                if (f0 + CHUNK < F) issue(f0 + CHUNK, b ^ 1);        // the next chunk travels while the caller consumes this one
                MVS_HIP(hipEventSynchronize(ev[b]));
                if (f0 == 0) L.first_chunk_ms = now_ms() - L.t_ready;
                fn(user, f0, std::min(F, f0 + CHUNK) - f0, hp + f0, ctx->stage_view[b].p, ctx->stage_cost[b].p);
            }
        } catch (...) { for (int k = 0; k < 2; ++k) if (ev[k]) (void)hipEventDestroy(ev[k]); throw; }
        for (int k = 0; k < 2; ++k) (void)hipEventDestroy(ev[k]);
        if (shape_out) { memset(shape_out, 0, sizeof(*shape_out)); shape_out->n_faces = F; shape_out->n_views = ctx->csr_views; shape_out->nnz = nnz; }
    } catch (const StatusError& e) { L.st = api_fail(e.st, e.what()); }
      catch (const std::exception& e) { L.st = api_fail(MVS_ERR_HIP, e.what()); }
      catch (...) { L.st = api_fail(MVS_ERR_INVALID, "the chunk callback threw"); }   // nothing may unwind through the C ABI
    L.t_done = now_ms();
    return L;
}

mvs_status data_costs_stream_impl(const mvs_mesh* mesh, const mvs_view* views, uint32_t n_views, const mvs_image_source* images, const mvs_settings* settings,
                                  mvs_csr_chunk_fn fn, void* user, mvs_csr* shape_out, mvs_dc_stats* stats) {
    if (!mesh || !views || !settings || !fn) return api_fail(MVS_ERR_INVALID, "null argument");
    if (n_views > 65535u) return api_fail(MVS_ERR_TOO_MANY_VIEWS, "Exeeded maximal number of views");   /* calculate_data_costs.cpp:315-318 */
    return data_costs_call(mesh, views, n_views, images, settings, stats,
        [&](mvs_ctx* ctx) { return stream_table_out(ctx, fn, user, shape_out); },
        [&](const DcCall& c) {
            char buf[640];
            snprintf(buf, sizeof(buf), "{\"call\": \"mvs_data_costs_stream\", \"ctx_ms\": %.3f, \"mesh_h2d_ms\": %.3f, \"images_h2d_ms\": %.3f, \"compute_ms\": %.3f, \"first_chunk_ms\": %.3f, "
                     "\"chunks_and_callbacks_ms\": %.3f, \"fingerprint\": \"device\", \"dc_ranges\": %u, \"table_kept_on_device\": %s}",
                     c.t[1] - c.t[0], c.t[2] - c.t[1], c.t[3] - c.t[2], c.left.t_ready - c.t[3], c.left.first_chunk_ms, c.left.t_done - c.left.t_ready, c.n_ranges, c.kept ? "true" : "false");
            g_call_profile = buf;
        });
}

// make a context, run body(ctx) -- what it throws becomes the status --, destroy the context
template <class Body>
mvs_status with_temporary_context(Body&& body) {
    mvs_ctx* ctx = nullptr;
    mvs_status st = mvs_ctx_create(default_device(), &ctx);
    if (st != MVS_OK) return st;
    mvs_status inner = MVS_OK;
    st = api_guard([&] { inner = body(ctx); });
    mvs_ctx_destroy(ctx);
    return st != MVS_OK ? st : inner;
}
}  // namespace

extern "C" {

// ---------------- one-shot host drop-ins ----------------
mvs_status mvs_data_costs(const mvs_mesh* mesh, const mvs_view* views, uint32_t n_views, const mvs_settings* settings,
                          mvs_csr* out, mvs_dc_stats* stats) {
    if (!mesh || !views || !settings || !out) return api_fail(MVS_ERR_INVALID, "null argument");
    /* calculate_data_costs.cpp:315-318 */
    if (n_views > 65535u) return api_fail(MVS_ERR_TOO_MANY_VIEWS, "Exeeded maximal number of views");
    return data_costs_call(mesh, views, n_views, nullptr, settings, stats,
        [&](mvs_ctx* ctx) {   // the whole table into the caller's arrays, fingerprinted on the host
            (void)hipStreamSynchronize(ctx->stream);
            const double t_ready = now_ms();
            const mvs_status st = mvs_ctx_costs_download(ctx, out, nullptr);
            const double t_done = now_ms();
            return TableLeft{st, st == MVS_OK && stash_enabled() ? csr_fingerprint(out) : 0, t_ready, t_done, 0.0};
        },
        [&](const DcCall& c) {
            char buf[512];
            snprintf(buf, sizeof(buf), "{\"call\": \"mvs_data_costs\", \"ctx_ms\": %.3f, \"mesh_h2d_ms\": %.3f, \"images_h2d_ms\": %.3f, \"compute_ms\": %.3f, \"download_ms\": %.3f, "
                     "\"fingerprint_ms\": %.3f, \"dc_ranges\": %u, \"table_kept_on_device\": %s}",
                     c.t[1] - c.t[0], c.t[2] - c.t[1], c.t[3] - c.t[2], c.left.t_ready - c.t[3], c.left.t_done - c.left.t_ready, c.t_parked - c.left.t_done, c.n_ranges, c.kept ? "true" : "false");
            g_call_profile = buf;
        });
}
/* wall-clock breakdown (JSON object) of the last one-shot call -- mvs_data_costs / mvs_view_selection -- of the calling thread */
const char* mvs_last_call_profile(void) { return g_call_profile.c_str(); }
void mvs_release_cached(void) {
    g_stash.release_all();
    release_upload_rings();   // (a pinned upload ring is allocated again by the next host-image upload to its device)
}

/* tex::calculate_data_costs with the result streamed out in chunks of faces (see mvs_viewsel.h) */
mvs_status mvs_data_costs_stream(const mvs_mesh* mesh, const mvs_view* views, uint32_t n_views, const mvs_settings* settings,
                                 mvs_csr_chunk_fn fn, void* user, mvs_csr* shape_out, mvs_dc_stats* stats) {
    return data_costs_stream_impl(mesh, views, n_views, nullptr, settings, fn, user, shape_out, stats);
}
/* ... with the host images supplied view by view (mvs_image_source): host memory bounded by max_in_flight decoded images */
mvs_status mvs_data_costs_stream_from(const mvs_mesh* mesh, const mvs_view* views, uint32_t n_views, const mvs_image_source* images, const mvs_settings* settings,
                                      mvs_csr_chunk_fn fn, void* user, mvs_csr* shape_out, mvs_dc_stats* stats) {
    if (!images || !images->acquire || !images->release) return api_fail(MVS_ERR_INVALID, "null argument");
    return data_costs_stream_impl(mesh, views, n_views, images, settings, fn, user, shape_out, stats);
}

/* tex::view_selection on the table parked by mvs_data_costs / mvs_data_costs_stream, identified by its fingerprint (see mvs_viewsel.h) */
mvs_status mvs_view_selection_cached(uint64_t fingerprint, uint32_t n_faces, uint32_t n_views, uint64_t nnz, const uint32_t* adj_ptr, const uint32_t* adj,
                                     const mvs_mrf_params* params, uint32_t* labels_out, mvs_mrf_stats* stats) {
    if (!adj_ptr || !adj || !labels_out) return api_fail(MVS_ERR_INVALID, "null argument");
    double t[3]; t[0] = now_ms();
    mvs_ctx* ctx = stash_enabled() ? g_stash.take_table(fingerprint, TableShape{n_faces, n_views, nnz}) : nullptr;
    if (!ctx) return api_fail(MVS_ERR_STATE, "no parked table with this fingerprint");
    t[1] = now_ms();
    mvs_status st = mvs_ctx_view_selection(ctx, adj_ptr, adj, 0, params, labels_out, 0, stats);
    t[2] = now_ms();
    park_spare_or_destroy(ctx, st == MVS_OK);
    char buf[256];
    snprintf(buf, sizeof(buf), "{\"call\": \"mvs_view_selection_cached\", \"lookup_ms\": %.3f, \"solve_ms\": %.3f, \"table_reused_on_device\": true}", t[1] - t[0], t[2] - t[1]);
    g_call_profile = buf;
    return st;
}

mvs_status mvs_view_selection(const mvs_csr* costs, const uint32_t* adj_ptr, const uint32_t* adj, const mvs_mrf_params* params,
                              uint32_t* labels_out, mvs_mrf_stats* stats) {
    if (!costs || !adj_ptr || !adj || !labels_out) return api_fail(MVS_ERR_INVALID, "null argument");
    double t[4]; t[0] = now_ms();
    mvs_ctx* ctx = nullptr;
    // the table mvs_data_costs handed out (same shape, same fingerprint)?  Then it is still on the parked context's device
    const TableShape shape{costs->n_faces, costs->n_views, costs->nnz};
    if (stash_enabled() && costs->col_ptr && (costs->nnz == 0 || (costs->view_id && costs->cost)) && g_stash.shape_matches(shape))
        ctx = g_stash.take_table(csr_fingerprint(costs), shape);
    t[1] = now_ms();
    const bool reused = ctx != nullptr;
    mvs_status st = MVS_OK;
    if (!reused) {
        ctx = stash_enabled() ? g_stash.take_spare() : nullptr;
        if (!ctx) st = mvs_ctx_create(default_device(), &ctx);
        if (st != MVS_OK) return st;
        st = mvs_ctx_costs_upload(ctx, costs, 0);
    }
    t[2] = now_ms();
    if (st == MVS_OK) st = mvs_ctx_view_selection(ctx, adj_ptr, adj, 0, params, labels_out, 0, stats);
    t[3] = now_ms();
    park_spare_or_destroy(ctx, stash_enabled() && st == MVS_OK);
    char buf[384];
    snprintf(buf, sizeof(buf), "{\"call\": \"mvs_view_selection\", \"fingerprint_ms\": %.3f, \"ctx_and_table_upload_ms\": %.3f, \"solve_ms\": %.3f, \"table_reused_on_device\": %s}",
             t[1] - t[0], t[2] - t[1], t[3] - t[2], reused ? "true" : "false");
    g_call_profile = buf;
    return st;
}

// ---------------- the calls on a temporary context ----------------
/* the undistortion step of from_images_and_camera_files (generate_texture_views.cpp:153-165) */
mvs_status mvs_undistort_image(const uint8_t* rgb, int32_t width, int32_t height, float flen, float dist0, float dist1, uint8_t* out) {
    if (!rgb || !out || width < 1 || height < 1) return api_fail(MVS_ERR_INVALID, "bad argument");
    const size_t bytes = (size_t)width * height * 3;
    if (dist0 == 0.0f) { memcpy(out, rgb, bytes); return MVS_OK; }        /* :153 -- only a non-zero first coefficient undistorts */
    if (!(flen > 0.0f)) return api_fail(MVS_ERR_INVALID, "undistortion needs a positive focal length");
    return with_temporary_context([&](mvs_ctx* ctx) {
        DBuf<uint8_t> a, b; a.ensure(bytes + 16); b.ensure(bytes + 16);
        MVS_HIP(hipMemcpyAsync(a.p, rgb, bytes, hipMemcpyHostToDevice, ctx->stream));
        undistort_image(ctx, a.p, b.p, width, height, (double)flen, (double)dist0, (double)dist1);
        MVS_HIP(hipMemcpyAsync(out, b.p, bytes, hipMemcpyDeviceToHost, ctx->stream));
        MVS_HIP(hipStreamSynchronize(ctx->stream));
        return MVS_OK;
    });
}

/* tex::postprocess_face_infos (texturing.h:71-74; calculate_data_costs.cpp:253-306) */
mvs_status mvs_postprocess_face_infos(uint32_t n_faces, uint32_t n_views, const uint32_t* info_ptr, const uint16_t* view_id, const float* quality,
                                      const float* mean_color, const mvs_settings* settings, mvs_csr* out, mvs_dc_stats* stats) {
    if (!info_ptr || !settings || !out) return api_fail(MVS_ERR_INVALID, "null argument");
    const size_t n = info_ptr[n_faces];
    if (n && (!view_id || !quality)) return api_fail(MVS_ERR_INVALID, "null argument");
    if (settings->outlier_removal != MVS_OUTLIER_NONE && n && !mean_color) return api_fail(MVS_ERR_INVALID, "outlier removal needs the mean colours");
    for (uint32_t i = 0; i < n_faces; ++i) if (info_ptr[i + 1] < info_ptr[i]) return api_fail(MVS_ERR_INVALID, "info_ptr must ascend");
    for (size_t k = 0; k < n; ++k) if (view_id[k] >= n_views) return api_fail(MVS_ERR_INVALID, "view id out of range");
    return with_temporary_context([&](mvs_ctx* ctx) {
        // every face's list reversed (see dc_postprocess)
        std::vector<uint16_t> rv(n + 1); std::vector<float> rq(n + 1), rc(mean_color ? 3 * n + 3 : 3);
        for (uint32_t i = 0; i < n_faces; ++i) {
            const size_t a = info_ptr[i], b = info_ptr[i + 1];
            for (size_t k = a; k < b; ++k) {
                const size_t d = a + (b - 1 - k);
                rv[d] = view_id[k]; rq[d] = quality[k];
                if (mean_color) { rc[3 * d] = mean_color[3 * k]; rc[3 * d + 1] = mean_color[3 * k + 1]; rc[3 * d + 2] = mean_color[3 * k + 2]; }
            }
        }
        dc_postprocess(ctx, n_faces, n_views, info_ptr, rv.data(), rq.data(), rc.data(), settings);
        dc_phase2(ctx);
        dc_phase3(ctx, stats);
        return mvs_ctx_costs_download(ctx, out, nullptr);
    });
}

}  // extern "C"
