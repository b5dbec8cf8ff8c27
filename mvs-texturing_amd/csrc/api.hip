// api.hip -- the context-level part of the C ABI of include/mvs_viewsel.h: the error string, roctx ranges, context create / destroy /
// options / profile, mesh and views (host images through the pinned upload ring), the data-cost phases, table download / upload, the
// adjacency hand-over and the wrappers of the .spt / .vec files (spt_io.h).  The solver's host loop is solve.hip; the calls that bring
// their own context -- the host-pointer drop-ins for tex::calculate_data_costs / tex::view_selection -- are oneshot.hip.
#include "view_input.h"
#include "spt_io.h"

#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

using namespace mvs;

static thread_local std::string g_last_error;

namespace mvs { mvs_status api_fail(mvs_status st, const std::string& msg) { g_last_error = msg; return st; } }

#include <dlfcn.h>
namespace mvs {
namespace {
struct Roctx { int (*push)(const char*) = nullptr; int (*pop)() = nullptr; };
const Roctx& roctx() {
    static Roctx R;
    static std::once_flag once;
    std::call_once(once, [] {
        const char* e = getenv("MVS_ROCTX");
        if (e && e[0] == '0') return;
        void* h = nullptr;
        for (const char* name : {"libroctx64.so.4", "libroctx64.so", "/opt/rocm/lib/libroctx64.so.4"}) { h = dlopen(name, RTLD_NOW | RTLD_GLOBAL); if (h) break; }
        if (!h) return;
        R.push = reinterpret_cast<int (*)(const char*)>(dlsym(h, "roctxRangePushA"));
        R.pop = reinterpret_cast<int (*)()>(dlsym(h, "roctxRangePop"));
        if (!R.push || !R.pop) { R.push = nullptr; R.pop = nullptr; }
    });
    return R;
}
}  // namespace
RoctxRange::RoctxRange(const char* name) : on(false) { const Roctx& R = roctx(); if (R.push) { (void)R.push(name); on = true; } }
RoctxRange::~RoctxRange() { if (on) (void)roctx().pop(); }
int default_device() { const char* e = getenv("MVS_DEVICE"); return e ? std::max(0, atoi(e)) : 0; }
// MVS_DC_RANGE_PAIRS (0 when unset): read where a context is made and again by every one-shot call, whose contexts outlive the call
uint64_t env_dc_range_pairs() { const char* e = getenv("MVS_DC_RANGE_PAIRS"); return e ? (uint64_t)std::max(0ll, atoll(e)) : 0ull; }
}  // namespace mvs

static float compute_cos_limit() {
    const float c = host_cos_limit();  // dmath.h
    if (!(c == c)) throw StatusError(MVS_ERR_UNSUPPORTED, "host acosf is not monotone around cos(75 deg)");
    return c;
}

namespace mvs {
// The adjacency lists arrive in the caller's numbering (UniGraph, uni_graph.h:22).  A table that lives in the library's own order
// (ctx->t_perm; k_order.hip) gets them renumbered on the device, list order kept; `table_order` = the lists already are in the
// table's order (the sharded driver renumbers once for all its calls).
void set_adjacency(mvs_ctx* ctx, const uint32_t* adj_ptr, const uint32_t* adj, int on_device, bool table_order) {
    const size_t F = ctx->csr_faces;
    if (ctx->t_perm && !ctx->t_pos && !table_order)
        throw StatusError(MVS_ERR_STATE, "the active table covers a face range of the library's order: view selection needs the table of the whole mesh (or option face_order = 0)");
    const bool renumber = ctx->t_perm != nullptr && !table_order;
    if (on_device && !renumber) { ctx->r_adj_ptr = adj_ptr; ctx->r_adj = adj; ctx->r_adj_edges_known = false; return; }
    size_t E = 0;
    if (on_device) {
        uint32_t e32 = 0;
        MVS_HIP(hipMemcpyAsync(&e32, adj_ptr + F, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
        MVS_HIP(hipStreamSynchronize(ctx->stream));
        E = e32;
    } else E = adj_ptr[F];
    const uint32_t* d_ptr = adj_ptr; const uint32_t* d_adj = adj;
    if (!on_device) {
        DBuf<uint32_t>& sp = renumber ? ctx->a_stage_ptr : ctx->m_adj_ptr; DBuf<uint32_t>& sa = renumber ? ctx->a_stage : ctx->m_adj;
        sp.ensure(F + 2); sa.ensure(E + 1);
        MVS_HIP(hipMemcpyAsync(sp.p, adj_ptr, (F + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
        if (E) MVS_HIP(hipMemcpyAsync(sa.p, adj, E * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
        MVS_HIP(hipStreamSynchronize(ctx->stream));
        d_ptr = sp.p; d_adj = sa.p;
    }
    if (renumber) adjacency_to_table_order(ctx, d_ptr, d_adj, E);
    ctx->r_adj_ptr = ctx->m_adj_ptr.p; ctx->r_adj = ctx->m_adj.p;
    ctx->r_adj_edges = (uint32_t)E; ctx->r_adj_edges_known = true;   // (mrf_setup need not read it back again)
}
}  // namespace mvs

// ---- host images -> device through a ring of library-owned pinned buffers (mvs_scene_set_views) ----
namespace {
enum class UploadRoute { Ring, Register, Pageable };
UploadRoute upload_route() {
    if (const char* e = getenv("MVS_HOST_UPLOAD")) {
        if (!strcmp(e, "register")) return UploadRoute::Register;
        if (!strcmp(e, "pageable")) return UploadRoute::Pageable;
        return UploadRoute::Ring;
    }
    if (const char* e = getenv("MVS_PIN_HOST_IMAGES")) return e[0] == '0' ? UploadRoute::Pageable : UploadRoute::Register;
    return UploadRoute::Ring;
}
struct UploadPiece { const uint8_t* src; uint8_t* dst; size_t bytes; };
// One ring per device and process (an upload holds its mutex: uploads to one device share one PCIe link anyway): two pinned slots of
// SLOT bytes per copy thread, an event per slot.
struct UploadRing {
    // 16 MB per copy: at 4 MB the per-copy overhead of the runtime showed (42.7 GB/s whatever the thread count, against 52.5 GB/s for copies
    // from caller pages pinned in place, BASELINE config 3's 1.89 GB of images; profiles/EXPERIMENTS.md round 5)
    static constexpr size_t SLOT = 16u << 20; static constexpr unsigned MAX_THREADS = 8, SLOTS = 2 * MAX_THREADS;
    std::mutex m; uint8_t* buf[SLOTS] = {}; hipEvent_t ev[SLOTS] = {}; bool used[SLOTS] = {};
    void ensure(unsigned slots) {
        for (unsigned k = 0; k < slots; ++k) {
            if (!buf[k]) MVS_HIP(hipHostMalloc((void**)&buf[k], SLOT, hipHostMallocPortable));
            if (!ev[k]) MVS_HIP(hipEventCreateWithFlags(&ev[k], hipEventDisableTiming));
        }
    }
    void release() {
        std::lock_guard<std::mutex> lock(m);
        for (unsigned k = 0; k < SLOTS; ++k) { if (ev[k]) (void)hipEventDestroy(ev[k]); if (buf[k]) (void)hipHostFree(buf[k]); ev[k] = nullptr; buf[k] = nullptr; used[k] = false; }
    }
};
constexpr int RING_DEVICES = 16;
UploadRing g_ring[RING_DEVICES];
}  // namespace
namespace mvs { void release_upload_rings() { for (auto& r : g_ring) r.release(); } }
namespace {
unsigned upload_threads() {
    if (const char* e = getenv("MVS_UPLOAD_THREADS")) return (unsigned)std::max(1, std::min(atoi(e), (int)UploadRing::MAX_THREADS));
    return std::max(1u, std::min(UploadRing::MAX_THREADS, std::thread::hardware_concurrency() / 2));
}
// The images are cut into SLOT-sized chunks; copy thread t takes the chunks t, t + T, ... and alternates between its two slots: wait
// until the slot's previous copy has left it (its event), fill it from the caller's pageable memory, queue the slot's copy to the
// device and the event behind it.  No thread waits for another one: while the copy engine drains one slot of a thread the thread
// fills its other slot, and T threads keep T copies in flight.  (Copies of different chunks write different ranges: their order on
// the stream does not matter; the stream is drained before the function returns.)
void upload_through_ring(mvs_ctx* ctx, const std::vector<UploadPiece>& pieces) {
    if (ctx->device < 0 || ctx->device >= RING_DEVICES) throw StatusError(MVS_ERR_UNSUPPORTED, "upload ring: device index out of range");
    UploadRing& R = g_ring[ctx->device];
    std::lock_guard<std::mutex> lock(R.m);
    struct Chunk { const uint8_t* src; uint8_t* dst; size_t n; };
    std::vector<Chunk> chunks;
    for (const UploadPiece& p : pieces) for (size_t o = 0; o < p.bytes; o += UploadRing::SLOT) chunks.push_back(Chunk{p.src + o, p.dst + o, std::min(UploadRing::SLOT, p.bytes - o)});
    const unsigned T = (unsigned)std::max<size_t>(1, std::min<size_t>(upload_threads(), chunks.size()));
    R.ensure(2 * T);
    hipStream_t s = ctx->stream; const int device = ctx->device;
    struct Drain { hipStream_t s; UploadRing& R; ~Drain() { (void)hipStreamSynchronize(s); for (bool& u : R.used) u = false; } } drain{s, R};   // no copy still reads a slot when the lock is released
    std::mutex em; std::string error; std::atomic<bool> failed{false};
    auto work = [&](unsigned t) {
        try {
            MVS_HIP(hipSetDevice(device));
            unsigned turn = 0;
            for (size_t c = t; c < chunks.size() && !failed.load(std::memory_order_relaxed); c += T, turn ^= 1u) {
                const unsigned k = 2 * t + turn;
                if (R.used[k]) MVS_HIP(hipEventSynchronize(R.ev[k]));
                memcpy(R.buf[k], chunks[c].src, chunks[c].n);
                MVS_HIP(hipMemcpyAsync(chunks[c].dst, R.buf[k], chunks[c].n, hipMemcpyHostToDevice, s));
                MVS_HIP(hipEventRecord(R.ev[k], s));
                R.used[k] = true;
            }
        } catch (const std::exception& e) { failed.store(true); std::lock_guard<std::mutex> l(em); if (error.empty()) error = e.what(); }
    };
    // (a thread that cannot be started -- EAGAIN -- must not take the process down with joinable threads in a dying vector: the guard joins
    //  whatever was started, the chunks of the missing threads are copied by this one)
    struct Joiner { std::vector<std::thread> th; ~Joiner() { for (auto& x : th) if (x.joinable()) x.join(); } } pool;
    pool.th.reserve(T);
    std::vector<unsigned> mine{0u};
    for (unsigned t = 1; t < T; ++t) {
        try { pool.th.emplace_back(work, t); } catch (const std::system_error&) { mine.push_back(t); }
    }
    for (unsigned t : mine) work(t);
    for (auto& x : pool.th) x.join();
    if (failed.load()) throw HipError("image upload: " + error);
}
}  // namespace
namespace mvs {
void upload_pieces_through_ring(mvs_ctx* ctx, const uint8_t* const* src, uint8_t* const* dst, const size_t* bytes, size_t n) {
    std::vector<UploadPiece> pieces;
    for (size_t k = 0; k < n; ++k) if (bytes[k]) pieces.push_back(UploadPiece{src[k], dst[k], bytes[k]});
    if (!pieces.empty()) upload_through_ring(ctx, pieces);
}
}  // namespace mvs

extern "C" {

const char* mvs_last_error(void) { return g_last_error.c_str(); }

const char* mvs_status_string(mvs_status s) {
    switch (s) {
        case MVS_OK: return "ok";
        case MVS_ERR_INVALID: return "invalid argument";
        case MVS_ERR_TOO_MANY_FACES: return "Exeeded maximal number of faces";
        case MVS_ERR_TOO_MANY_VIEWS: return "Exeeded maximal number of views";
        case MVS_ERR_LABELING: return "Incorrect labeling";
        case MVS_ERR_HIP: return "HIP error";
        case MVS_ERR_STATE: return "invalid call order";
        case MVS_ERR_UNSUPPORTED: return "unsupported";
    }
    return "?";
}

void mvs_mrf_default_params(mvs_mrf_params* p) {
    p->max_sweeps = 200; p->min_sweeps = 20; p->window = 5; p->min_improvement = 0.005f;
    p->damping = 0.2f; p->rho = 0.8f; p->icm_iters = 50; p->region_rounds = 0;
}
void mvs_default_settings(mvs_settings* s) {  /* settings.h:85-90 */
    s->data_term = MVS_DATA_TERM_GMI; s->outlier_removal = MVS_OUTLIER_NONE; s->geometric_visibility_test = 1;
}

mvs_status mvs_ctx_create(int device, mvs_ctx** out) {
    if (!out) return api_fail(MVS_ERR_INVALID, "out is null");
    *out = nullptr;
    MVS_API_BEGIN
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) throw HipError("no HIP device available (this library has no CPU fallback)");
    if (device < 0 || device >= n) throw StatusError(MVS_ERR_INVALID, "bad device index");
    MVS_HIP(hipSetDevice(device));
    mvs_ctx* c = new mvs_ctx;
    c->device = device;
    MVS_HIP(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    c->own_stream = true;
    c->cos_limit = compute_cos_limit();
    // MVS_INFO_WAVE_AREA overrides the default footprint area above which the lane-group sampler takes over (0: every
    // footprint in the reference's serial fp64 order, i.e. bit-exact qualities); mvs_set_option("info_wave_area") still wins
    if (const char* e = getenv("MVS_INFO_WAVE_AREA")) c->info_wave_area = std::max(0, atoi(e));
    // MVS_DC_RANGE_PAIRS: the option "dc_range_pairs" for the one-shot entry points and the link-time drop-in (mvs_set_option still wins)
    c->dc_range_pairs = env_dc_range_pairs();
    if (const char* e = getenv("MVS_BVH_UPPER_MIN_FACES")) c->bvh_upper_min_faces = (uint32_t)std::max(0ll, atoll(e));   // (test runs: 0 puts every mesh of the suite through the upper levels of the face order)
    c->counters.ensure(64);
    MVS_HIP(hipMalloc((void**)&c->words, sizeof(SolverWords)));
    MVS_HIP(hipMemset(c->words, 0, sizeof(SolverWords)));
    *out = c;
    MVS_API_END
}

void mvs_ctx_destroy(mvs_ctx* ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    for (auto* b : ctx->own_rgb) delete b;
    mvs::gsl_release(ctx); mvs::texpatch_release(ctx); mvs::lsl_release(ctx); mvs::atlas_release(ctx); mvs::model_release(ctx); mvs::debug_release(ctx); mvs::glb_release(ctx); mvs::png_release(ctx); mvs::jpeg_release(ctx); mvs::jpegdec_release(ctx); mvs::pngdec_release(ctx); mvs::lens_release(ctx); mvs::level_release(ctx); mvs::viewmask_release(ctx);
    mvs::sweep_graph_release(ctx);
    if (ctx->aux_stream) { (void)hipStreamSynchronize(ctx->aux_stream); (void)hipStreamDestroy(ctx->aux_stream); }
    if (ctx->ev_fork) (void)hipEventDestroy(ctx->ev_fork);
    if (ctx->ev_join) (void)hipEventDestroy(ctx->ev_join);
    if (ctx->words) (void)hipFree(ctx->words);
    if (ctx->h_kd_flags) (void)hipHostFree(ctx->h_kd_flags);
    if (ctx->h_icm) (void)hipHostFree(ctx->h_icm);
    if (ctx->h_rb) (void)hipHostFree(ctx->h_rb);
    if (ctx->h_seq) (void)hipHostFree(ctx->h_seq);
    if (ctx->h_ring) (void)hipHostFree(ctx->h_ring);
    if (ctx->own_stream && ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

mvs_status mvs_ctx_set_stream(mvs_ctx* ctx, void* hip_stream) {
    if (!ctx) return api_fail(MVS_ERR_INVALID, "ctx is null");
    MVS_API_BEGIN
    MVS_HIP(hipStreamSynchronize(ctx->stream));
    if (ctx->own_stream && ctx->stream) MVS_HIP(hipStreamDestroy(ctx->stream));
    // NULL is a valid handle: the (legacy) default stream, which is what torch.cuda.current_stream() is
    // unless the caller switched streams
    ctx->stream = (hipStream_t)hip_stream; ctx->own_stream = false;
    MVS_API_END
}

mvs_status mvs_ctx_synchronize(mvs_ctx* ctx) {
    if (!ctx) return api_fail(MVS_ERR_INVALID, "ctx is null");
    MVS_API_BEGIN
    MVS_HIP(hipStreamSynchronize(ctx->stream));
    MVS_API_END
}

mvs_status mvs_set_option(mvs_ctx* ctx, const char* name, int64_t value) {
    if (!ctx || !name) return api_fail(MVS_ERR_INVALID, "null argument");
    const std::string n(name);
    if (n == "count_rays") ctx->count_rays = value != 0;
    else if (n == "stats") ctx->stats = value != 0;
    else if (n == "verbose") ctx->verbose = value != 0;
    else if (n == "info_wave_area") ctx->info_wave_area = (int)std::max<int64_t>(0, std::min<int64_t>(value, 1 << 30));
    else if (n == "info_wave_area_words") ctx->info_wave_area_words = (int)std::max<int64_t>(1, std::min<int64_t>(value, 1 << 30));
    else if (n == "info_words") ctx->info_words = value != 0;
    else if (n == "info_cert_shift") ctx->info_cert_shift = (int)std::max<int64_t>(0, std::min<int64_t>(value, 40));
    else if (n == "max_labels") { if (value < 0 || value > 65535) return api_fail(MVS_ERR_INVALID, "max_labels: 0 (off) .. 65535"); ctx->max_labels = (int)value; }
    else if (n == "dc_range_pairs") { if (value < 0) return api_fail(MVS_ERR_INVALID, "dc_range_pairs: 0 (one range) or the (face, view) pairs of a range"); ctx->dc_range_pairs = (uint64_t)value; }
    else if (n == "profile") ctx->profile = value != 0;
    else if (n == "prep_fused") ctx->prep_fused = value != 0;
    else if (n == "ray_xcd") ctx->ray_xcd = (int)value;
    else if (n == "mrf_xcd") ctx->mrf_xcd = (int)value;
    else if (n == "mrf_lag") ctx->mrf_lag = (int)value;
    else if (n == "mrf_force_generic") ctx->mrf_force_generic = value != 0;
    else if (n == "mrf_force_lists") ctx->mrf_force_lists = value != 0;
    else if (n == "mrf_graph") ctx->mrf_graph = value != 0;
    else if (n == "mrf_blocks_per_cu") ctx->mrf_blocks_per_cu = std::max(0, (int)value);
    else if (n == "bvh_upper_min_faces") { ctx->kd_disabled = false; ctx->bvh_upper_min_faces = (uint32_t)std::max<int64_t>(0, std::min<int64_t>(value, 0xFFFFFFFFll)); ctx->order_pinned = false; }
    else if (n == "bvh_window") { ctx->kd_disabled = false; ctx->bvh_window = (uint32_t)std::max<int64_t>(0, std::min<int64_t>(value, 0x40000000)); ctx->order_pinned = false; }   // 0 = whole mesh, 1 = no upper-level cuts; otherwise rounded up to a power of two by the builder
    else if (n == "jpegdec_subseq_bytes") { if (value < 16 || value > 128 || value % 4) return api_fail(MVS_ERR_INVALID, "jpegdec_subseq_bytes: a multiple of 4 in 16 .. 128"); ctx->jpegdec_subseq = (uint32_t)value; }
    else if (n == "face_order") { ctx->face_order = value != 0 ? 1 : 0; ctx->order_pinned = false; }   // takes effect with the next data-cost pass (the active table keeps the order it was made in)
    else return api_fail(MVS_ERR_INVALID, "unknown option " + n);
    return MVS_OK;
}

// JSON object {"stage": [total_ms, count], ...} of the spans recorded since the last call
mvs_status mvs_ctx_get_profile(mvs_ctx* ctx, char* buf, size_t buf_size) {
    if (!ctx || !buf || buf_size < 3) return api_fail(MVS_ERR_INVALID, "null argument");
    MVS_API_BEGIN
    MVS_HIP(hipStreamSynchronize(ctx->stream));
    std::vector<std::string> names; std::vector<double> ms; std::vector<int> cnt;
    for (auto& sp : ctx->prof_spans) {
        float t = 0.0f;
        MVS_HIP(hipEventElapsedTime(&t, sp.a, sp.b));
        size_t k = 0;
        for (; k < names.size(); ++k) if (names[k] == sp.name) break;
        if (k == names.size()) { names.push_back(sp.name); ms.push_back(0.0); cnt.push_back(0); }
        ms[k] += t; cnt[k] += 1;
        if (sp.owns_a) ctx->prof_pool.push_back(sp.a);
        ctx->prof_pool.push_back(sp.b);
    }
    ctx->prof_spans.clear();
    std::string out = "{";
    for (size_t k = 0; k < names.size(); ++k) {
        char tmp[160];
        snprintf(tmp, sizeof(tmp), "%s\"%s\": [%.6f, %d]", k ? ", " : "", names[k].c_str(), ms[k], cnt[k]);
        out += tmp;
    }
    out += "}";
    if (out.size() + 1 > buf_size) throw StatusError(MVS_ERR_INVALID, "profile buffer too small");
    memcpy(buf, out.c_str(), out.size() + 1);
    MVS_API_END
}

mvs_status mvs_scene_set_mesh(mvs_ctx* ctx, const mvs_mesh* mesh, int on_device) {
    if (!ctx || !mesh || !mesh->verts || !mesh->faces || !mesh->face_normals) return api_fail(MVS_ERR_INVALID, "null argument");
    MVS_CTX_API_BEGIN
    const size_t NV = mesh->n_verts, F = mesh->n_faces;
    if (on_device) {
        ctx->d_verts = mesh->verts; ctx->d_faces = mesh->faces; ctx->d_normals = mesh->face_normals;
    } else {
        ctx->own_verts.ensure(3 * NV + 4); ctx->own_faces.ensure(3 * F + 4); ctx->own_normals.ensure(3 * F + 4);
        MVS_HIP(hipMemcpyAsync(ctx->own_verts.p, mesh->verts, 3 * NV * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
        MVS_HIP(hipMemcpyAsync(ctx->own_faces.p, mesh->faces, 3 * F * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
        MVS_HIP(hipMemcpyAsync(ctx->own_normals.p, mesh->face_normals, 3 * F * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
        MVS_HIP(hipStreamSynchronize(ctx->stream));
        ctx->d_verts = ctx->own_verts.p; ctx->d_faces = ctx->own_faces.p; ctx->d_normals = ctx->own_normals.p;
    }
    ctx->n_verts = mesh->n_verts; ctx->n_faces = mesh->n_faces;
    ctx->face_begin = 0; ctx->face_end = mesh->n_faces;
    ctx->have_costs = false; ctx->dc_phase = 0;
    ctx->order_pinned = false; ctx->iv = nullptr; ctx->kd_disabled = false; ctx->kd_pending = 0;   // another mesh: whatever layout a shard pinned is gone
    MVS_API_END
}

static mvs_status set_views_impl(mvs_ctx* ctx, const mvs_view* views, uint32_t n_views, int rgb_on_device, const mvs_image_source* src);
mvs_status mvs_scene_set_views(mvs_ctx* ctx, const mvs_view* views, uint32_t n_views, int rgb_on_device) { return set_views_impl(ctx, views, n_views, rgb_on_device, nullptr); }
/* the same with host images that exist only while they are needed: see mvs_image_source in the header */
mvs_status mvs_scene_set_views_from(mvs_ctx* ctx, const mvs_view* views, uint32_t n_views, const mvs_image_source* src) {
    if (!src || !src->acquire || !src->release) return api_fail(MVS_ERR_INVALID, "null argument");
    return set_views_impl(ctx, views, n_views, 0, src);
}
static mvs_status set_views_impl(mvs_ctx* ctx, const mvs_view* views, uint32_t n_views, int rgb_on_device, const mvs_image_source* src) {
    if (!ctx || (!views && n_views)) return api_fail(MVS_ERR_INVALID, "null argument");
    MVS_CTX_API_BEGIN
    view_input_begin(ctx, VIEW_SCRATCH_DEFAULT);   // (a refusal leaves the context without views: view_input.h)
    own_images_keep(ctx, rgb_on_device ? 0u : n_views);
    std::vector<ViewParams> hv(n_views, ViewParams{});
    // Host images.  The caller's buffers are pageable, and a pageable hipMemcpyAsync is staged through the driver's bounce buffer at
    // ~13 GB/s (1.9 GB of BASELINE config 3: 146 ms).  Three routes (environment MVS_HOST_UPLOAD; DESIGN.md "Boundary"):
    //   ring      (default) host threads copy the images, cut into 16 MB pieces, into a ring of LIBRARY-OWNED pinned buffers
    //             (hipHostMalloc, allocated once per process) while the copy engine drains the pieces filled before: nothing of
    //             the caller's address space is ever registered with the driver;
    //   register  the caller's pages pinned in place for the duration of the call (hipHostRegister; MVS_PIN_HOST_IMAGES=1 is the
    //             older spelling): the fastest route, but user-pointer registrations of pages the process keeps churning ended
    //             GPU test runs with an abort() inside the runtime (profiles/EXPERIMENTS.md) -- opt-in only;
    //   pageable  plain copies from the caller's memory (MVS_PIN_HOST_IMAGES=0).
    // every exit path -- a bad image, an allocation or copy that throws -- first drains the stream (copies may still read the
    // pinned pages) and then unregisters what was registered: the caller's memory never stays pinned behind a failed call
    struct Pinned {
        hipStream_t s; std::vector<void*> ptrs;
        ~Pinned() { if (ptrs.empty()) return; (void)hipStreamSynchronize(s); for (void* p : ptrs) (void)hipHostUnregister(p); }
    } pinned{ctx->stream, {}};
    UploadRoute route = rgb_on_device ? UploadRoute::Pageable : upload_route();
    if (src && route == UploadRoute::Register) route = UploadRoute::Ring;   // (pages that are handed back batch by batch are never registered)
    std::vector<UploadPiece> pieces;
    // Image SOURCE (mvs_scene_set_views_from): the caller's images exist only between acquire(j) and release(j), both called on THIS thread,
    // at most `max_in_flight` views at a time (calculate_data_costs.cpp:157-231 holds one decoded image at a time; a caller that loads all of
    // them first needs the whole scene's pixels in host memory).  A batch is acquired, copied to the device through the pinned ring and
    // released; whatever fails -- an image the caller cannot produce, a copy -- every view acquired so far is released before the call returns.
    struct Held {
        const mvs_image_source* src; std::vector<uint32_t> views;
        void release_all() { for (uint32_t j : views) src->release(src->user, j); views.clear(); }
        ~Held() { if (src) release_all(); }
    } held{src, {}};
    const uint32_t in_flight = src ? std::max<uint32_t>(1u, src->max_in_flight ? src->max_in_flight : 4u) : 0u;
    auto flush_batch = [&]() {
        if (!pieces.empty()) upload_through_ring(ctx, pieces);      // (returns with the stream drained: the caller's pixels are no longer read)
        pieces.clear();
        MVS_HIP(hipStreamSynchronize(ctx->stream));
        held.release_all();
    };
    for (uint32_t j = 0; j < n_views; ++j) {
        mvs_view v = views[j];
        if (src) {
            if (v.width < 2 || v.height < 2) throw StatusError(MVS_ERR_INVALID, "view " + std::to_string(j) + ": bad image");
            v.rgb = src->acquire(src->user, j);
            if (!v.rgb) throw StatusError(MVS_ERR_INVALID, "view " + std::to_string(j) + ": the image source has no image");
            held.views.push_back(j);
        }
        if (v.width < 2 || v.height < 2 || !v.rgb) throw StatusError(MVS_ERR_INVALID, "view " + std::to_string(j) + ": bad image");
        ViewParams& p = hv[j];
        p = view_params_of(v);
        if (rgb_on_device) p.rgb = v.rgb;
        else {
            uint8_t* image = own_image(ctx, j, v);
            const size_t bytes = (size_t)v.width * v.height * 3;
            p.rgb = image;
            if (route == UploadRoute::Ring && bytes >= (1u << 18)) { pieces.push_back(UploadPiece{v.rgb, image, bytes}); if (src && held.views.size() >= in_flight) flush_batch(); continue; }
            if (route == UploadRoute::Register && bytes >= (1u << 20) && hipHostRegister(const_cast<uint8_t*>(v.rgb), bytes, hipHostRegisterDefault) == hipSuccess) pinned.ptrs.push_back(const_cast<uint8_t*>(v.rgb));
            else (void)hipGetLastError();   // not registered: clear the sticky error, copy from pageable memory
            MVS_HIP(hipMemcpyAsync(image, v.rgb, bytes, hipMemcpyHostToDevice, ctx->stream));
            if (src && held.views.size() >= in_flight) flush_batch();
        }
    }
    if (src) flush_batch();
    if (!pieces.empty()) upload_through_ring(ctx, pieces);
    MVS_HIP(hipStreamSynchronize(ctx->stream));
    view_input_commit(ctx, hv, n_views);
    MVS_API_END
}

mvs_status mvs_scene_set_face_range(mvs_ctx* ctx, uint32_t begin, uint32_t end) {
    if (!ctx) return api_fail(MVS_ERR_INVALID, "ctx is null");
    if (begin > end || end > ctx->n_faces) return api_fail(MVS_ERR_INVALID, "bad face range");
    ctx->face_begin = begin; ctx->face_end = end;
    ctx->have_costs = false; ctx->dc_phase = 0;
    return MVS_OK;
}

mvs_status mvs_ctx_dc_phase1(mvs_ctx* ctx, const mvs_settings* settings) {
    if (!ctx || !settings) return api_fail(MVS_ERR_INVALID, "null argument");
    MVS_CTX_API_BEGIN
    dc_phase1(ctx, settings);
    MVS_API_END
}
mvs_status mvs_ctx_dc_phase2(mvs_ctx* ctx) {
    if (!ctx) return api_fail(MVS_ERR_INVALID, "ctx is null");
    MVS_CTX_API_BEGIN
    dc_phase2(ctx);
    MVS_API_END
}
mvs_status mvs_ctx_dc_phase3(mvs_ctx* ctx, mvs_dc_stats* stats) {
    if (!ctx) return api_fail(MVS_ERR_INVALID, "ctx is null");
    MVS_CTX_API_BEGIN
    dc_phase3(ctx, stats);
    MVS_API_END
}

mvs_status mvs_ctx_data_costs(mvs_ctx* ctx, const mvs_settings* settings, mvs_dc_stats* stats) {
    if (!ctx || !settings) return api_fail(MVS_ERR_INVALID, "null argument");
    MVS_CTX_API_BEGIN
    RoctxRange range("Calculating data costs");   /* texrecon.cpp:118 */
    dc_run(ctx, settings, stats);   // the three phases, or the ranged walk (option "dc_range_pairs")
    MVS_API_END
}

mvs_status mvs_ctx_dc_ranges(mvs_ctx* ctx, uint32_t* n_ranges, uint32_t* range_faces) {
    if (!ctx) return api_fail(MVS_ERR_INVALID, "ctx is null");
    if (ctx->dc_phase < 1) return api_fail(MVS_ERR_STATE, "no data-cost pass on this context");
    if (n_ranges) *n_ranges = ctx->dc_n_ranges;
    if (range_faces) *range_faces = ctx->dc_range_faces;
    return MVS_OK;
}

mvs_status mvs_ctx_prune_labels(mvs_ctx* ctx, uint32_t max_labels) {
    if (!ctx) return api_fail(MVS_ERR_INVALID, "ctx is null");
    MVS_CTX_API_BEGIN
    dc_prune_labels(ctx, max_labels);
    MVS_API_END
}

mvs_status mvs_ctx_costs_device(mvs_ctx* ctx, mvs_csr* v) {
    if (!ctx || !v) return api_fail(MVS_ERR_INVALID, "null argument");
    if (!ctx->have_costs) return api_fail(MVS_ERR_STATE, "no data costs on the device");
    v->n_faces = ctx->csr_faces; v->n_views = ctx->csr_views; v->nnz = ctx->csr_nnz;
    v->col_ptr = const_cast<uint32_t*>(ctx->r_ptr); v->view_id = const_cast<uint16_t*>(ctx->r_view); v->cost = const_cast<float*>(ctx->r_cost);
    return MVS_OK;
}

mvs_status mvs_ctx_costs_download(mvs_ctx* ctx, mvs_csr* out, float** quality_out) {
    if (!ctx || !out) return api_fail(MVS_ERR_INVALID, "null argument");
    if (!ctx->have_costs) return api_fail(MVS_ERR_STATE, "no data costs on the device");
    MVS_CTX_API_BEGIN
    const size_t F = ctx->csr_faces, nnz = ctx->csr_nnz;
    // a table kept in the library's own face order leaves in the caller's numbering (k_order.hip)
    const bool reordered = table_to_caller_order(ctx, quality_out != nullptr);
    const uint32_t* s_ptr = reordered ? ctx->u_ptr.p : ctx->r_ptr; const uint16_t* s_view = reordered ? ctx->u_view.p : ctx->r_view;
    const float* s_cost = reordered ? ctx->u_cost.p : ctx->r_cost; const float* s_q = reordered ? ctx->u_q.p : ctx->csr_q.p;
    // the caller's arrays: all of them or none (a failed allocation, copy or synchronisation hands everything back and reports it)
    out->n_faces = ctx->csr_faces; out->n_views = ctx->csr_views; out->nnz = nnz;
    out->col_ptr = nullptr; out->view_id = nullptr; out->cost = nullptr;
    if (quality_out) *quality_out = nullptr;
    struct Guard {
        mvs_csr* o; float** q; bool keep = false;
        ~Guard() { if (keep) return; free(o->col_ptr); free(o->view_id); free(o->cost); if (q) { free(*q); *q = nullptr; } memset(o, 0, sizeof(*o)); }
    } guard{out, quality_out};
    out->col_ptr = (uint32_t*)malloc((F + 1) * sizeof(uint32_t));
    out->view_id = (uint16_t*)malloc((nnz + 1) * sizeof(uint16_t));
    out->cost = (float*)malloc((nnz + 1) * sizeof(float));
    if (quality_out) *quality_out = (float*)malloc((nnz + 1) * sizeof(float));
    if (!out->col_ptr || !out->view_id || !out->cost || (quality_out && !*quality_out))
        throw StatusError(MVS_ERR_INVALID, "out of host memory for the downloaded table (" + std::to_string((F + 1) * 4 + (nnz + 1) * (quality_out ? 10 : 6)) + " bytes)");
    MVS_HIP(hipMemcpyAsync(out->col_ptr, s_ptr, (F + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    if (nnz) {
        MVS_HIP(hipMemcpyAsync(out->view_id, s_view, nnz * sizeof(uint16_t), hipMemcpyDeviceToHost, ctx->stream));
        MVS_HIP(hipMemcpyAsync(out->cost, s_cost, nnz * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    }
    if (quality_out) {
        if (nnz && ctx->csr_q_valid) MVS_HIP(hipMemcpyAsync(*quality_out, s_q, nnz * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
        else memset(*quality_out, 0, (nnz + 1) * sizeof(float));
    }
    MVS_HIP(hipStreamSynchronize(ctx->stream));
    guard.keep = true;
    MVS_API_END
}

void mvs_csr_free(mvs_csr* csr) {
    if (!csr) return;
    free(csr->col_ptr); free(csr->view_id); free(csr->cost);
    memset(csr, 0, sizeof(*csr));
}

mvs_status mvs_ctx_costs_upload(mvs_ctx* ctx, const mvs_csr* csr, int on_device) {
    if (!ctx || !csr || !csr->col_ptr) return api_fail(MVS_ERR_INVALID, "null argument");
    MVS_CTX_API_BEGIN
    const size_t F = csr->n_faces, nnz = csr->nnz;
    if (on_device) {
        ctx->r_ptr = csr->col_ptr; ctx->r_view = csr->view_id; ctx->r_cost = csr->cost;
    } else {
        ctx->csr_ptr.ensure(F + 2); ctx->csr_view.ensure(nnz + 1); ctx->csr_cost.ensure(nnz + 1);
        MVS_HIP(hipMemcpyAsync(ctx->csr_ptr.p, csr->col_ptr, (F + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
        if (nnz) {
            MVS_HIP(hipMemcpyAsync(ctx->csr_view.p, csr->view_id, nnz * sizeof(uint16_t), hipMemcpyHostToDevice, ctx->stream));
            MVS_HIP(hipMemcpyAsync(ctx->csr_cost.p, csr->cost, nnz * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
        }
        MVS_HIP(hipStreamSynchronize(ctx->stream));
        ctx->r_ptr = ctx->csr_ptr.p; ctx->r_view = ctx->csr_view.p; ctx->r_cost = ctx->csr_cost.p;
    }
    ctx->csr_faces = csr->n_faces; ctx->csr_views = csr->n_views; ctx->csr_nnz = nnz;
    ctx->have_costs = true; ctx->csr_q_valid = false;
    ctx->t_perm = nullptr; ctx->t_pos = nullptr; ctx->u_valid = false;   // the caller's table, the caller's order
    MVS_API_END
}

// ---------------- file-level boundary: the formats are spt_io.h, their messages become the call's error ----------------
static mvs_status file_status(mvs_status st, const std::string& msg) { return st == MVS_OK ? st : api_fail(st, msg); }
mvs_status mvs_write_spt(const mvs_csr* csr, const char* path) { std::string msg; return file_status(write_spt(csr, path, msg), msg); }
mvs_status mvs_read_spt(const char* path, mvs_csr* out) { std::string msg; return file_status(read_spt(path, out, msg), msg); }
mvs_status mvs_write_labeling_vec(const uint32_t* labels, uint32_t n_faces, const char* path) { std::string msg; return file_status(write_labeling_vec(labels, n_faces, path, msg), msg); }

}  // extern "C"
