// rows.h -- the host plumbing the post-processing rows f5 - f8 share (k_seam.hip, k_texpatch.hip, k_localseam.hip, k_atlas.hip):
//   launch and copy helpers, the rocprim two-call idiom (sort_scan.h), stage timers, the wrappers around an entry point's body, the staging of the
//   caller's adjacency and labels, and the reader / checker of a patch set; and what rows f9 - f11 and the image encoders need beside them: the host
//   clock, a row's buffers on first use, the model parameters' defaults, a loop on host threads (DESIGN.md section 4 "Shared plumbing").  Internal, header-only.
#pragma once
#include "ctx.h"
#include "sort_scan.h"

#include <atomic>
#include <chrono>
#include <thread>

namespace mvs {

inline unsigned grid(size_t n) { return (unsigned)std::max<size_t>(1, (n + 255) / 256); }   // blocks of 256 threads, at least one
inline double now_ms_host() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
// a row's per-context buffers (ctx->gsl, ctx->atlas, ...): allocated on first use, freed by the row's *_release
template <class Dev>
Dev& row_dev(Dev*& slot) { if (!slot) slot = new Dev(); return *slot; }
// the caller's model parameters, or the library's defaults (rows f9 and f11)
inline mvs_model_params params_or_default(const mvs_model_params* params) {
    mvs_model_params P;
    if (params) P = *params; else mvs_model_default_params(&P);
    return P;
}
// fn(i) for every i < n, one item per thread at a time on min(16, n) host threads, the calling one included; fn does not throw
template <class Fn>
void for_each_on_threads(uint32_t n, Fn&& fn) {
    std::atomic<uint32_t> next{0};
    auto work = [&] { for (uint32_t i = next.fetch_add(1); i < n; i = next.fetch_add(1)) fn(i); };
    std::vector<std::thread> pool;
    for (uint32_t t = 1; t < std::min<uint32_t>(16u, n); ++t) pool.emplace_back(work);
    work();
    for (auto& t : pool) t.join();
}

// ---- copies (all asynchronous on `s`: the caller drains the stream before the host side goes away) ----
template <class T>
T* host_copy(const T* d, size_t n, hipStream_t s) {   // a malloc'ed host copy of a device array (the *_free functions of the ABI release it)
    T* h = (T*)malloc(std::max<size_t>(n, 1) * sizeof(T));
    if (!h) throw StatusError(MVS_ERR_INVALID, "out of host memory");
    if (n) MVS_HIP(hipMemcpyAsync(h, d, n * sizeof(T), hipMemcpyDeviceToHost, s));
    return h;
}
template <class T>
const T* stage(DBuf<T>& buf, const T* src, size_t n, int on_device, hipStream_t s) {   // a caller's array where the kernels read it
    if (on_device) return src;
    buf.ensure(n + 1);
    if (n) MVS_HIP(hipMemcpyAsync(buf.p, src, n * sizeof(T), hipMemcpyHostToDevice, s));
    return buf.p;
}
template <class T>
void upload(DBuf<T>& buf, const T* h, size_t n, hipStream_t s) {
    buf.ensure(n + 1);
    if (n) MVS_HIP(hipMemcpyAsync(buf.p, h, n * sizeof(T), hipMemcpyHostToDevice, s));
}
template <class T>
void upload(DBuf<T>& buf, const std::vector<T>& h, hipStream_t s) { upload(buf, h.data(), h.size(), s); }

// (not a template, so it stays out of sort_scan.h: it would put its scan kernels into every file that includes that header)
inline void dev_inclusive_max_scan(mvs_ctx* ctx, uint32_t* in, uint32_t* out, size_t n) {
    with_sort_tmp(ctx, [&](void* t, size_t& b) { return rocprim::inclusive_scan(t, b, in, out, n, rocprim::maximum<uint32_t>(), ctx->stream); });
}

// ---- N timing events of one call: mark() records the next one on the stream, ms(a, b) is the time between marks a and b ----
template <int N>
struct StageTimer {
    hipEvent_t ev[N]; hipStream_t s; int n = 0;
    explicit StageTimer(hipStream_t stream) : s(stream) { for (auto& e : ev) MVS_HIP(hipEventCreate(&e)); }
    ~StageTimer() { for (auto& e : ev) (void)hipEventDestroy(e); }
    StageTimer(const StageTimer&) = delete;
    StageTimer& operator=(const StageTimer&) = delete;
    void mark() {
        if (n >= N) throw HipError("StageTimer: more marks than events");
        MVS_HIP(hipEventRecord(ev[n++], s));
    }
    float ms(int a, int b) const { float t = 0.0f; MVS_HIP(hipEventElapsedTime(&t, ev[a], ev[b])); return t; }
};

// ---- around the body of an entry point (api_guard: ctx.h) ----
// the row itself: `st` reaches the caller's stats whether run() returns or throws (after a throw the stream is drained first)
template <class Stats, class Run>
void run_with_stats(hipStream_t s, Stats* stats, const Stats& st, Run&& run) {
    try { run(); } catch (...) { (void)hipStreamSynchronize(s); if (stats) *stats = st; throw; }
    if (stats) *stats = st;
}
// host copies of a result: copies() fills *out with host_copy()s, which are complete on return; a failure frees what was made
template <class Out, class Copies>
void download(hipStream_t s, Out* out, void (*free_out)(Out*), Copies&& copies) {
    try { copies(); MVS_HIP(hipStreamSynchronize(s)); } catch (...) { (void)hipStreamSynchronize(s); free_out(out); throw; }
}

// ---- the caller's graph and labels on the device ----
struct RowGraph { const uint32_t* adj_ptr; const uint32_t* adj; const uint32_t* labels; uint32_t E; };
// adj_ptr [F + 1], adj [E], labels [F]: host arrays are uploaded (asynchronously: the entry point drains the stream once before it runs
// its row -- host buffers are borrowed for the call only) into the context's one set of buffers, device arrays are used where they
// are.  E = adj_ptr[F]; for a device-resident adjacency it is 0 unless `read_edges` (one blocking 4-byte read).  No face: all null.
inline RowGraph stage_graph(mvs_ctx* ctx, const uint32_t* adj_ptr, const uint32_t* adj, int adj_on_device, const uint32_t* labels, int labels_on_device,
                            bool read_edges = false) {
    const uint32_t F = ctx->n_faces;
    if (!F) return RowGraph{nullptr, nullptr, nullptr, 0u};
    hipStream_t s = ctx->stream;
    const uint32_t E = adj_on_device ? (read_edges ? read_u32(ctx, adj_ptr + F) : 0u) : adj_ptr[F];
    return RowGraph{stage(ctx->row_adj_ptr, adj_ptr, (size_t)F + 1, adj_on_device, s), stage(ctx->row_adj, adj, E, adj_on_device, s),
                    stage(ctx->row_labels, labels, F, labels_on_device, s), E};
}

// ---- a patch set's per-patch arrays on the host ----
struct PatchFrames { const unsigned long long* pix_ptr; const int4* box; const uint32_t* face_ptr; const uint32_t* label; };   // [NP + 1], [NP], [NP + 1], [NP] or null
// Reads pix_ptr, box, face_ptr and (want_label) label of `in` into ONE pinned buffer of the context -- a device-resident set in one
// drain of the stream -- and checks what every row relies on: no null array where the counts say there are entries (blending is the
// caller's business), pix_ptr and face_ptr start at 0 and end at the totals, and every patch has a frame of at least 1 x 1 whose pixel
// count is its pix_ptr range, and an ascending face_ptr.  Throws MVS_ERR_INVALID, `who` in front.  The views stay valid until the
// next call; the empty set gives pix_ptr = face_ptr = {0}.
inline PatchFrames read_patch_set(mvs_ctx* ctx, const mvs_patch_set& in, int on_device, bool want_label, const char* who) {
    const uint32_t NP = in.n_patches, L = in.n_listed;
    const uint64_t NPIX = in.n_pixels;
    const std::string w(who);
    if ((NP && (!in.box || !in.face_ptr || !in.pix_ptr || (want_label && !in.label))) || (L && (!in.faces || !in.texcoords)) || (NPIX && (!in.image || !in.validity)))
        throw StatusError(MVS_ERR_INVALID, w + ": null array in the patch set");
    static const unsigned long long zero64 = 0ull; static const uint32_t zero32 = 0u;
    PatchFrames f{&zero64, nullptr, &zero32, nullptr};
    if (NP) {
        const size_t b_pix = ((size_t)NP + 1) * sizeof(unsigned long long), b_box = (size_t)NP * sizeof(int4), b_face = ((size_t)NP + 1) * sizeof(uint32_t),
                     b_label = want_label ? (size_t)NP * sizeof(uint32_t) : 0;
        ctx->row_pin.ensure(b_pix + b_box + b_face + b_label);
        char* pin = ctx->row_pin.p;   // box, pix_ptr, face_ptr, label back to back: entries of 16, 8, 4 and 4 bytes, so each part is aligned
        const size_t o_pix = b_box, o_face = o_pix + b_pix, o_label = o_face + b_face;
        const struct { const void* src; size_t off, bytes; } part[4] = {{in.box, 0, b_box}, {in.pix_ptr, o_pix, b_pix}, {in.face_ptr, o_face, b_face}, {in.label, o_label, b_label}};
        for (const auto& q : part) {
            if (!q.bytes) continue;
            if (on_device) MVS_HIP(hipMemcpyAsync(pin + q.off, q.src, q.bytes, hipMemcpyDeviceToHost, ctx->stream));
            else memcpy(pin + q.off, q.src, q.bytes);
        }
        if (on_device) MVS_HIP(hipStreamSynchronize(ctx->stream));
        f = PatchFrames{(const unsigned long long*)(pin + o_pix), (const int4*)pin, (const uint32_t*)(pin + o_face), want_label ? (const uint32_t*)(pin + o_label) : nullptr};
    }
    const unsigned long long* hp = f.pix_ptr; const uint32_t* hf = f.face_ptr; const int4* hb = f.box;
    if (hp[0] != 0 || hf[0] != 0 || hp[NP] != NPIX || hf[NP] != L) throw StatusError(MVS_ERR_INVALID, w + ": pix_ptr / face_ptr do not match the totals");
    for (uint32_t p = 0; p < NP; ++p)
        if (hb[p].z < 1 || hb[p].w < 1 || hp[p + 1] < hp[p] || hp[p + 1] - hp[p] != (unsigned long long)hb[p].z * (unsigned long long)hb[p].w || hf[p + 1] < hf[p])
            throw StatusError(MVS_ERR_INVALID, w + ": patch " + std::to_string(p) + ": frame, pix_ptr and face_ptr do not agree");
    return f;
}

// The chunk tables of the kernels that give a block `chunk` pixels of one patch: patch p owns blocks [chunk_ptr[p], chunk_ptr[p + 1]),
// chunk_patch[block] = its patch.  Built from the host pix_ptr into h_ptr / h_patch and uploaded asynchronously FROM THOSE VECTORS: they
// are the caller's, and stay alive until the caller has drained the stream.  Returns the number of blocks.
inline uint32_t upload_chunk_tables(mvs_ctx* ctx, const unsigned long long* pix_ptr, uint32_t NP, uint32_t chunk, std::vector<uint32_t>& h_ptr,
                                    std::vector<uint32_t>& h_patch, DBuf<uint32_t>& d_ptr, DBuf<uint32_t>& d_patch) {
    h_ptr.assign((size_t)NP + 1, 0u); h_patch.clear();
    for (uint32_t p = 0; p < NP; ++p) {
        const uint32_t nc = (uint32_t)((pix_ptr[p + 1] - pix_ptr[p] + chunk - 1) / chunk);
        h_ptr[p + 1] = h_ptr[p] + nc;
        h_patch.insert(h_patch.end(), nc, p);
    }
    upload(d_ptr, h_ptr, ctx->stream); upload(d_patch, h_patch, ctx->stream);
    return h_ptr[NP];
}

// ---- row f6's buffers and its geometry half, which the debug model (row f10, k_debug.hip) shares ----
// per-context buffers of row f6, allocated on first use, freed with the context (texpatch_release)
struct TexPatchDev {
    PatchTables pt;
    DBuf<uint32_t> label, cnt, face_ptr, faces, epid, nchunk, chunk_ptr, win_in, win_near, big;
    DBuf<int4> box; DBuf<float> texcoords, image, adjust; DBuf<unsigned long long> npix, pix_ptr, c64; DBuf<uint8_t> validity, blending;
};
constexpr uint32_t TEXPATCH_CHUNK = 1024;   // pixels of one patch per block of the kernels that run on chunk_ptr (resolve, debug_patch_kernel)
// k_texpatch.hip: everything of row f6 before its pixels -- the input checks, build_patch_tables, label / box / face_ptr / faces /
// texcoords / pix_ptr / chunk_ptr in D and room for image, validity and blending; fills S.patches, merged, listed_faces, pixels and
// refuses max_pixels (`who` starts the messages).  Marks tm three times: begin, tables, lists.  *n_chunks (blocks of TEXPATCH_CHUNK
// pixels, chunk_ptr[n_patches]) arrives with the next drain of the stream.
void texpatch_geometry(mvs_ctx* ctx, TexPatchDev& D, const uint32_t* d_adj_ptr, const uint32_t* d_adj, const uint32_t* d_labels, const mvs_patch_params& P,
                       mvs_patch_stats& S, uint32_t& n_listed, uint64_t& n_pixels, uint32_t* n_chunks, StageTimer<5>& tm, const char* who);
// D as an mvs_patch_set: the context's device arrays, or malloc'ed host copies (mvs_patch_set_free)
void texpatch_output(mvs_ctx* ctx, TexPatchDev& D, uint32_t n_listed, uint64_t n_pixels, mvs_patch_set* out, int out_on_device);

}  // namespace mvs
