// k_model.hip -- row f9: tex::build_model + ObjModel::save + MaterialLib::save_to_files (DESIGN.md section 4 "Model output"): the text of
// the .obj and the .mtl formatted on the device, byte for byte what upstream's writers produce; the files written on the host, the atlas
// PNGs encoded there too (png_io.h; params.png_device 0) or on the device (k_png.hip; params.png_device 1), or JPEGs from the device (k_jpeg.hip;
// params.image_format 1: the `.jpg` in the .mtl's map_Kd lines is the one change in the text).  Three phases on the context's stream:
//   measure  one thread per line computes its length (fmt6.h), checks its indices and counts the floats of the wide route
//   scan     64-bit exclusive scan of the lengths (rocprim through rows.h); the section offsets are gathered from it
//   write    a block's 256 lines are contiguous in the file: thread = line formats into an LDS staging buffer laid out like the file from
//            a 16-byte aligned base, then the block stores the range with 16-byte vector stores (the at most 15 bytes in front of the
//            first and behind the last full chunk belong to chunks shared with the neighbours and go out as bytes).  A block whose
//            text exceeds the buffer takes as many passes as it needs, each over the longest run of whole lines that fits.
// The .mtl goes through the same three kernels with one "line" per material (its eight lines).
#include "image_routes.h"
#include "fmt6.h"
#include "png_io.h"
#include "jpeg_base.h"
#include "model_corner.h"

namespace mvs {

struct ModelDev {
    // staged inputs (host callers)
    DBuf<uint32_t> in_faces, in_tc_ptr, in_ids; DBuf<float> in_merged, in_normals;
    DBuf<uint32_t> sec; DBuf<char> name;
    DBuf<unsigned long long> len, off, mlen, moff, sec_bytes, c64;
    DBuf<char> obj, mtl;
    std::vector<uint64_t> h_sec, h_sec_bytes;   // the section arrays of an out_on_device result
    uint64_t obj_bytes = 0, mtl_bytes = 0;
};
void model_release(mvs_ctx* ctx) { delete ctx->model; ctx->model = nullptr; }

namespace {
typedef unsigned long long u64;
constexpr uint32_t LINES = 256;        // lines of a block
constexpr uint32_t STAGE = 16384;      // bytes of the LDS staging buffer: a typical block (256 lines of ~30 bytes) in one pass, 9 blocks per CU
constexpr uint32_t MAX_NAME = 255;     // longest line: a material's record = 166 + 255 + 2 x 10 bytes, far below STAGE - 15
enum { K_WIDE = 0, K_NONFINITE, K_BAD_FACE, K_BAD_ID, K_N };   // 64-bit counters

// ---- sinks: one emit() per source serves the measuring and the writing pass ----
struct CountSink {
    uint32_t n = 0, wide = 0, nonfinite = 0;
    __device__ void ch(char) { n += 1u; }
    __device__ void str(const char*, uint32_t k) { n += k; }
    __device__ void u32(uint32_t v) { n += fmt6::u32_len(v); }
    __device__ void filled4(uint32_t v) { n += max(4u, fmt6::u32_len(v)); }
    __device__ void flt(float x) {
        const uint32_t b = __float_as_uint(x);
        n += fmt6::float_len(b); wide += fmt6::is_wide(b) ? 1u : 0u; nonfinite += fmt6::is_nonfinite(b) ? 1u : 0u;
    }
};
struct PutSink {
    char* p;
    __device__ void ch(char c) { *p++ = c; }
    __device__ void str(const char* s, uint32_t k) { for (uint32_t i = 0; i < k; ++i) p[i] = s[i]; p += k; }
    __device__ void u32(uint32_t v) { p += fmt6::u32_put(p, v); }
    __device__ void filled4(uint32_t v) { const uint32_t k = max(4u, fmt6::u32_len(v)); fmt6::put_digits32(p, v, k); p += k; }   // util::string::get_filled(v, 4)
    __device__ void flt(float x) { const uint32_t b = __float_as_uint(x), k = fmt6::float_len(b); fmt6::float_put(p, b, k); p += k; }
};

// ---- the lines of the .obj ----
// sec [A + 5]: first line of the mtllib line (0), the v, vt and vn lines, group 0 .. A - 1, and the number of lines
struct ObjSource {
    const uint32_t* sec; uint32_t A, F;
    const float* verts; const float* merged; const float* normals;   // normals null: no vn lines, faces V/T
    const uint32_t* mesh_faces; const uint32_t* faces; const uint32_t* ids; const uint32_t* tc_ptr;
    const char* name; uint32_t name_len;

    // atlas of a line at or behind sec[4]: the last group that starts at or before it
    __device__ uint32_t group_of(uint32_t line) const {
        uint32_t lo = 0, hi = A;   // group lo starts at or before the line, group hi (or the end) behind it
        while (hi - lo > 1u) { const uint32_t mid = lo + (hi - lo) / 2u; if (sec[4 + mid] <= line) lo = mid; else hi = mid; }
        return lo;
    }
    // the line's text into the sink; bad[0] / bad[1]: face ids >= F, texcoord ids outside the atlas (such an entry prints index 0)
    template <class Sink>
    __device__ void emit(uint32_t line, Sink& k, uint32_t* bad) const {
        if (line == 0u) { k.str("mtllib ", 7); k.str(name, name_len); k.str(".mtl\n", 5); return; }
        if (line < sec[2]) { const float* v = verts + 3 * (size_t)(line - sec[1]); k.str("v ", 2); k.flt(v[0]); k.ch(' '); k.flt(v[1]); k.ch(' '); k.flt(v[2]); k.ch('\n'); return; }
        if (line < sec[3]) { const float* t = merged + 2 * (size_t)(line - sec[2]); k.str("vt ", 3); k.flt(t[0]); k.ch(' '); k.flt(1.0f - t[1]); k.ch('\n'); return; }
        if (line < sec[4]) { const float* v = normals + 3 * (size_t)(line - sec[3]); k.str("vn ", 3); k.flt(v[0]); k.ch(' '); k.flt(v[1]); k.ch(' '); k.flt(v[2]); k.ch('\n'); return; }
        const uint32_t a = group_of(line), first = sec[4 + a];
        if (line == first) { k.str("usemtl material", 15); k.filled4(a); k.ch('\n'); return; }
        const uint32_t e = (first - sec[4] - a) + (line - first - 1u);   // face_ptr[a] + position in the group
        const uint32_t tc0 = tc_ptr[a], tcn = tc_ptr[a + 1] - tc0;
        k.ch('f');
        for (uint32_t c = 0; c < 3u; ++c) {
            const ModelCorner m = model_corner(mesh_faces, F, faces, ids, tc0, tcn, e, c);
            if (!m.face_ok && c == 0u) bad[0] += 1u;
            if (!m.id_ok) bad[1] += 1u;
            const uint32_t v = m.face_ok ? m.v + 1u : 0u;
            k.ch(' '); k.u32(v); k.ch('/'); k.u32(m.id_ok ? m.g + 1u : 0u);
            if (normals) { k.ch('/'); k.u32(v); }
        }
        k.ch('\n');
    }
};

// ---- the "lines" of the .mtl: material a's record (material_lib.cpp:31-38) ----
struct MtlSource {
    const char* name; uint32_t name_len; uint32_t jpeg;   // jpeg: params.image_format 1, the one thing that changes the text
    template <class Sink>
    __device__ void emit(uint32_t a, Sink& k, uint32_t*) const {
        k.str("newmtl material", 15); k.filled4(a);
        k.str("\nKa 1.000000 1.000000 1.000000\nKd 1.000000 1.000000 1.000000\nKs 0.000000 0.000000 0.000000\nTr 0.000000\nillum 1\nNs 1.000000\nmap_Kd ", 130);
        k.str(name, name_len); k.str("_material", 9); k.filled4(a); k.str(jpeg ? "_map_Kd.jpg\n" : "_map_Kd.png\n", 12);
    }
};

template <class Src>
__global__ void __launch_bounds__(256) model_measure_kernel(Src S, uint32_t n, u64* __restrict__ len, u64* __restrict__ c64) {
    const uint32_t line = blockIdx.x * 256u + threadIdx.x;
    if (line > n) return;
    if (line == n) { len[n] = 0ull; return; }   // the scan leaves the total behind the last line
    CountSink k; uint32_t bad[2] = {0u, 0u};
    S.emit(line, k, bad);
    len[line] = k.n;
    if (k.wide) atomicAdd(&c64[K_WIDE], (u64)k.wide);
    if (k.nonfinite) atomicAdd(&c64[K_NONFINITE], (u64)k.nonfinite);
    if (bad[0]) atomicAdd(&c64[K_BAD_FACE], (u64)bad[0]);
    if (bad[1]) atomicAdd(&c64[K_BAD_ID], (u64)bad[1]);
}

__global__ void __launch_bounds__(256) model_section_bytes_kernel(const uint32_t* __restrict__ sec, uint32_t n_sec, const u64* __restrict__ off, u64* __restrict__ out) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n_sec) out[i] = off[sec[i]];
}

// off [n + 1]: byte offset of every line and the total; out: at least off[n] bytes, 16-byte aligned
template <class Src>
__global__ void __launch_bounds__(256) model_write_kernel(Src S, uint32_t n, const u64* __restrict__ off, char* __restrict__ out) {
    __shared__ uint4 stage4[STAGE / 16];
    char* stage = reinterpret_cast<char*>(stage4);
    const uint32_t tid = threadIdx.x, first = blockIdx.x * LINES, line = first + tid, end = min(n, first + LINES);
    const bool live = line < end;
    const u64 lo = live ? off[line] : 0ull, hi = live ? off[line + 1] : 0ull;
    uint32_t start = first;
    while (start < end) {   // one pass per run of whole lines that fits the buffer (block-uniform)
        const u64 wlo = off[start], abase = wlo & ~15ull;
        const bool in = live && line >= start && hi - abase <= (u64)STAGE;   // a prefix of the lines from `start` on: hi ascends
        const uint32_t cnt = (uint32_t)__syncthreads_count(in ? 1 : 0);     // (the barrier also ends the previous pass's reads of the buffer)
        if (cnt == 0u) return;                                              // a line longer than the buffer: the host never launches such a source
        if (in) { PutSink k{stage + (size_t)(lo - abase)}; uint32_t bad[2] = {0u, 0u}; S.emit(line, k, bad); }
        __syncthreads();
        const u64 whi = off[start + cnt];
        const u64 full_lo = (wlo + 15ull) & ~15ull, full_hi = whi & ~15ull;   // the 16-byte chunks that are all this pass's
        for (u64 g = full_lo + 16ull * tid; g + 16ull <= full_hi; g += 16ull * 256ull)
            *reinterpret_cast<uint4*>(out + g) = stage4[(size_t)(g - abase) / 16];
        const u64 head_end = full_lo < whi ? full_lo : whi, tail_lo = full_hi > head_end ? full_hi : head_end;
        if (tid < 16u) { const u64 g = wlo + tid; if (g < head_end) out[g] = stage[(size_t)(g - abase)]; }
        else if (tid < 32u) { const u64 g = tail_lo + (tid - 16u); if (g < whi) out[g] = stage[(size_t)(g - abase)]; }
        start += cnt;
    }
}

template <class T>
const T* read_to_pin(mvs_ctx* ctx, char* pin, const T* src, size_t n, int on_device) {
    if (on_device) MVS_HIP(hipMemcpyAsync(pin, src, n * sizeof(T), hipMemcpyDeviceToHost, ctx->stream));
    else memcpy(pin, src, n * sizeof(T));
    return (const T*)pin;
}

// measure, scan, write: leaves the text in D.obj / D.mtl (obj_bytes, mtl_bytes) and the section arrays in D.h_sec / h_sec_bytes
void run_model(mvs_ctx* ctx, ModelDev& D, const mvs_atlas_set& in, int on_device, const float* normals, int normals_on_device, const std::string& name,
               const mvs_model_params& P, mvs_model_stats& st) {
    hipStream_t s = ctx->stream;
    const uint32_t A = in.n_atlases, L = in.n_listed, NM = in.n_merged, NV = ctx->n_verts, F = ctx->n_faces;
    std::vector<uint32_t> hf, ht;
    model_check_set(ctx, in, on_device, "build_model", hf, ht);
    if (name.size() > MAX_NAME) throw StatusError(MVS_ERR_INVALID, "build_model: name longer than 255 bytes");
    const uint64_t n64 = 1ull + NV + NM + (normals ? (uint64_t)NV : 0ull) + A + L;
    if (n64 >= 0xFFFFFE00ull) throw StatusError(MVS_ERR_UNSUPPORTED, "build_model: too many lines for one call");
    const uint32_t n = (uint32_t)n64, NS = A + 5u;
    std::vector<uint32_t> h_sec(NS);
    h_sec[0] = 0u; h_sec[1] = 1u; h_sec[2] = 1u + NV; h_sec[3] = h_sec[2] + NM; h_sec[4] = h_sec[3] + (normals ? NV : 0u);
    for (uint32_t a = 1; a <= A; ++a) h_sec[4 + a] = h_sec[4] + a + hf[a];
    D.h_sec.assign(h_sec.begin(), h_sec.end());
    upload(D.sec, h_sec, s);
    upload(D.name, name.data(), name.size(), s);
    ObjSource S{D.sec.p, A, F, ctx->d_verts, nullptr, nullptr, ctx->d_faces, nullptr, nullptr, nullptr, D.name.p, (uint32_t)name.size()};
    S.faces = stage(D.in_faces, (const uint32_t*)in.faces, L, on_device, s);
    S.ids = stage(D.in_ids, (const uint32_t*)in.texcoord_ids, 3 * (size_t)L, on_device, s);
    S.merged = stage(D.in_merged, (const float*)in.texcoords_merged, 2 * (size_t)NM, on_device, s);
    S.tc_ptr = A ? stage(D.in_tc_ptr, (const uint32_t*)in.tc_ptr, (size_t)A + 1, on_device, s) : nullptr;
    S.normals = normals ? stage(D.in_normals, normals, 3 * (size_t)NV, normals_on_device, s) : nullptr;
    MtlSource M{D.name.p, (uint32_t)name.size(), P.image_format == 1 ? 1u : 0u};
    MVS_HIP(hipStreamSynchronize(s));   // host buffers are borrowed for the call only (h_sec and name are this function's)
    D.len.ensure((size_t)n + 1); D.off.ensure((size_t)n + 1); D.mlen.ensure((size_t)A + 1); D.moff.ensure((size_t)A + 1); D.sec_bytes.ensure(NS); D.c64.ensure(K_N);
    StageTimer<5> tm(s);
    // ---- measure ----
    tm.mark();
    MVS_HIP(hipMemsetAsync(D.c64.p, 0, K_N * sizeof(u64), s));
    hipLaunchKernelGGL(model_measure_kernel<ObjSource>, dim3(grid((size_t)n + 1)), dim3(256), 0, s, S, n, D.len.p, D.c64.p);
    MVS_LAUNCH_CHECK();
    hipLaunchKernelGGL(model_measure_kernel<MtlSource>, dim3(grid((size_t)A + 1)), dim3(256), 0, s, M, A, D.mlen.p, D.c64.p);
    MVS_LAUNCH_CHECK();
    tm.mark();
    // ---- scan ----
    dev_exclusive_scan(ctx, D.len.p, D.off.p, (size_t)n + 1);
    dev_exclusive_scan(ctx, D.mlen.p, D.moff.p, (size_t)A + 1);
    hipLaunchKernelGGL(model_section_bytes_kernel, dim3(grid(NS)), dim3(256), 0, s, (const uint32_t*)D.sec.p, NS, (const u64*)D.off.p, D.sec_bytes.p);
    MVS_LAUNCH_CHECK();
    tm.mark();
    // ---- the one read-back: totals, section offsets, counters ----
    ctx->row_pin.ensure(((size_t)NS + K_N + 1) * sizeof(u64));
    u64* pin = (u64*)ctx->row_pin.p;
    MVS_HIP(hipMemcpyAsync(pin, D.sec_bytes.p, NS * sizeof(u64), hipMemcpyDeviceToHost, s));
    MVS_HIP(hipMemcpyAsync(pin + NS, D.c64.p, K_N * sizeof(u64), hipMemcpyDeviceToHost, s));
    MVS_HIP(hipMemcpyAsync(pin + NS + K_N, D.moff.p + A, sizeof(u64), hipMemcpyDeviceToHost, s));
    MVS_HIP(hipStreamSynchronize(s));
    D.h_sec_bytes.assign(pin, pin + NS);
    const u64* c64 = pin + NS;
    const uint64_t obj_bytes = pin[NS - 1], mtl_bytes = pin[NS + K_N];
    for (int i = 0; i < 4; ++i) { st.lines[i] = h_sec[i + 1] - h_sec[i]; st.bytes[i] = pin[i + 1] - pin[i]; }
    st.lines[4] = n - h_sec[4]; st.bytes[4] = obj_bytes - pin[4];
    st.mtl_bytes = mtl_bytes; st.wide_values = c64[K_WIDE]; st.nonfinite_values = c64[K_NONFINITE];
    st.ms_measure = tm.ms(0, 1); st.ms_scan = tm.ms(1, 2);
    model_refuse_bad_ids(c64[K_BAD_FACE], c64[K_BAD_ID], "build_model");
    if (P.max_bytes && obj_bytes > P.max_bytes)
        throw StatusError(MVS_ERR_UNSUPPORTED, "build_model: " + std::to_string(obj_bytes) + " bytes of .obj text exceed max_bytes = " + std::to_string(P.max_bytes));
    // ---- write ----
    D.obj.ensure((size_t)obj_bytes + 16); D.mtl.ensure((size_t)mtl_bytes + 16);
    tm.mark();
    hipLaunchKernelGGL(model_write_kernel<ObjSource>, dim3((n + LINES - 1u) / LINES), dim3(256), 0, s, S, n, (const u64*)D.off.p, D.obj.p);
    MVS_LAUNCH_CHECK();
    if (A) {
        hipLaunchKernelGGL(model_write_kernel<MtlSource>, dim3((A + LINES - 1u) / LINES), dim3(256), 0, s, M, A, (const u64*)D.moff.p, D.mtl.p);
        MVS_LAUNCH_CHECK();
    }
    tm.mark();
    MVS_HIP(hipStreamSynchronize(s));
    st.ms_write = tm.ms(3, 4);
    D.obj_bytes = obj_bytes; D.mtl_bytes = mtl_bytes;
}

// a device range into a file of its own
mvs_status device_to_file(mvs_ctx* ctx, const char* d, uint64_t bytes, const std::string& path, double& ms_copy, std::string& msg) {
    png_detail::File file(fopen(path.c_str(), "wb"));
    if (!file) return png_detail::fail(msg, MVS_ERR_INVALID, "cannot open " + path);
    bool ok = device_to_stream(ctx, d, bytes, file.get(), ms_copy);
    if (fclose(file.release()) != 0) ok = false;
    return ok ? MVS_OK : png_detail::fail(msg, MVS_ERR_INVALID, "write error on " + path);
}

}  // namespace

// ---- what rows f9 and f11 (k_glb.hip) share: declared in ctx.h ----
std::string model_filled4(uint32_t a) { char b[16]; snprintf(b, sizeof(b), "%04u", a); return b; }

bool device_to_stream(mvs_ctx* ctx, const char* d, uint64_t bytes, FILE* f, double& ms_copy) {
    constexpr size_t CHUNK = 32u << 20;
    ctx->row_pin.ensure((size_t)std::min<uint64_t>(bytes, CHUNK) + 16);
    bool ok = true;
    for (uint64_t at = 0; ok && at < bytes; at += CHUNK) {
        const size_t k = (size_t)std::min<uint64_t>(CHUNK, bytes - at);
        const double t0 = now_ms_host();
        MVS_HIP(hipMemcpyAsync(ctx->row_pin.p, d + at, k, hipMemcpyDeviceToHost, ctx->stream));
        MVS_HIP(hipStreamSynchronize(ctx->stream));
        ms_copy += now_ms_host() - t0;
        ok = fwrite(ctx->row_pin.p, 1, k, f) == k;
    }
    return ok;
}

void model_check_set(mvs_ctx* ctx, const mvs_atlas_set& in, int on_device, const char* who, std::vector<uint32_t>& face_ptr, std::vector<uint32_t>& tc_ptr) {
    const uint32_t A = in.n_atlases, L = in.n_listed, NM = in.n_merged;
    const std::string w = std::string(who) + ": ";
    if (!ctx->d_verts || !ctx->d_faces) throw StatusError(MVS_ERR_STATE, w + "no mesh (mvs_scene_set_mesh first)");
    if ((A && (!in.face_ptr || !in.tc_ptr)) || (L && (!in.faces || !in.texcoord_ids)) || (NM && !in.texcoords_merged))
        throw StatusError(MVS_ERR_INVALID, w + "null array in the atlas set");
    if ((L || NM) && !A) throw StatusError(MVS_ERR_INVALID, w + "faces or texture coordinates without an atlas");
    // face_ptr and tc_ptr on the host: they must run from 0 to the totals
    face_ptr.assign((size_t)A + 1, 0u); tc_ptr.assign((size_t)A + 1, 0u);
    if (A) {
        const size_t b = ((size_t)A + 1) * sizeof(uint32_t);
        ctx->row_pin.ensure(2 * b);
        const uint32_t* hf = read_to_pin(ctx, ctx->row_pin.p, in.face_ptr, (size_t)A + 1, on_device);
        const uint32_t* ht = read_to_pin(ctx, ctx->row_pin.p + b, in.tc_ptr, (size_t)A + 1, on_device);
        if (on_device) MVS_HIP(hipStreamSynchronize(ctx->stream));
        face_ptr.assign(hf, hf + A + 1); tc_ptr.assign(ht, ht + A + 1);
    }
    if (face_ptr[0] != 0u || tc_ptr[0] != 0u || face_ptr[A] != L || tc_ptr[A] != NM) throw StatusError(MVS_ERR_INVALID, w + "face_ptr / tc_ptr do not run from 0 to the totals");
    for (uint32_t a = 0; a < A; ++a)
        if (face_ptr[a + 1] < face_ptr[a] || tc_ptr[a + 1] < tc_ptr[a]) throw StatusError(MVS_ERR_INVALID, w + "face_ptr / tc_ptr of atlas " + std::to_string(a) + " descend");
}

void model_refuse_bad_ids(uint64_t bad_faces, uint64_t bad_ids, const char* who) {
    if (bad_faces) throw StatusError(MVS_ERR_INVALID, std::string(who) + ": " + std::to_string(bad_faces) + " face ids are not below the number of faces");
    if (bad_ids) throw StatusError(MVS_ERR_INVALID, std::string(who) + ": " + std::to_string(bad_ids) + " texcoord ids lie outside their atlas's range");
}

void model_check_image_params(const mvs_model_params& P, const mvs_atlas_set& in, const char* who) {
    const std::string w = std::string(who) + ": ";
    if (P.image_format != 0 && P.image_format != 1) throw StatusError(MVS_ERR_INVALID, w + "image_format 0 (PNG) or 1 (JPEG)");
    if (P.image_format == 1) {
        std::string msg;
        if (P.png_level != 0 || P.png_device != 0) throw StatusError(MVS_ERR_INVALID, w + "image_format 1 takes png_level 0 and png_device 0");
        if (jpeg_base::check_params(P.jpeg_quality, P.jpeg_subsampling, msg) != MVS_OK) throw StatusError(MVS_ERR_INVALID, w + msg);
    }
    if (P.png_level < 0 || P.png_level > 9) throw StatusError(MVS_ERR_INVALID, w + "png_level 0 .. 9");
    if (P.png_device != 0 && P.png_device != 1) throw StatusError(MVS_ERR_INVALID, w + "png_device 0 or 1");
    if (P.png_device == 1 && P.png_level != 0) throw StatusError(MVS_ERR_INVALID, w + "png_device 1 takes png_level 0");
    if (P.png_level > 0 && in.n_atlases && !png_zlib_available()) throw StatusError(MVS_ERR_UNSUPPORTED, w + "libz.so.1 not found (png_level 0 needs no library)");
    if (in.n_atlases && (!in.atlas_size || !in.atlas_pix_ptr || (in.n_pixels && !in.image))) throw StatusError(MVS_ERR_INVALID, w + "null array in the atlas set");
}

void model_for_each_image(mvs_ctx* ctx, const mvs_atlas_set& in, int atlases_on_device, const mvs_model_params& P, const char* who, const ModelImageSink& sink) {
    // sizes and offsets on the host, the pixels copied once, one atlas per thread at a time
    hipStream_t s = ctx->stream;
    const uint32_t A = in.n_atlases;
    const std::string w = std::string(who) + ": ";
    ImageSet S{{}, {}, {0}};
    if (A) S = read_image_arrays(ctx, A, in.atlas_size, in.atlas_size, in.atlas_pix_ptr, atlases_on_device);
    const std::vector<uint32_t>& size = S.w; const std::vector<uint64_t>& pix = S.pix;
    if (pix[0] != 0 || pix[A] != in.n_pixels) throw StatusError(MVS_ERR_INVALID, w + "atlas_pix_ptr does not run from 0 to n_pixels");
    for (uint32_t a = 0; a < A; ++a)
        if (!size[a] || pix[a + 1] < pix[a] || pix[a + 1] - pix[a] != (uint64_t)size[a] * size[a]) throw StatusError(MVS_ERR_INVALID, w + "atlas " + std::to_string(a) + ": size and atlas_pix_ptr do not agree");
    EncodedFiles files;   // png_device 1 or image_format 1: the finished files, encoded on the device
    const bool on_dev = P.png_device || P.image_format == 1;
    std::vector<uint8_t> own;   // the host route's pixels of a device-resident set
    const uint8_t* image = in.image;
    if (A && atlases_on_device && !on_dev) {
        own.resize(3 * (size_t)in.n_pixels + 1);
        if (in.n_pixels) MVS_HIP(hipMemcpyAsync(own.data(), in.image, 3 * (size_t)in.n_pixels, hipMemcpyDeviceToHost, s));
        MVS_HIP(hipStreamSynchronize(s));
        image = own.data();
    }
    if (P.image_format == 1 && A) { mvs_jpeg_stats jst{}; jpeg_encode_images(ctx, A, size.data(), size.data(), pix.data(), in.image, atlases_on_device, P.jpeg_quality, P.jpeg_subsampling, files, jst); }
    else if (P.png_device && A) { mvs_png_stats pst{}; png_encode_images(ctx, A, size.data(), size.data(), pix.data(), in.image, atlases_on_device, files, pst); }
    std::atomic<int> failed{MVS_OK};
    std::vector<std::string> errs(A);
    for_each_on_threads(A, [&](uint32_t a) {
        mvs_status r;
        if (on_dev) r = sink(a, files.data + files.offsets[a], (size_t)(files.offsets[a + 1] - files.offsets[a]), errs[a]);
        else {
            std::vector<uint8_t> png;
            r = encode_png(image + 3 * (size_t)pix[a], size[a], size[a], P.png_level, png, errs[a]);
            if (r == MVS_OK) r = sink(a, png.data(), png.size(), errs[a]);
        }
        if (r != MVS_OK) failed.store(r);
    });
    if (failed.load() != MVS_OK)
        for (uint32_t a = 0; a < A; ++a) if (!errs[a].empty()) throw StatusError((mvs_status)failed.load(), w + errs[a]);
}

}  // namespace mvs

using namespace mvs;

extern "C" {

void mvs_model_default_params(mvs_model_params* p) {
    if (!p) return;
    p->max_bytes = 0; p->png_level = 0; p->png_device = 0;
    p->image_format = 0; p->jpeg_quality = 90; p->jpeg_subsampling = 1; p->glb_quantize = 0;
}

mvs_status mvs_ctx_build_model(mvs_ctx* ctx, const mvs_atlas_set* atlases, int atlases_on_device, const float* vertex_normals, int normals_on_device,
                               const char* name, const mvs_model_params* params, mvs_model_text* out, int out_on_device, mvs_model_stats* stats) {
    if (!ctx || !atlases || !name || !out) return api_fail(MVS_ERR_INVALID, "null argument");
    *out = mvs_model_text{};
    mvs_model_stats st{};
    if (stats) *stats = st;
    return api_guard([&] {
        MVS_HIP(hipSetDevice(ctx->device));
        hipStream_t s = ctx->stream;
        ModelDev& D = row_dev(ctx->model);
        const mvs_model_params P = params_or_default(params);
        run_with_stats(s, stats, st, [&] { run_model(ctx, D, *atlases, atlases_on_device, vertex_normals, normals_on_device, name, P, st); });
        const size_t NS = (size_t)atlases->n_atlases + 5;
        out->n_atlases = atlases->n_atlases; out->obj_bytes = D.obj_bytes; out->mtl_bytes = D.mtl_bytes;
        if (out_on_device) {
            out->obj = D.obj.p; out->mtl = D.mtl.p; out->section_ptr = D.h_sec.data(); out->section_bytes = D.h_sec_bytes.data();
        } else {
            download(s, out, mvs_model_text_free, [&] {
                out->obj = host_copy(D.obj.p, (size_t)D.obj_bytes, s); out->mtl = host_copy(D.mtl.p, (size_t)D.mtl_bytes, s);
                out->section_ptr = (uint64_t*)malloc(NS * sizeof(uint64_t)); out->section_bytes = (uint64_t*)malloc(NS * sizeof(uint64_t));
                if (!out->section_ptr || !out->section_bytes) throw StatusError(MVS_ERR_INVALID, "out of host memory");
                memcpy(out->section_ptr, D.h_sec.data(), NS * sizeof(uint64_t)); memcpy(out->section_bytes, D.h_sec_bytes.data(), NS * sizeof(uint64_t));
            });
        }
    });
}

void mvs_model_text_free(mvs_model_text* t) {
    if (!t) return;
    free(t->obj); free(t->mtl); free(t->section_ptr); free(t->section_bytes);
    *t = mvs_model_text{};
}

mvs_status mvs_ctx_save_model(mvs_ctx* ctx, const mvs_atlas_set* atlases, int atlases_on_device, const float* vertex_normals, int normals_on_device,
                              const char* prefix, const mvs_model_params* params, mvs_model_stats* stats) {
    if (!ctx || !atlases || !prefix) return api_fail(MVS_ERR_INVALID, "null argument");
    mvs_model_stats st{};
    if (stats) *stats = st;
    return api_guard([&] {
        MVS_HIP(hipSetDevice(ctx->device));
        hipStream_t s = ctx->stream;
        ModelDev& D = row_dev(ctx->model);
        const mvs_model_params P = params_or_default(params);
        const mvs_atlas_set& in = *atlases;
        model_check_image_params(P, in, "save_model");
        const std::string pre(prefix), name = pre.substr(pre.find_last_of('/') == std::string::npos ? 0 : pre.find_last_of('/') + 1);
        run_with_stats(s, stats, st, [&] {
            run_model(ctx, D, in, atlases_on_device, vertex_normals, normals_on_device, name, P, st);
            std::string msg; double ms_copy = 0.0;
            const double t0 = now_ms_host();
            mvs_status rc = device_to_file(ctx, D.obj.p, D.obj_bytes, pre + ".obj", ms_copy, msg);
            if (rc == MVS_OK) rc = device_to_file(ctx, D.mtl.p, D.mtl_bytes, pre + ".mtl", ms_copy, msg);
            st.ms_download = (float)ms_copy; st.ms_files = (float)(now_ms_host() - t0 - ms_copy);
            if (rc != MVS_OK) throw StatusError(rc, "save_model: " + msg);
            // ---- the images: one file per atlas, written by the thread that holds its bytes ----
            const double t1 = now_ms_host();
            try {
                model_for_each_image(ctx, in, atlases_on_device, P, "save_model", [&](uint32_t a, const uint8_t* bytes, size_t n, std::string& err) {
                    return write_file((pre + "_material" + model_filled4(a) + (P.image_format == 1 ? "_map_Kd.jpg" : "_map_Kd.png")).c_str(), bytes, n, err);
                });
            } catch (...) { st.ms_png = (float)(now_ms_host() - t1); throw; }
            st.ms_png = (float)(now_ms_host() - t1);
        });
    });
}

mvs_status mvs_write_png(const char* path, const uint8_t* rgb, uint32_t width, uint32_t height, int32_t level) {
    std::string msg;
    const mvs_status st = write_png(path, rgb, width, height, level, msg);
    return st == MVS_OK ? MVS_OK : api_fail(st, msg);
}

}  // extern "C"
