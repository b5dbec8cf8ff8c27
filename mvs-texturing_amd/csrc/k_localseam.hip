// k_localseam.hip -- row f7: tex::local_seam_leveling (local_seam_leveling.cpp:20-204, seam_leveling.cpp:16-91,
//   texture_patch.cpp:118-297, poisson_blending.cpp:21-138), labelled faces only; the tone mapping is not read here -- the row works on the patch images it is given.  The definition (DESIGN.md
//   section 4 "Local seam leveling") is shared with the CPU model of the tests (tests/tools/blend_model.cpp): every output is
//   bit-identical to it.  Phases, all on the context's stream:
//   topology  sorted (vertex, 3 * list entry + corner) keys give every vertex's infos (patches ascending, first entry first); one
//             thread per adjacency slot finds the seam edges in upstream's order, one per seam edge its projections and sample count;
//   colours   one thread per edge sample / per vertex: the mean of the bilinear samples over the projections in order;
//   writes    one thread per writer (vertex pixel or Bresenham line) walks its pixels twice: an integer atomicMax of its sequence
//             number per pixel, then the winner writes its colour (the colour depends on writer and pixel only) -- no float atomics;
//   mask      chessboard distance to the nearest invalid-or-outside pixel in two separable passes, sanitize / inner / last border,
//             then the unknowns (255 with four usable neighbours), their row-major ranks (one scan) and validity after the blend;
//   solve     one workgroup per patch, all iterations in one launch: p (pixel-indexed), r and the unknown list in LDS (or, for a
//             patch too large, in global memory: the same code on another pointer), x in the output image, the five-point product
//             recomputed instead of stored, the three channels together with their own scalars and stop state, every dot product
//             by the one tree of the definition (lane l of 1024 adds unknowns l, l + 1024, ... in order; the lanes halve): a workgroup of 256
//             owns four lanes per thread (LDS), one of 1024 one each (global memory).
#include "rows.h"
#include <cfloat>
#include <climits>
#include <cmath>

namespace mvs {

// per-context buffers of row f7, allocated on first use, freed with the context (lsl_release)
struct LslDev {
    // staged inputs (host callers)
    DBuf<uint32_t> in_label, in_face_ptr, in_faces; DBuf<int4> in_box; DBuf<float> in_texcoords, in_image;
    DBuf<unsigned long long> in_pix_ptr; DBuf<uint8_t> in_validity, in_blending;
    // topology
    DBuf<uint32_t> epid, flag, idx, info_head, vptr, sflag, sidx, edge_v, ep_cnt, ep_ptr, ep_patch, ep_c1, ep_c2, ep_edge, en, ecol_ptr, flags;
    DBuf<unsigned long long> keys, keys2, c64;
    // colours, writes
    DBuf<float> ecol, vcol; DBuf<uint32_t> win;
    // masks, solve
    DBuf<uint8_t> blendw, hv, unk; DBuf<uint32_t> rank, chunk_ptr, chunk_patch, n_unk, order, iters; DBuf<float> err, scratch; DBuf<unsigned long long> goff;
    // outputs
    DBuf<float> image; DBuf<uint8_t> validity, mask;
};
void lsl_release(mvs_ctx* ctx) { delete ctx->lsl; ctx->lsl = nullptr; }

namespace {
constexpr uint32_t CHUNK = 1024;              // pixels of one patch a per-pixel block handles
constexpr uint32_t LDS_MAX = 147456;           // dynamic LDS of a solve workgroup at most (the CU's 160 KiB less the 12 KiB of the reduction arrays and a margin)
constexpr uint32_t MAX_SAMPLES = 1u << 22;    // samples of one edge at most (texture coordinates are bounded by 2^20)
constexpr float TC_MAX = 1048576.0f;
enum { F_FACE = 0, F_LABEL, F_VERTEX, F_ADJ, F_TC, F_N };   // flag words
enum { K_SKIPPED = 0, K_SAMPLES, K_BAD_SAMPLES, K_VWRITES, K_LWRITES, K_WRITTEN, K_OUTSIDE, K_BAD_WRITES, K_STRIP, K_FIXED, K_DEMOTED, K_NSAMPLES, K_N };   // 64-bit counters

struct Patches {   // the patch set on the device
    uint32_t P, L; const uint32_t* label; const int4* box; const uint32_t* face_ptr; const uint32_t* faces; const float* texcoords;
    const unsigned long long* pix_ptr; const float* image; const uint8_t* validity; const uint8_t* blending;
};

// ---- topology ----
// one thread per list entry: its patch, the checks, its three keys (vertex << 32 | 3 e + k)
__global__ void ls_entry_kernel(Patches S, const uint32_t* __restrict__ mfaces, const uint32_t* __restrict__ labels, uint32_t F, uint32_t NV,
                                uint32_t* __restrict__ epid, unsigned long long* __restrict__ keys, uint32_t* __restrict__ flags) {
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= S.L) return;
    uint32_t lo = 0, hi = S.P;   // the last patch whose list starts at or before e (empty lists share their start with the next)
    while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (S.face_ptr[mid] <= e) lo = mid; else hi = mid; }
    epid[e] = lo;
    const uint32_t f = S.faces[e];
    bool ok = f < F;
    if (!ok) flags[F_FACE] = 1u;
    else if (labels[f] != S.label[lo]) flags[F_LABEL] = 1u;
    for (int k = 0; k < 6; ++k) { const float t = S.texcoords[6 * (size_t)e + k]; if (!(fabsf(t) <= TC_MAX)) flags[F_TC] = 1u; }
    for (int k = 0; k < 3; ++k) {
        uint32_t v = ok ? mfaces[3 * (size_t)f + k] : 0u;
        if (v >= NV) { flags[F_VERTEX] = 1u; v = 0u; }
        keys[3 * (size_t)e + k] = ((unsigned long long)v << 32) | (unsigned long long)(3u * e + (uint32_t)k);
    }
}
__device__ inline uint32_t key_v(unsigned long long k) { return (uint32_t)(k >> 32); }
__device__ inline uint32_t key_c(unsigned long long k) { return (uint32_t)k; }
// one thread per sorted key: 1 where a (vertex, patch) info starts
__global__ void ls_head_kernel(const unsigned long long* __restrict__ keys, uint32_t n, const uint32_t* __restrict__ epid, uint32_t* __restrict__ flag) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n) return;
    if (i == n) { flag[i] = 0u; return; }
    flag[i] = (i == 0 || key_v(keys[i]) != key_v(keys[i - 1]) || epid[key_c(keys[i]) / 3u] != epid[key_c(keys[i - 1]) / 3u]) ? 1u : 0u;
}
__global__ void ls_info_kernel(const uint32_t* __restrict__ flag, const uint32_t* __restrict__ idx, uint32_t n, uint32_t* __restrict__ info_head) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && flag[i]) info_head[idx[i]] = i;
}
// vptr[v] = the first sorted key of vertex v or a later one
__global__ void ls_vptr_kernel(const unsigned long long* __restrict__ keys, uint32_t n, uint32_t NV, uint32_t* __restrict__ vptr) {
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v > NV) return;
    uint32_t lo = 0, hi = n;
    while (lo < hi) { const uint32_t mid = lo + ((hi - lo) >> 1); if (key_v(keys[mid]) < v) lo = mid + 1; else hi = mid; }
    vptr[v] = lo;
}
// find_seam_edges: the shared vertices of two faces as upstream's double loop collects them; true when there are exactly two, distinct
__device__ inline bool shared_edge(const uint32_t* __restrict__ mfaces, uint32_t a, uint32_t b, uint32_t& v1, uint32_t& v2) {
    uint32_t n = 0, s[2] = {0u, 0u};
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) if (mfaces[3 * (size_t)a + i] == mfaces[3 * (size_t)b + j]) { if (n < 2) s[n] = mfaces[3 * (size_t)a + i]; ++n; }
    if (n != 2 || s[0] == s[1]) return false;
    v1 = min(s[0], s[1]); v2 = max(s[0], s[1]);
    return true;
}
// one thread per adjacency slot: fill = 0 flags the seam edges, fill = 1 writes them at their scanned places
__global__ void ls_seam_kernel(const uint32_t* __restrict__ adj_ptr, const uint32_t* __restrict__ adj, const uint32_t* __restrict__ labels,
                               const uint32_t* __restrict__ mfaces, uint32_t F, uint32_t NV, uint32_t E, int fill, uint32_t* __restrict__ sflag,
                               const uint32_t* __restrict__ sidx, uint32_t* __restrict__ edge_v, uint32_t* __restrict__ flags, unsigned long long* __restrict__ c64) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s > E) return;
    if (s == E) { if (!fill) sflag[s] = 0u; return; }
    if (fill) {
        if (!sflag[s]) return;
    } else sflag[s] = 0u;
    uint32_t lo = 0, hi = F;   // the node of this slot: the last one whose list starts at or before s
    while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (adj_ptr[mid] <= s) lo = mid; else hi = mid; }
    const uint32_t node = lo, a = adj[s];
    if (a >= F) { flags[F_ADJ] = 1u; return; }
    if (node > a || labels[node] == labels[a]) return;
    uint32_t v1, v2;
    if (!shared_edge(mfaces, node, a, v1, v2)) { if (!fill) atomicAdd(c64 + K_SKIPPED, 1ull); return; }
    if (v2 >= NV) { flags[F_VERTEX] = 1u; return; }   // a face outside every list may still hold a bad vertex id
    if (!fill) sflag[s] = 1u;
    else { edge_v[2 * (size_t)sidx[s]] = v1; edge_v[2 * (size_t)sidx[s] + 1] = v2; }
}
__device__ inline float norm2(float dx, float dy) { return sqrtf(dx * dx + dy * dy); }
// one thread per seam edge: its projections (find_mesh_edge_projections: one per patch holding a face with both vertices, patches
// ascending), then max_length and the sample count
__global__ void ls_eproj_kernel(uint32_t NE, const uint32_t* __restrict__ edge_v, const unsigned long long* __restrict__ keys,
                                const uint32_t* __restrict__ vptr, const uint32_t* __restrict__ epid, Patches S, const uint32_t* __restrict__ mfaces,
                                int fill, uint32_t* __restrict__ ep_cnt, const uint32_t* __restrict__ ep_ptr, uint32_t* __restrict__ ep_patch,
                                uint32_t* __restrict__ ep_c1, uint32_t* __restrict__ ep_c2, uint32_t* __restrict__ ep_edge, uint32_t* __restrict__ en,
                                uint32_t* __restrict__ flags, unsigned long long* __restrict__ c64) {
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e > NE) return;
    if (e == NE) { if (!fill) ep_cnt[e] = 0u; else en[e] = 0u; return; }
    const uint32_t v1 = edge_v[2 * (size_t)e], v2 = edge_v[2 * (size_t)e + 1];
    uint32_t cnt = 0, last = 0xFFFFFFFFu, head = 0, cur = 0xFFFFFFFFu;
    float max_length = 1.0f;
    for (uint32_t i = vptr[v1]; i < vptr[v1 + 1]; ++i) {
        const uint32_t c = key_c(keys[i]), le = c / 3u, p = epid[le];
        if (p != cur) { cur = p; head = i; }
        if (p == last) continue;
        const uint32_t f = S.faces[le];
        if (mfaces[3 * (size_t)f] != v2 && mfaces[3 * (size_t)f + 1] != v2 && mfaces[3 * (size_t)f + 2] != v2) continue;
        last = p;
        if (fill) {
            uint32_t lo = vptr[v2], hi = vptr[v2 + 1];   // v2's first key in patch p: entries of p are [face_ptr[p], face_ptr[p + 1])
            const uint32_t first = S.face_ptr[p];
            while (lo < hi) { const uint32_t mid = lo + ((hi - lo) >> 1); if (key_c(keys[mid]) / 3u < first) lo = mid + 1; else hi = mid; }
            const uint32_t c1 = key_c(keys[head]), c2 = key_c(keys[lo]);
            const size_t o = (size_t)ep_ptr[e] + cnt;
            ep_patch[o] = p; ep_c1[o] = c1; ep_c2[o] = c2; ep_edge[o] = e;
            const float length = norm2(S.texcoords[2 * (size_t)c1] - S.texcoords[2 * (size_t)c2], S.texcoords[2 * (size_t)c1 + 1] - S.texcoords[2 * (size_t)c2 + 1]);
            max_length = fmaxf(max_length, length);
        }
        ++cnt;
    }
    if (!fill) { ep_cnt[e] = cnt; return; }
    const float nf = ceilf(max_length * 2.0f);
    uint32_t n = 2u;
    if (!(nf <= (float)MAX_SAMPLES)) flags[F_TC] = 1u; else n = (uint32_t)nf;
    en[e] = n;
    atomicAdd(c64 + K_NSAMPLES, (unsigned long long)n);
}

// ---- colours ----
struct Frame { int w, h; unsigned long long base; };
__device__ inline Frame frame_of(const Patches& S, uint32_t p) { const int4 b = S.box[p]; return Frame{b.z, b.w, S.pix_ptr[p]}; }
// mve::Image<float>::linear_at (item 6 of "Global seam leveling" on the float image) and TexturePatch::valid_pixel(Vec2f)
__device__ inline bool linear_at(const Patches& S, const Frame& fr, float x, float y, float* out) {
    const float width = (float)fr.w, height = (float)fr.h;
    bool valid = 0.0f <= x && x < width && 0.0f <= y && y < height;
    const float W1 = (float)(fr.w - 1), H1 = (float)(fr.h - 1);
    x = (x < W1) ? x : W1; x = (0.0f < x) ? x : 0.0f;
    y = (y < H1) ? y : H1; y = (0.0f < y) ? y : 0.0f;
    const int fx = (int)x, fy = (int)y;
    const int fx1 = min(fx + 1, fr.w - 1), fy1 = min(fy + 1, fr.h - 1);
    const float w1 = x - (float)fx, w0 = 1.0f - w1, w3 = y - (float)fy, w2 = 1.0f - w3;
    const unsigned long long i1 = fr.base + (unsigned long long)fy * fr.w + fx, i2 = fr.base + (unsigned long long)fy * fr.w + fx1;
    const unsigned long long i3 = fr.base + (unsigned long long)fy1 * fr.w + fx, i4 = fr.base + (unsigned long long)fy1 * fr.w + fx1;
    for (int ch = 0; ch < 3; ++ch) {
        const float v1 = S.image[3 * i1 + ch], v2 = S.image[3 * i2 + ch], v3 = S.image[3 * i3 + ch], v4 = S.image[3 * i4 + ch];
        out[ch] = ((v1 * (w0 * w2) + v2 * (w1 * w2)) + v3 * (w0 * w3)) + v4 * (w1 * w3);
    }
    if (valid)
        valid = (w0 * w2 == 0.0f || S.validity[i1] == 255) && (w1 * w2 == 0.0f || S.validity[i2] == 255) &&
                (w0 * w3 == 0.0f || S.validity[i3] == 255) && (w1 * w3 == 0.0f || S.validity[i4] == 255);
    return valid;
}
// one thread per edge sample: mean_color_of_edge_point
__global__ void ls_edge_colour_kernel(uint32_t NS, uint32_t NE, const uint32_t* __restrict__ ecol_ptr, const uint32_t* __restrict__ en,
                                      const uint32_t* __restrict__ ep_ptr, const uint32_t* __restrict__ ep_patch, const uint32_t* __restrict__ ep_c1,
                                      const uint32_t* __restrict__ ep_c2, Patches S, float* __restrict__ ecol, unsigned long long* __restrict__ c64) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= NS) return;
    uint32_t lo = 0, hi = NE;   // every edge has at least two samples
    while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (ecol_ptr[mid] <= s) lo = mid; else hi = mid; }
    const uint32_t e = lo, j = s - ecol_ptr[e], n = en[e];
    const float t = (float)j / (float)(n - 1u);
    float sum[3] = {0.0f, 0.0f, 0.0f}, wsum = 0.0f;
    uint32_t bad = 0, taken = 0;
    for (uint32_t o = ep_ptr[e]; o < ep_ptr[e + 1]; ++o) {
        const float* a = S.texcoords + 2 * (size_t)ep_c1[o]; const float* b = S.texcoords + 2 * (size_t)ep_c2[o];
        const float px = a[0] * t + (1.0f - t) * b[0], py = a[1] * t + (1.0f - t) * b[1];
        float col[3];
        if (!linear_at(S, frame_of(S, ep_patch[o]), px, py, col)) ++bad;
        for (int ch = 0; ch < 3; ++ch) sum[ch] = sum[ch] + col[ch] * 1.0f;
        wsum = wsum + 1.0f; ++taken;
    }
    for (int ch = 0; ch < 3; ++ch) ecol[3 * (size_t)s + ch] = sum[ch] / wsum;
    if (taken) atomicAdd(c64 + K_SAMPLES, (unsigned long long)taken);
    if (bad) atomicAdd(c64 + K_BAD_SAMPLES, (unsigned long long)bad);
}
// one thread per vertex with more than one info: the mean over its infos in order
__global__ void ls_vertex_colour_kernel(uint32_t NV, const uint32_t* __restrict__ vptr, const uint32_t* __restrict__ idx, const uint32_t* __restrict__ info_head,
                                        const unsigned long long* __restrict__ keys, const uint32_t* __restrict__ epid, Patches S, float* __restrict__ vcol,
                                        unsigned long long* __restrict__ c64) {
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= NV) return;
    const uint32_t i0 = idx[vptr[v]], i1 = idx[vptr[v + 1]];
    if (i1 - i0 <= 1) return;
    float sum[3] = {0.0f, 0.0f, 0.0f}, wsum = 0.0f;
    uint32_t bad = 0;
    for (uint32_t i = i0; i < i1; ++i) {
        const uint32_t c = key_c(keys[info_head[i]]);
        float col[3];
        if (!linear_at(S, frame_of(S, epid[c / 3u]), S.texcoords[2 * (size_t)c], S.texcoords[2 * (size_t)c + 1], col)) ++bad;
        for (int ch = 0; ch < 3; ++ch) sum[ch] = sum[ch] + col[ch] * 1.0f;
        wsum = wsum + 1.0f;
    }
    for (int ch = 0; ch < 3; ++ch) vcol[3 * (size_t)v + ch] = sum[ch] / wsum;
    atomicAdd(c64 + K_SAMPLES, (unsigned long long)(i1 - i0));
    if (bad) atomicAdd(c64 + K_BAD_SAMPLES, (unsigned long long)bad);
}

// ---- writes ----
struct WriteOut { uint32_t* win; float* image; uint8_t* blendw; unsigned long long* c64; };
// pass 0: the winner word; pass 1: the winner writes.  seq = the write's place in upstream's sequence for this patch (any patch: the
// numbering is global and monotone inside every patch)
template <int PASS>
__device__ inline void put_pixel(const Patches& S, const Frame& fr, int x, int y, uint32_t seq, const float* col, const WriteOut& O, unsigned long long* counter) {
    if (x < 0 || y < 0 || x >= fr.w || y >= fr.h) { if (PASS == 0) { atomicAdd(counter, 1ull); atomicAdd(O.c64 + K_OUTSIDE, 1ull); } return; }
    const unsigned long long i = fr.base + (unsigned long long)y * fr.w + x;
    if (PASS == 0) {
        atomicAdd(counter, 1ull);
        if (S.validity[i] == 0) atomicAdd(O.c64 + K_BAD_WRITES, 1ull);
        atomicMax(O.win + i, seq);
    } else if (O.win[i] == seq) {
        O.image[3 * i] = col[0]; O.image[3 * i + 1] = col[1]; O.image[3 * i + 2] = col[2]; O.blendw[i] = 128;
        atomicAdd(O.c64 + K_WRITTEN, 1ull);
    }
}
template <int PASS>
__global__ void ls_write_kernel(uint32_t NI, uint32_t NEP, const uint32_t* __restrict__ info_head, const unsigned long long* __restrict__ keys,
                                const uint32_t* __restrict__ vptr, const uint32_t* __restrict__ idx, const uint32_t* __restrict__ epid,
                                const uint32_t* __restrict__ ep_patch, const uint32_t* __restrict__ ep_c1, const uint32_t* __restrict__ ep_c2,
                                const uint32_t* __restrict__ ep_edge, const uint32_t* __restrict__ en, const uint32_t* __restrict__ ecol_ptr,
                                const float* __restrict__ ecol, const float* __restrict__ vcol, Patches S, WriteOut O) {
    const uint32_t wid = blockIdx.x * blockDim.x + threadIdx.x;
    if (wid >= NI + NEP) return;
    if (wid < NI) {   // a vertex pixel: Vec2i(projection + 0.5f), C truncation
        const unsigned long long k = keys[info_head[wid]];
        const uint32_t v = key_v(k), c = key_c(k);
        if (idx[vptr[v + 1]] - idx[vptr[v]] <= 1) return;
        const int x = (int)(S.texcoords[2 * (size_t)c] + 0.5f), y = (int)(S.texcoords[2 * (size_t)c + 1] + 0.5f);
        put_pixel<PASS>(S, frame_of(S, epid[c / 3u]), x, y, wid + 1u, vcol + 3 * (size_t)v, O, O.c64 + K_VWRITES);
        return;
    }
    const uint32_t o = wid - NI, e = ep_edge[o], n = en[e];   // draw_line
    const float* col = ecol + 3 * (size_t)ecol_ptr[e];
    const Frame fr = frame_of(S, ep_patch[o]);
    const float* a = S.texcoords + 2 * (size_t)ep_c1[o]; const float* b = S.texcoords + 2 * (size_t)ep_c2[o];
    const int x0 = (int)(a[0] + 0.5f), y0 = (int)(a[1] + 0.5f), x1 = (int)(b[0] + 0.5f), y1 = (int)(b[1] + 0.5f);
    float tdx = (float)(x1 - x0), tdy = (float)(y1 - y0);
    const float length = sqrtf(tdx * tdx + tdy * tdy);
    const int dx = abs(x1 - x0), dy = abs(y1 - y0), sx = x0 < x1 ? 1 : -1, sy = y0 < y1 ? 1 : -1;
    int err = dx - dy, x = x0, y = y0;
    for (;;) {
        tdx = (float)(x1 - x); tdy = (float)(y1 - y);
        const float t = (length != 0.0f) ? sqrtf(tdx * tdx + tdy * tdy) / length : 0.5f;
        float c3[3];
        if (t < 1.0f && n > 1u) {
            uint32_t q = (uint32_t)floorf(t * (float)(n - 1u));
            if (q > n - 2u) q = n - 2u;   // t * (n - 1) can round up to n - 1: upstream would read past the end
            for (int ch = 0; ch < 3; ++ch) c3[ch] = (1.0f - t) * col[3 * (size_t)q + ch] + t * col[3 * (size_t)(q + 1u) + ch];
        } else {
            for (int ch = 0; ch < 3; ++ch) c3[ch] = col[3 * (size_t)(n - 1u) + ch];
        }
        put_pixel<PASS>(S, fr, x, y, wid + 1u, c3, O, O.c64 + K_LWRITES);
        if (x == x1 && y == y1) break;
        const int e2 = 2 * err;
        if (e2 > -dy) { err -= dy; x += sx; }
        if (e2 < dx) { err += dx; y += sy; }
    }
}

// ---- masks ----
// the patch and the pixel of thread t of a chunk block; false past the patch's end
__device__ inline bool chunk_pixel(const Patches& S, const uint32_t* __restrict__ chunk_ptr, const uint32_t* __restrict__ chunk_patch, uint32_t r,
                                   Frame& fr, int& x, int& y, unsigned long long& i) {
    const uint32_t p = chunk_patch[blockIdx.x];
    fr = frame_of(S, p);
    const unsigned long long j = (unsigned long long)(blockIdx.x - chunk_ptr[p]) * CHUNK + r * 256u + threadIdx.x;
    if (j >= (unsigned long long)fr.w * (unsigned long long)fr.h) return false;
    y = (int)(j / (unsigned long long)fr.w); x = (int)(j - (unsigned long long)y * (unsigned long long)fr.w);
    i = fr.base + j;
    return true;
}
// hv = min(cap, distance along the row to the nearest invalid pixel or the frame's outside)
__global__ void __launch_bounds__(256) ls_hv_kernel(Patches S, const uint32_t* __restrict__ chunk_ptr, const uint32_t* __restrict__ chunk_patch, int cap,
                                                    uint8_t* __restrict__ hv) {
    for (uint32_t r = 0; r < CHUNK / 256; ++r) {
        Frame fr; int x, y; unsigned long long i;
        if (!chunk_pixel(S, chunk_ptr, chunk_patch, r, fr, x, y, i)) return;
        int d = 0;
        if (S.validity[i] != 0) {
            d = min(min(x + 1, fr.w - x), cap);
            for (int k = 1; k < d; ++k) if (S.validity[i - k] == 0 || S.validity[i + k] == 0) { d = k; break; }
        }
        hv[i] = (uint8_t)d;
    }
}
// prepare_blending_mask in its distance form: d = chessboard distance to the nearest invalid-or-outside pixel (capped at strip + 2);
// sanitize on the mask after the writes, then d > strip: 0, d == strip + 1: 128
__global__ void __launch_bounds__(256) ls_mask_kernel(Patches S, const uint32_t* __restrict__ chunk_ptr, const uint32_t* __restrict__ chunk_patch, int strip,
                                                      const uint8_t* __restrict__ hv, const uint8_t* __restrict__ blendw, uint8_t* __restrict__ mask) {
    for (uint32_t r = 0; r < CHUNK / 256; ++r) {
        Frame fr; int x, y; unsigned long long i;
        if (!chunk_pixel(S, chunk_ptr, chunk_patch, r, fr, x, y, i)) return;
        int d = min((int)hv[i], min(y + 1, fr.h - y));
        for (int k = 1; k < d; ++k) {
            const int m = min((int)hv[i - (unsigned long long)k * fr.w], (int)hv[i + (unsigned long long)k * fr.w]);
            d = min(d, max(k, m));
        }
        uint8_t b = blendw[i];
        if (b == 128 && x >= 1 && y >= 1 && x < fr.w - 1 && y < fr.h - 1 &&
            blendw[i - 1] == 255 && blendw[i + 1] == 255 && blendw[i - fr.w] == 255 && blendw[i + fr.w] == 255) b = 255;
        if (d == strip + 1) b = 128; else if (d > strip) b = 0;
        mask[i] = b;
    }
}
// the unknowns (255, not on the frame's edge, no 4-neighbour of mask 0), the counts, validity after the blend
__global__ void __launch_bounds__(256) ls_class_kernel(Patches S, const uint32_t* __restrict__ chunk_ptr, const uint32_t* __restrict__ chunk_patch,
                                                       const uint8_t* __restrict__ mask, uint8_t* __restrict__ unk, uint8_t* __restrict__ validity,
                                                       unsigned long long* __restrict__ c64) {
    __shared__ uint32_t s_cnt[3];
    if (threadIdx.x < 3) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    uint32_t ns = 0, nf = 0, nd = 0;
    for (uint32_t r = 0; r < CHUNK / 256; ++r) {
        Frame fr; int x, y; unsigned long long i;
        if (!chunk_pixel(S, chunk_ptr, chunk_patch, r, fr, x, y, i)) break;
        const uint8_t m = mask[i];
        uint8_t u = 0;
        if (m == 255) {
            if (x >= 1 && y >= 1 && x < fr.w - 1 && y < fr.h - 1 && mask[i - 1] != 0 && mask[i + 1] != 0 && mask[i - fr.w] != 0 && mask[i + fr.w] != 0) { u = 1; ++ns; }
            else ++nd;
        } else if (m == 64 || m == 128) ++nf;
        unk[i] = u;
        validity[i] = (m == 64) ? (uint8_t)0 : S.validity[i];
    }
    if (ns) atomicAdd(&s_cnt[0], ns);
    if (nf) atomicAdd(&s_cnt[1], nf);
    if (nd) atomicAdd(&s_cnt[2], nd);
    __syncthreads();
    if (threadIdx.x == 0) {
        if (s_cnt[0]) atomicAdd(c64 + K_STRIP, (unsigned long long)s_cnt[0]);
        if (s_cnt[1]) atomicAdd(c64 + K_FIXED, (unsigned long long)s_cnt[1]);
        if (s_cnt[2]) atomicAdd(c64 + K_DEMOTED, (unsigned long long)s_cnt[2]);
    }
}
__global__ void ls_count_kernel(Patches S, const uint32_t* __restrict__ rank, uint32_t* __restrict__ n_unk) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p < S.P) n_unk[p] = rank[S.pix_ptr[p + 1]] - rank[S.pix_ptr[p]];
}

// ---- solve ----
constexpr uint32_t LANES = 1024;   // lanes of the reduction tree of item 9
// the tree of item 9 for three sums at once: lane l of 1024 holds the sequential sum of its unknowns l, l + 1024, ...; the lanes halve.
// A thread of a workgroup of THREADS owns the lanes t, t + THREADS, ...
template <int THREADS>
__device__ inline void block_sum3(const float (*v)[3], float* out, float* red) {
    constexpr int V = LANES / THREADS;
    const uint32_t t = threadIdx.x;
#pragma unroll
    for (int q = 0; q < V; ++q) { red[q * THREADS + t] = v[q][0]; red[LANES + q * THREADS + t] = v[q][1]; red[2 * LANES + q * THREADS + t] = v[q][2]; }
    __syncthreads();
    for (uint32_t s = LANES / 2; s >= 1; s >>= 1) {
        for (uint32_t i = t; i < s; i += THREADS) { red[i] = red[i] + red[i + s]; red[LANES + i] = red[LANES + i] + red[LANES + i + s]; red[2 * LANES + i] = red[2 * LANES + i] + red[2 * LANES + i + s]; }
        __syncthreads();
    }
    out[0] = red[0]; out[1] = red[LANES]; out[2] = red[2 * LANES];
    __syncthreads();
}
// every unknown of this thread, lane by lane: k = k0 + q * THREADS, in ascending order within each lane q
#define LS_FOR_UNKNOWNS(q, k)                                   \
    for (uint32_t k0 = t; k0 < n; k0 += LANES)                  \
        _Pragma("unroll") for (int q = 0; q < V; ++q)           \
            if (const uint32_t k = k0 + (uint32_t)q * THREADS; k < n)
// one workgroup per patch.  Working set: pv[3 npix] (p, pixel-indexed, 0 on fixed pixels), rv[3 n], list[n] -- in dynamic LDS
// (IN_LDS, 256 threads) or at goff[block] of the global scratch (1024 threads: these are the large patches).  x is the output image.
template <bool IN_LDS, int THREADS>
__global__ void __launch_bounds__(THREADS) ls_solve_kernel(Patches S, const uint32_t* __restrict__ order, const unsigned long long* __restrict__ goff,
                                                           float* __restrict__ scratch, const uint8_t* __restrict__ unk, const uint32_t* __restrict__ rank,
                                                           float* __restrict__ X, float tol, uint32_t max_iters, uint32_t* __restrict__ iters_out,
                                                           float* __restrict__ err_out) {
    constexpr int V = LANES / THREADS;
    extern __shared__ float smem[];
    __shared__ float red[3 * LANES];
    const uint32_t p = order[blockIdx.x], t = threadIdx.x;
    const Frame fr = frame_of(S, p);
    const uint32_t npix = (uint32_t)fr.w * (uint32_t)fr.h, r0 = rank[fr.base], n = rank[fr.base + npix] - r0;
    const int w = fr.w;
    float* pv = IN_LDS ? smem : scratch + goff[blockIdx.x];
    float* rv = pv + 3 * (size_t)npix;
    uint32_t* list = (uint32_t*)(rv + 3 * (size_t)n);
    for (uint32_t j = t; j < npix; j += THREADS) {
        const unsigned long long i = fr.base + j;
        const bool u = unk[i] != 0;
        if (u) list[rank[i] - r0] = j;
        for (int ch = 0; ch < 3; ++ch) pv[3 * (size_t)j + ch] = u ? X[3 * i + ch] : 0.0f;
    }
    __syncthreads();
    // the right-hand side (item 8, fixed neighbours folded in, sign flipped) and r0 = rhs - A x0
    float acc[V][3], acc2[V][3], bb[3], rr[3];
#pragma unroll
    for (int q = 0; q < V; ++q) for (int ch = 0; ch < 3; ++ch) { acc[q][ch] = 0.0f; acc2[q][ch] = 0.0f; }
    LS_FOR_UNKNOWNS(q, k) {
        const uint32_t j = list[k];
        const unsigned long long i = fr.base + j;
        const unsigned long long nb[4] = {i - w, i - 1, i + 1, i + w};
        for (int ch = 0; ch < 3; ++ch) {
            const float ls = (((-4.0f * S.image[3 * i + ch] + S.image[3 * nb[0] + ch]) + S.image[3 * nb[1] + ch]) + S.image[3 * nb[2] + ch]) + S.image[3 * nb[3] + ch];
            const float ld = (((-4.0f * X[3 * i + ch] + X[3 * nb[0] + ch]) + X[3 * nb[1] + ch]) + X[3 * nb[2] + ch]) + X[3 * nb[3] + ch];
            const float b = 1.0f * ls + 0.0f * ld;
            float rhs = -b;
            for (int m = 0; m < 4; ++m) if (!unk[nb[m]]) rhs = rhs + X[3 * nb[m] + ch];
            const float ax = (((4.0f * pv[3 * (size_t)j + ch] - pv[3 * (size_t)(j - w) + ch]) - pv[3 * (size_t)(j - 1) + ch]) - pv[3 * (size_t)(j + 1) + ch]) - pv[3 * (size_t)(j + w) + ch];
            const float r = rhs - ax;
            rv[3 * (size_t)k + ch] = r;
            acc[q][ch] = acc[q][ch] + rhs * rhs; acc2[q][ch] = acc2[q][ch] + r * r;
        }
    }
    block_sum3<THREADS>(acc, bb, red);
    block_sum3<THREADS>(acc2, rr, red);
    float thr[3], abs_new[3], err[3], alpha[3], beta[3];
    uint32_t it[3] = {0u, 0u, 0u};
    bool active[3];
    for (int ch = 0; ch < 3; ++ch) {
        thr[ch] = fmaxf((tol * tol) * bb[ch], FLT_MIN);
        err[ch] = bb[ch] != 0.0f ? sqrtf(rr[ch] / bb[ch]) : 0.0f;
        active[ch] = n != 0u && bb[ch] != 0.0f && !(rr[ch] < thr[ch]) && max_iters > 0u;
        abs_new[ch] = rr[ch]; alpha[ch] = 0.0f; beta[ch] = 0.0f;
    }
    for (uint32_t k = t; k < n; k += THREADS) { const uint32_t j = list[k]; for (int ch = 0; ch < 3; ++ch) pv[3 * (size_t)j + ch] = rv[3 * (size_t)k + ch]; }
    __syncthreads();
    while (active[0] || active[1] || active[2]) {
        float pap[3], r2[3];
#pragma unroll
        for (int q = 0; q < V; ++q) for (int ch = 0; ch < 3; ++ch) acc[q][ch] = 0.0f;
        LS_FOR_UNKNOWNS(q, k) {
            const uint32_t j = list[k];
            for (int ch = 0; ch < 3; ++ch) {
                const float pj = pv[3 * (size_t)j + ch];
                const float ap = (((4.0f * pj - pv[3 * (size_t)(j - w) + ch]) - pv[3 * (size_t)(j - 1) + ch]) - pv[3 * (size_t)(j + 1) + ch]) - pv[3 * (size_t)(j + w) + ch];
                acc[q][ch] = acc[q][ch] + pj * ap;
            }
        }
        block_sum3<THREADS>(acc, pap, red);
        for (int ch = 0; ch < 3; ++ch) if (active[ch]) alpha[ch] = abs_new[ch] / pap[ch];
#pragma unroll
        for (int q = 0; q < V; ++q) for (int ch = 0; ch < 3; ++ch) acc[q][ch] = 0.0f;
        LS_FOR_UNKNOWNS(q, k) {
            const uint32_t j = list[k];
            const unsigned long long i = fr.base + j;
            for (int ch = 0; ch < 3; ++ch) {
                float r = rv[3 * (size_t)k + ch];
                if (active[ch]) {
                    const float pj = pv[3 * (size_t)j + ch];
                    const float ap = (((4.0f * pj - pv[3 * (size_t)(j - w) + ch]) - pv[3 * (size_t)(j - 1) + ch]) - pv[3 * (size_t)(j + 1) + ch]) - pv[3 * (size_t)(j + w) + ch];
                    X[3 * i + ch] = X[3 * i + ch] + alpha[ch] * pj;
                    r = r - alpha[ch] * ap;
                    rv[3 * (size_t)k + ch] = r;
                }
                acc[q][ch] = acc[q][ch] + r * r;
            }
        }
        block_sum3<THREADS>(acc, r2, red);   // ends with a barrier: every read of p above is done
        bool upd[3];
        for (int ch = 0; ch < 3; ++ch) {
            upd[ch] = false;
            if (!active[ch]) continue;
            err[ch] = sqrtf(r2[ch] / bb[ch]);
            if (r2[ch] < thr[ch]) { active[ch] = false; continue; }
            ++it[ch];
            if (it[ch] >= max_iters) { active[ch] = false; continue; }
            beta[ch] = r2[ch] / abs_new[ch]; abs_new[ch] = r2[ch]; upd[ch] = true;
        }
        for (uint32_t k = t; k < n; k += THREADS) {
            const uint32_t j = list[k];
            for (int ch = 0; ch < 3; ++ch) if (upd[ch]) pv[3 * (size_t)j + ch] = rv[3 * (size_t)k + ch] + beta[ch] * pv[3 * (size_t)j + ch];
        }
        __syncthreads();
    }
    if (t < 3) { iters_out[3 * (size_t)p + t] = it[t]; err_out[3 * (size_t)p + t] = err[t]; }
}
#undef LS_FOR_UNKNOWNS

struct ToU32 { __host__ __device__ uint32_t operator()(uint8_t v) const { return (uint32_t)v; } };

// hp: host copy of pix_ptr (checked by the caller); the exclusive scans run over one entry more than their kernels flag: the total lands there
void run_lsl(mvs_ctx* ctx, LslDev& D, const uint32_t* d_adj_ptr, const uint32_t* d_adj, uint32_t E, const uint32_t* d_labels, const Patches& S,
             const unsigned long long* hp, const mvs_lsl_params& P, mvs_lsl_stats& st) {
    hipStream_t s = ctx->stream;
    const uint32_t F = ctx->n_faces, NV = ctx->n_verts, NP = S.P, L = S.L;
    const size_t NPIX = (size_t)hp[NP];
    StageTimer<6> tm(s);   // marks: begin, topology, colours, writes, masks, solve
    tm.mark();
    D.flags.ensure(F_N); D.c64.ensure(K_N);
    MVS_HIP(hipMemsetAsync(D.flags.p, 0, F_N * sizeof(uint32_t), s));
    MVS_HIP(hipMemsetAsync(D.c64.p, 0, K_N * sizeof(unsigned long long), s));
    auto check_flags = [&]() {
        uint32_t fl[F_N];
        MVS_HIP(hipMemcpyAsync(fl, D.flags.p, sizeof(fl), hipMemcpyDeviceToHost, s));
        MVS_HIP(hipStreamSynchronize(s));
        if (fl[F_FACE]) throw StatusError(MVS_ERR_LABELING, "local_seam_leveling: a listed face id is >= n_faces");
        if (fl[F_LABEL]) throw StatusError(MVS_ERR_LABELING, "local_seam_leveling: a listed face's label differs from its patch's");
        if (fl[F_VERTEX]) throw StatusError(MVS_ERR_INVALID, "local_seam_leveling: a face refers to a vertex >= n_verts");
        if (fl[F_ADJ]) throw StatusError(MVS_ERR_INVALID, "local_seam_leveling: an adjacency entry is >= n_faces");
        if (fl[F_TC]) throw StatusError(MVS_ERR_UNSUPPORTED, "local_seam_leveling: texture coordinates not finite or beyond 2^20");
    };
    // ---- topology ----
    const uint32_t NK = 3u * L;
    D.epid.ensure((size_t)L + 1); D.keys.ensure((size_t)NK + 1); D.keys2.ensure((size_t)NK + 1); D.flag.ensure((size_t)NK + 2); D.idx.ensure((size_t)NK + 2);
    D.vptr.ensure((size_t)NV + 2);
    if (L) { hipLaunchKernelGGL(ls_entry_kernel, dim3(grid(L)), dim3(256), 0, s, S, (const uint32_t*)ctx->d_faces, d_labels, F, NV, D.epid.p, D.keys.p, D.flags.p); MVS_LAUNCH_CHECK(); }
    check_flags();
    if (NK) dev_sort_keys(ctx, D.keys.p, D.keys2.p, (size_t)NK, 0, 64);
    const unsigned long long* keys = D.keys2.p;
    hipLaunchKernelGGL(ls_head_kernel, dim3(grid((size_t)NK + 1)), dim3(256), 0, s, keys, NK, (const uint32_t*)D.epid.p, D.flag.p); MVS_LAUNCH_CHECK();
    dev_exclusive_scan(ctx, (const uint32_t*)D.flag.p, D.idx.p, (size_t)NK + 1);
    const uint32_t NI = read_u32(ctx, D.idx.p + NK);
    D.info_head.ensure((size_t)NI + 1);
    if (NK) { hipLaunchKernelGGL(ls_info_kernel, dim3(grid(NK)), dim3(256), 0, s, (const uint32_t*)D.flag.p, (const uint32_t*)D.idx.p, NK, D.info_head.p); MVS_LAUNCH_CHECK(); }
    hipLaunchKernelGGL(ls_vptr_kernel, dim3(grid((size_t)NV + 1)), dim3(256), 0, s, keys, NK, NV, D.vptr.p); MVS_LAUNCH_CHECK();
    D.sflag.ensure((size_t)E + 2); D.sidx.ensure((size_t)E + 2);
    hipLaunchKernelGGL(ls_seam_kernel, dim3(grid((size_t)E + 1)), dim3(256), 0, s, d_adj_ptr, d_adj, d_labels, (const uint32_t*)ctx->d_faces, F, NV, E, 0, D.sflag.p,
                       (const uint32_t*)nullptr, (uint32_t*)nullptr, D.flags.p, D.c64.p);
    MVS_LAUNCH_CHECK();
    dev_exclusive_scan(ctx, (const uint32_t*)D.sflag.p, D.sidx.p, (size_t)E + 1);
    check_flags();
    const uint32_t NE = read_u32(ctx, D.sidx.p + E);
    D.edge_v.ensure(2 * (size_t)NE + 2); D.ep_cnt.ensure((size_t)NE + 2); D.ep_ptr.ensure((size_t)NE + 2); D.en.ensure((size_t)NE + 2); D.ecol_ptr.ensure((size_t)NE + 2);
    uint32_t NEP = 0, NS = 0;
    if (NE) {
        hipLaunchKernelGGL(ls_seam_kernel, dim3(grid((size_t)E + 1)), dim3(256), 0, s, d_adj_ptr, d_adj, d_labels, (const uint32_t*)ctx->d_faces, F, NV, E, 1, D.sflag.p,
                           (const uint32_t*)D.sidx.p, D.edge_v.p, D.flags.p, D.c64.p);
        MVS_LAUNCH_CHECK();
        auto eproj = [&](int fill) {
            hipLaunchKernelGGL(ls_eproj_kernel, dim3(grid((size_t)NE + 1)), dim3(256), 0, s, NE, (const uint32_t*)D.edge_v.p, keys, (const uint32_t*)D.vptr.p,
                               (const uint32_t*)D.epid.p, S, (const uint32_t*)ctx->d_faces, fill, D.ep_cnt.p, (const uint32_t*)D.ep_ptr.p, D.ep_patch.p, D.ep_c1.p,
                               D.ep_c2.p, D.ep_edge.p, D.en.p, D.flags.p, D.c64.p);
            MVS_LAUNCH_CHECK();
        };
        eproj(0);
        dev_exclusive_scan(ctx, (const uint32_t*)D.ep_cnt.p, D.ep_ptr.p, (size_t)NE + 1);
        NEP = read_u32(ctx, D.ep_ptr.p + NE);
        D.ep_patch.ensure((size_t)NEP + 1); D.ep_c1.ensure((size_t)NEP + 1); D.ep_c2.ensure((size_t)NEP + 1); D.ep_edge.ensure((size_t)NEP + 1);
        eproj(1);
        dev_exclusive_scan(ctx, (const uint32_t*)D.en.p, D.ecol_ptr.p, (size_t)NE + 1);
        check_flags();
        unsigned long long total = 0;
        MVS_HIP(hipMemcpyAsync(&total, D.c64.p + K_NSAMPLES, sizeof(total), hipMemcpyDeviceToHost, s));
        MVS_HIP(hipStreamSynchronize(s));
        if (total >= 0x40000000ull) throw StatusError(MVS_ERR_UNSUPPORTED, "local_seam_leveling: too many edge samples for one call");
        NS = (uint32_t)total;
    }
    if ((unsigned long long)NI + NEP >= 0xFFFFFFF0ull) throw StatusError(MVS_ERR_UNSUPPORTED, "local_seam_leveling: too many writers for one call");
    st.seam_edges = NE; st.vertex_infos = NI; st.edge_projections = NEP;
    tm.mark();
    // ---- colours ----
    D.ecol.ensure(3 * (size_t)NS + 3); D.vcol.ensure(3 * (size_t)NV + 3);
    if (NS) {
        hipLaunchKernelGGL(ls_edge_colour_kernel, dim3(grid(NS)), dim3(256), 0, s, NS, NE, (const uint32_t*)D.ecol_ptr.p, (const uint32_t*)D.en.p,
                           (const uint32_t*)D.ep_ptr.p, (const uint32_t*)D.ep_patch.p, (const uint32_t*)D.ep_c1.p, (const uint32_t*)D.ep_c2.p, S, D.ecol.p, D.c64.p);
        MVS_LAUNCH_CHECK();
    }
    if (NV && NI) {
        hipLaunchKernelGGL(ls_vertex_colour_kernel, dim3(grid(NV)), dim3(256), 0, s, NV, (const uint32_t*)D.vptr.p, (const uint32_t*)D.idx.p, (const uint32_t*)D.info_head.p,
                           keys, (const uint32_t*)D.epid.p, S, D.vcol.p, D.c64.p);
        MVS_LAUNCH_CHECK();
    }
    tm.mark();
    // ---- writes ----
    D.win.ensure(NPIX + 1); D.image.ensure(3 * NPIX + 3); D.blendw.ensure(NPIX + 1); D.mask.ensure(NPIX + 1); D.validity.ensure(NPIX + 1);
    D.hv.ensure(NPIX + 1); D.unk.ensure(NPIX + 2); D.rank.ensure(NPIX + 2);
    if (NPIX) {
        MVS_HIP(hipMemsetAsync(D.win.p, 0, NPIX * sizeof(uint32_t), s));
        MVS_HIP(hipMemcpyAsync(D.image.p, S.image, 3 * NPIX * sizeof(float), hipMemcpyDeviceToDevice, s));
        MVS_HIP(hipMemcpyAsync(D.blendw.p, S.blending, NPIX, hipMemcpyDeviceToDevice, s));
    }
    const uint32_t NW = NI + NEP;
    if (NW) {
        WriteOut O{D.win.p, D.image.p, D.blendw.p, D.c64.p};
#define LS_WRITE(PASS)                                                                                                                                   \
        hipLaunchKernelGGL(ls_write_kernel<PASS>, dim3(grid(NW)), dim3(256), 0, s, NI, NEP, (const uint32_t*)D.info_head.p, keys, (const uint32_t*)D.vptr.p, \
                           (const uint32_t*)D.idx.p, (const uint32_t*)D.epid.p, (const uint32_t*)D.ep_patch.p, (const uint32_t*)D.ep_c1.p,                 \
                           (const uint32_t*)D.ep_c2.p, (const uint32_t*)D.ep_edge.p, (const uint32_t*)D.en.p, (const uint32_t*)D.ecol_ptr.p,               \
                           (const float*)D.ecol.p, (const float*)D.vcol.p, S, O);                                                                          \
        MVS_LAUNCH_CHECK();
        LS_WRITE(0)
        LS_WRITE(1)
#undef LS_WRITE
    }
    tm.mark();
    // ---- masks ----
    std::vector<uint32_t> h_chunk_ptr, h_chunk_patch;   // read by the uploads: alive until the drain at the end of this phase
    const uint32_t NC = upload_chunk_tables(ctx, hp, NP, CHUNK, h_chunk_ptr, h_chunk_patch, D.chunk_ptr, D.chunk_patch);
    D.n_unk.ensure((size_t)NP + 1);
    std::vector<uint32_t> h_unk(NP, 0);
    if (NC) {
        const int strip = (int)P.strip_width;
        hipLaunchKernelGGL(ls_hv_kernel, dim3(NC), dim3(256), 0, s, S, (const uint32_t*)D.chunk_ptr.p, (const uint32_t*)D.chunk_patch.p, strip + 2, D.hv.p); MVS_LAUNCH_CHECK();
        hipLaunchKernelGGL(ls_mask_kernel, dim3(NC), dim3(256), 0, s, S, (const uint32_t*)D.chunk_ptr.p, (const uint32_t*)D.chunk_patch.p, strip, (const uint8_t*)D.hv.p,
                           (const uint8_t*)D.blendw.p, D.mask.p);
        MVS_LAUNCH_CHECK();
        hipLaunchKernelGGL(ls_class_kernel, dim3(NC), dim3(256), 0, s, S, (const uint32_t*)D.chunk_ptr.p, (const uint32_t*)D.chunk_patch.p, (const uint8_t*)D.mask.p,
                           D.unk.p, D.validity.p, D.c64.p);
        MVS_LAUNCH_CHECK();
        MVS_HIP(hipMemsetAsync(D.unk.p + NPIX, 0, 1, s));
        dev_exclusive_scan(ctx, rocprim::make_transform_iterator((const uint8_t*)D.unk.p, ToU32()), D.rank.p, NPIX + 1);
        hipLaunchKernelGGL(ls_count_kernel, dim3(grid(NP)), dim3(256), 0, s, S, (const uint32_t*)D.rank.p, D.n_unk.p); MVS_LAUNCH_CHECK();
        MVS_HIP(hipMemcpyAsync(h_unk.data(), D.n_unk.p, (size_t)NP * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    }
    tm.mark();
    MVS_HIP(hipStreamSynchronize(s));
    // ---- solve: patches with unknowns, largest working set first; tiers of LDS, the rest in global memory ----
    D.iters.ensure(3 * (size_t)NP + 3); D.err.ensure(3 * (size_t)NP + 3);
    MVS_HIP(hipMemsetAsync(D.iters.p, 0, 3 * (size_t)NP * sizeof(uint32_t), s));
    MVS_HIP(hipMemsetAsync(D.err.p, 0, 3 * (size_t)NP * sizeof(float), s));
    std::vector<uint32_t> ord;
    auto need = [&](uint32_t p) { return 12ull * (hp[p + 1] - hp[p]) + 16ull * h_unk[p]; };
    for (uint32_t p = 0; p < NP; ++p) if (h_unk[p]) ord.push_back(p);
    std::stable_sort(ord.begin(), ord.end(), [&](uint32_t a, uint32_t b) { return need(a) > need(b); });
    const unsigned long long lds_cap = std::min<unsigned long long>(P.lds_bytes, LDS_MAX);
    size_t n_global = 0;
    while (n_global < ord.size() && need(ord[n_global]) > lds_cap) ++n_global;
    std::vector<unsigned long long> h_goff(n_global + 1, 0);
    for (size_t k = 0; k < n_global; ++k) { h_goff[k + 1] = h_goff[k] + need(ord[k]) / 4; st.pixels_global += hp[ord[k] + 1] - hp[ord[k]]; }
    st.patches_global = n_global; st.patches_lds = ord.size() - n_global;
    if (!ord.empty() && P.max_iterations > 0) {
        D.order.ensure(ord.size() + 1); D.goff.ensure(n_global + 1); D.scratch.ensure((size_t)h_goff[n_global] + 4);
        MVS_HIP(hipMemcpyAsync(D.order.p, ord.data(), ord.size() * sizeof(uint32_t), hipMemcpyHostToDevice, s));
        MVS_HIP(hipMemcpyAsync(D.goff.p, h_goff.data(), (n_global + 1) * sizeof(unsigned long long), hipMemcpyHostToDevice, s));
        if (n_global) {
            hipLaunchKernelGGL((ls_solve_kernel<false, 1024>), dim3((unsigned)n_global), dim3(1024), 0, s, S, (const uint32_t*)D.order.p, (const unsigned long long*)D.goff.p,
                               D.scratch.p, (const uint8_t*)D.unk.p, (const uint32_t*)D.rank.p, D.image.p, P.tolerance, P.max_iterations, D.iters.p, D.err.p);
            MVS_LAUNCH_CHECK();
        }
        MVS_HIP(hipFuncSetAttribute((const void*)ls_solve_kernel<true, 256>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_MAX));
        size_t a = n_global;   // tiers: a launch's workgroups ask for the LDS of its largest patch, at most twice what its smallest needs
        while (a < ord.size()) {
            const unsigned long long top = need(ord[a]);
            size_t b = a + 1;
            while (b < ord.size() && 2 * need(ord[b]) > top) ++b;
            hipLaunchKernelGGL((ls_solve_kernel<true, 256>), dim3((unsigned)(b - a)), dim3(256), (size_t)top, s, S, (const uint32_t*)D.order.p + a, (const unsigned long long*)nullptr,
                               (float*)nullptr, (const uint8_t*)D.unk.p, (const uint32_t*)D.rank.p, D.image.p, P.tolerance, P.max_iterations, D.iters.p, D.err.p);
            MVS_LAUNCH_CHECK();
            a = b;
        }
    }
    tm.mark();
    std::vector<uint32_t> h_it(3 * (size_t)NP); std::vector<float> h_err(3 * (size_t)NP);
    unsigned long long c64[K_N];
    if (NP) {
        MVS_HIP(hipMemcpyAsync(h_it.data(), D.iters.p, h_it.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        MVS_HIP(hipMemcpyAsync(h_err.data(), D.err.p, h_err.size() * sizeof(float), hipMemcpyDeviceToHost, s));
    }
    MVS_HIP(hipMemcpyAsync(c64, D.c64.p, sizeof(c64), hipMemcpyDeviceToHost, s));
    MVS_HIP(hipStreamSynchronize(s));
    for (uint32_t p = 0; p < NP; ++p) {
        bool hit = false;
        for (int ch = 0; ch < 3; ++ch) {
            const uint32_t k = h_it[3 * (size_t)p + ch];
            st.iterations_total += k; st.iterations_max = std::max(st.iterations_max, k); st.error_max = std::max(st.error_max, h_err[3 * (size_t)p + ch]);
            hit = hit || (P.max_iterations > 0 && k >= P.max_iterations);
        }
        if (hit) ++st.hit_max_iterations;
    }
    st.skipped_pairs = c64[K_SKIPPED]; st.colour_samples = c64[K_SAMPLES]; st.invalid_samples = c64[K_BAD_SAMPLES];
    st.vertex_writes = c64[K_VWRITES]; st.line_writes = c64[K_LWRITES]; st.written_pixels = c64[K_WRITTEN]; st.outside_frame = c64[K_OUTSIDE];
    st.invalid_writes = c64[K_BAD_WRITES]; st.strip_pixels = c64[K_STRIP]; st.fixed_pixels = c64[K_FIXED]; st.demoted = c64[K_DEMOTED];
    st.ms_topology = tm.ms(0, 1); st.ms_colours = tm.ms(1, 2); st.ms_writes = tm.ms(2, 3); st.ms_mask = tm.ms(3, 4); st.ms_solve = tm.ms(4, 5);
    st.ms_total = tm.ms(0, 5);
}

}  // namespace
}  // namespace mvs

using namespace mvs;

extern "C" {

void mvs_lsl_default_params(mvs_lsl_params* p) {
    if (!p) return;
    p->tolerance = 1e-6f; p->max_iterations = 700; p->strip_width = 20; p->lds_bytes = LDS_MAX;
}

mvs_status mvs_ctx_local_seam_leveling(mvs_ctx* ctx, const uint32_t* adj_ptr, const uint32_t* adj, int adj_on_device, const uint32_t* labels,
                                       int labels_on_device, const mvs_patch_set* patches, int patches_on_device, const mvs_lsl_params* params,
                                       mvs_lsl_result* out, int out_on_device, mvs_lsl_stats* stats) {
    if (!ctx || !out || !patches) return api_fail(MVS_ERR_INVALID, "null argument");
    if (!ctx->d_verts || !ctx->d_faces) return api_fail(MVS_ERR_STATE, "local seam leveling needs the mesh (mvs_scene_set_mesh)");
    const uint32_t F = ctx->n_faces;
    if (F && (!adj_ptr || !adj || !labels)) return api_fail(MVS_ERR_INVALID, "null argument");
    *out = mvs_lsl_result{};
    mvs_lsl_stats st{};
    if (stats) *stats = st;
    return api_guard([&] {
        MVS_HIP(hipSetDevice(ctx->device));
        hipStream_t s = ctx->stream;
        LslDev& D = row_dev(ctx->lsl);
        mvs_lsl_params P;
        if (params) P = *params; else mvs_lsl_default_params(&P);
        if (P.strip_width > 250) throw StatusError(MVS_ERR_INVALID, "local_seam_leveling: strip_width above 250");
        if (!(P.tolerance >= 0.0f)) throw StatusError(MVS_ERR_INVALID, "local_seam_leveling: negative tolerance");
        const mvs_patch_set& in = *patches;
        const uint32_t NP = in.n_patches, L = in.n_listed;
        const uint64_t NPIX = in.n_pixels;
        if (NPIX && !in.blending) throw StatusError(MVS_ERR_INVALID, "local_seam_leveling: null array in the patch set");
        const PatchFrames h = read_patch_set(ctx, in, patches_on_device, true, "local_seam_leveling");   // the small per-patch arrays are read on the host as well
        const unsigned long long* hp = h.pix_ptr;
        if (NPIX >= 0xFFFFFF00ull || (uint64_t)L * 3u >= 0xFFFFFF00ull) throw StatusError(MVS_ERR_UNSUPPORTED, "local_seam_leveling: too many pixels or list entries for one call");
        for (uint32_t p = 0; p < NP; ++p) {
            if (hp[p + 1] - hp[p] >= 0x10000000ull) throw StatusError(MVS_ERR_UNSUPPORTED, "local_seam_leveling: a patch of 2^28 pixels or more");
            if (h.label[p] == 0) throw StatusError(MVS_ERR_UNSUPPORTED, "local_seam_leveling: a patch of label 0");
        }
        const RowGraph g = stage_graph(ctx, adj_ptr, adj, adj_on_device, labels, labels_on_device, true);   // E sizes the seam search
        Patches S{};
        S.P = NP; S.L = L;
        S.label = stage(D.in_label, (const uint32_t*)in.label, NP, patches_on_device, s);
        S.box = stage(D.in_box, (const int4*)in.box, NP, patches_on_device, s);
        S.face_ptr = stage(D.in_face_ptr, (const uint32_t*)in.face_ptr, (size_t)NP + (NP ? 1 : 0), patches_on_device, s);
        S.faces = stage(D.in_faces, (const uint32_t*)in.faces, L, patches_on_device, s);
        S.texcoords = stage(D.in_texcoords, (const float*)in.texcoords, 6 * (size_t)L, patches_on_device, s);
        S.pix_ptr = stage(D.in_pix_ptr, (const unsigned long long*)in.pix_ptr, (size_t)NP + (NP ? 1 : 0), patches_on_device, s);
        S.image = stage(D.in_image, (const float*)in.image, 3 * (size_t)NPIX, patches_on_device, s);
        S.validity = stage(D.in_validity, (const uint8_t*)in.validity, (size_t)NPIX, patches_on_device, s);
        S.blending = stage(D.in_blending, (const uint8_t*)in.blending, (size_t)NPIX, patches_on_device, s);
        MVS_HIP(hipStreamSynchronize(s));   // host buffers are borrowed for the call only
        run_with_stats(s, stats, st, [&] { run_lsl(ctx, D, g.adj_ptr, g.adj, g.E, g.labels, S, hp, P, st); });
        out->n_patches = NP; out->n_pixels = NPIX;
        if (out_on_device) {
            out->image = D.image.p; out->validity = D.validity.p; out->blending = D.mask.p;
        } else {
            download(s, out, mvs_lsl_result_free, [&] {
                out->image = host_copy(D.image.p, 3 * (size_t)NPIX, s); out->validity = host_copy(D.validity.p, (size_t)NPIX, s);
                out->blending = host_copy(D.mask.p, (size_t)NPIX, s);
            });
        }
    });
}

void mvs_lsl_result_free(mvs_lsl_result* r) {
    if (!r) return;
    free(r->image); free(r->validity); free(r->blending);
    *r = mvs_lsl_result{};
}

}  // extern "C"
