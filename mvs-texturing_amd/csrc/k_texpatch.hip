// k_texpatch.hip -- row f6: generate_texture_patches for the labelled faces (generate_texture_patches.cpp:78-138, :484-508) and
//   TexturePatch::adjust_colors (texture_patch.cpp:41-122), tone mapping `none` or `gamma` (resolve is instantiated on the mode: under
//   gamma the crop is the context's table at its bytes, tone.h, so adjust_colors works on linearised values).  The definition (DESIGN.md section 4 "Texture
//   patches") is shared with the CPU model of the tests (tests/tools/patch_model.cpp): every output is bit-identical to it.
//   The first half of the file builds the tables rows f5 and f6 share (candidates, boxes, the merge, patch ids: build_patch_tables).
//   Row f6 then runs: one thread per candidate (label, frame, sizes), three scans (face_ptr, the 64-bit pix_ptr, chunk_ptr), one
//   thread per labelled face (its list entry and texture coordinates), mark (a lane group of 8 per list entry, a block for the large
//   ones: integer atomicMax / atomicMin of the list position into two winner words per pixel -- order-free, so every run gives the
//   same bits) and resolve (one thread per pixel in chunks of one patch: the winner's barycentrics again with the identical
//   expression, crop + adjustment, the two masks).  No float atomics anywhere.
#include "rows.h"
#include "tone.h"
#include <cfloat>
#include <climits>

namespace mvs {

namespace {
constexpr uint32_t NONE = 0xFFFFFFFFu;
enum { F_LABEL = 0, F_VERTEX, F_BOX, F_N };   // flag words of PatchTables

// ---- the shared tables (items 3-4 of "Global seam leveling") ----
__global__ void pt_check_kernel(const uint32_t* __restrict__ faces, const uint32_t* __restrict__ labels, uint32_t F, uint32_t NV, uint32_t n_views,
                                uint32_t* __restrict__ flags) {
    const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F) return;
    if (labels[f] > n_views) flags[F_LABEL] = 1u;   // rare: plain racy store of the same value
    if (faces[3 * f] >= NV || faces[3 * f + 1] >= NV || faces[3 * f + 2] >= NV) flags[F_VERTEX] = 1u;
}
__global__ void pt_box_init_kernel(int4* __restrict__ box, uint32_t C) {
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < C) box[c] = make_int4(INT_MAX, INT_MAX, INT_MIN, INT_MIN);
}
// one thread per position of the component lists: the face's candidate, its place in it, its corners' pixel coordinates, the box
__global__ void pt_face_box_kernel(const uint32_t* __restrict__ comp_ptr, const uint32_t* __restrict__ comp_faces, uint32_t C, uint32_t F,
                                   const uint32_t* __restrict__ labels, const uint32_t* __restrict__ faces, const float* __restrict__ verts,
                                   const ViewParams* __restrict__ views, int4* __restrict__ box, float2* __restrict__ pc, uint32_t* __restrict__ fcand,
                                   uint32_t* __restrict__ fidx, uint32_t* __restrict__ flags) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= F) return;
    uint32_t lo = 0, hi = C;   // the last component starting at or before p
    while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (comp_ptr[mid] <= p) lo = mid; else hi = mid; }
    const uint32_t c = lo, f = comp_faces[p];
    fcand[f] = c; fidx[f] = p - comp_ptr[c];
    const uint32_t L = labels[f];
    if (!L) return;
    const ViewParams& vw = views[L - 1];
    int mnx = INT_MAX, mny = INT_MAX, mxx = INT_MIN, mxy = INT_MIN;
    bool ok = true;
    for (int k = 0; k < 3; ++k) {
        const uint32_t v = faces[3 * f + k];
        const V2 q = pixel_coords(vw, V3{verts[3 * (size_t)v], verts[3 * (size_t)v + 1], verts[3 * (size_t)v + 2]});
        pc[3 * (size_t)f + k] = make_float2(q.x, q.y);
        const float fx = floorf(q.x), fy = floorf(q.y), cx = ceilf(q.x), cy = ceilf(q.y);
        if (!(fx >= 0.0f && fy >= 0.0f && cx <= (float)(vw.width - 1) && cy <= (float)(vw.height - 1))) { ok = false; continue; }
        mnx = min(mnx, (int)fx); mny = min(mny, (int)fy); mxx = max(mxx, (int)cx); mxy = max(mxy, (int)cy);
    }
    if (!ok) { flags[F_BOX] = 1u; return; }
    atomicMin(&box[c].x, mnx); atomicMin(&box[c].y, mny); atomicMax(&box[c].z, mxx); atomicMax(&box[c].w, mxy);
}
// one thread per label: upstream's merge loop (generate_texture_patches.cpp:484-508) over the label's candidates in order; the frame
// gets its border (min - 1) first.  parent / off: the candidate that absorbed this one and where its list starts in that one's list.
__global__ void pt_merge_kernel(const uint32_t* __restrict__ label_ptr, uint32_t n_labels, const uint32_t* __restrict__ comp_ptr, int4* __restrict__ box,
                                uint32_t* __restrict__ parent, uint32_t* __restrict__ off, uint32_t* __restrict__ len, uint32_t* __restrict__ alive,
                                unsigned long long* __restrict__ n_merged) {
    const uint32_t L = blockIdx.x * blockDim.x + threadIdx.x;
    if (L >= n_labels) return;
    const uint32_t c0 = label_ptr[L], c1 = label_ptr[L + 1];
    for (uint32_t c = c0; c < c1; ++c) {
        parent[c] = NONE; off[c] = 0; len[c] = comp_ptr[c + 1] - comp_ptr[c]; alive[c] = L ? 1u : 0u;
        if (L) { int4 b = box[c]; b.x -= 1; b.y -= 1; box[c] = b; }
    }
    if (!L) return;
    unsigned long long merged = 0;
    for (uint32_t i = c0; i < c1; ++i) {
        if (!alive[i]) continue;
        const int4 a = box[i];
        for (uint32_t j = c0; j < c1; ++j) {
            if (j == i || !alive[j]) continue;
            const int4 s = box[j];
            if (s.x >= a.x && s.z <= a.z && s.y >= a.y && s.w <= a.w) { parent[j] = i; off[j] = len[i]; len[i] += len[j]; alive[j] = 0u; ++merged; }
        }
    }
    if (merged) atomicAdd(n_merged, merged);
}
__global__ void pt_cand_final_kernel(const uint32_t* __restrict__ parent, const uint32_t* __restrict__ off, const uint32_t* __restrict__ pscan,
                                     uint32_t C, uint32_t* __restrict__ cand_pid, uint32_t* __restrict__ cand_pos) {
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    uint32_t r = c, p0 = 0;
    while (parent[r] != NONE) { p0 += off[r]; r = parent[r]; }
    cand_pid[c] = pscan[r]; cand_pos[c] = p0;
}
__global__ void pt_face_patch_kernel(const uint32_t* __restrict__ labels, const uint32_t* __restrict__ fcand, const uint32_t* __restrict__ fidx,
                                     const uint32_t* __restrict__ cand_pid, const uint32_t* __restrict__ cand_pos, uint32_t F,
                                     uint32_t* __restrict__ fpid, uint32_t* __restrict__ fpos) {
    const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F) return;
    const uint32_t c = fcand[f];
    fpid[f] = labels[f] ? cand_pid[c] : NONE; fpos[f] = cand_pos[c] + fidx[f];
}
}  // namespace

void patch_check_inputs(mvs_ctx* ctx, PatchTables& T, const uint32_t* d_labels, const char* who) {
    hipStream_t s = ctx->stream;
    const uint32_t F = ctx->n_faces, NV = ctx->n_verts, V = ctx->n_views;
    T.flags.ensure(F_N); T.merged.ensure(1); T.views.ensure(V);
    MVS_HIP(hipMemsetAsync(T.flags.p, 0, F_N * sizeof(uint32_t), s));
    MVS_HIP(hipMemsetAsync(T.merged.p, 0, sizeof(unsigned long long), s));
    MVS_HIP(hipMemcpyAsync(T.views.p, ctx->h_views.data(), V * sizeof(ViewParams), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(pt_check_kernel, dim3(grid(F)), dim3(256), 0, s, ctx->d_faces, d_labels, F, NV, V, T.flags.p); MVS_LAUNCH_CHECK();
    uint32_t fl[F_N];
    MVS_HIP(hipMemcpyAsync(fl, T.flags.p, sizeof(fl), hipMemcpyDeviceToHost, s));
    MVS_HIP(hipStreamSynchronize(s));
    if (fl[F_LABEL]) throw StatusError(MVS_ERR_LABELING, std::string(who) + ": a label is greater than the number of views");
    if (fl[F_VERTEX]) throw StatusError(MVS_ERR_INVALID, std::string(who) + ": a face refers to a vertex >= n_verts");
}

void build_patch_tables(mvs_ctx* ctx, PatchTables& T, const uint32_t* d_adj_ptr, const uint32_t* d_adj, const uint32_t* d_labels, const char* who) {
    hipStream_t s = ctx->stream;
    const uint32_t F = ctx->n_faces, V = ctx->n_views;
    const uint32_t C = get_subgraphs(ctx, d_adj_ptr, d_adj, d_labels, F, V + 1);
    const uint32_t* comp_ptr = ctx->p_comp_ptr.p; const uint32_t* comp_faces = ctx->p_comp_faces.p; const uint32_t* label_ptr = ctx->p_label_ptr.p;
    T.box.ensure((size_t)C + 1); T.pc.ensure(3 * (size_t)F + 1); T.fcand.ensure((size_t)F + 1); T.fidx.ensure((size_t)F + 1);
    T.parent.ensure((size_t)C + 1); T.off.ensure((size_t)C + 1); T.len.ensure((size_t)C + 1); T.alive.ensure((size_t)C + 1);
    T.pscan.ensure((size_t)C + 2); T.cand_pid.ensure((size_t)C + 1); T.cand_pos.ensure((size_t)C + 1); T.fpid.ensure((size_t)F + 1); T.fpos.ensure((size_t)F + 1);
    hipLaunchKernelGGL(pt_box_init_kernel, dim3(grid(C)), dim3(256), 0, s, T.box.p, C); MVS_LAUNCH_CHECK();
    hipLaunchKernelGGL(pt_face_box_kernel, dim3(grid(F)), dim3(256), 0, s, comp_ptr, comp_faces, C, F, d_labels, ctx->d_faces, ctx->d_verts,
                       (const ViewParams*)T.views.p, T.box.p, T.pc.p, T.fcand.p, T.fidx.p, T.flags.p);
    MVS_LAUNCH_CHECK();
    if (read_u32(ctx, T.flags.p + F_BOX)) throw StatusError(MVS_ERR_LABELING, std::string(who) + ": a labelled face leaves its view's image");
    hipLaunchKernelGGL(pt_merge_kernel, dim3(grid(V + 1)), dim3(256), 0, s, label_ptr, V + 1, comp_ptr, T.box.p, T.parent.p, T.off.p, T.len.p,
                       T.alive.p, T.merged.p);
    MVS_LAUNCH_CHECK();
    exclusive_scan_u32(ctx, T.alive.p, T.pscan.p, C, T.pscan.p + C);
    unsigned long long merged = 0;
    MVS_HIP(hipMemcpyAsync(&merged, T.merged.p, sizeof(merged), hipMemcpyDeviceToHost, s));
    T.n_patches = read_u32(ctx, T.pscan.p + C);
    T.C = C; T.n_merged = merged;
    hipLaunchKernelGGL(pt_cand_final_kernel, dim3(grid(C)), dim3(256), 0, s, T.parent.p, T.off.p, T.pscan.p, C, T.cand_pid.p, T.cand_pos.p); MVS_LAUNCH_CHECK();
    hipLaunchKernelGGL(pt_face_patch_kernel, dim3(grid(F)), dim3(256), 0, s, d_labels, T.fcand.p, T.fidx.p, T.cand_pid.p, T.cand_pos.p, F, T.fpid.p, T.fpos.p);
    MVS_LAUNCH_CHECK();
}

// ---- row f6 (TexPatchDev: rows.h) ----
void texpatch_release(mvs_ctx* ctx) { delete ctx->texpatch; ctx->texpatch = nullptr; }

namespace {
constexpr uint32_t CHUNK = TEXPATCH_CHUNK;   // pixels of one patch a resolve block handles (4 per thread, 256 apart: coalesced rows)
constexpr uint32_t GROUP = 8;             // lanes of mark_kernel per list entry
constexpr uint32_t SMALL_MAX = 512;       // pixel ranges above this many pixels go to a block each (mark_big_kernel)
constexpr uint32_t BIG_BLOCKS = 2048;     // grid of mark_big_kernel: blocks stride over the list of large entries
enum { K_DEGENERATE = 0, K_VALID, K_NEAR, K_BIG, K_N };   // 64-bit counters

// one thread per candidate: a survivor's label, frame, list length and pixel count under its patch id
__global__ void tp_patch_kernel(const uint32_t* __restrict__ comp_ptr, const uint32_t* __restrict__ comp_faces, const uint32_t* __restrict__ labels,
                                const int4* __restrict__ cbox, const uint32_t* __restrict__ alive, const uint32_t* __restrict__ pscan,
                                const uint32_t* __restrict__ len, uint32_t C, uint32_t* __restrict__ label, int4* __restrict__ box,
                                uint32_t* __restrict__ cnt, unsigned long long* __restrict__ npix, uint32_t* __restrict__ nchunk) {
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C || !alive[c]) return;
    const uint32_t p = pscan[c];
    const int4 b = cbox[c];
    const int w = b.z - b.x + 2, h = b.w - b.y + 2;
    const unsigned long long n = (unsigned long long)w * (unsigned long long)h;
    label[p] = labels[comp_faces[comp_ptr[c]]]; box[p] = make_int4(b.x, b.y, w, h);
    cnt[p] = len[c]; npix[p] = n; nchunk[p] = (uint32_t)((n + CHUNK - 1) / CHUNK);
}
// one thread per face: a labelled face's list entry -- its id, its patch, its corners in the patch's pixels through the chain of frames
__global__ void tp_entry_kernel(const uint32_t* __restrict__ labels, uint32_t F, const uint32_t* __restrict__ fcand, const uint32_t* __restrict__ fpid,
                                const uint32_t* __restrict__ fpos, const uint32_t* __restrict__ parent, const int4* __restrict__ cbox,
                                const float2* __restrict__ pc, const uint32_t* __restrict__ face_ptr, uint32_t* __restrict__ faces,
                                uint32_t* __restrict__ epid, float* __restrict__ texcoords) {
    const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F || !labels[f]) return;
    const uint32_t p = fpid[f];
    const size_t e = (size_t)face_ptr[p] + fpos[f];
    faces[e] = f; epid[e] = p;
    for (int k = 0; k < 3; ++k) {
        uint32_t c = fcand[f];
        int4 b = cbox[c];
        const float2 q = pc[3 * (size_t)f + k];
        float x = q.x - (float)b.x, y = q.y - (float)b.y;
        for (uint32_t up = parent[c]; up != NONE; up = parent[c]) {
            const int4 bp = cbox[up];
            x = x + (float)(b.x - bp.x); y = y + (float)(b.y - bp.y);
            c = up; b = bp;
        }
        texcoords[6 * e + 2 * k] = x; texcoords[6 * e + 2 * k + 1] = y;
    }
}

// Tri of a list entry (dmath.h foot_setup_px: detT, bounding box, area) and what adjust_colors derives from it
struct EntryTri { FootSetup s; float n23, n13, n12; int x0, y0, x1, y1; };
__device__ inline void entry_tri(const float* __restrict__ tc, EntryTri& t) {
    t.s.p1 = V2{tc[0], tc[1]}; t.s.p2 = V2{tc[2], tc[3]}; t.s.p3 = V2{tc[4], tc[5]};
    foot_setup_px(t.s);
}
__device__ inline float norm2(float dx, float dy) { return sqrtf(dx * dx + dy * dy); }
// Tri::get_barycentric_coords (tri.h:50-56)
__device__ inline void bary(const FootSetup& s, int xi, int yi, float& alpha, float& beta, float& gamma) {
    const float x = (float)xi, y = (float)yi;
    alpha = ((s.t2.y - s.t3.y) * (x - s.t3.x) + (s.t3.x - s.t2.x) * (y - s.t3.y)) / s.detT;
    beta = ((s.t3.y - s.t1.y) * (x - s.t3.x) + (s.t1.x - s.t3.x) * (y - s.t3.y)) / s.detT;
    gamma = 1.0f - alpha - beta;
}
__device__ inline float min3(float a, float b, float c) { float m = a; if (b < m) m = b; if (c < m) m = c; return m; }   // Vector::minimum (std::min_element)
// the pixel range of texture_patch.cpp:56-62, clamped to the patch (upstream asserts it lies inside; the clamp never bites on frames
// built by item 1 and keeps every index in bounds regardless)
__device__ inline void entry_range(EntryTri& t, int w, int h) {
    t.x0 = max((int)floorf(t.s.aabb_min_x) - 1, 0); t.y0 = max((int)floorf(t.s.aabb_min_y) - 1, 0);
    t.x1 = min((int)ceilf(t.s.aabb_max_x) + 1, w); t.y1 = min((int)ceilf(t.s.aabb_max_y) + 1, h);
    t.n23 = norm2(t.s.t2.x - t.s.t3.x, t.s.t2.y - t.s.t3.y); t.n13 = norm2(t.s.t1.x - t.s.t3.x, t.s.t1.y - t.s.t3.y);
    t.n12 = norm2(t.s.t1.x - t.s.t2.x, t.s.t1.y - t.s.t2.y);
}
__device__ inline void mark_pixel(const EntryTri& t, int x, int y, uint32_t pos, unsigned long long base, int w, uint32_t* __restrict__ win_in,
                                  uint32_t* __restrict__ win_near) {
    float a, b, g;
    bary(t.s, x, y, a, b, g);
    const unsigned long long i = base + (unsigned long long)y * (unsigned long long)w + (unsigned long long)x;
    if (min3(a, b, g) >= 0.0f) { atomicMax(win_in + i, pos + 1u); return; }
    const float sqrt_2 = 1.41421354f;   // float(sqrt(2.0))
    const float ha = 2.0f * -a * t.s.area / t.n23, hb = 2.0f * -b * t.s.area / t.n13, hc = 2.0f * -g * t.s.area / t.n12;
    if (ha > sqrt_2 || hb > sqrt_2 || hc > sqrt_2) return;
    atomicMin(win_near + i, pos);
}
// GROUP lanes per list entry walk its pixel range; an entry of more than SMALL_MAX pixels is left to mark_big_kernel
__global__ void __launch_bounds__(256) tp_mark_kernel(uint32_t n_listed, const uint32_t* __restrict__ epid, const uint32_t* __restrict__ face_ptr,
                                                      const float* __restrict__ texcoords, const int4* __restrict__ box,
                                                      const unsigned long long* __restrict__ pix_ptr, uint32_t* __restrict__ win_in,
                                                      uint32_t* __restrict__ win_near, uint32_t* __restrict__ big, unsigned long long* __restrict__ c64) {
    const size_t gt = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t e = gt / GROUP;
    const uint32_t lane = (uint32_t)(gt % GROUP);
    if (e >= n_listed) return;
    EntryTri t;
    entry_tri(texcoords + 6 * e, t);
    if (t.s.area < FLT_EPSILON) { if (lane == 0) atomicAdd(c64 + K_DEGENERATE, 1ull); return; }
    const uint32_t p = epid[e];
    const int4 b = box[p];
    entry_range(t, b.z, b.w);
    if (t.x1 <= t.x0 || t.y1 <= t.y0) return;
    const uint32_t rw = (uint32_t)(t.x1 - t.x0), n = rw * (uint32_t)(t.y1 - t.y0);
    if (n > SMALL_MAX) { if (lane == 0) big[atomicAdd((unsigned int*)(c64 + K_BIG), 1u)] = (uint32_t)e; return; }   // low word of the 64-bit counter: at most n_listed
    const uint32_t pos = (uint32_t)e - face_ptr[p];
    const unsigned long long base = pix_ptr[p];
    for (uint32_t i = lane; i < n; i += GROUP) mark_pixel(t, t.x0 + (int)(i % rw), t.y0 + (int)(i / rw), pos, base, b.z, win_in, win_near);
}
__global__ void __launch_bounds__(256) tp_mark_big_kernel(const uint32_t* __restrict__ big, const unsigned long long* __restrict__ c64,
                                                          const uint32_t* __restrict__ epid, const uint32_t* __restrict__ face_ptr,
                                                          const float* __restrict__ texcoords, const int4* __restrict__ box,
                                                          const unsigned long long* __restrict__ pix_ptr, uint32_t* __restrict__ win_in,
                                                          uint32_t* __restrict__ win_near) {
    const uint32_t nb = (uint32_t)c64[K_BIG];
    for (uint32_t k = blockIdx.x; k < nb; k += gridDim.x) {
        const size_t e = big[k];
        EntryTri t;
        entry_tri(texcoords + 6 * e, t);
        const uint32_t p = epid[e];
        const int4 b = box[p];
        entry_range(t, b.z, b.w);
        const uint32_t rw = (uint32_t)(t.x1 - t.x0), n = rw * (uint32_t)(t.y1 - t.y0);
        const uint32_t pos = (uint32_t)e - face_ptr[p];
        const unsigned long long base = pix_ptr[p];
        for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) mark_pixel(t, t.x0 + (int)(i % rw), t.y0 + (int)(i / rw), pos, base, b.z, win_in, win_near);
    }
}
// one block per chunk of CHUNK pixels of one patch: the winner of every pixel, its adjustment, crop + adjustment, the masks
template <int TONE>
__global__ void __launch_bounds__(256) tp_resolve_kernel(const float* __restrict__ tone, uint32_t P, const uint32_t* __restrict__ chunk_ptr, const uint32_t* __restrict__ label,
                                                         const int4* __restrict__ box, const uint32_t* __restrict__ face_ptr,
                                                         const uint32_t* __restrict__ faces, const float* __restrict__ texcoords,
                                                         const unsigned long long* __restrict__ pix_ptr, const ViewParams* __restrict__ views,
                                                         const float* __restrict__ adjust, const uint32_t* __restrict__ win_in,
                                                         const uint32_t* __restrict__ win_near, float* __restrict__ image, uint8_t* __restrict__ validity,
                                                         uint8_t* __restrict__ blending, unsigned long long* __restrict__ c64) {
    __shared__ uint32_t s_valid, s_near;
    if (threadIdx.x == 0) { s_valid = 0; s_near = 0; }
    __syncthreads();
    uint32_t lo = 0, hi = P;   // the last patch whose chunks start at or before this one (patches without pixels do not exist: w, h >= 2)
    while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (chunk_ptr[mid] <= blockIdx.x) lo = mid; else hi = mid; }
    const uint32_t p = lo;
    const int4 b = box[p];
    const unsigned long long base = pix_ptr[p], n = (unsigned long long)b.z * (unsigned long long)b.w;
    const unsigned long long j0 = (unsigned long long)(blockIdx.x - chunk_ptr[p]) * CHUNK;
    const ViewParams& vw = views[label[p] - 1];
    const uint32_t e0 = face_ptr[p];
    uint32_t nv = 0, nn = 0;
    for (uint32_t r = 0; r < CHUNK / 256; ++r) {
        const unsigned long long j = j0 + r * 256u + threadIdx.x;
        if (j >= n) break;
        const int y = (int)(j / (unsigned long long)b.z), x = (int)(j - (unsigned long long)y * (unsigned long long)b.z);
        const unsigned long long i = base + j;
        const uint32_t wi = win_in[i], wn = win_near[i];
        if (wi == 0u && wn == NONE) {
            image[3 * i] = 0.0f; image[3 * i + 1] = 0.0f; image[3 * i + 2] = 0.0f; validity[i] = 0; blending[i] = 0;
            continue;
        }
        const size_t e = (size_t)e0 + (wi ? wi - 1u : wn);
        EntryTri t;
        entry_tri(texcoords + 6 * e, t);
        float w1, w2, w3;
        bary(t.s, x, y, w1, w2, w3);
        const float* av = adjust ? adjust + 9 * (size_t)faces[e] : nullptr;
        const int vx = b.x + x, vy = b.y + y;
        const bool in_view = vx >= 0 && vy >= 0 && vx < vw.width && vy < vw.height;
        const uint8_t* px = in_view ? vw.rgb + ((size_t)vy * vw.width + vx) * 3 : nullptr;
        for (int c = 0; c < 3; ++c) {
            const float v1 = av ? av[c] : 0.0f, v2 = av ? av[3 + c] : 0.0f, v3 = av ? av[6 + c] : 0.0f;
            const float adj = (v1 * w1 + v2 * w2) + v3 * w3;                                  // math::interpolate
            float crop;
            if (TONE == TONE_GAMMA) crop = tone[in_view ? px[c] : (c == 1 ? 0 : 255)];         // bytes, fill included, through the table
            else crop = in_view ? (float)px[c] / 255.0f : (c == 1 ? 0.0f : 1.0f);              // the crop's fill (255, 0, 255)
            image[3 * i + c] = crop + adj;
        }
        validity[i] = 255; blending[i] = wi ? 255 : 64;
        ++nv; if (!wi) ++nn;
    }
    if (nv) atomicAdd(&s_valid, nv);
    if (nn) atomicAdd(&s_near, nn);
    __syncthreads();
    if (threadIdx.x == 0) {
        if (s_valid) atomicAdd(c64 + K_VALID, (unsigned long long)s_valid);
        if (s_near) atomicAdd(c64 + K_NEAR, (unsigned long long)s_near);
    }
}

}  // namespace

// the geometry half of row f6, which the debug model (k_debug.hip) runs as well: checks, patch tables, per-patch label / frame / sizes,
// the three scans, the lists and texture coordinates, and room for the pixel arrays.  Marks tm three times (begin, tables, lists).
// *n_chunks arrives with the next drain of the stream.
void texpatch_geometry(mvs_ctx* ctx, TexPatchDev& D, const uint32_t* d_adj_ptr, const uint32_t* d_adj, const uint32_t* d_labels, const mvs_patch_params& P,
                       mvs_patch_stats& S, uint32_t& n_listed, uint64_t& n_pixels, uint32_t* n_chunks, StageTimer<5>& tm, const char* who) {
    hipStream_t s = ctx->stream;
    const uint32_t F = ctx->n_faces;
    PatchTables& T = D.pt;
    const std::string w(who);
    tm.mark();
    patch_check_inputs(ctx, T, d_labels, who);
    build_patch_tables(ctx, T, d_adj_ptr, d_adj, d_labels, who);
    tm.mark();
    // geometry, sizes, the three scans, the lists
    const uint32_t NP = T.n_patches, C = T.C;
    D.label.ensure((size_t)NP + 1); D.box.ensure((size_t)NP + 1); D.cnt.ensure((size_t)NP + 2); D.face_ptr.ensure((size_t)NP + 2);
    D.npix.ensure((size_t)NP + 2); D.pix_ptr.ensure((size_t)NP + 2); D.nchunk.ensure((size_t)NP + 2); D.chunk_ptr.ensure((size_t)NP + 2);
    D.c64.ensure(K_N);
    MVS_HIP(hipMemsetAsync(D.c64.p, 0, K_N * sizeof(unsigned long long), s));
    MVS_HIP(hipMemsetAsync(D.npix.p, 0, ((size_t)NP + 1) * sizeof(unsigned long long), s));   // entry NP stays 0: the scan of NP + 1 leaves the total there
    hipLaunchKernelGGL(tp_patch_kernel, dim3(grid(C)), dim3(256), 0, s, (const uint32_t*)ctx->p_comp_ptr.p, (const uint32_t*)ctx->p_comp_faces.p, d_labels,
                       (const int4*)T.box.p, (const uint32_t*)T.alive.p, (const uint32_t*)T.pscan.p, (const uint32_t*)T.len.p, C, D.label.p, D.box.p,
                       D.cnt.p, D.npix.p, D.nchunk.p);
    MVS_LAUNCH_CHECK();
    exclusive_scan_u32(ctx, D.cnt.p, D.face_ptr.p, NP, D.face_ptr.p + NP);
    dev_exclusive_scan(ctx, D.npix.p, D.pix_ptr.p, (size_t)NP + 1);
    unsigned long long total = 0; uint32_t listed = 0;
    MVS_HIP(hipMemcpyAsync(&total, D.pix_ptr.p + NP, sizeof(total), hipMemcpyDeviceToHost, s));
    MVS_HIP(hipMemcpyAsync(&listed, D.face_ptr.p + NP, sizeof(listed), hipMemcpyDeviceToHost, s));
    MVS_HIP(hipStreamSynchronize(s));
    n_listed = listed; n_pixels = total;
    S.patches = NP; S.merged = T.n_merged; S.listed_faces = listed; S.pixels = total;
    if (P.max_pixels && total > P.max_pixels)
        throw StatusError(MVS_ERR_UNSUPPORTED, w + ": " + std::to_string(total) + " pixels exceed params.max_pixels = " + std::to_string(P.max_pixels));
    if (total / CHUNK + NP >= 0x7FFFFFFFull) throw StatusError(MVS_ERR_UNSUPPORTED, w + ": too many pixels for one call");
    exclusive_scan_u32(ctx, D.nchunk.p, D.chunk_ptr.p, NP, D.chunk_ptr.p + NP);
    D.faces.ensure((size_t)listed + 1); D.epid.ensure((size_t)listed + 1); D.big.ensure((size_t)listed + 1); D.texcoords.ensure(6 * (size_t)listed + 6);
    hipLaunchKernelGGL(tp_entry_kernel, dim3(grid(F)), dim3(256), 0, s, d_labels, F, (const uint32_t*)T.fcand.p, (const uint32_t*)T.fpid.p,
                       (const uint32_t*)T.fpos.p, (const uint32_t*)T.parent.p, (const int4*)T.box.p, (const float2*)T.pc.p,
                       (const uint32_t*)D.face_ptr.p, D.faces.p, D.epid.p, D.texcoords.p);
    MVS_LAUNCH_CHECK();
    MVS_HIP(hipMemcpyAsync(n_chunks, D.chunk_ptr.p + NP, sizeof(*n_chunks), hipMemcpyDeviceToHost, s));
    tm.mark();
    D.image.ensure(3 * (size_t)total + 3); D.validity.ensure((size_t)total + 1); D.blending.ensure((size_t)total + 1);
}
// the set as the caller receives it: the context's device arrays, or malloc'ed host copies
void texpatch_output(mvs_ctx* ctx, TexPatchDev& D, uint32_t n_listed, uint64_t n_pixels, mvs_patch_set* out, int out_on_device) {
    hipStream_t s = ctx->stream;
    const uint32_t NP = D.pt.n_patches;
    out->n_patches = NP; out->n_listed = n_listed; out->n_pixels = n_pixels;
    if (out_on_device) {
        out->label = D.label.p; out->box = (int32_t*)D.box.p; out->face_ptr = D.face_ptr.p; out->faces = D.faces.p; out->texcoords = D.texcoords.p;
        out->pix_ptr = (uint64_t*)D.pix_ptr.p; out->image = D.image.p; out->validity = D.validity.p; out->blending = D.blending.p;
    } else {
        download(s, out, mvs_patch_set_free, [&] {
            out->label = host_copy(D.label.p, NP, s); out->box = host_copy((const int32_t*)D.box.p, 4 * (size_t)NP, s);
            out->face_ptr = host_copy(D.face_ptr.p, (size_t)NP + 1, s); out->faces = host_copy(D.faces.p, n_listed, s);
            out->texcoords = host_copy(D.texcoords.p, 6 * (size_t)n_listed, s);
            out->pix_ptr = host_copy((const uint64_t*)D.pix_ptr.p, (size_t)NP + 1, s);
            out->image = host_copy(D.image.p, 3 * (size_t)n_pixels, s); out->validity = host_copy(D.validity.p, (size_t)n_pixels, s);
            out->blending = host_copy(D.blending.p, (size_t)n_pixels, s);
        });
    }
}

namespace {
// the whole row on the context's stream; the pixel arrays are left in D
void run_texpatch(mvs_ctx* ctx, TexPatchDev& D, const uint32_t* d_adj_ptr, const uint32_t* d_adj, const uint32_t* d_labels, const float* d_adjust,
                  const mvs_patch_params& P, mvs_patch_stats& S, uint32_t& n_listed, uint64_t& n_pixels) {
    hipStream_t s = ctx->stream;
    StageTimer<5> tm(s);   // marks: begin, tables, lists, mark, resolve
    uint32_t n_chunks = 0;
    const uint32_t tone = tone_mode(P.tone_mapping, "texture_patches");
    const float* d_tone = tone == TONE_GAMMA ? tone_table_dev(ctx) : nullptr;
    texpatch_geometry(ctx, D, d_adj_ptr, d_adj, d_labels, P, S, n_listed, n_pixels, &n_chunks, tm, "texture_patches");
    PatchTables& T = D.pt;
    const uint32_t NP = T.n_patches, listed = n_listed;
    const unsigned long long total = n_pixels;
    // mark
    D.win_in.ensure((size_t)total + 1); D.win_near.ensure((size_t)total + 1);
    MVS_HIP(hipMemsetAsync(D.win_in.p, 0, (size_t)total * sizeof(uint32_t), s));
    MVS_HIP(hipMemsetAsync(D.win_near.p, 0xFF, (size_t)total * sizeof(uint32_t), s));
    if (listed) {
        hipLaunchKernelGGL(tp_mark_kernel, dim3(grid((size_t)listed * GROUP)), dim3(256), 0, s, listed, (const uint32_t*)D.epid.p, (const uint32_t*)D.face_ptr.p,
                           (const float*)D.texcoords.p, (const int4*)D.box.p, (const unsigned long long*)D.pix_ptr.p, D.win_in.p, D.win_near.p, D.big.p, D.c64.p);
        MVS_LAUNCH_CHECK();
        hipLaunchKernelGGL(tp_mark_big_kernel, dim3(BIG_BLOCKS), dim3(256), 0, s, (const uint32_t*)D.big.p, (const unsigned long long*)D.c64.p,
                           (const uint32_t*)D.epid.p, (const uint32_t*)D.face_ptr.p, (const float*)D.texcoords.p, (const int4*)D.box.p,
                           (const unsigned long long*)D.pix_ptr.p, D.win_in.p, D.win_near.p);
        MVS_LAUNCH_CHECK();
    }
    tm.mark();
    // resolve
    MVS_HIP(hipStreamSynchronize(s));   // n_chunks
    if (n_chunks) {
        auto* resolve = tone == TONE_GAMMA ? tp_resolve_kernel<TONE_GAMMA> : tp_resolve_kernel<TONE_NONE>;
        hipLaunchKernelGGL(resolve, dim3(n_chunks), dim3(256), 0, s, d_tone, NP, (const uint32_t*)D.chunk_ptr.p, (const uint32_t*)D.label.p,
                           (const int4*)D.box.p, (const uint32_t*)D.face_ptr.p, (const uint32_t*)D.faces.p, (const float*)D.texcoords.p,
                           (const unsigned long long*)D.pix_ptr.p, (const ViewParams*)T.views.p, d_adjust, (const uint32_t*)D.win_in.p,
                           (const uint32_t*)D.win_near.p, D.image.p, D.validity.p, D.blending.p, D.c64.p);
        MVS_LAUNCH_CHECK();
    }
    tm.mark();
    unsigned long long c64[K_N];
    MVS_HIP(hipMemcpyAsync(c64, D.c64.p, sizeof(c64), hipMemcpyDeviceToHost, s));
    MVS_HIP(hipStreamSynchronize(s));
    S.degenerate_faces = c64[K_DEGENERATE]; S.valid_pixels = c64[K_VALID]; S.near_pixels = c64[K_NEAR];
    S.ms_tables = tm.ms(0, 1); S.ms_lists = tm.ms(1, 2); S.ms_mark = tm.ms(2, 3); S.ms_resolve = tm.ms(3, 4);
    S.ms_total = tm.ms(0, 4);
}

}  // namespace
}  // namespace mvs

using namespace mvs;

extern "C" {

void mvs_patch_default_params(mvs_patch_params* p) {
    if (!p) return;
    p->max_pixels = 0; p->tone_mapping = MVS_TONE_NONE; p->reserved = 0;
}

mvs_status mvs_ctx_texture_patches(mvs_ctx* ctx, const uint32_t* adj_ptr, const uint32_t* adj, int adj_on_device, const uint32_t* labels,
                                   int labels_on_device, const float* corner_adjust, int adjust_on_device, const mvs_patch_params* params,
                                   mvs_patch_set* out, int out_on_device, mvs_patch_stats* stats) {
    if (!ctx || !out) return api_fail(MVS_ERR_INVALID, "null argument");
    if (!ctx->d_verts || !ctx->d_faces || ctx->n_views == 0 || ctx->h_views.size() < ctx->n_views)
        return api_fail(MVS_ERR_STATE, "texture patches need the mesh and the views (mvs_scene_set_mesh, mvs_scene_set_views)");
    const uint32_t F = ctx->n_faces;
    if (F && (!adj_ptr || !adj || !labels)) return api_fail(MVS_ERR_INVALID, "null argument");
    *out = mvs_patch_set{};
    mvs_patch_stats S{};
    return api_guard([&] {
        MVS_HIP(hipSetDevice(ctx->device));
        hipStream_t s = ctx->stream;
        TexPatchDev& D = row_dev(ctx->texpatch);
        mvs_patch_params P;
        if (params) P = *params; else mvs_patch_default_params(&P);
        const RowGraph g = stage_graph(ctx, adj_ptr, adj, adj_on_device, labels, labels_on_device);
        const float* d_adjust = corner_adjust && F ? stage(D.adjust, corner_adjust, 9 * (size_t)F, adjust_on_device, s) : corner_adjust;
        if (F) MVS_HIP(hipStreamSynchronize(s));   // host buffers are borrowed for the call only
        uint32_t n_listed = 0; uint64_t n_pixels = 0;
        run_with_stats(s, stats, S, [&] { run_texpatch(ctx, D, g.adj_ptr, g.adj, g.labels, d_adjust, P, S, n_listed, n_pixels); });
        texpatch_output(ctx, D, n_listed, n_pixels, out, out_on_device);
    });
}

void mvs_patch_set_free(mvs_patch_set* r) {
    if (!r) return;
    free(r->label); free(r->box); free(r->face_ptr); free(r->faces); free(r->texcoords); free(r->pix_ptr); free(r->image); free(r->validity); free(r->blending);
    *r = mvs_patch_set{};
}

}  // extern "C"
