// k_seam.hip -- row f5: tex::global_seam_leveling (libs/tex/global_seam_leveling.cpp), tone mapping `none` or `gamma` (the b sampler is
//   instantiated on the mode: under gamma a texel is the context's table at its byte, tone.h), together with the
//   parts of generate_texture_patches it reads (candidate boxes and merges, generate_texture_patches.cpp:78-138 / :484-508 -- the
//   tables of build_patch_tables, k_texpatch.hip, which row f6 builds with the same functions; the vertex projections
//   merge_vertex_projection_infos keeps, :40-65).  The definition (DESIGN.md section 4 "Global seam leveling", items
//   1-9) is shared with the CPU model of the tests (tests/tools/seam_model.cpp): every output is bit-identical to it on any device.
//   Structure: sorted (vertex, value) pairs for the vertex -> faces lists, the vertex rows and the rings; one thread per face
//   (boxes), per label (the merge loop is sequential), per candidate (frame chains) -- those three in k_texpatch.hip --, per vertex (A rows), per A row (seam edges and
//   the b sampler: each row's accumulation order is fixed), per x row (Lhs, Rhs).
//   Solve: Jacobi-preconditioned CG on the three channels at once, each with its own alpha, beta and stop state; two launches per
//   iteration (the SpMV forms p = z + beta p on the fly for every column it reads; the update forms x, r and the next partials),
//   replayed as a linear captured graph of GSL_GRAPH_ITERS iterations; a device word says when every channel has stopped.
//   Reductions follow the fixed two-level tree of item 8 (grid from x_rows only), so the bits do not depend on the device.
#include "rows.h"
#include "tone.h"
#include <cfloat>
#include <climits>

namespace mvs {

namespace {
constexpr uint32_t NONE = 0xFFFFFFFFu;
constexpr unsigned long long NONE64 = ~0ull;
constexpr uint32_t RED_BLOCKS = 1024;       // level one of the reduction tree: at most this many blocks of 256 (item 8)
constexpr int GSL_GRAPH_ITERS = 16;         // CG iterations per graph replay (even: the ping-pong buffers alternate by iteration)
// partial-sum slots of RED_BLOCKS floats: [0, 3) p.Ap per channel; 3 + 6 q + {0: r.r, 3: r.z} + c for the parity q; [15, 18) sums of x
constexpr uint32_t SLOT_RR = 3, SLOT_MEAN = 15, SLOTS = 18;
enum { C_SEAM = 0, C_SAMPLES, C_GAMMA2, C_LOWER, C_N };                            // 64-bit counters
enum { F_DONE = 0, F_N };                                                          // flag words
}  // namespace

struct GslChan { float rhs2, thr, rz, err; uint32_t active, iters, pad0, pad1; };
struct GslState { GslChan ch[3]; uint32_t k, pad[3]; };

// per-context buffers of row f5, allocated on first use, freed with the context (gsl_release)
struct GslDev {
    DBuf<unsigned long long> keys, keys2; DBuf<uint32_t> flag, pos, cnt;
    DBuf<uint32_t> vf_ptr, vf, x_ptr, x_label, x_vert, ring_ptr, ring;
    PatchTables pt;
    DBuf<uint32_t> a_ptr, a_col, a_vert; DBuf<float> b;
    DBuf<uint32_t> lhs_ptr, lhs_col; DBuf<float> lhs_val, invdiag, rhs;
    DBuf<float> x, r, p, ap, xadj, corner, part;
    DBuf<GslState> st; DBuf<unsigned long long> c64; DBuf<uint32_t> flags;
    hipStream_t cap = nullptr;
    uint32_t NV = 0, F = 0, XR = 0, AR = 0; uint64_t NNZ = 0; bool valid = false;   // shapes of the last successful call
    ~GslDev() { if (cap) (void)hipStreamDestroy(cap); }
};
void gsl_release(mvs_ctx* ctx) { delete ctx->gsl; ctx->gsl = nullptr; }

namespace {

// the device arrays the per-row kernels read
struct GslView {
    const float* verts; const uint32_t* faces; const uint32_t* labels;
    const uint32_t* vf_ptr; const uint32_t* vf; const uint32_t* x_ptr; const uint32_t* x_label; const uint32_t* ring_ptr; const uint32_t* ring;
    const int4* box; const float2* pc; const uint32_t* fcand; const uint32_t* parent; const uint32_t* fpid; const uint32_t* fpos;
    const ViewParams* views;
    const float* tone;   // the 256 texel values of tone mapping `gamma` (null under `none`)
};

// ---- 1. (vertex, value) pairs -> CSR (the checks on labels and faces: patch_check_inputs, k_texpatch.hip) ----
// what 0: (vertex, face), a repeated corner once; 1: (vertex, label) of the labelled faces; 2: (vertex, other corner) -- keys row << 32 | value
__global__ void gsl_key_kernel(const uint32_t* __restrict__ faces, const uint32_t* __restrict__ labels, uint32_t F, int what, unsigned long long* __restrict__ keys) {
    const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F) return;
    const unsigned long long a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
    if (what == 0) {
        keys[3 * f] = a << 32 | f; keys[3 * f + 1] = b != a ? (b << 32 | f) : NONE64; keys[3 * f + 2] = (c != a && c != b) ? (c << 32 | f) : NONE64;
    } else if (what == 1) {
        const unsigned long long L = labels[f];
        keys[3 * f] = L ? (a << 32 | L) : NONE64; keys[3 * f + 1] = L ? (b << 32 | L) : NONE64; keys[3 * f + 2] = L ? (c << 32 | L) : NONE64;
    } else {
        keys[6 * f] = a != b ? (a << 32 | b) : NONE64; keys[6 * f + 1] = a != c ? (a << 32 | c) : NONE64;
        keys[6 * f + 2] = b != a ? (b << 32 | a) : NONE64; keys[6 * f + 3] = b != c ? (b << 32 | c) : NONE64;
        keys[6 * f + 4] = c != a ? (c << 32 | a) : NONE64; keys[6 * f + 5] = c != b ? (c << 32 | b) : NONE64;
    }
}
__global__ void gsl_unique_flag_kernel(const unsigned long long* __restrict__ keys, uint32_t n, uint32_t* __restrict__ flag) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const unsigned long long k = keys[i];
    flag[i] = (k != NONE64 && (i == 0 || keys[i - 1] != k)) ? 1u : 0u;
}
__global__ void gsl_unique_compact_kernel(const unsigned long long* __restrict__ keys, const uint32_t* __restrict__ flag, const uint32_t* __restrict__ pos,
                                          uint32_t n, uint32_t* __restrict__ val, uint32_t* __restrict__ row_of, uint32_t* __restrict__ cnt) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !flag[i]) return;
    const uint32_t row = (uint32_t)(keys[i] >> 32);
    val[pos[i]] = (uint32_t)keys[i];
    if (row_of) row_of[pos[i]] = row;
    atomicAdd(cnt + row, 1u);
}

// ---- 3. patches: build_patch_tables (k_texpatch.hip), shared with row f6 ----

// ---- 4.-6. seam edges, projections, samples ----
__device__ inline bool in_list(const uint32_t* a, uint32_t b0, uint32_t b1, uint32_t x) {
    for (uint32_t i = b0; i < b1; ++i) if (a[i] == x) return true;
    return false;
}
__device__ inline float edge_len(const float* verts, uint32_t v, uint32_t u) {
    const float dx = verts[3 * (size_t)u] - verts[3 * (size_t)v], dy = verts[3 * (size_t)u + 1] - verts[3 * (size_t)v + 1];
    const float dz = verts[3 * (size_t)u + 2] - verts[3 * (size_t)v + 2];
    return sqrtf((dx * dx + dy * dy) + dz * dz);
}
// face pairs j < k on the edge (v, u) whose labels are {l1, l2}: the seam-edge entries of the edge
__device__ uint32_t seam_entries(const GslView& g, uint32_t v, uint32_t u, uint32_t l1, uint32_t l2) {
    const uint32_t a0 = g.vf_ptr[v], a1 = g.vf_ptr[v + 1], b0 = g.vf_ptr[u], b1 = g.vf_ptr[u + 1];
    uint32_t n = 0;
    for (uint32_t i = a0; i < a1; ++i) {
        const uint32_t f = g.vf[i];
        if (!in_list(g.vf, b0, b1, f)) continue;
        for (uint32_t j = i + 1; j < a1; ++j) {
            const uint32_t h = g.vf[j];
            if (!in_list(g.vf, b0, b1, h)) continue;
            uint32_t la = g.labels[f], lb = g.labels[h];
            if (!(la < lb)) { const uint32_t t = la; la = lb; lb = t; }
            if (la == l1 && lb == l2) ++n;
        }
    }
    return n;
}
__device__ inline uint32_t find_row(const GslView& g, uint32_t v, uint32_t l) {
    for (uint32_t t = g.x_ptr[v]; t < g.x_ptr[v + 1]; ++t) if (g.x_label[t] == l) return t;
    return NONE;
}
// item 4: v's projection in patch P -- the first face of P's list holding v, through its candidate's chain of frames
__device__ float2 vproj(const GslView& g, uint32_t v, uint32_t P) {
    uint32_t best = NONE, bf = 0;
    for (uint32_t i = g.vf_ptr[v]; i < g.vf_ptr[v + 1]; ++i) { const uint32_t f = g.vf[i]; if (g.fpid[f] == P && g.fpos[f] < best) { best = g.fpos[f]; bf = f; } }
    uint32_t k = 0;
    while (k < 2 && g.faces[3 * (size_t)bf + k] != v) ++k;
    uint32_t c = g.fcand[bf];
    int4 b = g.box[c];
    const float2 q = g.pc[3 * (size_t)bf + k];
    float x = q.x - (float)b.x, y = q.y - (float)b.y;
    for (uint32_t p = g.parent[c]; p != NONE; p = g.parent[c]) {
        const int4 bp = g.box[p];
        x = x + (float)(b.x - bp.x); y = y + (float)(b.y - bp.y);
        c = p; b = bp;
    }
    return make_float2(x, y);
}
template <int TONE>
__device__ inline float texel(const ViewParams& vw, const float* __restrict__ tone, int x, int y, int ch) {
    if (TONE == TONE_GAMMA) {   // the crop in bytes, fill included, through the table (generate_texture_patches.cpp:126-132)
        if (x < 0 || y < 0 || x >= vw.width || y >= vw.height) return tone[ch == 1 ? 0 : 255];
        return tone[vw.rgb[((size_t)y * vw.width + x) * 3 + ch]];
    }
    if (x < 0 || y < 0 || x >= vw.width || y >= vw.height) return ch == 1 ? 0.0f : 1.0f;   // the crop's fill (255, 0, 255)
    return (float)vw.rgb[((size_t)y * vw.width + x) * 3 + ch] / 255.0f;
}
// sample_edge (global_seam_leveling.cpp:26-44) on the patch with frame bx of view vw; bilinear as item 6
template <int TONE>
__device__ void sample_edge(const ViewParams& vw, const float* __restrict__ tone, int4 bx, float2 p1, float2 p2, float* out, unsigned long long& ns) {
    const int pw = bx.z - bx.x + 2, ph = bx.w - bx.y + 2;
    const float W1 = (float)(pw - 1), H1 = (float)(ph - 1);
    const float dx = p2.x - p1.x, dy = p2.y - p1.y;
    const float nrm = sqrtf(dx * dx + dy * dy);
    const uint32_t n = (uint32_t)((nrm < 1.0f ? 1.0f : nrm) * 2.0f);
    float acc[3] = {0.0f, 0.0f, 0.0f}, wsum = 0.0f;
    for (uint32_t s = 0; s < n; ++s) {
        const float fraction = (float)s / (float)(n - 1);
        float x = p1.x + dx * fraction, y = p1.y + dy * fraction;
        x = (x < W1) ? x : W1; x = (0.0f < x) ? x : 0.0f;
        y = (y < H1) ? y : H1; y = (0.0f < y) ? y : 0.0f;
        const int fx = (int)x, fy = (int)y;
        const int fx1 = min(fx + 1, pw - 1), fy1 = min(fy + 1, ph - 1);
        const float w1 = x - (float)fx, w0 = 1.0f - w1, w3 = y - (float)fy, w2 = 1.0f - w3;
        const float w = 1.0f - fraction;
        for (int ch = 0; ch < 3; ++ch) {
            const float v1 = texel<TONE>(vw, tone, fx + bx.x, fy + bx.y, ch), v2 = texel<TONE>(vw, tone, fx1 + bx.x, fy + bx.y, ch);
            const float v3 = texel<TONE>(vw, tone, fx + bx.x, fy1 + bx.y, ch), v4 = texel<TONE>(vw, tone, fx1 + bx.x, fy1 + bx.y, ch);
            const float col = ((v1 * (w0 * w2) + v2 * (w1 * w2)) + v3 * (w0 * w3)) + v4 * (w1 * w3);
            acc[ch] = acc[ch] + col * w;
        }
        wsum = wsum + w;
    }
    ns += n;
    for (int ch = 0; ch < 3; ++ch) out[ch] = acc[ch] / wsum;
}
// A rows of a vertex: label pairs (j < k) with at least one seam edge; fill = 0 counts, else writes the rows from a_ptr[v]
__global__ void gsl_a_rows_kernel(GslView g, uint32_t NV, int fill, uint32_t* __restrict__ acnt, const uint32_t* __restrict__ a_ptr,
                                  uint32_t* __restrict__ a_col, uint32_t* __restrict__ a_vert) {
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= NV) return;
    const uint32_t x0 = g.x_ptr[v], m = g.x_ptr[v + 1] - x0;
    uint32_t n = 0;
    for (uint32_t j = 0; j < m; ++j)
        for (uint32_t k = j + 1; k < m; ++k) {
            const uint32_t l1 = g.x_label[x0 + j], l2 = g.x_label[x0 + k];
            bool any = false;
            for (uint32_t e = g.ring_ptr[v]; e < g.ring_ptr[v + 1] && !any; ++e) {
                const uint32_t u = g.ring[e];
                any = edge_len(g.verts, v, u) != 0.0f && seam_entries(g, v, u, l1, l2) != 0;
            }
            if (!any) continue;
            if (fill) { const uint32_t r = a_ptr[v] + n; a_col[2 * r] = x0 + j; a_col[2 * r + 1] = x0 + k; a_vert[r] = v; }
            ++n;
        }
    if (!fill) acnt[v] = n;
}
// b of one A row (calculate_difference, global_seam_leveling.cpp:76-138): seam-edge entries in ring order, per entry the edge's patches
// of label l1 / l2 in ascending id, each sampled from p(v) to p(u) and accumulated with the edge's 3-D length
template <int TONE>
__global__ void gsl_b_kernel(GslView g, uint32_t AR, const uint32_t* __restrict__ a_col, const uint32_t* __restrict__ a_vert,
                             float* __restrict__ b, unsigned long long* __restrict__ c64) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= AR) return;
    const uint32_t v = a_vert[r], l1 = g.x_label[a_col[2 * r]], l2 = g.x_label[a_col[2 * r + 1]];
    float c1[3] = {0.0f, 0.0f, 0.0f}, c2[3] = {0.0f, 0.0f, 0.0f}, w1 = 0.0f, w2 = 0.0f;
    unsigned long long seam = 0, ns = 0;
    const uint32_t a0 = g.vf_ptr[v], a1 = g.vf_ptr[v + 1];
    for (uint32_t e = g.ring_ptr[v]; e < g.ring_ptr[v + 1]; ++e) {
        const uint32_t u = g.ring[e];
        const float len = edge_len(g.verts, v, u);
        if (len == 0.0f) continue;
        const uint32_t entries = seam_entries(g, v, u, l1, l2);
        seam += entries;
        const uint32_t b0 = g.vf_ptr[u], b1 = g.vf_ptr[u + 1];
        for (uint32_t rep = 0; rep < entries; ++rep) {
            uint32_t last = 0; bool first = true;
            for (;;) {   // the next patch id above `last` among the edge's faces of label l1 / l2
                uint32_t P = NONE, PL = 0, Pf = 0;
                for (uint32_t i = a0; i < a1; ++i) {
                    const uint32_t f = g.vf[i], L = g.labels[f];
                    if ((L != l1 && L != l2) || !in_list(g.vf, b0, b1, f)) continue;
                    const uint32_t pid = g.fpid[f];
                    if ((first || pid > last) && pid < P) { P = pid; PL = L; Pf = f; }
                }
                if (P == NONE) break;
                first = false; last = P;
                uint32_t root = g.fcand[Pf];
                while (g.parent[root] != NONE) root = g.parent[root];
                float col[3];
                sample_edge<TONE>(g.views[PL - 1], g.tone, g.box[root], vproj(g, v, P), vproj(g, u, P), col, ns);
                if (PL == l1) { for (int ch = 0; ch < 3; ++ch) c1[ch] = c1[ch] + col[ch] * len; w1 = w1 + len; }
                else { for (int ch = 0; ch < 3; ++ch) c2[ch] = c2[ch] + col[ch] * len; w2 = w2 + len; }
            }
        }
    }
    for (int ch = 0; ch < 3; ++ch) b[3 * (size_t)r + ch] = c2[ch] / w2 - c1[ch] / w1;
    atomicAdd(c64 + C_SEAM, seam); atomicAdd(c64 + C_SAMPLES, ns);
}

// ---- 5.+7. Gamma, Lhs = AtA + GtG (full symmetric rows, columns ascending), Rhs = At b ----
__global__ void gsl_lhs_count_kernel(GslView g, uint32_t XR, const uint32_t* __restrict__ x_vert, const uint32_t* __restrict__ a_ptr,
                                     const uint32_t* __restrict__ a_col, uint32_t* __restrict__ lcnt, unsigned long long* __restrict__ c64) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= XR) return;
    const uint32_t v = x_vert[i], l = g.x_label[i];
    uint32_t n = 0, low = 0, cnt = 0;
    for (uint32_t e = g.ring_ptr[v]; e < g.ring_ptr[v + 1]; ++e) {
        const uint32_t u = g.ring[e];
        if (find_row(g, u, l) != NONE) { ++n; if (u < v) ++low; }
    }
    for (uint32_t r = a_ptr[v]; r < a_ptr[v + 1]; ++r) {
        const uint32_t ca = a_col[2 * r], cb = a_col[2 * r + 1];
        if (ca != i && cb != i) continue;
        ++cnt; if ((ca == i ? cb : ca) < i) ++low;
    }
    const uint32_t diag = (cnt || n) ? 1u : 0u;
    lcnt[i] = n + cnt + diag;
    atomicAdd(c64 + C_GAMMA2, (unsigned long long)n); atomicAdd(c64 + C_LOWER, (unsigned long long)(low + diag));
}
__global__ void gsl_lhs_fill_kernel(GslView g, uint32_t XR, const uint32_t* __restrict__ x_vert, const uint32_t* __restrict__ a_ptr,
                                    const uint32_t* __restrict__ a_col, const float* __restrict__ b, const uint32_t* __restrict__ lhs_ptr, float gam,
                                    uint32_t* __restrict__ lhs_col, float* __restrict__ lhs_val, float* __restrict__ invdiag, float* __restrict__ rhs) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= XR) return;
    const uint32_t v = x_vert[i], l = g.x_label[i], x0 = g.x_ptr[v], m = g.x_ptr[v + 1] - x0, j = i - x0;
    uint32_t o = lhs_ptr[i], n = 0;
    for (uint32_t e = g.ring_ptr[v]; e < g.ring_ptr[v + 1]; ++e) {
        const uint32_t u = g.ring[e], c = find_row(g, u, l);
        if (c == NONE) continue;
        ++n;
        if (u < v) { lhs_col[o] = c; lhs_val[o] = -gam; ++o; }
    }
    uint32_t cnt = 0;
    float acc[3] = {0.0f, 0.0f, 0.0f};
    for (uint32_t r = a_ptr[v]; r < a_ptr[v + 1]; ++r) {
        const uint32_t ca = a_col[2 * r], cb = a_col[2 * r + 1];
        if (ca != i && cb != i) continue;
        ++cnt;
        const float coef = ca == i ? 1.0f : -1.0f;
        for (int ch = 0; ch < 3; ++ch) acc[ch] = acc[ch] + coef * b[3 * (size_t)r + ch];
    }
    for (int ch = 0; ch < 3; ++ch) rhs[(size_t)ch * XR + i] = acc[ch];
    float gs = 0.0f;
    for (uint32_t t = 0; t < n; ++t) gs = gs + gam;
    float d = 0.0f;
    for (uint32_t k = 0; k < m; ++k) {
        if (k == j) {
            if (cnt && n) d = (float)cnt + gs; else if (cnt) d = (float)cnt; else if (n) d = gs;
            if (cnt || n) { lhs_col[o] = i; lhs_val[o] = d; ++o; }
            continue;
        }
        const uint32_t lo = min(j, k) + x0, hi = max(j, k) + x0;
        bool partner = false;
        for (uint32_t r = a_ptr[v]; r < a_ptr[v + 1] && !partner; ++r) partner = a_col[2 * r] == lo && a_col[2 * r + 1] == hi;
        if (partner) { lhs_col[o] = x0 + k; lhs_val[o] = -1.0f; ++o; }
    }
    for (uint32_t e = g.ring_ptr[v]; e < g.ring_ptr[v + 1]; ++e) {
        const uint32_t u = g.ring[e];
        if (u <= v) continue;
        const uint32_t c = find_row(g, u, l);
        if (c != NONE) { lhs_col[o] = c; lhs_val[o] = -gam; ++o; }
    }
    invdiag[i] = d != 0.0f ? 1.0f / d : 1.0f;
}

// ---- 8. CG ----
// the halving tree of item 8 over the block's 256 values (every thread calls it)
__device__ inline float block_sum(float v, float* sh) {
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) { if (t < s) sh[t] = sh[t] + sh[t + s]; __syncthreads(); }
    const float r = sh[0];
    __syncthreads();
    return r;
}
__device__ inline float level2(const float* part, uint32_t NB, float* sh) {
    float a = 0.0f;
    for (uint32_t j = threadIdx.x; j < NB; j += 256) a = a + part[j];
    return block_sum(a, sh);
}
__global__ void __launch_bounds__(256) gsl_cg_init_kernel(uint32_t n, uint32_t NB, const float* __restrict__ rhs, const float* __restrict__ invdiag,
                                                          float* __restrict__ x, float* __restrict__ r, float* __restrict__ part, GslState* __restrict__ st,
                                                          uint32_t* __restrict__ flags) {
    __shared__ float sh[256];
    const uint32_t T = (n + 255) / 256;
    float rr[3] = {0.0f, 0.0f, 0.0f}, rz[3] = {0.0f, 0.0f, 0.0f};
    for (uint32_t tile = blockIdx.x; tile < T; tile += NB) {
        const uint32_t i = tile * 256 + threadIdx.x;
        if (i >= n) continue;
        const float di = invdiag[i];
        for (int c = 0; c < 3; ++c) {
            const float ri = rhs[(size_t)c * n + i];
            r[(size_t)c * n + i] = ri; x[(size_t)c * n + i] = 0.0f;
            const float zi = di * ri;
            rr[c] = rr[c] + ri * ri; rz[c] = rz[c] + ri * zi;
        }
    }
    for (int c = 0; c < 3; ++c) {
        const float a = block_sum(rr[c], sh), z = block_sum(rz[c], sh);
        if (threadIdx.x == 0) { part[(SLOT_RR + c) * RED_BLOCKS + blockIdx.x] = a; part[(SLOT_RR + 3 + c) * RED_BLOCKS + blockIdx.x] = z; }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        GslState s{};
        for (int c = 0; c < 3; ++c) s.ch[c].active = 1u;
        st[0] = s; flags[F_DONE] = 0u;
    }
}
// iteration k, parity q = k & 1: decide every channel from the partials of r.r and r.z (the previous update's, or the initial ones),
// then tmp = Lhs p with p_k = z + beta p_{k-1} formed for every column read (p_0 = z), p_k stored, partials of p.Ap.
// State: st[q] read, st[q ^ 1] and the final copy st[2] written by block 0; every block takes the same decision from the same bits.
__global__ void __launch_bounds__(256) gsl_cg_spmv_kernel(uint32_t q, uint32_t n, uint32_t NB, const uint32_t* __restrict__ lhs_ptr,
                                                          const uint32_t* __restrict__ lhs_col, const float* __restrict__ lhs_val,
                                                          const float* __restrict__ invdiag, const float* __restrict__ r, float* __restrict__ p,
                                                          float* __restrict__ ap, float* __restrict__ part, GslState* __restrict__ st,
                                                          uint32_t* __restrict__ flags, float tol2, uint32_t max_iters) {
    __shared__ float sh[256];
    __shared__ float s_beta[3];
    __shared__ uint32_t s_act[3], s_first, s_any, s_done;
    if (threadIdx.x == 0) s_done = __hip_atomic_load(flags + F_DONE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // block 0 may set it meanwhile:
    __syncthreads();                                                                                                // one decision per block
    if (s_done) return;
    float rr[3], rz[3];
    for (int c = 0; c < 3; ++c) {
        rr[c] = level2(part + (SLOT_RR + 6 * q + c) * RED_BLOCKS, NB, sh);
        rz[c] = level2(part + (SLOT_RR + 6 * q + 3 + c) * RED_BLOCKS, NB, sh);
    }
    if (threadIdx.x == 0) {
        GslState s = st[q];
        const uint32_t k = s.k;
        uint32_t any = 0;
        for (int c = 0; c < 3; ++c) {
            GslChan& C = s.ch[c];
            float beta = 0.0f;
            if (C.active) {
                if (k == 0) {
                    C.rhs2 = rr[c];
                    if (rr[c] == 0.0f) { C.active = 0; C.iters = 0; C.err = 0.0f; }
                    else {
                        const float t = tol2 * rr[c];
                        C.thr = (t < FLT_MIN) ? FLT_MIN : t;
                        if (rr[c] < C.thr || max_iters == 0) { C.active = 0; C.iters = 0; C.err = sqrtf(rr[c] / C.rhs2); }
                        else C.rz = rz[c];
                    }
                } else if (rr[c] < C.thr) { C.active = 0; C.iters = k - 1; C.err = sqrtf(rr[c] / C.rhs2); }
                else if (k >= max_iters) { C.active = 0; C.iters = k; C.err = sqrtf(rr[c] / C.rhs2); }
                else { beta = rz[c] / C.rz; C.rz = rz[c]; }
            }
            s_beta[c] = beta; s_act[c] = C.active; any |= C.active;
        }
        s.k = k + 1;
        s_first = k == 0 ? 1u : 0u; s_any = any;
        if (blockIdx.x == 0) {
            st[q ^ 1u] = s; st[2] = s;
            if (!any) __hip_atomic_store(flags + F_DONE, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    __syncthreads();
    if (!s_any) return;
    const bool first = s_first != 0;
    const float* pold = p + (size_t)(q ^ 1u) * 3 * n;
    float* pnew = p + (size_t)q * 3 * n;
    const uint32_t T = (n + 255) / 256;
    float acc[3] = {0.0f, 0.0f, 0.0f};
    for (uint32_t tile = blockIdx.x; tile < T; tile += NB) {
        const uint32_t i = tile * 256 + threadIdx.x;
        if (i >= n) continue;
        float s[3] = {0.0f, 0.0f, 0.0f};
        for (uint32_t e = lhs_ptr[i]; e < lhs_ptr[i + 1]; ++e) {
            const uint32_t j = lhs_col[e];
            const float val = lhs_val[e], dj = invdiag[j];
            for (int c = 0; c < 3; ++c) {
                if (!s_act[c]) continue;
                const float zj = dj * r[(size_t)c * n + j];
                const float pj = first ? zj : zj + s_beta[c] * pold[(size_t)c * n + j];
                s[c] = s[c] + val * pj;
            }
        }
        const float di = invdiag[i];
        for (int c = 0; c < 3; ++c) {
            if (!s_act[c]) continue;
            const float zi = di * r[(size_t)c * n + i];
            const float pi = first ? zi : zi + s_beta[c] * pold[(size_t)c * n + i];
            pnew[(size_t)c * n + i] = pi; ap[(size_t)c * n + i] = s[c];
            acc[c] = acc[c] + pi * s[c];
        }
    }
    for (int c = 0; c < 3; ++c) {
        const float t = block_sum(acc[c], sh);
        if (threadIdx.x == 0) part[c * RED_BLOCKS + blockIdx.x] = t;
    }
}
// iteration k, parity q: alpha = rz / p.Ap, x += alpha p, r -= alpha tmp, partials of r.r and r.z (z = invdiag r) for iteration k + 1
__global__ void __launch_bounds__(256) gsl_cg_update_kernel(uint32_t q, uint32_t n, uint32_t NB, const float* __restrict__ invdiag, float* __restrict__ x,
                                                            float* __restrict__ r, const float* __restrict__ p, const float* __restrict__ ap,
                                                            float* __restrict__ part, const GslState* __restrict__ st, uint32_t* __restrict__ flags) {
    __shared__ float sh[256];
    __shared__ float s_alpha[3];
    __shared__ uint32_t s_act[3], s_done;
    if (threadIdx.x == 0) s_done = __hip_atomic_load(flags + F_DONE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    if (s_done) return;
    float pap[3];
    for (int c = 0; c < 3; ++c) pap[c] = level2(part + c * RED_BLOCKS, NB, sh);
    if (threadIdx.x == 0) {
        const GslState& s = st[q ^ 1u];
        for (int c = 0; c < 3; ++c) { s_act[c] = s.ch[c].active; s_alpha[c] = s.ch[c].active ? s.ch[c].rz / pap[c] : 0.0f; }
    }
    __syncthreads();
    const float* pk = p + (size_t)q * 3 * n;
    const uint32_t T = (n + 255) / 256;
    float rr[3] = {0.0f, 0.0f, 0.0f}, rz[3] = {0.0f, 0.0f, 0.0f};
    for (uint32_t tile = blockIdx.x; tile < T; tile += NB) {
        const uint32_t i = tile * 256 + threadIdx.x;
        if (i >= n) continue;
        const float di = invdiag[i];
        for (int c = 0; c < 3; ++c) {
            if (!s_act[c]) continue;
            const size_t o = (size_t)c * n + i;
            x[o] = x[o] + s_alpha[c] * pk[o];
            const float ri = r[o] - s_alpha[c] * ap[o];
            r[o] = ri;
            const float zi = di * ri;
            rr[c] = rr[c] + ri * ri; rz[c] = rz[c] + ri * zi;
        }
    }
    for (int c = 0; c < 3; ++c) {
        const float a = block_sum(rr[c], sh), z = block_sum(rz[c], sh);
        if (threadIdx.x == 0) {
            part[(SLOT_RR + 6 * (q ^ 1u) + c) * RED_BLOCKS + blockIdx.x] = a;
            part[(SLOT_RR + 6 * (q ^ 1u) + 3 + c) * RED_BLOCKS + blockIdx.x] = z;
        }
    }
}
// x -= sum(x) / x_rows: partials, then every block reduces them and writes x_adjust interleaved per row
__global__ void __launch_bounds__(256) gsl_mean_part_kernel(uint32_t n, uint32_t NB, const float* __restrict__ x, float* __restrict__ part) {
    __shared__ float sh[256];
    const uint32_t T = (n + 255) / 256;
    float acc[3] = {0.0f, 0.0f, 0.0f};
    for (uint32_t tile = blockIdx.x; tile < T; tile += NB) {
        const uint32_t i = tile * 256 + threadIdx.x;
        if (i < n) for (int c = 0; c < 3; ++c) acc[c] = acc[c] + x[(size_t)c * n + i];
    }
    for (int c = 0; c < 3; ++c) { const float t = block_sum(acc[c], sh); if (threadIdx.x == 0) part[(SLOT_MEAN + c) * RED_BLOCKS + blockIdx.x] = t; }
}
__global__ void __launch_bounds__(256) gsl_mean_apply_kernel(uint32_t n, uint32_t NB, const float* __restrict__ x, const float* __restrict__ part, float* __restrict__ xadj) {
    __shared__ float sh[256];
    float mean[3];
    for (int c = 0; c < 3; ++c) mean[c] = level2(part + (SLOT_MEAN + c) * RED_BLOCKS, NB, sh) / (float)n;
    const uint32_t T = (n + 255) / 256;
    for (uint32_t tile = blockIdx.x; tile < T; tile += NB) {
        const uint32_t i = tile * 256 + threadIdx.x;
        if (i < n) for (int c = 0; c < 3; ++c) xadj[3 * (size_t)i + c] = x[(size_t)c * n + i] - mean[c];
    }
}
// ---- 9. per-corner adjustments ----
__global__ void gsl_corner_kernel(GslView g, uint32_t F, const float* __restrict__ xadj, float* __restrict__ corner) {
    const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F) return;
    const uint32_t L = g.labels[f];
    for (int k = 0; k < 3; ++k) {
        const uint32_t row = L ? find_row(g, g.faces[3 * (size_t)f + k], L) : NONE;
        for (int c = 0; c < 3; ++c) corner[9 * (size_t)f + 3 * k + c] = row != NONE ? xadj[3 * (size_t)row + c] : 0.0f;
    }
}

// distinct (row, value) pairs among G.keys[0, n) as CSR: ptr[rows + 1], val ascending inside a row, row_of[entry] = row (optional)
uint32_t pairs_csr(mvs_ctx* ctx, GslDev& G, uint32_t n, uint32_t rows, DBuf<uint32_t>& ptr, DBuf<uint32_t>& val, DBuf<uint32_t>* row_of) {
    hipStream_t s = ctx->stream;
    G.cnt.ensure((size_t)rows + 1); ptr.ensure((size_t)rows + 2);
    MVS_HIP(hipMemsetAsync(G.cnt.p, 0, ((size_t)rows + 1) * sizeof(uint32_t), s));
    uint32_t total = 0;
    if (n) {
        G.keys2.ensure(n); G.flag.ensure(n); G.pos.ensure((size_t)n + 1);
        dev_sort_keys(ctx, G.keys.p, G.keys2.p, n, 0, 64);
        hipLaunchKernelGGL(gsl_unique_flag_kernel, dim3(grid(n)), dim3(256), 0, s, G.keys2.p, n, G.flag.p); MVS_LAUNCH_CHECK();
        exclusive_scan_u32(ctx, G.flag.p, G.pos.p, n, G.pos.p + n);
        total = read_u32(ctx, G.pos.p + n);
        val.ensure((size_t)total + 1);
        if (row_of) row_of->ensure((size_t)total + 1);
        hipLaunchKernelGGL(gsl_unique_compact_kernel, dim3(grid(n)), dim3(256), 0, s, G.keys2.p, G.flag.p, G.pos.p, n, val.p,
                           row_of ? row_of->p : (uint32_t*)nullptr, G.cnt.p);
        MVS_LAUNCH_CHECK();
    } else {
        val.ensure(1);
        if (row_of) row_of->ensure(1);
    }
    exclusive_scan_u32(ctx, G.cnt.p, ptr.p, rows, ptr.p + rows);
    return total;
}

// the whole stage on the context's stream; host copies of nothing -- the caller reads what it needs
void run_gsl(mvs_ctx* ctx, GslDev& G, const uint32_t* d_adj_ptr, const uint32_t* d_adj, const uint32_t* d_labels, const mvs_gsl_params& P,
             mvs_gsl_stats& S) {
    hipStream_t s = ctx->stream;
    const uint32_t F = ctx->n_faces, NV = ctx->n_verts;
    G.valid = false;
    const uint32_t tone = tone_mode(P.tone_mapping, "global_seam_leveling");
    StageTimer<6> tm(s);   // marks: begin, rows, patches, system, solve, output
    tm.mark();
    G.flags.ensure(F_N); G.c64.ensure(C_N);
    MVS_HIP(hipMemsetAsync(G.flags.p, 0, F_N * sizeof(uint32_t), s));
    MVS_HIP(hipMemsetAsync(G.c64.p, 0, C_N * sizeof(unsigned long long), s));
    // 1.-2. inputs checked; vertex -> faces, vertex rows, rings
    patch_check_inputs(ctx, G.pt, d_labels, "global_seam_leveling");
    if ((uint64_t)F * 6 >= 0xFFFFFFFFull) throw StatusError(MVS_ERR_INVALID, "global_seam_leveling: too many faces");
    G.keys.ensure(6 * (size_t)F + 1);
    hipLaunchKernelGGL(gsl_key_kernel, dim3(grid(F)), dim3(256), 0, s, ctx->d_faces, d_labels, F, 0, G.keys.p); MVS_LAUNCH_CHECK();
    pairs_csr(ctx, G, 3 * F, NV, G.vf_ptr, G.vf, nullptr);
    hipLaunchKernelGGL(gsl_key_kernel, dim3(grid(F)), dim3(256), 0, s, ctx->d_faces, d_labels, F, 1, G.keys.p); MVS_LAUNCH_CHECK();
    const uint32_t XR = pairs_csr(ctx, G, 3 * F, NV, G.x_ptr, G.x_label, &G.x_vert);
    hipLaunchKernelGGL(gsl_key_kernel, dim3(grid(F)), dim3(256), 0, s, ctx->d_faces, d_labels, F, 2, G.keys.p); MVS_LAUNCH_CHECK();
    pairs_csr(ctx, G, 6 * F, NV, G.ring_ptr, G.ring, nullptr);
    tm.mark();
    // 3. candidates (components of every label), boxes, merges, patch ids
    PatchTables& T = G.pt;
    build_patch_tables(ctx, T, d_adj_ptr, d_adj, d_labels, "global_seam_leveling");
    const uint32_t n_patches = T.n_patches;
    tm.mark();
    // 4.-7. A rows, b, Lhs, Rhs
    const GslView gv{ctx->d_verts, ctx->d_faces, d_labels, G.vf_ptr.p, G.vf.p, G.x_ptr.p, G.x_label.p, G.ring_ptr.p, G.ring.p,
                     T.box.p, T.pc.p, T.fcand.p, T.parent.p, T.fpid.p, T.fpos.p, T.views.p, tone == TONE_GAMMA ? tone_table_dev(ctx) : nullptr};
    G.cnt.ensure((size_t)std::max(NV, XR) + 1); G.a_ptr.ensure((size_t)NV + 2);
    hipLaunchKernelGGL(gsl_a_rows_kernel, dim3(grid(NV)), dim3(256), 0, s, gv, NV, 0, G.cnt.p, (const uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr);
    MVS_LAUNCH_CHECK();
    exclusive_scan_u32(ctx, G.cnt.p, G.a_ptr.p, NV, G.a_ptr.p + NV);
    const uint32_t AR = read_u32(ctx, G.a_ptr.p + NV);
    G.a_col.ensure(2 * (size_t)AR + 2); G.a_vert.ensure((size_t)AR + 1); G.b.ensure(3 * (size_t)AR + 3);
    hipLaunchKernelGGL(gsl_a_rows_kernel, dim3(grid(NV)), dim3(256), 0, s, gv, NV, 1, (uint32_t*)nullptr, (const uint32_t*)G.a_ptr.p, G.a_col.p, G.a_vert.p);
    MVS_LAUNCH_CHECK();
    if (tone == TONE_GAMMA) hipLaunchKernelGGL(gsl_b_kernel<TONE_GAMMA>, dim3(grid(AR)), dim3(256), 0, s, gv, AR, G.a_col.p, G.a_vert.p, G.b.p, G.c64.p);
    else hipLaunchKernelGGL(gsl_b_kernel<TONE_NONE>, dim3(grid(AR)), dim3(256), 0, s, gv, AR, G.a_col.p, G.a_vert.p, G.b.p, G.c64.p);
    MVS_LAUNCH_CHECK();
    G.lhs_ptr.ensure((size_t)XR + 2);
    hipLaunchKernelGGL(gsl_lhs_count_kernel, dim3(grid(XR)), dim3(256), 0, s, gv, XR, G.x_vert.p, G.a_ptr.p, G.a_col.p, G.cnt.p, G.c64.p); MVS_LAUNCH_CHECK();
    exclusive_scan_u32(ctx, G.cnt.p, G.lhs_ptr.p, XR, G.lhs_ptr.p + XR);
    const uint32_t NNZ = read_u32(ctx, G.lhs_ptr.p + XR);
    G.lhs_col.ensure((size_t)NNZ + 1); G.lhs_val.ensure((size_t)NNZ + 1); G.invdiag.ensure((size_t)XR + 1); G.rhs.ensure(3 * (size_t)XR + 3);
    const float gam = P.lambda * P.lambda;
    hipLaunchKernelGGL(gsl_lhs_fill_kernel, dim3(grid(XR)), dim3(256), 0, s, gv, XR, G.x_vert.p, G.a_ptr.p, G.a_col.p, G.b.p, G.lhs_ptr.p, gam,
                       G.lhs_col.p, G.lhs_val.p, G.invdiag.p, G.rhs.p);
    MVS_LAUNCH_CHECK();
    tm.mark();
    // 8. the solve
    G.x.ensure(3 * (size_t)XR + 3); G.r.ensure(3 * (size_t)XR + 3); G.p.ensure(6 * (size_t)XR + 6); G.ap.ensure(3 * (size_t)XR + 3);
    G.xadj.ensure(3 * (size_t)XR + 3); G.part.ensure((size_t)SLOTS * RED_BLOCKS); G.st.ensure(3);
    GslState fin{};
    if (XR) {
        const uint32_t NB = std::min<uint32_t>(RED_BLOCKS, (XR + 255) / 256);
        const float tol2 = P.tolerance * P.tolerance;
        hipLaunchKernelGGL(gsl_cg_init_kernel, dim3(NB), dim3(256), 0, s, XR, NB, G.rhs.p, G.invdiag.p, G.x.p, G.r.p, G.part.p, G.st.p, G.flags.p);
        MVS_LAUNCH_CHECK();
        if (!G.cap) MVS_HIP(hipStreamCreateWithFlags(&G.cap, hipStreamNonBlocking));
        hipGraph_t graph = nullptr; hipGraphExec_t exec = nullptr;
        MVS_HIP(hipStreamBeginCapture(G.cap, hipStreamCaptureModeThreadLocal));
        for (int it = 0; it < GSL_GRAPH_ITERS; ++it) {
            const uint32_t q = (uint32_t)(it & 1);
            hipLaunchKernelGGL(gsl_cg_spmv_kernel, dim3(NB), dim3(256), 0, G.cap, q, XR, NB, G.lhs_ptr.p, G.lhs_col.p, G.lhs_val.p, G.invdiag.p, G.r.p,
                               G.p.p, G.ap.p, G.part.p, G.st.p, G.flags.p, tol2, P.max_iterations);
            hipLaunchKernelGGL(gsl_cg_update_kernel, dim3(NB), dim3(256), 0, G.cap, q, XR, NB, G.invdiag.p, G.x.p, G.r.p, G.p.p, G.ap.p, G.part.p,
                               G.st.p, G.flags.p);
        }
        const hipError_t ce = hipStreamEndCapture(G.cap, &graph);
        if (ce != hipSuccess || !graph) { (void)hipGetLastError(); throw HipError("global_seam_leveling: capture of the CG loop failed"); }
        const hipError_t ie = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
        (void)hipGraphDestroy(graph);
        if (ie != hipSuccess) { (void)hipGetLastError(); throw HipError("global_seam_leveling: instantiation of the CG loop failed"); }
        struct ExecGuard { hipGraphExec_t e; ~ExecGuard() { (void)hipGraphExecDestroy(e); } } eg{exec};
        // every replay runs GSL_GRAPH_ITERS iterations or returns at once; a channel stops by iteration max_iterations + 1 at the latest
        const uint64_t max_replays = ((uint64_t)P.max_iterations + 1 + GSL_GRAPH_ITERS - 1) / GSL_GRAPH_ITERS + 1;
        uint32_t done = 0;
        for (uint64_t k = 0; k < max_replays && !done; ++k) {
            MVS_HIP(hipGraphLaunch(exec, s));
            read_words(ctx, G.flags.p + F_DONE, &done, 1);
        }
        if (!done) throw HipError("global_seam_leveling: the CG loop did not stop");
        MVS_HIP(hipMemcpyAsync(&fin, G.st.p + 2, sizeof(GslState), hipMemcpyDeviceToHost, s));
        tm.mark();
        hipLaunchKernelGGL(gsl_mean_part_kernel, dim3(NB), dim3(256), 0, s, XR, NB, G.x.p, G.part.p); MVS_LAUNCH_CHECK();
        hipLaunchKernelGGL(gsl_mean_apply_kernel, dim3(NB), dim3(256), 0, s, XR, NB, G.x.p, G.part.p, G.xadj.p); MVS_LAUNCH_CHECK();
    } else {
        tm.mark();
    }
    // 9.
    G.corner.ensure(9 * (size_t)F + 9);
    hipLaunchKernelGGL(gsl_corner_kernel, dim3(grid(F)), dim3(256), 0, s, gv, F, G.xadj.p, G.corner.p); MVS_LAUNCH_CHECK();
    tm.mark();
    unsigned long long c64[C_N];
    MVS_HIP(hipMemcpyAsync(c64, G.c64.p, sizeof(c64), hipMemcpyDeviceToHost, s));
    MVS_HIP(hipStreamSynchronize(s));
    S = mvs_gsl_stats{};
    S.patches = n_patches; S.merged = T.n_merged; S.x_rows = XR; S.a_rows = AR; S.gamma_rows = c64[C_GAMMA2] / 2;
    S.lhs_nnz_lower = c64[C_LOWER]; S.seam_edges = c64[C_SEAM]; S.samples = c64[C_SAMPLES];
    for (int c = 0; c < 3; ++c) { S.iterations[c] = XR ? fin.ch[c].iters : 0u; S.error[c] = XR ? fin.ch[c].err : 0.0f; }
    S.ms_rows = tm.ms(0, 1); S.ms_patches = tm.ms(1, 2); S.ms_system = tm.ms(2, 3); S.ms_solve = tm.ms(3, 4); S.ms_output = tm.ms(4, 5);
    S.ms_total = tm.ms(0, 5);
    G.NV = NV; G.F = F; G.XR = XR; G.AR = AR; G.NNZ = NNZ; G.valid = true;
}

}  // namespace
}  // namespace mvs

using namespace mvs;

extern "C" {

void mvs_gsl_default_params(mvs_gsl_params* p) {
    if (!p) return;
    p->tolerance = 1e-4f; p->max_iterations = 1000; p->lambda = 0.1f; p->tone_mapping = MVS_TONE_NONE;
}

mvs_status mvs_ctx_global_seam_leveling(mvs_ctx* ctx, const uint32_t* adj_ptr, const uint32_t* adj, int adj_on_device, const uint32_t* labels,
                                        int labels_on_device, const mvs_gsl_params* params, mvs_gsl_result* out, int out_on_device,
                                        mvs_gsl_stats* stats) {
    if (!ctx || !out) return api_fail(MVS_ERR_INVALID, "null argument");
    if (!ctx->d_verts || !ctx->d_faces || ctx->n_views == 0 || ctx->h_views.size() < ctx->n_views)
        return api_fail(MVS_ERR_STATE, "global seam leveling needs the mesh and the views (mvs_scene_set_mesh, mvs_scene_set_views)");
    const uint32_t F = ctx->n_faces, NV = ctx->n_verts;
    if (F && (!adj_ptr || !adj || !labels)) return api_fail(MVS_ERR_INVALID, "null argument");
    *out = mvs_gsl_result{};
    return api_guard([&] {
        MVS_HIP(hipSetDevice(ctx->device));
        hipStream_t s = ctx->stream;
        GslDev& G = row_dev(ctx->gsl);
        mvs_gsl_params P;
        if (params) P = *params; else mvs_gsl_default_params(&P);
        const RowGraph g = stage_graph(ctx, adj_ptr, adj, adj_on_device, labels, labels_on_device);
        if (F && (!adj_on_device || !labels_on_device)) MVS_HIP(hipStreamSynchronize(s));   // host buffers are borrowed for the call only
        mvs_gsl_stats S{};
        run_gsl(ctx, G, g.adj_ptr, g.adj, g.labels, P, S);
        if (stats) *stats = S;
        out->n_verts = NV; out->n_faces = F; out->x_rows = G.XR;
        if (out_on_device) {
            out->x_ptr = G.x_ptr.p; out->x_label = G.x_label.p; out->x_adjust = G.xadj.p; out->corner_adjust = G.corner.p;
        } else {
            download(s, out, mvs_gsl_result_free, [&] {
                out->x_ptr = host_copy(G.x_ptr.p, (size_t)NV + 1, s); out->x_label = host_copy(G.x_label.p, G.XR, s);
                out->x_adjust = host_copy(G.xadj.p, 3 * (size_t)G.XR, s); out->corner_adjust = host_copy(G.corner.p, 9 * (size_t)F, s);
            });
        }
    });
}

void mvs_gsl_result_free(mvs_gsl_result* r) {
    if (!r) return;
    free(r->x_ptr); free(r->x_label); free(r->x_adjust); free(r->corner_adjust);
    r->x_ptr = r->x_label = nullptr; r->x_adjust = r->corner_adjust = nullptr;
}

mvs_status mvs_ctx_gsl_system(mvs_ctx* ctx, mvs_gsl_system* out) {
    if (!ctx || !out) return api_fail(MVS_ERR_INVALID, "null argument");
    if (!ctx->gsl || !ctx->gsl->valid) return api_fail(MVS_ERR_STATE, "no global seam leveling on this context");
    *out = mvs_gsl_system{};
    return api_guard([&] {
        MVS_HIP(hipSetDevice(ctx->device));
        hipStream_t s = ctx->stream;
        GslDev& G = *ctx->gsl;
        const uint32_t XR = G.XR, AR = G.AR;
        std::vector<uint32_t> ptr((size_t)XR + 1), col(G.NNZ + 1); std::vector<float> val(G.NNZ + 1), rhs(3 * (size_t)XR + 1), x(3 * (size_t)XR + 1);
        MVS_HIP(hipMemcpyAsync(ptr.data(), G.lhs_ptr.p, ((size_t)XR + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        if (G.NNZ) {
            MVS_HIP(hipMemcpyAsync(col.data(), G.lhs_col.p, G.NNZ * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
            MVS_HIP(hipMemcpyAsync(val.data(), G.lhs_val.p, G.NNZ * sizeof(float), hipMemcpyDeviceToHost, s));
        }
        if (XR) {
            MVS_HIP(hipMemcpyAsync(rhs.data(), G.rhs.p, 3 * (size_t)XR * sizeof(float), hipMemcpyDeviceToHost, s));
            MVS_HIP(hipMemcpyAsync(x.data(), G.x.p, 3 * (size_t)XR * sizeof(float), hipMemcpyDeviceToHost, s));
        }
        out->x_rows = XR; out->a_rows = AR;
        try {
            out->a_col = host_copy(G.a_col.p, 2 * (size_t)AR, s); out->b = host_copy(G.b.p, 3 * (size_t)AR, s);
            MVS_HIP(hipStreamSynchronize(s));
            uint64_t nl = 0;
            for (uint32_t i = 0; i < XR; ++i) for (uint32_t e = ptr[i]; e < ptr[i + 1]; ++e) nl += col[e] <= i;
            out->lhs_nnz = nl;
            out->lhs_ptr = (uint32_t*)malloc(((size_t)XR + 1) * sizeof(uint32_t)); out->lhs_col = (uint32_t*)malloc((nl + 1) * sizeof(uint32_t));
            out->lhs_val = (float*)malloc((nl + 1) * sizeof(float));
            out->rhs = (float*)malloc((3 * (size_t)XR + 1) * sizeof(float)); out->x_raw = (float*)malloc((3 * (size_t)XR + 1) * sizeof(float));
            if (!out->lhs_ptr || !out->lhs_col || !out->lhs_val || !out->rhs || !out->x_raw) throw StatusError(MVS_ERR_INVALID, "out of host memory");
            uint64_t o = 0;
            out->lhs_ptr[0] = 0;
            for (uint32_t i = 0; i < XR; ++i) {
                for (uint32_t e = ptr[i]; e < ptr[i + 1]; ++e) if (col[e] <= i) { out->lhs_col[o] = col[e]; out->lhs_val[o] = val[e]; ++o; }
                out->lhs_ptr[i + 1] = (uint32_t)o;
            }
            for (uint32_t i = 0; i < XR; ++i) for (int c = 0; c < 3; ++c) { out->rhs[3 * (size_t)i + c] = rhs[(size_t)c * XR + i]; out->x_raw[3 * (size_t)i + c] = x[(size_t)c * XR + i]; }
        } catch (...) { (void)hipStreamSynchronize(s); mvs_gsl_system_free(out); throw; }
    });
}

void mvs_gsl_system_free(mvs_gsl_system* s) {
    if (!s) return;
    free(s->lhs_ptr); free(s->lhs_col); free(s->lhs_val); free(s->rhs); free(s->a_col); free(s->b); free(s->x_raw);
    s->lhs_ptr = s->lhs_col = s->a_col = nullptr; s->lhs_val = s->rhs = s->b = s->x_raw = nullptr;
}

}  // extern "C"
