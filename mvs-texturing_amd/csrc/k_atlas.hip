// k_atlas.hip -- row f8: tex::generate_texture_atlases (generate_texture_atlases.cpp:35-166, texture_atlas.cpp:19-253,
//   rectangular_bin.cpp:19-70), tone mapping `none` or `gamma` (compose is instantiated on the mode, tone.h).  The definition (DESIGN.md section 4 "Texture atlases") is shared with the CPU
//   model of the tests (tests/tools/atlas_model.cpp): every output is bit-identical to it.  Phases (all but the first on the context's stream):
//   pack      on the host, inside the call: upstream's loops over vectors (a one-workgroup device packer was built and measured slower than
//             one host thread at config 3: profiles/EXPERIMENTS.md "Row f8: the packer", profiles/atlas_c3_device_packer.json, the kernel in
//             profiles/atlas_device_packer.patch); ms_pack is host time: ordering, packing, per-patch tables and their uploads;
//   compose   one thread per patch pixel: float_to_byte_image (DEFINED HERE, item 5) and the scatter of image and mask;
//   pad       apply_edge_padding as levels: sweep n fills every pixel that has a neighbour of level n from its neighbours of level
//             <= n; one launch per sweep over all atlases that still pad (reads: levels <= n, writes: unset pixels -- no race);
//   texcoords one thread per list entry writes faces and coordinates; two stable radix sorts ((atlas, x) over y) group equal
//             coordinates with their first occurrence in front; heads ranked by first index give upstream's ids.
#include "rows.h"
#include "tone.h"
#include <algorithm>
#include <cmath>
#include <numeric>

namespace mvs {

// per-context buffers of row f8, allocated on first use, freed with the context (atlas_release)
struct AtlasDev {
    // staged inputs (host callers)
    DBuf<uint32_t> in_faces; DBuf<float> in_texcoords, in_image; DBuf<uint8_t> in_validity;
    // per-patch / per-atlas tables
    DBuf<int2> wh; DBuf<int4> place; DBuf<unsigned long long> ppix, abase; DBuf<uint32_t> chunk_ptr, chunk_patch, asize, ord_patch, ord_ptr, in_face_ptr, corner_start;
    // pixels
    DBuf<uint8_t> mask, lev; DBuf<unsigned long long> c64;
    // texcoords
    DBuf<uint32_t> entry_atlas, ykey, ykey2, idx, idx2, flag, headpos, first, rank; DBuf<unsigned long long> xkey, xkey2;
    // outputs
    DBuf<uint8_t> image; DBuf<uint32_t> o_atlas_size, o_patch_atlas, o_patch_order, o_face_ptr, faces, o_tc_ptr, ids; DBuf<int32_t> o_patch_pos;
    DBuf<unsigned long long> o_pix_ptr; DBuf<float> texcoords, merged;
};
void atlas_release(mvs_ctx* ctx) { delete ctx->atlas; ctx->atlas = nullptr; }

namespace {
constexpr uint32_t MAX_SIZE = 8192, PREF_SIZE = 4096, MIN_SIZE = 256;
constexpr uint32_t CHUNK = 1024;          // pixels of one patch a compose block handles
enum { K_VALID = 0, K_PADDED, K_BAD_TC, K_N };           // 64-bit counters

// ---- pack (on the host: profiles/EXPERIMENTS.md "Row f8: the packer") ----
struct HostPack { std::vector<uint32_t> atlas, seq, size; std::vector<int2> pos; uint32_t peak = 0; };

// item 2: calculate_texture_size on the remaining list (sorted positions)
uint32_t texture_size(const std::vector<int2>& wh, const std::vector<uint32_t>& rem) {
    uint32_t size = MAX_SIZE;
    while (true) {
        uint32_t total_area = 0u, max_width = 0u, max_height = 0u;
        const uint32_t pad = size >> 7;
        for (uint32_t id : rem) {
            const int2 p = wh[id];
            const uint32_t width = (uint32_t)p.x + 2u * pad, height = (uint32_t)p.y + 2u * pad, psize = (uint32_t)(p.x * p.y);
            max_width = std::max(max_width, width); max_height = std::max(max_height, height);
            const uint32_t area = width * height, waste = area - psize;
            if (static_cast<double>(waste) / (double)psize > 1.0) break;
            total_area += area;                                              // 32-bit, wrap included
        }
        if (size > PREF_SIZE && max_width < PREF_SIZE && max_height < PREF_SIZE && total_area / (PREF_SIZE * PREF_SIZE) < 8u) { size = PREF_SIZE; continue; }
        if (size <= MIN_SIZE) return MIN_SIZE;
        if (max_height < size / 2u && max_width < size / 2u && static_cast<double>(total_area) / (double)(size * size) < 0.2) { size = size / 2u; continue; }
        return size;
    }
}

// items 3 and 4: wh[k] = patch k of the sorted list; H.atlas / pos / seq are indexed by k
void pack_host(const std::vector<int2>& wh, HostPack& H) {
    const uint32_t N = (uint32_t)wh.size();
    H.atlas.assign(N, 0u); H.seq.assign(N, 0u); H.pos.assign(N, make_int2(0, 0)); H.size.clear(); H.peak = 0u;
    std::vector<uint32_t> rem(N), next;
    std::iota(rem.begin(), rem.end(), 0u);
    std::vector<int4> fr;
    uint32_t seq = 0u;
    auto area = [](const int4& q) { return (q.z - q.x) * (q.w - q.y); };
    while (!rem.empty()) {
        const uint32_t size = texture_size(wh, rem), A = (uint32_t)H.size.size();
        const int pad = (int)(size >> 7);
        H.size.push_back(size);
        fr.assign(1, make_int4(0, 0, (int)size, (int)size));
        H.peak = std::max(H.peak, 1u);
        next.clear();
        for (uint32_t id : rem) {
            const int W = wh[id].x + 2 * pad, Hh = wh[id].y + 2 * pad;
            uint32_t best = size * size; size_t best_r = fr.size();
            for (size_t r = 0; r < fr.size(); ++r) {
                const int4& f = fr[r];
                if (W <= f.z - f.x && Hh <= f.w - f.y) {
                    const uint32_t score = (uint32_t)(area(f) - W * Hh);
                    if (score < best) { best = score; best_r = r; }           // strict: the first minimum in list order
                }
            }
            if (best_r == fr.size()) { next.push_back(id); continue; }
            const int4 b = fr[best_r];
            fr.erase(fr.begin() + (ptrdiff_t)best_r);
            const int x1 = b.x + W, y1 = b.y + Hh;
            const int4 h_top = make_int4(b.x, y1, b.z, b.w), h_bottom = make_int4(x1, b.y, b.z, y1);
            const int4 v_left = make_int4(b.x, y1, x1, b.w), v_right = make_int4(x1, b.y, b.z, b.w);
            float hr = 1.0f, vr = 1.0f;
            if (area(h_top) != 0 && area(h_bottom) != 0) hr = static_cast<float>(area(h_top)) / static_cast<float>(area(h_bottom));
            if (area(v_left) != 0 && area(v_right) != 0) vr = static_cast<float>(area(v_left)) / static_cast<float>(area(v_right));
            const bool vertical = std::abs(1.0f - hr) < std::abs(1.0f - vr);
            const int4 q0 = vertical ? v_left : h_top, q1 = vertical ? v_right : h_bottom;
            if (area(q0) != 0) fr.push_back(q0);
            if (area(q1) != 0) fr.push_back(q1);
            H.peak = std::max(H.peak, (uint32_t)fr.size());
            H.atlas[id] = A; H.pos[id] = make_int2(b.x, b.y); H.seq[id] = seq++;
        }
        if (next.size() == rem.size()) throw StatusError(MVS_ERR_HIP, "texture_atlases: an atlas took no patch (internal error)");   // the invariant of item 2
        rem.swap(next);
    }
}

// ---- compose ----
// place[p] = (x0, y0, atlas size, atlas): where patch pixel (0, 0) lands; abase[atlas]: first pixel of the atlas; ppix: the set's pix_ptr
struct Placement { const int4* place; const unsigned long long* abase; const unsigned long long* ppix; const int2* wh; };

__device__ inline uint8_t float_to_byte(float x) {   // DEFINED HERE: mve::image::float_to_byte_image(img, 0.0f, 1.0f) on one value
    float v = (0.0f < x) ? x : 0.0f;                  // std::max(0.0f, x): a NaN becomes 0
    v = (v < 1.0f) ? v : 1.0f;                        // std::min(1.0f, v)
    v = (255.0f * (v - 0.0f)) / (1.0f - 0.0f);
    return (uint8_t)(v + 0.5f);
}

template <int TONE>   // TONE_GAMMA: gamma_correct(image, 1.0f / 2.2f) of generate_texture_atlases.cpp:102-104 in front of the quantisation
__global__ void __launch_bounds__(256) at_compose_kernel(Placement T, const uint32_t* __restrict__ chunk_ptr, const uint32_t* __restrict__ chunk_patch,
                                                         const float* __restrict__ image, const uint8_t* __restrict__ validity, uint8_t* __restrict__ out,
                                                         uint8_t* __restrict__ mask, uint8_t* __restrict__ lev, unsigned long long* __restrict__ c64) {
    const uint32_t p = chunk_patch[blockIdx.x];
    const uint32_t first = (blockIdx.x - chunk_ptr[p]) * CHUNK;
    const int4 pl = T.place[p];
    const int2 wh = T.wh[p];
    const unsigned long long src0 = T.ppix[p], dst0 = T.abase[pl.w];
    const uint32_t npix = (uint32_t)wh.x * (uint32_t)wh.y;
    uint32_t valid = 0;
    for (uint32_t i = first + threadIdx.x; i < min(first + CHUNK, npix); i += 256) {
        const uint32_t sy = i / (uint32_t)wh.x, sx = i - sy * (uint32_t)wh.x;
        const unsigned long long s = src0 + i;
        const unsigned long long d = dst0 + (unsigned long long)(pl.y + (int)sy) * (unsigned long long)pl.z + (unsigned long long)(pl.x + (int)sx);
        for (int c = 0; c < 3; ++c) {
            if (TONE == TONE_GAMMA) out[3ull * d + c] = float_to_byte(gamma_pow(image[3ull * s + c], TONE_INV_POWER));
            else out[3ull * d + c] = float_to_byte(image[3ull * s + c]);
        }
        const uint8_t v = validity[s];
        mask[d] = v;
        if (v == 255) { lev[d] = 0; ++valid; }
    }
    if (valid) atomicAdd(c64 + K_VALID, (unsigned long long)valid);
}

// ---- pad ----
// sweep n (item 7): an unset pixel (validity != 255 in sweep 0, == 0 later) with a neighbour of level n becomes level n + 1, its colour the
// weighted mean over its neighbours of level <= n, j outer, i inner
__global__ void __launch_bounds__(256) at_pad_kernel(const unsigned long long* __restrict__ abase, const uint32_t* __restrict__ asize, uint32_t A, uint32_t n,
                                                     const uint8_t* __restrict__ mask, uint8_t* lev, uint8_t* image, unsigned long long* __restrict__ c64) {
    const unsigned long long g0 = (unsigned long long)blockIdx.x * 256ull;   // atlases are multiples of 256 pixels: a block lies in one
    uint32_t lo = 0, hi = A;
    while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (abase[mid] <= g0) lo = mid; else hi = mid; }
    const int size = (int)asize[lo];
    if (n > (uint32_t)(size >> 7)) return;
    const unsigned long long base = abase[lo];
    const unsigned long long l = g0 - base + threadIdx.x;
    const int y = (int)(l / (unsigned long long)size), x = (int)(l - (unsigned long long)y * (unsigned long long)size);
    const unsigned long long g = base + l;
    bool fill = false;
    uint8_t nb[9];
    if (lev[g] == 255 && (n == 0 ? mask[g] != 255 : mask[g] == 0)) {
        for (int j = -1; j <= 1; ++j) for (int i = -1; i <= 1; ++i) {
            const int nx = x + i, ny = y + j;
            uint8_t v = 255;
            if (0 <= nx && nx < size && 0 <= ny && ny < size) v = lev[base + (unsigned long long)ny * (unsigned long long)size + (unsigned long long)nx];
            nb[(j + 1) * 3 + (i + 1)] = v;
            fill = fill || v == (uint8_t)n;
        }
    }
    if (fill) {
        for (int c = 0; c < 3; ++c) {
            float norm = 0.0f, value = 0.0f;
            for (int j = -1; j <= 1; ++j) for (int i = -1; i <= 1; ++i) {
                if (nb[(j + 1) * 3 + (i + 1)] <= (uint8_t)n) {
                    const float w = (float)((2 - abs(i)) * (2 - abs(j))) / 16.0f;
                    const unsigned long long q = base + (unsigned long long)(y + j) * (unsigned long long)size + (unsigned long long)(x + i);
                    norm += w;
                    value += ((float)image[3ull * q + c] / 255.0f) * w;
                }
            }
            image[3ull * g + c] = (uint8_t)((value / norm) * 255.0f);
        }
        lev[g] = (uint8_t)(n + 1u);
    }
    const unsigned long long bal = __ballot(fill);
    if (bal && (threadIdx.x & 63u) == (uint32_t)(__ffsll((long long)bal) - 1)) atomicAdd(c64 + K_PADDED, (unsigned long long)__popcll(bal));
}

// ---- texcoords ----
__device__ inline uint32_t tc_key(float v) {   // equal keys <=> equal floats (finite): -0.0f and 0.0f collide
    uint32_t u = __float_as_uint(v);
    if (u == 0x80000000u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
// one thread per output list entry e: ord_ptr [P + 1] = first output entry of the k-th inserted patch (ord_patch[k])
__global__ void at_texcoord_kernel(uint32_t L, uint32_t P, const uint32_t* __restrict__ ord_ptr, const uint32_t* __restrict__ ord_patch,
                                   const uint32_t* __restrict__ in_face_ptr, const uint32_t* __restrict__ in_faces, const float* __restrict__ in_tc,
                                   const int4* __restrict__ place, uint32_t* __restrict__ faces, float* __restrict__ tc, uint32_t* __restrict__ entry_atlas,
                                   uint32_t* __restrict__ ykey, uint32_t* __restrict__ idx, unsigned long long* __restrict__ c64) {
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= L) return;
    uint32_t lo = 0, hi = P;   // the last inserted patch whose entries start at or before e (patches without faces share their start with the next)
    while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (ord_ptr[mid] <= e) lo = mid; else hi = mid; }
    const uint32_t p = ord_patch[lo];
    const uint32_t src = in_face_ptr[p] + (e - ord_ptr[lo]);
    const int4 pl = place[p];
    const float ox = (float)pl.x, oy = (float)pl.y, fs = (float)pl.z;
    faces[e] = in_faces[src];
    entry_atlas[e] = (uint32_t)pl.w;
    for (int k = 0; k < 3; ++k) {
        const float tx = (in_tc[6 * (size_t)src + 2 * k] + ox) / fs, ty = (in_tc[6 * (size_t)src + 2 * k + 1] + oy) / fs;
        if (!(fabsf(tx) <= 3.4028234e38f) || !(fabsf(ty) <= 3.4028234e38f)) c64[K_BAD_TC] = 1ull;      // not finite: the call refuses (merge_texcoords has no order for a NaN)
        tc[6 * (size_t)e + 2 * k] = tx; tc[6 * (size_t)e + 2 * k + 1] = ty;
        ykey[3 * (size_t)e + k] = tc_key(ty); idx[3 * (size_t)e + k] = 3u * e + (uint32_t)k;
    }
}
__global__ void at_xkey_kernel(uint32_t NC, const uint32_t* __restrict__ idx, const float* __restrict__ tc, const uint32_t* __restrict__ entry_atlas,
                               unsigned long long* __restrict__ xkey) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= NC) return;
    const uint32_t j = idx[i];
    xkey[i] = ((unsigned long long)entry_atlas[j / 3u] << 32) | (unsigned long long)tc_key(tc[2 * (size_t)j]);
}
// sorted position i: headpos = i where a group of equal (atlas, x, y) starts, else 0; first[corner] = 1 for the corner in front of its group
__global__ void at_head_kernel(uint32_t NC, const uint32_t* __restrict__ idx, const unsigned long long* __restrict__ xkey, const float* __restrict__ tc,
                               uint32_t* __restrict__ headpos, uint32_t* __restrict__ first) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i > NC) return;
    if (i == NC) { first[NC] = 0u; return; }
    const uint32_t j = idx[i];
    bool head = i == 0;
    if (!head) head = xkey[i] != xkey[i - 1] || tc_key(tc[2 * (size_t)j + 1]) != tc_key(tc[2 * (size_t)idx[i - 1] + 1]);
    headpos[i] = head ? i : 0u;
    first[j] = head ? 1u : 0u;
}
__global__ void at_ids_kernel(uint32_t NC, const uint32_t* __restrict__ idx, const uint32_t* __restrict__ headpos, const uint32_t* __restrict__ rank,
                              const uint32_t* __restrict__ first, const uint32_t* __restrict__ entry_atlas, const uint32_t* __restrict__ corner_start,
                              const float* __restrict__ tc, uint32_t* __restrict__ ids, float* __restrict__ merged) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= NC) return;
    const uint32_t j = idx[i], h = idx[headpos[i]];
    ids[j] = rank[h] - rank[corner_start[entry_atlas[j / 3u]]];
    if (first[j]) { merged[2 * (size_t)rank[j]] = tc[2 * (size_t)j]; merged[2 * (size_t)rank[j] + 1] = tc[2 * (size_t)j + 1]; }
}
__global__ void at_tcptr_kernel(uint32_t A, const uint32_t* __restrict__ corner_start, const uint32_t* __restrict__ rank, uint32_t* __restrict__ tc_ptr) {
    const uint32_t a = blockIdx.x * blockDim.x + threadIdx.x;
    if (a <= A) tc_ptr[a] = rank[corner_start[a]];
}

// host arrays that asynchronous copies read or write: owned by the caller of run_atlas, which drains the stream before they go
struct HostTables {
    HostPack H;
    std::vector<int2> wh_patch; std::vector<int4> place; std::vector<uint32_t> patch_atlas, ord_patch, ord_ptr, face_ptr, corner, chunk_ptr, chunk_patch;
    std::vector<int32_t> pos; std::vector<unsigned long long> abase;
    uint32_t n_merged = 0; unsigned long long c64[K_N] = {};
};

struct Input { uint32_t NP, L; unsigned long long NPIX; const uint32_t* faces; const float* texcoords; const float* image; const uint8_t* validity; };

// hb / hp / hf: host copies of box [NP], pix_ptr and face_ptr [NP + 1] (checked by the caller, alive until the stream is drained)
void run_atlas(mvs_ctx* ctx, AtlasDev& D, const Input& in, const int4* hb, const unsigned long long* hp, const uint32_t* hf, HostTables& T,
               const mvs_atlas_params& P, mvs_atlas_stats& st, mvs_atlas_set& set) {
    hipStream_t s = ctx->stream;
    const uint32_t NP = in.NP, L = in.L;
    StageTimer<4> tm(s);   // marks: compose begins / ends, pad ends, texcoords end
    // ---- pack (host time: ordering, packing, the per-patch tables and their uploads) ----
    const double t_pack = now_ms_host();
    // item 1: popped from the back, then a stable sort by size, descending
    std::vector<uint32_t> order(NP);
    for (uint32_t k = 0; k < NP; ++k) order[k] = NP - 1u - k;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return hb[a].z * hb[a].w > hb[b].z * hb[b].w; });
    std::vector<int2> h_wh(NP);                   // sizes in packing order
    std::vector<int2>& h_wh_patch = T.wh_patch;   // sizes by patch id
    h_wh_patch.assign(NP, make_int2(0, 0));
    for (uint32_t k = 0; k < NP; ++k) { h_wh[k] = make_int2(hb[order[k]].z, hb[order[k]].w); h_wh_patch[k] = make_int2(hb[k].z, hb[k].w); }
    HostPack& H = T.H;
    pack_host(h_wh, H);
    const std::vector<uint32_t>& k_atlas = H.atlas; const std::vector<uint32_t>& k_seq = H.seq; const std::vector<uint32_t>& h_size = H.size;
    const std::vector<int2>& k_pos = H.pos;
    const uint32_t A = (uint32_t)h_size.size();
    std::vector<unsigned long long>& h_abase = T.abase;
    h_abase.assign((size_t)A + 1, 0ull);
    for (uint32_t a = 0; a < A; ++a) {
        const uint32_t z = h_size[a];
        h_abase[a + 1] = h_abase[a] + (unsigned long long)z * z;
        ++st.atlases_by_size[z == 256 ? 0 : z == 512 ? 1 : z == 1024 ? 2 : z == 2048 ? 3 : z == 4096 ? 4 : 5];
    }
    const unsigned long long NPIXA = h_abase[A];
    st.atlases = A; st.pixels = NPIXA; st.free_rects_peak = H.peak;
    st.ms_pack = (float)(now_ms_host() - t_pack);
    if (P.max_pixels && NPIXA > P.max_pixels)
        throw StatusError(MVS_ERR_UNSUPPORTED, "texture_atlases: " + std::to_string(NPIXA) + " atlas pixels exceed max_pixels = " + std::to_string(P.max_pixels));
    // the per-patch tables: placement, insertion order, output face ranges
    std::vector<int4>& h_place = T.place; std::vector<uint32_t>& h_patch_atlas = T.patch_atlas; std::vector<uint32_t>& h_ord_patch = T.ord_patch;
    std::vector<uint32_t>& h_ord_ptr = T.ord_ptr; std::vector<uint32_t>& h_face_ptr = T.face_ptr; std::vector<uint32_t>& h_corner = T.corner;
    std::vector<int32_t>& h_pos = T.pos;
    h_place.assign(NP, make_int4(0, 0, 0, 0)); h_patch_atlas.assign(NP, 0u); h_ord_patch.assign(NP, 0u); h_ord_ptr.assign((size_t)NP + 1, 0u);
    h_face_ptr.assign((size_t)A + 1, 0u); h_corner.assign((size_t)A + 1, 0u); h_pos.assign(2 * (size_t)NP, 0);
    for (uint32_t k = 0; k < NP; ++k) {
        const uint32_t p = order[k], a = k_atlas[k];
        if (a >= A || k_seq[k] >= NP) throw StatusError(MVS_ERR_HIP, "texture_atlases: the packer's output is out of range (internal error)");
        const int pad = (int)(h_size[a] >> 7);
        if (k_pos[k].x < 0 || k_pos[k].y < 0 || k_pos[k].x + hb[p].z + 2 * pad > (int)h_size[a] || k_pos[k].y + hb[p].w + 2 * pad > (int)h_size[a])
            throw StatusError(MVS_ERR_HIP, "texture_atlases: the packer placed a patch outside its atlas (internal error)");
        h_place[p] = make_int4(k_pos[k].x + pad, k_pos[k].y + pad, (int)h_size[a], (int)a);
        h_patch_atlas[p] = a; h_pos[2 * (size_t)p] = k_pos[k].x; h_pos[2 * (size_t)p + 1] = k_pos[k].y;
        h_ord_patch[k_seq[k]] = p;
    }
    for (uint32_t k = 0; k < NP; ++k) {
        const uint32_t p = h_ord_patch[k];
        h_ord_ptr[k + 1] = h_ord_ptr[k] + (hf[p + 1] - hf[p]);
        h_face_ptr[h_patch_atlas[p] + 1] = h_ord_ptr[k + 1];   // insertion order is grouped by atlas, and every atlas holds a patch
    }
    for (uint32_t a = 0; a <= A; ++a) h_corner[a] = 3u * h_face_ptr[a];
    upload(D.place, h_place, s); upload(D.abase, h_abase, s); upload(D.asize, h_size, s); upload(D.ppix, hp, (size_t)NP + 1, s);
    const uint32_t NC = upload_chunk_tables(ctx, hp, NP, CHUNK, T.chunk_ptr, T.chunk_patch, D.chunk_ptr, D.chunk_patch);
    upload(D.ord_patch, h_ord_patch, s); upload(D.ord_ptr, h_ord_ptr, s);
    upload(D.in_face_ptr, hf, (size_t)NP + 1, s); upload(D.corner_start, h_corner, s); upload(D.wh, h_wh_patch, s);
    upload(D.o_atlas_size, h_size, s); upload(D.o_pix_ptr, h_abase, s); upload(D.o_patch_atlas, h_patch_atlas, s); upload(D.o_patch_pos, h_pos, s);
    upload(D.o_patch_order, h_ord_patch, s); upload(D.o_face_ptr, h_face_ptr, s);
    st.ms_pack = (float)(now_ms_host() - t_pack);
    // ---- compose (device time from here on: clearing image, mask and levels; quantise and scatter) ----
    tm.mark();
    D.image.ensure(3 * (size_t)NPIXA + 3); D.mask.ensure((size_t)NPIXA + 1); D.lev.ensure((size_t)NPIXA + 1); D.c64.ensure(K_N);
    MVS_HIP(hipMemsetAsync(D.c64.p, 0, K_N * sizeof(unsigned long long), s));
    if (NPIXA) {
        MVS_HIP(hipMemsetAsync(D.image.p, 0, 3 * (size_t)NPIXA, s));
        MVS_HIP(hipMemsetAsync(D.mask.p, 0, (size_t)NPIXA, s));
        MVS_HIP(hipMemsetAsync(D.lev.p, 0xFF, (size_t)NPIXA, s));
    }
    if (NC) {
        Placement T{D.place.p, D.abase.p, D.ppix.p, D.wh.p};
        auto* compose = P.tone_mapping == TONE_GAMMA ? at_compose_kernel<TONE_GAMMA> : at_compose_kernel<TONE_NONE>;
        hipLaunchKernelGGL(compose, dim3(NC), dim3(256), 0, s, T, (const uint32_t*)D.chunk_ptr.p, (const uint32_t*)D.chunk_patch.p, in.image, in.validity,
                           D.image.p, D.mask.p, D.lev.p, D.c64.p);
        MVS_LAUNCH_CHECK();
    }
    tm.mark();
    // ---- pad ----
    uint32_t max_pad = 0;
    for (uint32_t a = 0; a < A; ++a) max_pad = std::max(max_pad, h_size[a] >> 7);
    if (NPIXA) {
        if (NPIXA / 256ull >= 0x7FFFFFFFull) throw StatusError(MVS_ERR_UNSUPPORTED, "texture_atlases: too many atlas pixels for one call");
        for (uint32_t n = 0; n <= max_pad; ++n) {
            hipLaunchKernelGGL(at_pad_kernel, dim3((unsigned)(NPIXA / 256ull)), dim3(256), 0, s, (const unsigned long long*)D.abase.p, (const uint32_t*)D.asize.p, A, n,
                               (const uint8_t*)D.mask.p, D.lev.p, D.image.p, D.c64.p);
            MVS_LAUNCH_CHECK();
        }
    }
    tm.mark();
    // ---- texcoords and merge_texcoords ----
    const uint32_t NCR = 3u * L;
    D.faces.ensure((size_t)L + 1); D.texcoords.ensure(6 * (size_t)L + 6); D.entry_atlas.ensure((size_t)L + 1); D.ids.ensure((size_t)NCR + 1); D.merged.ensure(2 * (size_t)NCR + 2);
    D.ykey.ensure((size_t)NCR + 1); D.ykey2.ensure((size_t)NCR + 1); D.idx.ensure((size_t)NCR + 1); D.idx2.ensure((size_t)NCR + 1); D.xkey.ensure((size_t)NCR + 1);
    D.xkey2.ensure((size_t)NCR + 1); D.headpos.ensure((size_t)NCR + 1); D.first.ensure((size_t)NCR + 2); D.rank.ensure((size_t)NCR + 2); D.o_tc_ptr.ensure((size_t)A + 2);
    uint32_t& n_merged = T.n_merged;
    n_merged = 0;
    if (L) {
        hipLaunchKernelGGL(at_texcoord_kernel, dim3(grid(L)), dim3(256), 0, s, L, NP, (const uint32_t*)D.ord_ptr.p, (const uint32_t*)D.ord_patch.p, (const uint32_t*)D.in_face_ptr.p,
                           in.faces, in.texcoords, (const int4*)D.place.p, D.faces.p, D.texcoords.p, D.entry_atlas.p, D.ykey.p, D.idx.p, D.c64.p);
        MVS_LAUNCH_CHECK();
        dev_sort_pairs(ctx, D.ykey.p, D.ykey2.p, D.idx.p, D.idx2.p, (size_t)NCR, 0, 32);
        hipLaunchKernelGGL(at_xkey_kernel, dim3(grid(NCR)), dim3(256), 0, s, NCR, (const uint32_t*)D.idx2.p, (const float*)D.texcoords.p, (const uint32_t*)D.entry_atlas.p, D.xkey.p);
        MVS_LAUNCH_CHECK();
        dev_sort_pairs(ctx, D.xkey.p, D.xkey2.p, D.idx2.p, D.idx.p, (size_t)NCR, 0, 64);
        hipLaunchKernelGGL(at_head_kernel, dim3(grid((size_t)NCR + 1)), dim3(256), 0, s, NCR, (const uint32_t*)D.idx.p, (const unsigned long long*)D.xkey2.p,
                           (const float*)D.texcoords.p, D.headpos.p, D.first.p);
        MVS_LAUNCH_CHECK();
        dev_inclusive_max_scan(ctx, D.headpos.p, D.ykey.p, (size_t)NCR);   // ykey: the head's position, per sorted position
        dev_exclusive_scan(ctx, D.first.p, D.rank.p, (size_t)NCR + 1);
        hipLaunchKernelGGL(at_ids_kernel, dim3(grid(NCR)), dim3(256), 0, s, NCR, (const uint32_t*)D.idx.p, (const uint32_t*)D.ykey.p, (const uint32_t*)D.rank.p,
                           (const uint32_t*)D.first.p, (const uint32_t*)D.entry_atlas.p, (const uint32_t*)D.corner_start.p, (const float*)D.texcoords.p, D.ids.p, D.merged.p);
        MVS_LAUNCH_CHECK();
        hipLaunchKernelGGL(at_tcptr_kernel, dim3(grid((size_t)A + 1)), dim3(256), 0, s, A, (const uint32_t*)D.corner_start.p, (const uint32_t*)D.rank.p, D.o_tc_ptr.p);
        MVS_LAUNCH_CHECK();
        MVS_HIP(hipMemcpyAsync(&n_merged, D.rank.p + NCR, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    } else {
        MVS_HIP(hipMemsetAsync(D.o_tc_ptr.p, 0, ((size_t)A + 1) * sizeof(uint32_t), s));
    }
    tm.mark();
    unsigned long long* c64 = T.c64;
    MVS_HIP(hipMemcpyAsync(c64, D.c64.p, K_N * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    MVS_HIP(hipStreamSynchronize(s));
    if (c64[K_BAD_TC]) throw StatusError(MVS_ERR_UNSUPPORTED, "texture_atlases: texture coordinates that are not finite");
    st.valid_pixels = c64[K_VALID]; st.padded_pixels = c64[K_PADDED]; st.merged_texcoords = n_merged;
    st.ms_compose = tm.ms(0, 1); st.ms_pad = tm.ms(1, 2); st.ms_texcoords = tm.ms(2, 3);
    st.ms_total = st.ms_pack + st.ms_compose + st.ms_pad + st.ms_texcoords;
    set.n_atlases = A; set.n_patches = NP; set.n_listed = L; set.n_merged = n_merged; set.n_pixels = NPIXA;
}

}  // namespace
}  // namespace mvs

using namespace mvs;

extern "C" {

void mvs_atlas_default_params(mvs_atlas_params* p) {
    if (!p) return;
    p->max_pixels = 0; p->tone_mapping = MVS_TONE_NONE; p->reserved = 0;
}

mvs_status mvs_ctx_texture_atlases(mvs_ctx* ctx, const mvs_patch_set* patches, int patches_on_device, const mvs_atlas_params* params, mvs_atlas_set* out,
                                   int out_on_device, mvs_atlas_stats* stats) {
    if (!ctx || !out || !patches) return api_fail(MVS_ERR_INVALID, "null argument");
    *out = mvs_atlas_set{};
    mvs_atlas_stats st{};
    if (stats) *stats = st;
    return api_guard([&] {
        MVS_HIP(hipSetDevice(ctx->device));
        hipStream_t s = ctx->stream;
        AtlasDev& D = row_dev(ctx->atlas);
        mvs_atlas_params P;
        if (params) P = *params; else mvs_atlas_default_params(&P);
        tone_mode(P.tone_mapping, "texture_atlases");
        const mvs_patch_set& in = *patches;
        const uint32_t NP = in.n_patches, L = in.n_listed;
        const uint64_t NPIX = in.n_pixels;
        const PatchFrames h = read_patch_set(ctx, in, patches_on_device, false, "texture_atlases");   // the per-patch frames on the host
        const int4* hb = h.box; const unsigned long long* hp = h.pix_ptr; const uint32_t* hf = h.face_ptr;
        if ((uint64_t)L * 3u >= 0xFFFFFF00ull) throw StatusError(MVS_ERR_UNSUPPORTED, "texture_atlases: too many list entries for one call");
        for (uint32_t p = 0; p < NP; ++p)
            if (hb[p].z + 128 >= (int)MAX_SIZE || hb[p].w + 128 >= (int)MAX_SIZE)
                throw StatusError(MVS_ERR_UNSUPPORTED, "texture_atlases: patch " + std::to_string(p) + " does not fit the largest atlas (upstream's assertion)");
        Input I{NP, L, NPIX, nullptr, nullptr, nullptr, nullptr};
        I.faces = stage(D.in_faces, (const uint32_t*)in.faces, L, patches_on_device, s);
        I.texcoords = stage(D.in_texcoords, (const float*)in.texcoords, 6 * (size_t)L, patches_on_device, s);
        I.image = stage(D.in_image, (const float*)in.image, 3 * (size_t)NPIX, patches_on_device, s);
        I.validity = stage(D.in_validity, (const uint8_t*)in.validity, (size_t)NPIX, patches_on_device, s);
        MVS_HIP(hipStreamSynchronize(s));   // host buffers are borrowed for the call only
        mvs_atlas_set set{};
        HostTables T;                       // outlives the drain of the stream below
        run_with_stats(s, stats, st, [&] { run_atlas(ctx, D, I, hb, hp, hf, T, P, st, set); });
        *out = set;
        const size_t A = set.n_atlases, NC = 3 * (size_t)L;
        if (out_on_device) {
            out->atlas_size = D.o_atlas_size.p; out->atlas_pix_ptr = (uint64_t*)D.o_pix_ptr.p; out->image = D.image.p; out->patch_atlas = D.o_patch_atlas.p;
            out->patch_pos = D.o_patch_pos.p; out->patch_order = D.o_patch_order.p; out->face_ptr = D.o_face_ptr.p; out->faces = D.faces.p; out->texcoords = D.texcoords.p;
            out->tc_ptr = D.o_tc_ptr.p; out->texcoords_merged = D.merged.p; out->texcoord_ids = D.ids.p;
        } else {
            download(s, out, mvs_atlas_set_free, [&] {
                out->atlas_size = host_copy(D.o_atlas_size.p, A, s); out->atlas_pix_ptr = (uint64_t*)host_copy(D.o_pix_ptr.p, A + 1, s);
                out->image = host_copy(D.image.p, 3 * (size_t)set.n_pixels, s); out->patch_atlas = host_copy(D.o_patch_atlas.p, NP, s);
                out->patch_pos = host_copy(D.o_patch_pos.p, 2 * (size_t)NP, s); out->patch_order = host_copy(D.o_patch_order.p, NP, s);
                out->face_ptr = host_copy(D.o_face_ptr.p, A + 1, s); out->faces = host_copy(D.faces.p, L, s); out->texcoords = host_copy(D.texcoords.p, 2 * NC, s);
                out->tc_ptr = host_copy(D.o_tc_ptr.p, A + 1, s); out->texcoords_merged = host_copy(D.merged.p, 2 * (size_t)set.n_merged, s);
                out->texcoord_ids = host_copy(D.ids.p, NC, s);
            });
        }
    });
}

void mvs_atlas_set_free(mvs_atlas_set* a) {
    if (!a) return;
    free(a->atlas_size); free(a->atlas_pix_ptr); free(a->image); free(a->patch_atlas); free(a->patch_pos); free(a->patch_order); free(a->face_ptr); free(a->faces);
    free(a->texcoords); free(a->tc_ptr); free(a->texcoords_merged); free(a->texcoord_ids);
    *a = mvs_atlas_set{};
}

}  // extern "C"
