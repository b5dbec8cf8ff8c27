// k_glb.hip -- row f11: the textured model as one binary glTF 2.0 file (DESIGN.md section 4 "Model output" item 8; not in upstream, defined
// here).  A glTF vertex has ONE index for position and texture coordinate, so the distinct (global coordinate g, mesh vertex v) pairs among
// the 3 n_listed corners are found, numbered in ascending (g, v) and gathered on the device.  Five phases on the context's stream:
//   keys     one thread per corner: its pair as the integer key g << vbits | v (vbits = the bits n_verts needs) behind model_corner.h's checks
//   sort     rocprim radix sort of (key, corner) over the bits that n_merged and n_verts need
//   number   head flags of the sorted keys (the non-finite values of every head's vertex are counted here), an exclusive scan of them,
//            and first[a] = the number of the first pair at or behind tc_ptr[a], read off the sorted keys by binary search
//   indices  sorted position i -> indices[corner] = number - first[atlas] (the one scattered store), every head's key into the pair list
//   gather   256 consecutive pairs per block, pair = lane: the attributes go through LDS images laid out like the file and leave as 16-byte
//            stores (the at most 3 dwords in front of and behind a block's aligned part go out singly); POSITION's bounds per atlas on the
//            order-preserving integer image of the floats: wave shuffles, LDS across the waves, then integer atomicMin / atomicMax --
//            6 per block whose pairs share an atlas, per lane in the few blocks that straddle a range's end.  No float atomics anywhere.
// The JSON chunk (O(n_atlases)) is formatted on the host; the PNGs are save_model's (k_model.hip model_for_each_image).
// params.glb_quantize 1 (item 10, KHR_mesh_quantization) keeps keys, sort and number and runs its own three passes behind them:
//   indices  as above, but every corner looks up its primitive's index width (16 bits up to 65 535 vertices) and byte offset: one 2- or
//            4-byte store, and the last corner of an odd 16-bit primitive adds the two bytes of padding
//   bounds   the pair list, one pair per lane: the six words of POSITION's bounds over the WHOLE file, folded on the device by the
//            reduction of the gather (the grid is one for the file, so that a vertex of two atlases lands on one point)
//   gather   256 pairs per block again: the attributes are quantised in fp64 (+ - * / sqrt, conversions: the same bits as the
//            restatement's) into LDS images of 8 / 4 / 4 bytes per vertex -- POSITION by one 8-byte LDS store per lane, which is free of
//            bank conflicts where two 4-byte stores at a stride of 8 bytes are not -- and leave through store_block_range; the bounds per
//            atlas are those of the stored integers; texture coordinates outside [0, 1] and normals of length 0 are counted
#include "rows.h"
#include "png_io.h"
#include "model_corner.h"

namespace mvs {

struct GlbDev {
    DBuf<uint32_t> in_faces, in_face_ptr, in_tc_ptr, in_ids; DBuf<float> in_merged, in_normals;   // staged inputs (host callers)
    DBuf<unsigned long long> key, key_sorted, pair, c64;
    DBuf<uint32_t> corner, corner_sorted, head, rank, first, lo, hi;
    DBuf<uint32_t> idx_off, file_bounds;   // glb_quantize 1: every atlas's byte offset in the index part; lo [3] | hi [3] over the whole file
    DBuf<uint4> geo;   // POSITION | TEXCOORD_0 | NORMAL | indices, as in the file
    mvs_glb_quant_stats quant_stats{};   // of the last call (mvs_ctx_glb_quant_stats)
};
void glb_release(mvs_ctx* ctx) { delete ctx->glb; ctx->glb = nullptr; }

namespace {
typedef unsigned long long u64;
enum { K_BAD_FACE = 0, K_BAD_ID, K_BAD_VERT, K_NONFINITE, K_TC_RANGE, K_ZERO_NORMAL, K_N };   // 64-bit counters

// the order-preserving integer image of a float's bits: -nan < -inf < ... < -0 < +0 < ... < +inf < +nan as unsigned integers
__host__ __device__ inline uint32_t order_image(uint32_t bits) { return (bits & 0x80000000u) ? ~bits : bits | 0x80000000u; }
__host__ __device__ inline uint32_t order_bits(uint32_t image) { return (image & 0x80000000u) ? image ^ 0x80000000u : ~image; }
__device__ inline bool nonfinite_bits(uint32_t b) { return (b & 0x7F800000u) == 0x7F800000u; }

// ---- keys ----
__global__ void __launch_bounds__(256) glb_keys_kernel(uint32_t C, uint32_t A, uint32_t F, uint32_t NV, uint32_t vbits, const uint32_t* __restrict__ face_ptr,
                                                       const uint32_t* __restrict__ tc_ptr, const uint32_t* __restrict__ faces, const uint32_t* __restrict__ ids,
                                                       const uint32_t* __restrict__ mesh_faces, u64* __restrict__ key, uint32_t* __restrict__ corner, u64* __restrict__ c64) {
    const uint32_t c = blockIdx.x * 256u + threadIdx.x;
    if (c >= C) return;
    const uint32_t e = c / 3u, k = c - 3u * e, a = model_range_of(face_ptr, A, e), tc0 = tc_ptr[a];
    ModelCorner m = model_corner(mesh_faces, F, faces, ids, tc0, tc_ptr[a + 1] - tc0, e, k);
    const bool v_ok = m.v < NV;   // (a bad face gives vertex 0: a mesh with faces has a vertex, or the count below refuses the call)
    if (!m.face_ok && k == 0u) atomicAdd(&c64[K_BAD_FACE], 1ull);
    if (!m.id_ok) atomicAdd(&c64[K_BAD_ID], 1ull);
    if (m.face_ok && !v_ok) atomicAdd(&c64[K_BAD_VERT], 1ull);
    key[c] = ((u64)m.g << vbits) | (u64)(v_ok ? m.v : 0u);
    corner[c] = c;
}

// ---- number ----
// head [C + 1]: 1 where a sorted key differs from the one in front, head[C] = 0 (the scan leaves the number of pairs there)
__global__ void __launch_bounds__(256) glb_heads_kernel(uint32_t C, uint32_t NV, uint32_t vbits, const u64* __restrict__ ks, const float* __restrict__ verts,
                                                        const float* __restrict__ normals, uint32_t* __restrict__ head, u64* __restrict__ c64) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i > C) return;
    if (i == C) { head[C] = 0u; return; }
    const u64 k = ks[i];
    const bool h = i == 0u || ks[i - 1] != k;
    head[i] = h ? 1u : 0u;
    if (!h) return;
    const uint32_t v = (uint32_t)(k & ((1ull << vbits) - 1ull));
    if (v >= NV) return;   // (only after a refused corner)
    uint32_t bad = 0;
    for (uint32_t j = 0; j < 3u; ++j) {
        bad += nonfinite_bits(__float_as_uint(verts[3 * (size_t)v + j])) ? 1u : 0u;
        if (normals) bad += nonfinite_bits(__float_as_uint(normals[3 * (size_t)v + j])) ? 1u : 0u;
    }
    if (bad) atomicAdd(&c64[K_NONFINITE], (u64)bad);
}

// first [A + 1]: the number of the first pair whose coordinate is at or behind tc_ptr[a] (rank [C + 1]: the scan of head)
__global__ void __launch_bounds__(256) glb_first_kernel(uint32_t A, uint32_t C, uint32_t vbits, const uint32_t* __restrict__ tc_ptr, const u64* __restrict__ ks,
                                                        const uint32_t* __restrict__ rank, uint32_t* __restrict__ first) {
    const uint32_t a = blockIdx.x * 256u + threadIdx.x;
    if (a > A) return;
    const u64 want = (u64)tc_ptr[a] << vbits;
    uint32_t lo = 0, hi = C;   // keys in front of lo are below `want`, keys from hi on are not
    while (lo < hi) { const uint32_t mid = lo + (hi - lo) / 2u; if (ks[mid] < want) lo = mid + 1u; else hi = mid; }
    first[a] = rank[lo];
}

// ---- indices ----
__global__ void __launch_bounds__(256) glb_indices_kernel(uint32_t C, uint32_t A, const u64* __restrict__ ks, const uint32_t* __restrict__ cs, const uint32_t* __restrict__ head,
                                                          const uint32_t* __restrict__ rank, const uint32_t* __restrict__ face_ptr, const uint32_t* __restrict__ first,
                                                          uint32_t* __restrict__ indices, u64* __restrict__ pair) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= C) return;
    const uint32_t h = head[i], number = rank[i] + h - 1u, c = cs[i];   // (rank counts the heads in front: a head's own number, one less behind it)
    indices[c] = number - first[model_range_of(face_ptr, A, c / 3u)];
    if (h) pair[number] = ks[i];
}

// ---- gather ----
// One section's share of a block through its LDS image: the block owns dwords [d0, d0 + len) of out (a 16-byte aligned buffer), which lie
// in `stage` from index d0 & 3 on, so that aligned chunks of the file are aligned chunks of the image.
__device__ inline void store_block_range(uint32_t* __restrict__ out, const uint32_t* stage, uint64_t d0, uint32_t len, uint32_t tid) {
    const uint64_t base = d0 & ~3ull, end = d0 + len;
    const uint64_t full_lo = (d0 + 3ull) & ~3ull, full_hi = end & ~3ull;   // the 16-byte chunks that are all this block's
    for (uint64_t d = full_lo + 4ull * tid; d + 4ull <= full_hi; d += 4ull * 256ull)
        *reinterpret_cast<uint4*>(out + d) = *reinterpret_cast<const uint4*>(stage + (size_t)(d - base));
    const uint64_t head_end = full_lo < end ? full_lo : end, tail_lo = full_hi > head_end ? full_hi : head_end;
    if (tid < 4u) { const uint64_t d = d0 + tid; if (d < head_end) out[d] = stage[(size_t)(d - base)]; }
    else if (tid < 8u) { const uint64_t d = tail_lo + (tid - 4u); if (d < end) out[d] = stage[(size_t)(d - base)]; }
}

__device__ inline uint32_t wave_min(uint32_t x) { for (int m = 32; m >= 1; m >>= 1) x = min(x, (uint32_t)__shfl_xor((int)x, m, 64)); return x; }
__device__ inline uint32_t wave_max(uint32_t x) { for (int m = 32; m >= 1; m >>= 1) x = max(x, (uint32_t)__shfl_xor((int)x, m, 64)); return x; }

// mn / mx of the block's lanes into lo3 [3] / hi3 [3]: wave shuffles, LDS across the four waves, then 6 integer atomics
__device__ inline void block_bounds(uint32_t (&mn)[3], uint32_t (&mx)[3], uint32_t (*s_red)[6], uint32_t* __restrict__ lo3, uint32_t* __restrict__ hi3, uint32_t tid) {
    for (uint32_t j = 0; j < 3u; ++j) { mn[j] = wave_min(mn[j]); mx[j] = wave_max(mx[j]); }
    if ((tid & 63u) == 0u) for (uint32_t j = 0; j < 3u; ++j) { s_red[tid >> 6][j] = mn[j]; s_red[tid >> 6][3 + j] = mx[j]; }
    __syncthreads();
    if (tid < 3u) atomicMin(&lo3[tid], min(min(s_red[0][tid], s_red[1][tid]), min(s_red[2][tid], s_red[3][tid])));
    else if (tid < 6u) atomicMax(&hi3[tid - 3u], max(max(s_red[0][tid], s_red[1][tid]), max(s_red[2][tid], s_red[3][tid])));
}

// a gather block's bounds per atlas (lo / hi [3 A]); s_atlas: the atlas of the block's first and last pair, written before the last barrier.
// Block-uniform branch -- the numbers ascend with the atlas, so equal ends mean one atlas; the few blocks that straddle a range's end
// go per lane.
__device__ inline void store_atlas_bounds(uint32_t (&mn)[3], uint32_t (&mx)[3], uint32_t a, bool live, uint32_t (*s_red)[6], const uint32_t* s_atlas,
                                          uint32_t* __restrict__ lo, uint32_t* __restrict__ hi, uint32_t tid) {
    if (s_atlas[0] == s_atlas[1]) {
        block_bounds(mn, mx, s_red, lo + 3 * (size_t)s_atlas[0], hi + 3 * (size_t)s_atlas[0], tid);
    } else if (live) {
        for (uint32_t j = 0; j < 3u; ++j) { atomicMin(&lo[3 * (size_t)a + j], mn[j]); atomicMax(&hi[3 * (size_t)a + j], mx[j]); }
    }
}

// out: dwords; POSITION at dword 0, TEXCOORD_0 at uv_at, NORMAL at nrm_at (normals null: absent).  lo / hi [3 A]: the bounds' images.
__global__ void __launch_bounds__(256) glb_gather_kernel(uint32_t NP, uint32_t A, uint32_t vbits, const u64* __restrict__ pair, const float* __restrict__ verts,
                                                         const float* __restrict__ merged, const float* __restrict__ normals, const uint32_t* __restrict__ first,
                                                         uint32_t* __restrict__ out, uint64_t uv_at, uint64_t nrm_at, uint32_t* __restrict__ lo, uint32_t* __restrict__ hi) {
    __shared__ uint4 s_pos4[(3 * 256 + 4) / 4 + 1], s_uv4[(2 * 256 + 4) / 4 + 1], s_nrm4[(3 * 256 + 4) / 4 + 1];
    __shared__ uint32_t s_red[4][6], s_atlas[2];
    uint32_t* s_pos = reinterpret_cast<uint32_t*>(s_pos4); uint32_t* s_uv = reinterpret_cast<uint32_t*>(s_uv4); uint32_t* s_nrm = reinterpret_cast<uint32_t*>(s_nrm4);
    const uint32_t tid = threadIdx.x, p0 = blockIdx.x * 256u, n = min(256u, NP - p0), p = p0 + tid;
    const bool live = tid < n;
    const uint64_t pos_d0 = 3ull * p0, uv_d0 = uv_at + 2ull * p0, nrm_d0 = nrm_at + 3ull * p0;
    uint32_t mn[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, mx[3] = {0u, 0u, 0u}, a = 0u;
    if (live) {
        const u64 k = pair[p];
        const uint32_t v = (uint32_t)(k & ((1ull << vbits) - 1ull)), g = (uint32_t)(k >> vbits);
        a = model_range_of(first, A, p);
        for (uint32_t j = 0; j < 3u; ++j) {
            const uint32_t b = __float_as_uint(verts[3 * (size_t)v + j]), im = order_image(b);
            s_pos[(pos_d0 & 3ull) + 3u * tid + j] = b; mn[j] = im; mx[j] = im;
            if (normals) s_nrm[(nrm_d0 & 3ull) + 3u * tid + j] = __float_as_uint(normals[3 * (size_t)v + j]);
        }
        for (uint32_t j = 0; j < 2u; ++j) s_uv[(uv_d0 & 3ull) + 2u * tid + j] = __float_as_uint(merged[2 * (size_t)g + j]);
        if (tid == 0u) s_atlas[0] = a;
        if (tid == n - 1u) s_atlas[1] = a;
    }
    __syncthreads();
    store_block_range(out, s_pos, pos_d0, 3u * n, tid);
    store_block_range(out, s_uv, uv_d0, 2u * n, tid);
    if (normals) store_block_range(out, s_nrm, nrm_d0, 3u * n, tid);
    store_atlas_bounds(mn, mx, a, live, s_red, s_atlas, lo, hi, tid);
}

// ---- glb_quantize 1 (item 10) ----
// The arithmetic of the item, written once for the kernels and the host's JSON: fp64 + - * / sqrt and conversions only, under
// -ffp-contract=off, so the host, the device and the numpy restatement give the same bits.
__host__ __device__ inline float float_of_image(uint32_t image) { const uint32_t b = order_bits(image); float x; memcpy(&x, &b, 4); return x; }
// E: the largest of the three extents of the file-wide bounds fb = lo images [3] | hi images [3]
__host__ __device__ inline double grid_extent(const uint32_t* fb) {
    double E = 0.0;
    for (int j = 0; j < 3; ++j) { const double d = (double)float_of_image(fb[3 + j]) - (double)float_of_image(fb[j]); if (d > E) E = d; }
    return E;
}
__host__ __device__ inline uint32_t quant_position(float x, float lo, double E) {   // lo <= x <= hi, all finite
    if (E == 0.0) return 0u;
    const double t = (((double)x - (double)lo) / E) * 65535.0 + 0.5;
    const uint32_t q = (uint32_t)t;   // truncation: halves round up
    return q < 65535u ? q : 65535u;
}
__host__ __device__ inline bool texcoord_storable(float u) { return u >= 0.0f && u <= 1.0f; }   // (false for nan; -0 is 0)
__host__ __device__ inline uint32_t quant_texcoord(float u) { return texcoord_storable(u) ? (uint32_t)((double)u * 65535.0 + 0.5) : 0u; }
// c = (component / length) * 127 to a BYTE in [-127, 127], halves away from zero; the byte's bits
__host__ __device__ inline uint32_t quant_normal(double c) {
    const double m = c < 0.0 ? -c : c;
    uint32_t r = (uint32_t)(m + 0.5);
    if (r > 127u) r = 127u;
    return (c < 0.0 ? 0u - r : r) & 0xFFu;
}

// indices: glb_indices_kernel with the width and the place of every primitive looked up per corner.  idx: the index part's first byte
// (4-byte aligned); idx_off [A]: atlas a's byte offset in it, a multiple of 4.  An atlas of at most 65 535 pairs takes 2-byte indices,
// and where its 3 n corners are an odd number its last corner stores the 2 zero bytes behind them as well.
__global__ void __launch_bounds__(256) glb_quant_indices_kernel(uint32_t C, uint32_t A, const u64* __restrict__ ks, const uint32_t* __restrict__ cs, const uint32_t* __restrict__ head,
                                                                const uint32_t* __restrict__ rank, const uint32_t* __restrict__ face_ptr, const uint32_t* __restrict__ first,
                                                                const uint32_t* __restrict__ idx_off, uint8_t* __restrict__ idx, u64* __restrict__ pair) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= C) return;
    const uint32_t h = head[i], number = rank[i] + h - 1u, c = cs[i];
    const uint32_t a = model_range_of(face_ptr, A, c / 3u), f0 = first[a], e0 = face_ptr[a];
    const uint32_t local = c - 3u * e0, corners = 3u * (face_ptr[a + 1] - e0), value = number - f0;
    uint8_t* at = idx + idx_off[a];
    if (first[a + 1] - f0 > 65535u) {
        reinterpret_cast<uint32_t*>(at)[local] = value;
    } else {
        uint16_t* at16 = reinterpret_cast<uint16_t*>(at);
        at16[local] = (uint16_t)value;
        if (local == corners - 1u && (corners & 1u)) at16[corners] = (uint16_t)0u;
    }
    if (h) pair[number] = ks[i];
}

// bounds: fb = lo [3] | hi [3] (preset to all ones / zero), the images of POSITION's bounds over every pair of the file.  One pair per
// lane and round; at most 1024 blocks, so that the six words take a few thousand atomics however long the list is.
__global__ void __launch_bounds__(256) glb_bounds_kernel(uint32_t NP, uint32_t vbits, const u64* __restrict__ pair, const float* __restrict__ verts, uint32_t* __restrict__ fb) {
    __shared__ uint32_t s_red[4][6];
    uint32_t mn[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, mx[3] = {0u, 0u, 0u};
    for (uint64_t p = (uint64_t)blockIdx.x * 256u + threadIdx.x; p < NP; p += (uint64_t)gridDim.x * 256u) {
        const uint32_t v = (uint32_t)(pair[p] & ((1ull << vbits) - 1ull));
        for (uint32_t j = 0; j < 3u; ++j) { const uint32_t im = order_image(__float_as_uint(verts[3 * (size_t)v + j])); mn[j] = min(mn[j], im); mx[j] = max(mx[j], im); }
    }
    block_bounds(mn, mx, s_red, fb, fb + 3, threadIdx.x);
}

// gather: glb_gather_kernel's blocks, LDS images and stores with 8 / 4 / 4 bytes per vertex: POSITION as three 16-bit steps of the file's
// grid and two zero bytes, TEXCOORD_0 as two 16-bit fractions, NORMAL as the unit normal in three bytes and a zero byte.  lo / hi [3 A]:
// the bounds of the STORED integers per atlas.  c64: K_TC_RANGE per component, K_ZERO_NORMAL per pair.
__global__ void __launch_bounds__(256) glb_quant_gather_kernel(uint32_t NP, uint32_t A, uint32_t vbits, const u64* __restrict__ pair, const float* __restrict__ verts,
                                                               const float* __restrict__ merged, const float* __restrict__ normals, const uint32_t* __restrict__ first,
                                                               const uint32_t* __restrict__ fb, uint32_t* __restrict__ out, uint64_t uv_at, uint64_t nrm_at,
                                                               uint32_t* __restrict__ lo, uint32_t* __restrict__ hi, u64* __restrict__ c64) {
    __shared__ uint4 s_pos4[2 * 256 / 4], s_uv4[(256 + 4) / 4 + 1], s_nrm4[(256 + 4) / 4 + 1];
    __shared__ uint32_t s_red[4][6], s_atlas[2];
    uint32_t* s_pos = reinterpret_cast<uint32_t*>(s_pos4); uint32_t* s_uv = reinterpret_cast<uint32_t*>(s_uv4); uint32_t* s_nrm = reinterpret_cast<uint32_t*>(s_nrm4);
    const uint32_t tid = threadIdx.x, p0 = blockIdx.x * 256u, n = min(256u, NP - p0), p = p0 + tid;
    const bool live = tid < n;
    const uint64_t pos_d0 = 2ull * p0, uv_d0 = uv_at + p0, nrm_d0 = nrm_at + p0;   // (pos_d0 is a multiple of 4: the image starts at s_pos[0])
    uint32_t mn[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, mx[3] = {0u, 0u, 0u}, a = 0u;
    if (live) {
        const u64 k = pair[p];
        const uint32_t v = (uint32_t)(k & ((1ull << vbits) - 1ull)), g = (uint32_t)(k >> vbits);
        a = model_range_of(first, A, p);
        const double E = grid_extent(fb);
        uint32_t q[3];
        for (uint32_t j = 0; j < 3u; ++j) { q[j] = quant_position(verts[3 * (size_t)v + j], float_of_image(fb[j]), E); mn[j] = q[j]; mx[j] = q[j]; }
        reinterpret_cast<uint2*>(s_pos)[tid] = make_uint2(q[0] | (q[1] << 16), q[2]);   // one 8-byte LDS store
        const float u0 = merged[2 * (size_t)g], u1 = merged[2 * (size_t)g + 1];
        s_uv[(uv_d0 & 3ull) + tid] = quant_texcoord(u0) | (quant_texcoord(u1) << 16);
        const uint32_t bad = (texcoord_storable(u0) ? 0u : 1u) + (texcoord_storable(u1) ? 0u : 1u);
        if (bad) atomicAdd(&c64[K_TC_RANGE], (u64)bad);
        if (normals) {
            const double x = (double)normals[3 * (size_t)v], y = (double)normals[3 * (size_t)v + 1], z = (double)normals[3 * (size_t)v + 2];
            const double l = sqrt((x * x + y * y) + z * z);
            uint32_t packed = 0u;
            if (l == 0.0) atomicAdd(&c64[K_ZERO_NORMAL], 1ull);
            else packed = quant_normal((x / l) * 127.0) | (quant_normal((y / l) * 127.0) << 8) | (quant_normal((z / l) * 127.0) << 16);
            s_nrm[(nrm_d0 & 3ull) + tid] = packed;
        }
        if (tid == 0u) s_atlas[0] = a;
        if (tid == n - 1u) s_atlas[1] = a;
    }
    __syncthreads();
    store_block_range(out, s_pos, pos_d0, 2u * n, tid);
    store_block_range(out, s_uv, uv_d0, n, tid);
    if (normals) store_block_range(out, s_nrm, nrm_d0, n, tid);
    store_atlas_bounds(mn, mx, a, live, s_red, s_atlas, lo, hi, tid);
}

inline unsigned bits_for(uint32_t count) { unsigned b = 1; while (b < 32u && (1ull << b) < (u64)count) ++b; return b; }   // bits that hold 0 .. count - 1, at least 1

// a finite float as a JSON number that reads back to the same float: %.9g, with ".0" behind a bare integer so that a reader keeps it a
// float (and -0 its sign)
std::string fmt_float(uint32_t bits) {
    float x; memcpy(&x, &bits, 4);
    char b[32]; snprintf(b, sizeof(b), "%.9g", (double)x);
    std::string t(b);
    if (t.find_first_of(".e") == std::string::npos) t += ".0";
    return t;
}

// a finite double as a JSON number that reads back to the same double: %.17g, with ".0" behind a bare integer
std::string fmt_double(double x) {
    char b[40]; snprintf(b, sizeof(b), "%.17g", x);
    std::string t(b);
    if (t.find_first_of(".e") == std::string::npos) t += ".0";
    return t;
}

// what a call leaves for its writer
struct GlbParts {
    std::string json;                         // padded with spaces
    uint64_t geometry_bytes = 0, bin_bytes = 0;   // bin_bytes: the BIN chunk's data, padded (0: no BIN chunk)
    std::vector<std::vector<uint8_t>> png;    // per atlas (empty: no images)
    std::vector<uint64_t> png_at;             // offsets in the BIN chunk
    uint64_t file_bytes = 0;
};

void refuse_size(uint64_t bytes, const mvs_model_params& P, const char* who) {
    if (bytes >= 0xFFFFFFFFull) throw StatusError(MVS_ERR_UNSUPPORTED, std::string(who) + ": " + std::to_string(bytes) + " bytes do not fit one .glb (below 2^32 - 1)");
    if (P.max_bytes && bytes > P.max_bytes) throw StatusError(MVS_ERR_UNSUPPORTED, std::string(who) + ": " + std::to_string(bytes) + " bytes exceed max_bytes = " + std::to_string(P.max_bytes));
}

// keys .. gather and the PNGs: leaves the geometry in D.geo and everything else in `G`
void run_glb(mvs_ctx* ctx, GlbDev& D, const mvs_atlas_set& in, int on_device, const float* normals_in, int normals_on_device, const mvs_model_params& P,
             mvs_glb_stats& st, GlbParts& G, const char* who) {
    hipStream_t s = ctx->stream;
    mvs_glb_quant_stats& qs = D.quant_stats;
    qs = mvs_glb_quant_stats{};
    const uint32_t A = in.n_atlases, L = in.n_listed, NM = in.n_merged, NV = ctx->n_verts, F = ctx->n_faces;
    std::vector<uint32_t> hf, ht;
    model_check_set(ctx, in, on_device, who, hf, ht);
    if (P.glb_quantize != 0 && P.glb_quantize != 1) throw StatusError(MVS_ERR_INVALID, std::string(who) + ": glb_quantize must be 0 or 1, not " + std::to_string(P.glb_quantize));
    const bool quant = P.glb_quantize == 1;
    const bool images = A && in.atlas_size && in.image;   // a text-only set has neither
    if (images) model_check_image_params(P, in, who);
    st.indices = 3ull * L;
    for (uint32_t a = 0; a < A; ++a) st.primitives += hf[a + 1] > hf[a] ? 1u : 0u;
    refuse_size(28ull + 12ull * L, mvs_model_params{0, 0, 0}, who);   // the format's own limit on the indices alone (so 3 L < 2^30 below); max_bytes waits for the numbering
    // (glb_quantize 1 keeps this check on 4-byte indices: the widths are not known before the numbering, and the bound on 3 L is what the kernels rely on)
    const uint32_t C = 3u * L;
    const unsigned vbits = bits_for(NV), gbits = bits_for(NM);
    // ---- inputs where the kernels read them ----
    const uint32_t* d_faces = stage(D.in_faces, (const uint32_t*)in.faces, L, on_device, s);
    const uint32_t* d_ids = stage(D.in_ids, (const uint32_t*)in.texcoord_ids, 3 * (size_t)L, on_device, s);
    const float* d_merged = stage(D.in_merged, (const float*)in.texcoords_merged, 2 * (size_t)NM, on_device, s);
    const uint32_t* d_face_ptr; const uint32_t* d_tc_ptr;
    if (A) { d_face_ptr = stage(D.in_face_ptr, (const uint32_t*)in.face_ptr, (size_t)A + 1, on_device, s); d_tc_ptr = stage(D.in_tc_ptr, (const uint32_t*)in.tc_ptr, (size_t)A + 1, on_device, s); }
    else { upload(D.in_face_ptr, hf, s); upload(D.in_tc_ptr, ht, s); d_face_ptr = D.in_face_ptr.p; d_tc_ptr = D.in_tc_ptr.p; }   // the one zero of each
    const float* d_normals = normals_in ? stage(D.in_normals, normals_in, 3 * (size_t)NV, normals_on_device, s) : nullptr;
    MVS_HIP(hipStreamSynchronize(s));   // host buffers are borrowed for the call only
    D.key.ensure((size_t)C + 1); D.key_sorted.ensure((size_t)C + 1); D.corner.ensure((size_t)C + 1); D.corner_sorted.ensure((size_t)C + 1);
    D.head.ensure((size_t)C + 1); D.rank.ensure((size_t)C + 1); D.first.ensure((size_t)A + 1); D.c64.ensure(K_N);
    D.lo.ensure(3 * (size_t)A + 1); D.hi.ensure(3 * (size_t)A + 1);
    StageTimer<8> tm(s);
    // ---- keys ----
    tm.mark();
    MVS_HIP(hipMemsetAsync(D.c64.p, 0, K_N * sizeof(u64), s));
    if (C) {
        hipLaunchKernelGGL(glb_keys_kernel, dim3(grid(C)), dim3(256), 0, s, C, A, F, NV, (uint32_t)vbits, d_face_ptr, d_tc_ptr, d_faces, d_ids, (const uint32_t*)ctx->d_faces,
                           D.key.p, D.corner.p, D.c64.p);
        MVS_LAUNCH_CHECK();
    }
    tm.mark();
    // ---- sort ----
    if (C) dev_sort_pairs(ctx, (const u64*)D.key.p, D.key_sorted.p, (const uint32_t*)D.corner.p, D.corner_sorted.p, (size_t)C, 0u, vbits + gbits);
    tm.mark();
    // ---- number ----
    hipLaunchKernelGGL(glb_heads_kernel, dim3(grid((size_t)C + 1)), dim3(256), 0, s, C, NV, (uint32_t)vbits, (const u64*)D.key_sorted.p, (const float*)ctx->d_verts, d_normals,
                       D.head.p, D.c64.p);
    MVS_LAUNCH_CHECK();
    dev_exclusive_scan(ctx, (const uint32_t*)D.head.p, D.rank.p, (size_t)C + 1);
    hipLaunchKernelGGL(glb_first_kernel, dim3(grid((size_t)A + 1)), dim3(256), 0, s, A, C, (uint32_t)vbits, d_tc_ptr, (const u64*)D.key_sorted.p, (const uint32_t*)D.rank.p, D.first.p);
    MVS_LAUNCH_CHECK();
    tm.mark();
    // ---- the one read-back of the numbering: counters, first[] ----
    std::vector<uint32_t> first((size_t)A + 1);
    u64 c64[K_N];
    MVS_HIP(hipMemcpyAsync(c64, D.c64.p, sizeof(c64), hipMemcpyDeviceToHost, s));
    MVS_HIP(hipMemcpyAsync(first.data(), D.first.p, ((size_t)A + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    MVS_HIP(hipStreamSynchronize(s));
    st.ms_keys = tm.ms(0, 1); st.ms_sort = tm.ms(1, 2); st.ms_number = tm.ms(2, 3);
    model_refuse_bad_ids(c64[K_BAD_FACE], c64[K_BAD_ID], who);
    if (c64[K_BAD_VERT]) throw StatusError(MVS_ERR_INVALID, std::string(who) + ": " + std::to_string(c64[K_BAD_VERT]) + " corners name a vertex that is not below the number of vertices");
    const uint32_t NP = first[A];
    // the layout: item 8's, or item 10's -- 8 / 4 / 4 bytes per vertex, and per atlas 2-byte indices up to 65 535 vertices, every atlas
    // from a multiple of 4 (a host scan over the atlases)
    const uint64_t pos_stride = quant ? 8u : 12u, uv_stride = quant ? 4u : 8u, nrm_stride = quant ? 4u : 12u;
    std::vector<uint32_t> idx_off(quant ? (size_t)A + 1 : 0);
    uint64_t idx_bytes = 4ull * C;
    if (quant) {
        uint64_t at = 0;
        for (uint32_t a = 0; a < A; ++a) {
            idx_off[a] = (uint32_t)at;
            const bool narrow = first[a + 1] - first[a] <= 65535u;
            if (hf[a + 1] > hf[a] && narrow) ++qs.index16_primitives;
            at += ((narrow ? 6ull : 12ull) * (hf[a + 1] - hf[a]) + 3ull) & ~3ull;
        }
        idx_off[A] = (uint32_t)at; idx_bytes = at;
    }
    const uint64_t pos_bytes = pos_stride * NP, uv_bytes = uv_stride * NP, nrm_bytes = d_normals ? nrm_stride * NP : 0ull;
    const uint64_t uv_at = pos_bytes, nrm_at = uv_at + uv_bytes, idx_at = nrm_at + nrm_bytes;   // every part a multiple of 4 bytes: no padding between them
    G.geometry_bytes = idx_at + idx_bytes;
    st.vertices = NP; st.geometry_bytes = G.geometry_bytes; st.nonfinite_values = c64[K_NONFINITE];
    st.file_bytes = 12ull + 8ull + (G.geometry_bytes ? 8ull + G.geometry_bytes : 0ull);   // what is known so far: the headers and the geometry
    if (c64[K_NONFINITE]) throw StatusError(MVS_ERR_UNSUPPORTED, std::string(who) + ": " + std::to_string(c64[K_NONFINITE]) + " position or normal values of referenced vertices are not finite");
    refuse_size(st.file_bytes, P, who);
    // ---- indices ----
    D.geo.ensure((size_t)(G.geometry_bytes / 16) + 2); D.pair.ensure((size_t)NP + 1);
    uint32_t* geo = reinterpret_cast<uint32_t*>(D.geo.p);
    if (quant) upload(D.idx_off, idx_off, s);   // (in front of the mark: the phase is the kernel)
    tm.mark();
    if (C && !quant) {
        hipLaunchKernelGGL(glb_indices_kernel, dim3(grid(C)), dim3(256), 0, s, C, A, (const u64*)D.key_sorted.p, (const uint32_t*)D.corner_sorted.p, (const uint32_t*)D.head.p,
                           (const uint32_t*)D.rank.p, d_face_ptr, (const uint32_t*)D.first.p, geo + idx_at / 4, D.pair.p);
        MVS_LAUNCH_CHECK();
    } else if (C) {
        hipLaunchKernelGGL(glb_quant_indices_kernel, dim3(grid(C)), dim3(256), 0, s, C, A, (const u64*)D.key_sorted.p, (const uint32_t*)D.corner_sorted.p, (const uint32_t*)D.head.p,
                           (const uint32_t*)D.rank.p, d_face_ptr, (const uint32_t*)D.first.p, (const uint32_t*)D.idx_off.p, reinterpret_cast<uint8_t*>(geo) + idx_at, D.pair.p);
        MVS_LAUNCH_CHECK();
    }
    tm.mark();
    // ---- bounds (glb_quantize 1): the file's six words stay on the device for the gather; the host reads them with the atlases' ----
    if (quant) {
        D.file_bounds.ensure(6);
        MVS_HIP(hipMemsetAsync(D.file_bounds.p, 0xFF, 3 * sizeof(uint32_t), s)); MVS_HIP(hipMemsetAsync(D.file_bounds.p + 3, 0, 3 * sizeof(uint32_t), s));
        if (NP) {
            hipLaunchKernelGGL(glb_bounds_kernel, dim3(std::min<size_t>(grid(NP), 1024)), dim3(256), 0, s, NP, (uint32_t)vbits, (const u64*)D.pair.p, (const float*)ctx->d_verts, D.file_bounds.p);
            MVS_LAUNCH_CHECK();
        }
    }
    tm.mark();
    // ---- gather ----
    if (A) { MVS_HIP(hipMemsetAsync(D.lo.p, 0xFF, 3 * (size_t)A * sizeof(uint32_t), s)); MVS_HIP(hipMemsetAsync(D.hi.p, 0, 3 * (size_t)A * sizeof(uint32_t), s)); }
    if (NP && quant) {
        hipLaunchKernelGGL(glb_quant_gather_kernel, dim3(grid(NP)), dim3(256), 0, s, NP, A, (uint32_t)vbits, (const u64*)D.pair.p, (const float*)ctx->d_verts, d_merged, d_normals,
                           (const uint32_t*)D.first.p, (const uint32_t*)D.file_bounds.p, geo, (uint64_t)(uv_at / 4), (uint64_t)(nrm_at / 4), D.lo.p, D.hi.p, D.c64.p);
        MVS_LAUNCH_CHECK();
    } else if (NP) {
        hipLaunchKernelGGL(glb_gather_kernel, dim3(grid(NP)), dim3(256), 0, s, NP, A, (uint32_t)vbits, (const u64*)D.pair.p, (const float*)ctx->d_verts, d_merged, d_normals,
                           (const uint32_t*)D.first.p, geo, (uint64_t)(uv_at / 4), (uint64_t)(nrm_at / 4), D.lo.p, D.hi.p);
        MVS_LAUNCH_CHECK();
    }
    tm.mark();
    std::vector<uint32_t> lo(3 * (size_t)A), hi(3 * (size_t)A);
    if (A) {
        MVS_HIP(hipMemcpyAsync(lo.data(), D.lo.p, lo.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        MVS_HIP(hipMemcpyAsync(hi.data(), D.hi.p, hi.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    }
    uint32_t fb[6] = {0, 0, 0, 0, 0, 0};
    if (quant) {
        MVS_HIP(hipMemcpyAsync(fb, D.file_bounds.p, sizeof(fb), hipMemcpyDeviceToHost, s));
        MVS_HIP(hipMemcpyAsync(c64, D.c64.p, sizeof(c64), hipMemcpyDeviceToHost, s));
    }
    MVS_HIP(hipStreamSynchronize(s));
    st.ms_indices = tm.ms(4, 5); qs.ms_bounds = quant ? tm.ms(5, 6) : 0.0f; st.ms_gather = tm.ms(6, 7);
    qs.zero_normals = c64[K_ZERO_NORMAL]; qs.texcoords_out_of_range = c64[K_TC_RANGE];
    if (c64[K_TC_RANGE]) throw StatusError(MVS_ERR_UNSUPPORTED, std::string(who) + ": " + std::to_string(c64[K_TC_RANGE]) + " texture coordinate values of referenced pairs are nan or outside [0, 1]: glb_quantize 1 cannot store them");
    // ---- the PNGs: save_model's, byte for byte ----
    const double t_png = now_ms_host();
    G.png_at.clear(); G.png.clear();
    if (images) {
        G.png.resize(A);
        model_for_each_image(ctx, in, on_device, P, who, [&](uint32_t a, const uint8_t* bytes, size_t n, std::string&) { G.png[a].assign(bytes, bytes + n); return MVS_OK; });
    }
    st.ms_png = (float)(now_ms_host() - t_png);
    uint64_t at = G.geometry_bytes;
    for (const auto& f : G.png) { G.png_at.push_back(at); at += ((uint64_t)f.size() + 3ull) & ~3ull; }
    st.image_bytes = at - G.geometry_bytes;
    G.bin_bytes = at;
    uint64_t buffer_bytes = G.geometry_bytes;   // the buffer ends with its last part, the chunk with that part's padding
    if (!G.png.empty()) buffer_bytes = G.png_at.back() + G.png.back().size();
    // ---- JSON ----
    const double t_json = now_ms_host();
    std::string j;
    j.reserve(1024 + 1024 * (size_t)A);
    auto num = [](uint64_t v) { return std::to_string(v); };
    const bool nrm = d_normals != nullptr;
    const uint32_t view_idx = nrm ? 3u : 2u, per = nrm ? 4u : 3u;   // buffer views: POSITION, TEXCOORD_0, [NORMAL], indices, then one per image
    j += "{\"asset\":{\"version\":\"2.0\",\"generator\":\"mvs-texturing_amd\"},\"scene\":0,";
    if (quant) j += "\"extensionsUsed\":[\"KHR_mesh_quantization\"],\"extensionsRequired\":[\"KHR_mesh_quantization\"],";
    if (st.primitives) {
        j += "\"scenes\":[{\"nodes\":[0]}],\"nodes\":[{\"mesh\":0";
        if (quant) {   // the grid: stored integer q of axis k is the point lo[k] + q S
            const double E = grid_extent(fb), S = E == 0.0 ? 1.0 : E / 65535.0;
            j += ",\"translation\":[";
            for (int k = 0; k < 3; ++k) j += (k ? "," : "") + fmt_float(order_bits(fb[k]));
            j += "],\"scale\":[" + fmt_double(S) + "," + fmt_double(S) + "," + fmt_double(S) + "]";
        }
        j += "}],\"meshes\":[{\"primitives\":[";
        uint32_t q = 0;
        for (uint32_t a = 0; a < A; ++a) {
            if (hf[a + 1] == hf[a]) continue;
            if (q) j += ",";
            j += "{\"attributes\":{\"POSITION\":" + num(per * q) + ",\"TEXCOORD_0\":" + num(per * q + 1u);
            if (nrm) j += ",\"NORMAL\":" + num(per * q + 2u);
            j += "},\"indices\":" + num(per * q + per - 1u) + ",\"material\":" + num(a) + ",\"mode\":4}";
            ++q;
        }
        j += "]}],\"accessors\":[";
        q = 0;
        for (uint32_t a = 0; a < A; ++a) {
            if (hf[a + 1] == hf[a]) continue;
            if (q++) j += ",";
            const uint64_t f0 = first[a], cnt = first[a + 1] - first[a];
            if (quant) {
                j += "{\"bufferView\":0,\"byteOffset\":" + num(8ull * f0) + ",\"componentType\":5123,\"count\":" + num(cnt) + ",\"type\":\"VEC3\",\"min\":[";
                for (int k = 0; k < 3; ++k) j += (k ? "," : "") + num(lo[3 * (size_t)a + k]);
                j += "],\"max\":[";
                for (int k = 0; k < 3; ++k) j += (k ? "," : "") + num(hi[3 * (size_t)a + k]);
                j += "]},{\"bufferView\":1,\"byteOffset\":" + num(4ull * f0) + ",\"componentType\":5123,\"normalized\":true,\"count\":" + num(cnt) + ",\"type\":\"VEC2\"},";
                if (nrm) j += "{\"bufferView\":2,\"byteOffset\":" + num(4ull * f0) + ",\"componentType\":5120,\"normalized\":true,\"count\":" + num(cnt) + ",\"type\":\"VEC3\"},";
                j += "{\"bufferView\":" + num(view_idx) + ",\"byteOffset\":" + num(idx_off[a]) + ",\"componentType\":" + (cnt <= 65535u ? "5123" : "5125") + ",\"count\":" +
                     num(3ull * (hf[a + 1] - hf[a])) + ",\"type\":\"SCALAR\"}";
                continue;
            }
            j += "{\"bufferView\":0,\"byteOffset\":" + num(12ull * f0) + ",\"componentType\":5126,\"count\":" + num(cnt) + ",\"type\":\"VEC3\",\"min\":[";
            for (int k = 0; k < 3; ++k) j += (k ? "," : "") + fmt_float(order_bits(lo[3 * (size_t)a + k]));
            j += "],\"max\":[";
            for (int k = 0; k < 3; ++k) j += (k ? "," : "") + fmt_float(order_bits(hi[3 * (size_t)a + k]));
            j += "]},{\"bufferView\":1,\"byteOffset\":" + num(8ull * f0) + ",\"componentType\":5126,\"count\":" + num(cnt) + ",\"type\":\"VEC2\"},";
            if (nrm) j += "{\"bufferView\":2,\"byteOffset\":" + num(12ull * f0) + ",\"componentType\":5126,\"count\":" + num(cnt) + ",\"type\":\"VEC3\"},";
            j += "{\"bufferView\":" + num(view_idx) + ",\"byteOffset\":" + num(12ull * hf[a]) + ",\"componentType\":5125,\"count\":" + num(3ull * (hf[a + 1] - hf[a])) + ",\"type\":\"SCALAR\"}";
        }
        j += "],";
    } else {
        j += "\"scenes\":[{}],";
    }
    if (A) {
        j += "\"materials\":[";
        for (uint32_t a = 0; a < A; ++a) {
            j += std::string(a ? "," : "") + "{\"name\":\"material" + model_filled4(a) + "\",\"pbrMetallicRoughness\":{";
            if (images) j += "\"baseColorTexture\":{\"index\":" + num(a) + "},";
            j += "\"metallicFactor\":0,\"roughnessFactor\":1}}";
        }
        j += "],";
    }
    if (images) {
        const uint32_t v0 = st.primitives ? view_idx + 1u : 0u;   // the image views follow the geometry's, where there is geometry
        j += "\"textures\":[";
        for (uint32_t a = 0; a < A; ++a) j += std::string(a ? "," : "") + "{\"sampler\":0,\"source\":" + num(a) + "}";
        j += "],\"images\":[";
        for (uint32_t a = 0; a < A; ++a) j += std::string(a ? "," : "") + "{\"bufferView\":" + num(v0 + a) + (P.image_format == 1 ? ",\"mimeType\":\"image/jpeg\"}" : ",\"mimeType\":\"image/png\"}");
        j += "],\"samplers\":[{\"magFilter\":9729,\"minFilter\":9729,\"wrapS\":33071,\"wrapT\":33071}],";
    }
    if (G.bin_bytes) {
        j += "\"bufferViews\":[";
        bool any = false;
        if (st.primitives) {
            j += "{\"buffer\":0,\"byteOffset\":0,\"byteLength\":" + num(pos_bytes) + ",\"byteStride\":" + num(pos_stride) + ",\"target\":34962},";
            j += "{\"buffer\":0,\"byteOffset\":" + num(uv_at) + ",\"byteLength\":" + num(uv_bytes) + ",\"byteStride\":" + num(uv_stride) + ",\"target\":34962},";
            if (nrm) j += "{\"buffer\":0,\"byteOffset\":" + num(nrm_at) + ",\"byteLength\":" + num(nrm_bytes) + ",\"byteStride\":" + num(nrm_stride) + ",\"target\":34962},";
            j += "{\"buffer\":0,\"byteOffset\":" + num(idx_at) + ",\"byteLength\":" + num(idx_bytes) + ",\"target\":34963}";
            any = true;
        }
        for (size_t a = 0; a < G.png.size(); ++a) {
            j += std::string(any ? "," : "") + "{\"buffer\":0,\"byteOffset\":" + num(G.png_at[a]) + ",\"byteLength\":" + num(G.png[a].size()) + "}";
            any = true;
        }
        j += "],\"buffers\":[{\"byteLength\":" + num(buffer_bytes) + "}],";
    }
    j.back() = '}';   // (every branch above ends with a comma)
    j.resize((j.size() + 3) & ~(size_t)3, ' ');
    G.json.swap(j);
    st.json_bytes = G.json.size();
    G.file_bytes = 12ull + 8ull + G.json.size() + (G.bin_bytes ? 8ull + G.bin_bytes : 0ull);
    st.file_bytes = G.file_bytes;
    st.ms_file = (float)(now_ms_host() - t_json);
    refuse_size(G.file_bytes, P, who);
}

inline void put_le32(uint8_t* p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24); }

// the bytes in front of the geometry: file header, JSON chunk, BIN chunk header
std::vector<uint8_t> glb_front(const GlbParts& G) {
    std::vector<uint8_t> h(20 + G.json.size() + (G.bin_bytes ? 8 : 0));
    put_le32(&h[0], 0x46546C67u); put_le32(&h[4], 2u); put_le32(&h[8], (uint32_t)G.file_bytes);
    put_le32(&h[12], (uint32_t)G.json.size()); put_le32(&h[16], 0x4E4F534Au);
    memcpy(&h[20], G.json.data(), G.json.size());
    if (G.bin_bytes) { put_le32(&h[20 + G.json.size()], (uint32_t)G.bin_bytes); put_le32(&h[24 + G.json.size()], 0x004E4942u); }
    return h;
}

}  // namespace
}  // namespace mvs

using namespace mvs;

extern "C" {

mvs_status mvs_ctx_build_glb(mvs_ctx* ctx, const mvs_atlas_set* atlases, int atlases_on_device, const float* vertex_normals, int normals_on_device,
                             const mvs_model_params* params, mvs_glb* out, mvs_glb_stats* stats) {
    if (!ctx || !atlases || !out) return api_fail(MVS_ERR_INVALID, "null argument");
    *out = mvs_glb{};
    mvs_glb_stats st{};
    if (stats) *stats = st;
    return api_guard([&] {
        MVS_HIP(hipSetDevice(ctx->device));
        hipStream_t s = ctx->stream;
        GlbDev& D = row_dev(ctx->glb);
        const mvs_model_params P = params_or_default(params);
        run_with_stats(s, stats, st, [&] {
            GlbParts G;
            run_glb(ctx, D, *atlases, atlases_on_device, vertex_normals, normals_on_device, P, st, G, "build_glb");
            const double t0 = now_ms_host();
            const std::vector<uint8_t> front = glb_front(G);
            uint8_t* file = (uint8_t*)malloc((size_t)G.file_bytes);
            if (!file) throw StatusError(MVS_ERR_INVALID, "out of host memory");
            out->data = file; out->n_bytes = G.file_bytes;
            memcpy(file, front.data(), front.size());
            uint8_t* bin = file + front.size();
            double ms_copy = 0.0;
            if (G.geometry_bytes) {
                const double t1 = now_ms_host();
                download(s, out, mvs_glb_free, [&] { MVS_HIP(hipMemcpyAsync(bin, D.geo.p, (size_t)G.geometry_bytes, hipMemcpyDeviceToHost, s)); });
                ms_copy = now_ms_host() - t1;
            }
            for (size_t a = 0; a < G.png.size(); ++a) {
                memcpy(bin + G.png_at[a], G.png[a].data(), G.png[a].size());
                memset(bin + G.png_at[a] + G.png[a].size(), 0, (size_t)((0 - G.png[a].size()) & 3u));
            }
            st.ms_download = (float)ms_copy; st.ms_file += (float)(now_ms_host() - t0 - ms_copy);
        });
    });
}

mvs_status mvs_ctx_save_glb(mvs_ctx* ctx, const mvs_atlas_set* atlases, int atlases_on_device, const float* vertex_normals, int normals_on_device,
                            const char* path, const mvs_model_params* params, mvs_glb_stats* stats) {
    if (!ctx || !atlases || !path) return api_fail(MVS_ERR_INVALID, "null argument");
    mvs_glb_stats st{};
    if (stats) *stats = st;
    return api_guard([&] {
        MVS_HIP(hipSetDevice(ctx->device));
        hipStream_t s = ctx->stream;
        GlbDev& D = row_dev(ctx->glb);
        const mvs_model_params P = params_or_default(params);
        run_with_stats(s, stats, st, [&] {
            GlbParts G;
            run_glb(ctx, D, *atlases, atlases_on_device, vertex_normals, normals_on_device, P, st, G, "save_glb");
            const double t0 = now_ms_host();
            const std::vector<uint8_t> front = glb_front(G);
            png_detail::File file(fopen(path, "wb"));
            FILE* f = file.get();
            if (!f) throw StatusError(MVS_ERR_INVALID, std::string("save_glb: cannot open ") + path);
            double ms_copy = 0.0;
            bool ok = fwrite(front.data(), 1, front.size(), f) == front.size();
            try {   // no partial file stays behind a failure
                if (ok) ok = device_to_stream(ctx, reinterpret_cast<const char*>(D.geo.p), G.geometry_bytes, f, ms_copy);
            } catch (...) { file.reset(); (void)remove(path); throw; }
            static const uint8_t zeros[4] = {0, 0, 0, 0};
            for (size_t a = 0; ok && a < G.png.size(); ++a) {
                const size_t n = G.png[a].size(), pad = (size_t)((0 - n) & 3u);
                ok = (!n || fwrite(G.png[a].data(), 1, n, f) == n) && (!pad || fwrite(zeros, 1, pad, f) == pad);
            }
            if (fclose(file.release()) != 0) ok = false;
            st.ms_download = (float)ms_copy; st.ms_file += (float)(now_ms_host() - t0 - ms_copy);
            if (!ok) { (void)remove(path); throw StatusError(MVS_ERR_INVALID, std::string("save_glb: write error on ") + path); }
        });
    });
}

mvs_status mvs_ctx_glb_quant_stats(mvs_ctx* ctx, mvs_glb_quant_stats* out) {
    if (!ctx || !out) return api_fail(MVS_ERR_INVALID, "null argument");
    *out = ctx->glb ? ctx->glb->quant_stats : mvs_glb_quant_stats{};
    return MVS_OK;
}

void mvs_glb_free(mvs_glb* g) {
    if (!g) return;
    free(g->data);
    *g = mvs_glb{};
}

}  // extern "C"
