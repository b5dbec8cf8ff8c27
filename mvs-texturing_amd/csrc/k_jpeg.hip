// k_jpeg.hip -- the JPEG route of rows f9 and f11 on the device (DESIGN.md section 4 "Model output" item 9; the definition is jpeg_base.h,
// which the host twin shares).  All images of a call go through one set of launches on the context's stream:
//   segment  one workgroup per restart segment (R = 8 MCUs).  The pixel rows of its MCUs come into LDS with aligned 16-byte loads; a thread
//            per sample does colour and subsampling, a thread per value each of the two DCT passes (the cosine table sits in LDS, rows 9
//            words apart) and the quantiser, which leaves the coefficients in zig-zag order, blocks 33 words apart.  Then one wave per
//            block, a lane per coefficient: the ballot of the non-zero lanes gives every lane its run of zeros, a wave scan the bit offset
//            of its code inside the block; the DC difference reads the previous block of the same component out of LDS.  One wave scans
//            the blocks' bits (at most 48), and every lane ORs its codes into a zeroed LDS image of the output (LDS atomics: OR and
//            integer sums commute, the bytes do not depend on the order of the threads).  Thread t then owns a run of the image's bytes:
//            their 0xFF count, a workgroup scan, and the stuffed bytes -- with the RST marker behind them -- into the LDS that pixels and
//            coefficients no longer need; 16-byte stores take them to the segment's slot, beside its byte count.
//   gather   a 64-bit scan of the sizes, then every segment is copied behind its predecessors: the entropy data of all images, back to
//            back.  SOI .. SOS and EOI are written on the host (jpeg_base.h's header()).
// Slots are sized by the worst case of R (segment_worst_bytes: 19 970 bytes at 4:2:0, 9 986 at 4:4:4, rounded up to 16): config 3's 88
// atlases are 15 968 segments at 4:2:0, 319 MB of slots for 98 MB of pixels (4:4:4: 63 872 segments, 639 MB) -- a measuring launch would run the whole transform twice.
#include "image_routes.h"
#include "jpeg_base.h"

namespace mvs {

using namespace jpeg_base;

struct JpegDev {
    DBuf<uint8_t> in, slots, out;
    DBuf<uint32_t> t32, sizes, tables; DBuf<unsigned long long> t64, off, stuffed;
};
void jpeg_release(mvs_ctx* ctx) { delete ctx->jpeg; ctx->jpeg = nullptr; }

namespace {
typedef unsigned long long u64;
constexpr uint32_t THREADS = 256, WAVES = THREADS / 64;
constexpr uint32_t COEF_PITCH = 66;                                       // int16 per block: 33 words, so a lane per block would hit 32 banks as well
constexpr uint32_t PIX_BYTES = R * 16 * 16 * 3;                           // 6144
constexpr uint32_t SMP_BYTES = MAX_BLOCKS * 64;                           // 3072 (int8)
constexpr uint32_t TMP_BYTES = MAX_BLOCKS * 64 * 2;                       // 6144 (int16: pass 1, then the lanes' bit offsets)
constexpr uint32_t COEF_BYTES = MAX_BLOCKS * COEF_PITCH * 2;              // 6336 (int16)
constexpr uint32_t WORK_BYTES = PIX_BYTES + SMP_BYTES + TMP_BYTES + COEF_BYTES;   // 21696
constexpr uint32_t IMAGE_WORDS = MAX_BLOCKS * BLOCK_BYTES / 4 + 2;        // the unstuffed output and the word a code may reach into
constexpr uint32_t STUFFED_MAX = MAX_BLOCKS * BLOCK_BYTES * 2 + 2;        // 19970
static_assert((STUFFED_MAX + 15) / 16 * 16 <= WORK_BYTES, "the stuffed bytes reuse the pixels' and coefficients' LDS");
static_assert(STUFFED_MAX == R * MAX_MCU_BLOCKS * BLOCK_BYTES * 2 + 2, "segment_worst_bytes(1)");
inline uint32_t slot_bytes(uint32_t sub) { return (segment_worst_bytes(sub) + 15u) / 16u * 16u; }

struct SegLds {
    alignas(16) uint8_t work[WORK_BYTES];   // pixels | samples | pass 1 | coefficients; later the stuffed bytes
    alignas(16) uint32_t image[IMAGE_WORDS];
    Tables T;
    uint32_t scan[THREADS];
    uint32_t block_bits[64], block_off[64];
    uint32_t mcu_nx[R];
    uint32_t total_bits;
};
static_assert(sizeof(SegLds) <= 40 * 1024, "four workgroups per CU in 160 KiB of LDS");

struct Segs { const uint32_t* seg_ptr; const uint32_t* width; const uint32_t* height; const u64* pix; uint32_t K, sub, slot; };   // seg_ptr [K + 1]; pix: first pixel

__device__ void lds_put(uint32_t* w, uint32_t pos, uint32_t bits, uint32_t n) {
    uint32_t hi, lo;
    put_words(pos, bits, n, hi, lo);
    if (hi) atomicOr(&w[pos >> 5], hi);
    if (lo) atomicOr(&w[(pos >> 5) + 1u], lo);
}

// what lane `lane` of the wave that codes block b emits: `zrl` ZRL codes, then `bits` of `n` bits, then (lane 63 alone) EOB
struct LaneCode { uint32_t zrl, bits, n; bool eob; };
__device__ LaneCode lane_code(const SegLds& L, const int16_t* coef, uint32_t sub, uint32_t b, uint32_t t, uint32_t lane) {
    int32_t v = coef[b * COEF_PITCH + lane];
    if (lane == 0u) { const int pb = prev_block(sub, b); if (pb >= 0) v -= coef[(uint32_t)pb * COEF_PITCH]; }
    const u64 nz = __ballot(lane == 0u || v != 0);
    LaneCode c{0u, 0u, 0u, false};
    if (lane == 0u) dc_symbol(L.T, t, v, c.bits, c.n);
    else if (v != 0) {
        const u64 below = nz & ((1ull << lane) - 1ull);          // bit 0 is set: the DC lane
        const uint32_t run = lane - 1u - (63u - (uint32_t)__clzll((long long)below));
        c.zrl = run >> 4;
        ac_symbol(L.T, t, run & 15u, v, c.bits, c.n);
    }
    c.eob = lane == 63u && v == 0;                               // the last coefficient is zero: the block ends with EOB
    return c;
}

__global__ void __launch_bounds__(THREADS) jpeg_segment_kernel(Segs S, const uint8_t* __restrict__ image, const uint32_t* __restrict__ tables, uint8_t* __restrict__ slots,
                                                               uint32_t* __restrict__ sizes, u64* __restrict__ stuffed) {
    extern __shared__ uint4 lds_raw[];
    SegLds& L = *reinterpret_cast<SegLds*>(lds_raw);
    uint8_t* pixels = L.work;
    int8_t* smp = reinterpret_cast<int8_t*>(L.work + PIX_BYTES);
    int16_t* tmp = reinterpret_cast<int16_t*>(L.work + PIX_BYTES + SMP_BYTES);
    int16_t* coef = reinterpret_cast<int16_t*>(L.work + PIX_BYTES + SMP_BYTES + TMP_BYTES);
    const uint32_t tid = threadIdx.x, c = blockIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t k = owner_of(S.seg_ptr, S.K, c), si = c - S.seg_ptr[k];
    const uint32_t w = S.width[k], h = S.height[k], sub = S.sub, B = mcu_blocks(sub), lg = mcu_shift(sub), M = 1u << lg;
    const uint32_t mw = (w + M - 1u) >> lg, mh = (h + M - 1u) >> lg, total = mw * mh, m0 = si * R;
    const uint32_t nm = total - m0 < R ? total - m0 : R, nb = nm * B;
    const bool last = c + 1u == S.seg_ptr[k + 1u];
    for (uint32_t i = tid; i < sizeof(Tables) / 4u; i += THREADS) reinterpret_cast<uint32_t*>(&L.T)[i] = tables[i];
    for (uint32_t i = tid; i < IMAGE_WORDS; i += THREADS) L.image[i] = 0u;
    if (tid < nm) { const uint32_t x0 = ((m0 + tid) % mw) << lg; L.mcu_nx[tid] = w - x0 < M ? w - x0 : M; }
    // ---- the pixel rows of the MCUs: four lanes per row, each an aligned 16-byte piece of the image (a piece that holds one byte of the
    //      image lies in the image's pages); rows below the image repeat its last row here, columns right of it when they are read ----
    const uint8_t* base = image + 3ull * S.pix[k];
    for (uint32_t item = tid; item < (nm << lg) * 4u; item += THREADS) {
        const uint32_t row = item >> 2, q = item & 3u, j = row >> lg, y = row & (M - 1u), m = m0 + j;
        const uint32_t x0 = (m % mw) << lg, gy0 = ((m / mw) << lg) + y, gy = gy0 < h ? gy0 : h - 1u, nx = w - x0 < M ? w - x0 : M;
        const uint8_t* a = base + 3ull * ((u64)gy * w + x0);
        const uintptr_t lo = (uintptr_t)a, hi = lo + 3u * nx, g = (lo & ~(uintptr_t)15) + 16u * q;
        if (g >= hi) continue;
        const uint4 v = *reinterpret_cast<const uint4*>(g);
        const uint32_t word[4] = {v.x, v.y, v.z, v.w};
        uint8_t* d = pixels + (size_t)row * (3u * M);
        for (uint32_t i = 0; i < 16u; ++i) {
            const uintptr_t p = g + i;
            if (p >= lo && p < hi) d[p - lo] = (uint8_t)(word[i >> 2] >> (8u * (i & 3u)));
        }
    }
    __syncthreads();
    // ---- colour and subsampling: a thread per sample ----
    for (uint32_t i = tid; i < nb * 64u; i += THREADS) {
        const uint32_t b = i >> 6, p = i & 63u, j = b / B, bi = b - j * B, nx = L.mcu_nx[j];
        const uint8_t* mp = pixels + (size_t)j * (3u * M * M);
        auto px = [&](uint32_t x, uint32_t y, uint32_t ch) -> int32_t { return mp[(y * M + (x < nx ? x : nx - 1u)) * 3u + ch]; };
        smp[i] = (int8_t)mcu_sample(px, sub, bi, p & 7u, p >> 3);
    }
    __syncthreads();
    // ---- the two passes and the quantiser: a thread per value ----
    for (uint32_t i = tid; i < nb * 64u; i += THREADS) {
        const int8_t* s = smp + (i & ~7u);
        tmp[i] = (int16_t)dct_round1(dct_sum(&L.T.cosine[(i & 7u) * COS_PITCH], [&](uint32_t x) -> int32_t { return s[x]; }));
    }
    __syncthreads();
    for (uint32_t i = tid; i < nb * 64u; i += THREADS) {
        const uint32_t b = i >> 6, p = i & 63u, bi = b % B;
        const int16_t* t = tmp + (i & ~63u) + (p & 7u);
        const int32_t f = dct_round2(dct_sum(&L.T.cosine[(p >> 3) * COS_PITCH], [&](uint32_t y) -> int32_t { return t[8u * y]; }));
        coef[b * COEF_PITCH + L.T.zz_pos[p]] = (int16_t)quantise(f, L.T.quant[block_table(sub, bi)][p], p != 0u);
    }
    __syncthreads();
    // ---- the bits of every block: a wave per block, a lane per coefficient; tmp takes the lanes' offsets inside the block ----
    uint16_t* lane_off = reinterpret_cast<uint16_t*>(tmp);
    for (uint32_t b = wave; b < nb; b += WAVES) {
        const uint32_t t = block_table(sub, b % B);
        const LaneCode lc = lane_code(L, coef, sub, b, t, lane);
        const uint32_t mine = lc.zrl * (L.T.ac[t][ZRL] >> 16) + lc.n + (lc.eob ? L.T.ac[t][EOB] >> 16 : 0u);
        uint32_t incl = mine;
        for (uint32_t d = 1; d < 64u; d <<= 1) { const uint32_t x = __shfl_up(incl, d); if (lane >= d) incl += x; }
        lane_off[b * 64u + lane] = (uint16_t)(incl - mine);
        if (lane == 63u) L.block_bits[b] = incl;
    }
    __syncthreads();
    if (wave == 0u) {   // the blocks' offsets: at most 48 of them
        const uint32_t mine = lane < nb ? L.block_bits[lane] : 0u;
        uint32_t incl = mine;
        for (uint32_t d = 1; d < 64u; d <<= 1) { const uint32_t x = __shfl_up(incl, d); if (lane >= d) incl += x; }
        L.block_off[lane] = incl - mine;
        if (lane == 63u) L.total_bits = incl;
    }
    __syncthreads();
    // ---- the codes into the image ----
    for (uint32_t b = wave; b < nb; b += WAVES) {
        const uint32_t t = block_table(sub, b % B);
        const LaneCode lc = lane_code(L, coef, sub, b, t, lane);
        uint32_t pos = L.block_off[b] + lane_off[b * 64u + lane];
        const uint32_t zrl = L.T.ac[t][ZRL], eob = L.T.ac[t][EOB];
        for (uint32_t z = 0; z < lc.zrl; ++z) { lds_put(L.image, pos, zrl & 0xFFFFu, zrl >> 16); pos += zrl >> 16; }
        lds_put(L.image, pos, lc.bits, lc.n);
        if (lc.eob) lds_put(L.image, pos + lc.n, eob & 0xFFFFu, eob >> 16);
    }
    const uint32_t bits = L.total_bits, pad = (8u - (bits & 7u)) & 7u, nbytes = (bits + pad) >> 3;
    if (tid == 0u) lds_put(L.image, bits, (1u << pad) - 1u, pad);
    __syncthreads();   // (pixels, samples and coefficients are dead from here on)
    // ---- stuffing: thread t owns bytes [t per, t per + per) of the image ----
    const uint32_t per = (nbytes + THREADS - 1u) / THREADS, begin = tid * per < nbytes ? tid * per : nbytes, end = begin + per < nbytes ? begin + per : nbytes;
    uint32_t ff = 0;
    for (uint32_t i = begin; i < end; ++i) ff += image_byte(L.image, i) == 0xFFu ? 1u : 0u;
    L.scan[tid] = ff;
    __syncthreads();
    for (uint32_t d = 1; d < THREADS; d <<= 1) {
        const uint32_t x = tid >= d ? L.scan[tid - d] : 0u;
        __syncthreads();
        L.scan[tid] += x;
        __syncthreads();
    }
    const uint32_t all_ff = L.scan[THREADS - 1u];
    uint8_t* out8 = L.work;
    uint32_t o = begin + L.scan[tid] - ff;
    for (uint32_t i = begin; i < end; ++i) {
        const uint32_t v = image_byte(L.image, i);
        out8[o++] = (uint8_t)v;
        if (v == 0xFFu) out8[o++] = 0u;
    }
    uint32_t bytes = nbytes + all_ff;
    if (!last) {
        if (tid == 0u) { out8[bytes] = 0xFFu; out8[bytes + 1u] = (uint8_t)(0xD0u + (si & 7u)); }
        bytes += 2u;
    }
    __syncthreads();
    uint4* dst = reinterpret_cast<uint4*>(slots + (u64)c * S.slot);
    for (uint32_t idx = tid; idx < (bytes + 15u) / 16u; idx += THREADS) dst[idx] = reinterpret_cast<const uint4*>(L.work)[idx];
    if (tid == 0u) { sizes[c] = bytes; if (all_ff) atomicAdd(stuffed, (u64)all_ff); }
}

}  // namespace

// width, height [n], pix [n + 1]: host arrays, already checked against each other; image: 3 bytes per pixel, host or device
void jpeg_encode_images(mvs_ctx* ctx, uint32_t n, const uint32_t* width, const uint32_t* height, const uint64_t* pix, const uint8_t* image, int image_on_device,
                        int quality, int subsampling, EncodedFiles& out, mvs_jpeg_stats& st) {
    hipStream_t s = ctx->stream;
    JpegDev& D = row_dev(ctx->jpeg);
    std::string msg;
    mvs_status rc = check_params(quality, subsampling, msg);
    for (uint32_t k = 0; rc == MVS_OK && k < n; ++k) rc = check_frame(width[k], height[k], msg);
    if (rc != MVS_OK) throw StatusError(rc, msg);
    const uint32_t sub = (uint32_t)subsampling, lg = mcu_shift(sub), M = 1u << lg, slot = slot_bytes(sub);
    std::vector<uint32_t> h32(3 * (size_t)n + 1, 0u);   // seg_ptr [n + 1], width [n], height [n]
    std::vector<u64> h64(n);                            // pix [n]
    uint64_t nc64 = 0;
    for (uint32_t k = 0; k < n; ++k) {
        const uint64_t mcus = (uint64_t)((width[k] + M - 1u) >> lg) * ((height[k] + M - 1u) >> lg);
        nc64 += (mcus + R - 1u) / R;
        if (nc64 >= 0x7FFFFFFFull) throw StatusError(MVS_ERR_UNSUPPORTED, "encode_jpegs: too many segments for one call");
        h32[k + 1] = (uint32_t)nc64; h32[(size_t)n + 1 + k] = width[k]; h32[2 * (size_t)n + 1 + k] = height[k];
        h64[k] = pix[k];
    }
    const uint32_t NC = (uint32_t)nc64;
    Tables T;
    build_tables(quality, T);
    st.raw_bytes = 3ull * pix[n]; st.segments = NC;
    const uint8_t* d_image = stage(D.in, image, 3 * (size_t)pix[n], image_on_device, s);
    upload(D.t32, h32, s); upload(D.t64, h64, s);
    upload(D.tables, reinterpret_cast<const uint32_t*>(&T), sizeof(Tables) / 4, s);
    D.slots.ensure((size_t)NC * slot + 16); D.sizes.ensure((size_t)NC + 1); D.off.ensure((size_t)NC + 1); D.stuffed.ensure(1);
    D.out.ensure((size_t)NC * segment_worst_bytes(sub) + 32);
    const Segs S{D.t32.p, D.t32.p + n + 1, D.t32.p + 2 * (size_t)n + 1, D.t64.p, n, sub, slot};
    MVS_HIP(hipFuncSetAttribute((const void*)jpeg_segment_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(SegLds)));
    StageTimer<3> tm(s);
    tm.mark();
    MVS_HIP(hipMemsetAsync(D.stuffed.p, 0, sizeof(u64), s));
    if (NC) {
        hipLaunchKernelGGL(jpeg_segment_kernel, dim3(NC), dim3(THREADS), sizeof(SegLds), s, S, d_image, (const uint32_t*)D.tables.p, D.slots.p, D.sizes.p, D.stuffed.p);
        MVS_LAUNCH_CHECK();
    }
    tm.mark();
    // ---- gather: the entropy data of all images, back to back ----
    double ms_copy = 0.0;
    const std::vector<u64> h_off = pack_slots<0, 0>(ctx, nullptr, n, NC, slot, D.slots.p, D.sizes.p, D.off, D.out.p, D.stuffed.p, &st.stuffed_bytes, sizeof(u64), tm, ms_copy);
    st.ms_segment = tm.ms(0, 1); st.ms_gather = tm.ms(1, 2); st.ms_download = (float)ms_copy;
    // ---- the files: SOI .. SOS, the image's entropy data, EOI ----
    const double t1 = now_ms_host();
    out.offsets.assign((size_t)n + 1, 0);
    for (uint32_t k = 0; k < n; ++k) out.offsets[k + 1] = out.offsets[k] + HEADER_BYTES + (h_off[h32[k + 1]] - h_off[h32[k]]) + 2u;
    out.resize_data();
    std::vector<uint8_t> head;
    for (uint32_t k = 0; k < n; ++k) {
        head.clear();
        header(width[k], height[k], sub, T, head);
        if (head.size() != HEADER_BYTES) throw StatusError(MVS_ERR_INVALID, "encode_jpegs: header size");
        uint8_t* f = out.data + out.offsets[k];
        const size_t body = (size_t)(h_off[h32[k + 1]] - h_off[h32[k]]);
        memcpy(f, head.data(), HEADER_BYTES);
        memcpy(f + HEADER_BYTES, ctx->row_pin.p + h_off[h32[k]], body);
        f[HEADER_BYTES + body] = 0xFF; f[HEADER_BYTES + body + 1] = 0xD9;
    }
    st.jpeg_bytes = out.offsets[n];
    st.marker_bytes = (uint64_t)n * (HEADER_BYTES + 2u) + 2ull * (NC - n);
    st.ms_frame = (float)(now_ms_host() - t1);
}

}  // namespace mvs

using namespace mvs;

extern "C" {

mvs_status mvs_ctx_encode_jpegs(mvs_ctx* ctx, uint32_t n_images, const uint32_t* width, const uint32_t* height, const uint64_t* pix_ptr, const uint8_t* image, int on_device,
                                int32_t quality, int32_t subsampling, mvs_jpeg_set* out, mvs_jpeg_stats* stats) {
    if (!ctx || !out || (n_images && (!width || !height)) || !pix_ptr) return api_fail(MVS_ERR_INVALID, "null argument");
    return encode_entry(ctx, n_images, width, height, pix_ptr, image, on_device, out, stats, "encode_jpegs", [&](const ImageSet& S, EncodedFiles& F, mvs_jpeg_stats& st) {
        jpeg_encode_images(ctx, n_images, S.w.data(), S.h.data(), S.pix.data(), image, on_device, quality, subsampling, F, st);
    });
}

void mvs_jpeg_set_free(mvs_jpeg_set* p) { mvs_png_set_free(p); }

void mvs_jpeg_free(uint8_t* bytes) { free(bytes); }

mvs_status mvs_encode_jpeg(const uint8_t* rgb, uint32_t width, uint32_t height, int32_t quality, int32_t subsampling, uint8_t** out, uint64_t* out_bytes) {
    if (!out || !out_bytes) return api_fail(MVS_ERR_INVALID, "null argument");
    *out = nullptr; *out_bytes = 0;
    std::vector<uint8_t> v; std::string msg;
    return twin_out(encode_jpeg(rgb, width, height, quality, subsampling, v, msg), msg, v, out, out_bytes);
}

}  // extern "C"
