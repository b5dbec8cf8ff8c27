// k_png.hip -- row f9's compressed PNG route on the device (DESIGN.md section 4 "Model output" item 7; the definition is png_rle.h, which
// the host twin shares).  All images of a call go through one set of launches on the context's stream:
//   filter   one wave per image row: the five filters' costs, the choice, the filtered row into the stream of its image
//   chunk    one workgroup per 32 KiB chunk of a stream.  The chunk sits in LDS, thread t owns bytes [128 t, 128 t + 128) (segments are
//            33 words apart: the threads' byte reads fall into different banks).  Per segment the repeating positions at its head and
//            tail; two scans over the 256 segments give every thread the repeats in front of and behind its segment, which is all
//            png_rle::walk_tokens needs to evaluate the token rule position by position.  Three walks: the histogram (LDS atomics), the
//            bits per thread (scanned to bit offsets), the emission (codes ORed into an LDS image of the output with LDS atomics: OR and
//            integer sums commute, the bytes do not depend on the order of the threads).  Between the first two the workgroup builds the
//            code with png_rle's functions; thread 0 builds and writes the header while the others count.  The image goes out with
//            16-byte stores into the chunk's slot of CHUNK + 16 bytes, beside its byte count and Adler sums.
//   gather   a 64-bit scan of the chunks' byte counts, then every chunk is copied behind its predecessors: one contiguous zlib stream per
//            image.  The two header bytes and the Adler-32 (combined from the chunks' sums) are written on the host, which also frames
//            the PNGs (signature, IHDR, IDAT with its CRC, IEND: png_io.h's routines on the compressed bytes).
#include "image_routes.h"
#include "png_rle.h"

namespace mvs {

using namespace png_rle;

struct PngDev {
    DBuf<uint8_t> in, filt, slots, zout;
    DBuf<uint32_t> f32, t32, sizes; DBuf<unsigned long long> f64, t64, off, rows; DBuf<uint4> meta;   // f*: the filter pass's tables, t*: the streams'
};
void png_release(mvs_ctx* ctx) { delete ctx->png; ctx->png = nullptr; }

namespace {
typedef unsigned long long u64;
constexpr uint32_t THREADS = 256;
constexpr uint32_t SEG = CHUNK / THREADS;          // bytes of a thread's segment
constexpr uint32_t SEG_PITCH = SEG + 4;            // ... and their distance in LDS
constexpr uint32_t SLOT = CHUNK + 16;              // bytes of a chunk's output slot: at most n + 10 are used
constexpr uint64_t STREAM_ALIGN = 256;             // streams start at multiples of this in the filtered buffer
static_assert(SEG * THREADS == CHUNK && SEG % 16 == 0 && SLOT % 16 == 0, "segments and slots are whole 16-byte pieces");

// ---- filter pass ----
struct Images { const uint32_t* row_ptr; const uint32_t* width; const u64* pix; const u64* off; uint32_t K; };   // row_ptr [K + 1]; pix: first pixel; off: first byte of the stream

__global__ void __launch_bounds__(64) png_filter_kernel(Images I, const uint8_t* __restrict__ image, uint8_t* __restrict__ filt, u64* __restrict__ rows) {
    const uint32_t r = blockIdx.x, lane = threadIdx.x;
    const uint32_t k = owner_of(I.row_ptr, I.K, r), y = r - I.row_ptr[k], w = I.width[k];
    const u64 rb = 3ull * w;
    const uint8_t* cur = image + 3ull * (I.pix[k] + (u64)y * w);
    const uint8_t* up = y ? cur - rb : nullptr;
    uint8_t* out = filt + I.off[k] + (u64)y * (rb + 1ull);
    u64 cost[5] = {0, 0, 0, 0, 0};
    for (u64 x = lane; x < rb; x += 64u) {
        const uint32_t a = x >= 3u ? cur[x - 3u] : 0u, b = up ? up[x] : 0u, c = (up && x >= 3u) ? up[x - 3u] : 0u, v = cur[x];
        for (uint32_t t = 0; t < 5u; ++t) cost[t] += residual_cost(residual(t, v, a, b, c));
    }
    for (uint32_t t = 0; t < 5u; ++t)
        for (int o = 32; o; o >>= 1) cost[t] += __shfl_xor(cost[t], o);
    const uint32_t t = best_filter(cost);
    if (lane == 0u) { out[0] = (uint8_t)t; atomicAdd(&rows[t], 1ull); }
    for (u64 x = lane; x < rb; x += 64u) {
        const uint32_t a = x >= 3u ? cur[x - 3u] : 0u, b = up ? up[x] : 0u, c = (up && x >= 3u) ? up[x - 3u] : 0u;
        out[1u + x] = (uint8_t)residual(t, cur[x], a, b, c);
    }
}

// ---- chunk pass ----
struct Streams { const uint32_t* chunk_ptr; const u64* off; const u64* len; uint32_t K; };   // chunk_ptr [K + 1]; off, len [K]: the stream's bytes in the filtered buffer

struct BlockPar {   // a workgroup as png_rle's Par
    template <class F> __device__ void each(uint32_t n, F&& f) const { for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) f(i); }
    __device__ void sync() const { __syncthreads(); }
    __device__ bool lead() const { return threadIdx.x == 0u; }
    __device__ void add(uint32_t* p, uint32_t v) const { atomicAdd(p, v); }
};
struct LdsSink {    // ... and its bit sink: an image of the output in LDS words
    uint32_t* w;
    __device__ void put(uint32_t bit, uint32_t v, uint32_t) const {
        const u64 x = (u64)v << (bit & 31u);
        if ((uint32_t)x) atomicOr(&w[bit >> 5], (uint32_t)x);
        if (x >> 32) atomicOr(&w[(bit >> 5) + 1u], (uint32_t)(x >> 32));
    }
};
struct ChunkLds {
    alignas(16) uint32_t in[THREADS * SEG_PITCH / 4];
    alignas(16) uint32_t out[SLOT / 4];
    uint32_t freq[NLIT + 2];
    uint32_t scan_a[THREADS], scan_b[THREADS];
    uint16_t code[NLIT + 2]; uint8_t len[NLIT + 2];
    HuffWork W; Header H;
    uint32_t has_match, adler_a, adler_b;
};
static_assert(sizeof(ChunkLds) <= 80 * 1024, "two workgroups per CU in 160 KiB of LDS");
constexpr uint32_t FULL = 0x80000000u;   // a segment summary: the count of repeating positions | FULL when every position of the segment repeats

__global__ void __launch_bounds__(THREADS) png_chunk_kernel(Streams S, const uint8_t* __restrict__ filt, uint8_t* __restrict__ slots, uint32_t* __restrict__ sizes,
                                                            uint4* __restrict__ meta) {
    extern __shared__ uint4 lds_raw[];
    ChunkLds& L = *reinterpret_cast<ChunkLds*>(lds_raw);
    const uint32_t tid = threadIdx.x, c = blockIdx.x;
    const uint32_t k = owner_of(S.chunk_ptr, S.K, c);
    const u64 at = (u64)(c - S.chunk_ptr[k]) * CHUNK, left = S.len[k] - at;
    const uint32_t n = left < CHUNK ? (uint32_t)left : CHUNK;
    const bool last = c + 1u == S.chunk_ptr[k + 1u];
    const uint4* src = reinterpret_cast<const uint4*>(filt + S.off[k] + at);   // 16-byte aligned; the buffer ends at least 16 bytes behind the stream
    for (uint32_t idx = tid; idx < CHUNK / 16u; idx += THREADS) {
        const uint32_t p = 16u * idx;
        if (p >= n) break;
        const uint4 v = src[idx];
        uint32_t* d = &L.in[((p / SEG) * SEG_PITCH + (p % SEG)) / 4u];
        d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
    }
    for (uint32_t idx = tid; idx < SLOT / 16u; idx += THREADS) reinterpret_cast<uint4*>(L.out)[idx] = make_uint4(0u, 0u, 0u, 0u);
    for (uint32_t i = tid; i < NLIT + 2u; i += THREADS) L.freq[i] = 0u;
    if (tid == 0u) { L.has_match = 0u; L.adler_a = 0u; L.adler_b = 0u; }
    __syncthreads();
    const uint8_t* in8 = reinterpret_cast<const uint8_t*>(L.in);
    auto B = [in8](uint32_t i) -> uint32_t { return in8[(i / SEG) * SEG_PITCH + (i % SEG)]; };
    const uint32_t begin = tid * SEG < n ? tid * SEG : n, end = begin + SEG < n ? begin + SEG : n, seg = end - begin;
    // ---- the repeats at the head and the tail of the segment, and across the segments ----
    auto rep = [&](uint32_t i) -> bool { return i > 0u && B(i) == B(i - 1u); };
    uint32_t head = 0;
    while (head < seg && rep(begin + head)) ++head;
    uint32_t tail = head;
    if (head < seg) { tail = 0; while (rep(end - 1u - tail)) ++tail; }
    const uint32_t full = head == seg ? FULL : 0u;
    L.scan_a[tid] = tail | full; L.scan_b[tid] = head | full;
    __syncthreads();
    for (uint32_t d = 1; d < THREADS; d <<= 1) {   // scan_a[t]: the repeats that end with segment t; scan_b[t]: those that start with it
        const uint32_t x = tid >= d ? L.scan_a[tid - d] : FULL, y = tid + d < THREADS ? L.scan_b[tid + d] : FULL;
        const uint32_t ma = L.scan_a[tid], mb = L.scan_b[tid];
        __syncthreads();
        L.scan_a[tid] = (ma & FULL) ? ((x & ma & FULL) | ((x & ~FULL) + (ma & ~FULL))) : ma;
        L.scan_b[tid] = (mb & FULL) ? ((y & mb & FULL) | ((y & ~FULL) + (mb & ~FULL))) : mb;
        __syncthreads();
    }
    const uint32_t before = tid ? L.scan_a[tid - 1u] & ~FULL : 0u, after = tid + 1u < THREADS ? L.scan_b[tid + 1u] & ~FULL : 0u;
    // ---- walk 1: the histogram ----
    walk_tokens(B, begin, end, before, after, [&](uint32_t q, uint32_t t) {
        if (t == 1u) { atomicAdd(&L.freq[B(q)], 1u); return; }
        uint32_t eb, ev;
        atomicAdd(&L.freq[length_symbol(t, eb, ev)], 1u);
        L.has_match = 1u;
    });
    if (tid == 0u) L.freq[EOB] = 1u;
    __syncthreads();
    const BlockPar par;
    huff_lengths(par, L.freq, NLIT, LIT_BITS, L.len, L.W);
    huff_codes(par, L.len, NLIT, LIT_BITS, L.code, L.W);
    LdsSink sink{L.out};
    // ---- walk 2: the bits of every thread's tokens, beside thread 0's header ----
    uint32_t bits = 0;
    if (tid == 0u) { build_header(L.len, L.has_match != 0u, L.H, L.W); emit_header(sink, L.H); }
    walk_tokens(B, begin, end, before, after, [&](uint32_t q, uint32_t t) { bits += token_bits(L.len, t, B(q)); });
    L.scan_a[tid] = bits;
    __syncthreads();
    for (uint32_t d = 1; d < THREADS; d <<= 1) {
        const uint32_t x = tid >= d ? L.scan_a[tid - d] : 0u;
        __syncthreads();
        L.scan_a[tid] += x;
        __syncthreads();
    }
    const uint32_t body = L.scan_a[THREADS - 1u], D = L.H.bits + body + L.len[EOB];
    const bool dynamic = use_dynamic(D, n);
    uint32_t bytes;
    if (dynamic) {   // ---- walk 3: the codes into the image ----
        uint32_t pos = L.H.bits + L.scan_a[tid] - bits;
        walk_tokens(B, begin, end, before, after, [&](uint32_t q, uint32_t t) { pos += token_put(sink, pos, L.len, L.code, t, B(q)); });
        bytes = (D + 3u + 7u) / 8u + 4u;
        if (tid == 0u) { sink.put(L.H.bits + body, L.code[EOB], L.len[EOB]); trailer_put(sink, D, last); }
    } else {         // ---- one stored block: the header's bits go away, the chunk's bytes follow 5 bytes of block header ----
        __syncthreads();
        for (uint32_t idx = tid; idx < SLOT / 16u; idx += THREADS) reinterpret_cast<uint4*>(L.out)[idx] = make_uint4(0u, 0u, 0u, 0u);
        __syncthreads();
        uint8_t* o8 = reinterpret_cast<uint8_t*>(L.out);
        for (uint32_t i = tid; i < n; i += THREADS) o8[5u + i] = (uint8_t)B(i);
        bytes = n + 10u;
        if (tid == 0u) {
            o8[1] = (uint8_t)n; o8[2] = (uint8_t)(n >> 8); o8[3] = (uint8_t)~n; o8[4] = (uint8_t)(~n >> 8);
            o8[5u + n] = last ? 1 : 0; o8[8u + n] = 0xFF; o8[9u + n] = 0xFF;
        }
    }
    // ---- the chunk's Adler sums ----
    uint32_t A; uint64_t Bs;
    adler_span(B, begin, end, A, Bs);
    if (seg) { atomicAdd(&L.adler_a, A); atomicAdd(&L.adler_b, (uint32_t)((Bs + (u64)A * (n - end)) % ADLER_MOD)); }
    __syncthreads();
    uint4* dst = reinterpret_cast<uint4*>(slots + (u64)c * SLOT);
    for (uint32_t idx = tid; idx < (bytes + 15u) / 16u; idx += THREADS) dst[idx] = reinterpret_cast<const uint4*>(L.out)[idx];
    if (tid == 0u) { sizes[c] = bytes; meta[c] = make_uint4(bytes, L.adler_a % ADLER_MOD, L.adler_b % ADLER_MOD, dynamic ? 0u : 1u); }
}

// the zlib streams of a call on the host: stream k is z[k] bytes at base + begin[k] of the context's pinned buffer
struct ZStreams { std::vector<uint64_t> begin, bytes; uint8_t* base = nullptr; uint64_t chunks = 0, stored = 0; };

// the chunk and gather passes over K streams of D.filt (off: multiples of STREAM_ALIGN, the buffer ends at least 16 bytes behind the last
// stream), the download and the streams' header and checksum.  Marks tm twice (behind the chunk pass, behind the gather pass: stream k
// starts 16 k bytes behind its chunks' offset, its first chunk 2 further); ms_copy += the host time of the downloads.
void run_streams(mvs_ctx* ctx, PngDev& D, const std::vector<uint64_t>& off, const std::vector<uint64_t>& len, ZStreams& Z, StageTimer<4>& tm, double& ms_copy) {
    hipStream_t s = ctx->stream;
    const uint32_t K = (uint32_t)off.size();
    std::vector<uint32_t> cptr((size_t)K + 1, 0u);
    uint64_t nc64 = 0, raw = 0;
    for (uint32_t k = 0; k < K; ++k) {
        const uint64_t nck = (len[k] + CHUNK - 1) / CHUNK;
        if (len[k] >= MAX_STREAM || 2 + len[k] + 10 * nck + 4 >= MAX_STREAM) throw StatusError(MVS_ERR_UNSUPPORTED, "png: stream too large for one IDAT chunk");
        nc64 += nck; raw += len[k];
        if (nc64 >= 0x7FFFFFFFull) throw StatusError(MVS_ERR_UNSUPPORTED, "png: too many chunks for one call");
        cptr[k + 1] = (uint32_t)nc64;
    }
    const uint32_t NC = (uint32_t)nc64;
    std::vector<u64> h64(2 * (size_t)K);
    for (uint32_t k = 0; k < K; ++k) { h64[k] = off[k]; h64[(size_t)K + k] = len[k]; }
    upload(D.t32, cptr, s); upload(D.t64, h64, s);
    const Streams S{D.t32.p, D.t64.p, D.t64.p + K, K};
    D.slots.ensure((size_t)NC * SLOT + 16); D.sizes.ensure((size_t)NC + 1); D.meta.ensure((size_t)NC + 1); D.off.ensure((size_t)NC + 1);
    D.zout.ensure((size_t)(raw + 10ull * NC + 16ull * K + 32));
    MVS_HIP(hipFuncSetAttribute((const void*)png_chunk_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(ChunkLds)));
    if (NC) {
        hipLaunchKernelGGL(png_chunk_kernel, dim3(NC), dim3(THREADS), sizeof(ChunkLds), s, S, (const uint8_t*)D.filt.p, D.slots.p, D.sizes.p, D.meta.p);
        MVS_LAUNCH_CHECK();
    }
    tm.mark();
    std::vector<uint4> h_meta(NC);   // the chunks' sizes and sums
    const std::vector<u64> h_off = pack_slots<16, 2>(ctx, D.t32.p, K, NC, SLOT, D.slots.p, D.sizes.p, D.off, D.zout.p, D.meta.p, h_meta.data(), (size_t)NC * sizeof(uint4), tm, ms_copy);
    Z.base = (uint8_t*)ctx->row_pin.p; Z.begin.resize(K); Z.bytes.resize(K); Z.chunks = NC; Z.stored = 0;
    for (uint32_t k = 0; k < K; ++k) {
        uint8_t* z = Z.base + h_off[cptr[k]] + 16ull * k;
        uint64_t body = h_off[cptr[k + 1]] - h_off[cptr[k]];
        z[0] = 0x78; z[1] = 0x01;
        if (cptr[k] == cptr[k + 1]) { const uint8_t fin[5] = {1, 0, 0, 0xFF, 0xFF}; memcpy(z + 2, fin, 5); body = 5; }   // the empty stream: the final trailer alone
        uint32_t adler = 1u;
        for (uint32_t c = cptr[k]; c < cptr[k + 1]; ++c) {
            const uint64_t n = std::min<uint64_t>(CHUNK, len[k] - (uint64_t)(c - cptr[k]) * CHUNK);
            adler = adler_append(adler, h_meta[c].y, h_meta[c].z, n);
            Z.stored += h_meta[c].w;
        }
        uint8_t* a = z + 2 + body;
        a[0] = (uint8_t)(adler >> 24); a[1] = (uint8_t)(adler >> 16); a[2] = (uint8_t)(adler >> 8); a[3] = (uint8_t)adler;
        Z.begin[k] = (uint64_t)(z - Z.base); Z.bytes[k] = 2 + body + 4;
    }
}

}  // namespace

// width, height [n], pix [n + 1]: host arrays, already checked against each other; image: 3 bytes per pixel, host or device
void png_encode_images(mvs_ctx* ctx, uint32_t n, const uint32_t* width, const uint32_t* height, const uint64_t* pix, const uint8_t* image, int image_on_device,
                       EncodedFiles& out, mvs_png_stats& st) {
    hipStream_t s = ctx->stream;
    PngDev& D = row_dev(ctx->png);
    std::string msg;
    std::vector<uint32_t> h32(2 * (size_t)n + 1, 0u);   // row_ptr [n + 1], width [n]
    std::vector<u64> h64(2 * (size_t)n);               // pix [n], off [n]
    std::vector<uint64_t> off(n), len(n);
    uint64_t rows = 0, at = 0;
    for (uint32_t k = 0; k < n; ++k) {
        const mvs_status rc = check_frame(width[k], height[k], msg);
        if (rc != MVS_OK) throw StatusError(rc, msg);
        rows += height[k];
        if (rows >= 0x7FFFFFFFull) throw StatusError(MVS_ERR_UNSUPPORTED, "encode_pngs: too many rows for one call");
        h32[k + 1] = (uint32_t)rows; h32[(size_t)n + 1 + k] = width[k];
        h64[k] = pix[k]; h64[(size_t)n + k] = at;
        off[k] = at; len[k] = (3ull * width[k] + 1ull) * height[k];
        at = (at + len[k] + STREAM_ALIGN - 1) / STREAM_ALIGN * STREAM_ALIGN;
    }
    st.raw_bytes = 0;
    for (uint32_t k = 0; k < n; ++k) st.raw_bytes += len[k];
    const uint8_t* d_image = stage(D.in, image, 3 * (size_t)pix[n], image_on_device, s);
    upload(D.f32, h32, s); upload(D.f64, h64, s);
    D.filt.ensure((size_t)at + STREAM_ALIGN); D.rows.ensure(5);
    StageTimer<4> tm(s);
    tm.mark();
    MVS_HIP(hipMemsetAsync(D.rows.p, 0, 5 * sizeof(u64), s));
    if (rows) {
        const Images I{D.f32.p, D.f32.p + n + 1, D.f64.p, D.f64.p + n, n};
        hipLaunchKernelGGL(png_filter_kernel, dim3((uint32_t)rows), dim3(64), 0, s, I, d_image, D.filt.p, D.rows.p);
        MVS_LAUNCH_CHECK();
    }
    tm.mark();
    ZStreams Z; double ms_copy = 0.0;
    u64 h_rows[5];
    MVS_HIP(hipMemcpyAsync(h_rows, D.rows.p, sizeof(h_rows), hipMemcpyDeviceToHost, s));
    run_streams(ctx, D, off, len, Z, tm, ms_copy);   // (its first drain of the stream completes the copy above and the uploads' host side)
    st.ms_filter = tm.ms(0, 1); st.ms_chunk = tm.ms(1, 2); st.ms_gather = tm.ms(2, 3); st.ms_download = (float)ms_copy;
    st.chunks = Z.chunks; st.stored_chunks = Z.stored;
    for (int t = 0; t < 5; ++t) st.filter_rows[t] = h_rows[t];
    // ---- the files ----
    const double t0 = now_ms_host();
    out.offsets.assign((size_t)n + 1, 0);
    for (uint32_t k = 0; k < n; ++k) out.offsets[k + 1] = out.offsets[k] + Z.bytes[k] + PNG_FRAME;
    out.resize_data();
    for_each_on_threads(n, [&](uint32_t k) { frame_png(out.data + out.offsets[k], width[k], height[k], Z.base + Z.begin[k], (size_t)Z.bytes[k]); });   // the CRC of the compressed bytes is the work
    st.png_bytes = out.offsets[n];
    st.ms_frame = (float)(now_ms_host() - t0);
}

}  // namespace mvs

using namespace mvs;

extern "C" {

mvs_status mvs_ctx_encode_pngs(mvs_ctx* ctx, uint32_t n_images, const uint32_t* width, const uint32_t* height, const uint64_t* pix_ptr, const uint8_t* image, int on_device,
                               mvs_png_set* out, mvs_png_stats* stats) {
    if (!ctx || !out || (n_images && (!width || !height)) || !pix_ptr) return api_fail(MVS_ERR_INVALID, "null argument");
    return encode_entry(ctx, n_images, width, height, pix_ptr, image, on_device, out, stats, "encode_pngs", [&](const ImageSet& S, EncodedFiles& F, mvs_png_stats& st) {
        png_encode_images(ctx, n_images, S.w.data(), S.h.data(), S.pix.data(), image, on_device, F, st);
    });
}

void mvs_png_set_free(mvs_png_set* p) {
    if (!p) return;
    free(p->data); free(p->offsets);
    *p = mvs_png_set{};
}

void mvs_png_free(uint8_t* bytes) { free(bytes); }

mvs_status mvs_ctx_deflate_rle(mvs_ctx* ctx, const uint8_t* bytes, uint64_t n, int on_device, uint8_t** out, uint64_t* out_bytes) {
    if (!ctx || !out || !out_bytes || (n && !bytes)) return api_fail(MVS_ERR_INVALID, "null argument");
    *out = nullptr; *out_bytes = 0;
    return api_guard([&] {
        MVS_HIP(hipSetDevice(ctx->device));
        hipStream_t s = ctx->stream;
        if (n >= MAX_STREAM) throw StatusError(MVS_ERR_UNSUPPORTED, "deflate_rle: stream too large for one IDAT chunk");
        PngDev& D = row_dev(ctx->png);
        D.filt.ensure((size_t)n + STREAM_ALIGN);
        if (n) MVS_HIP(hipMemcpyAsync(D.filt.p, bytes, (size_t)n, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));
        StageTimer<4> tm(s);
        ZStreams Z; double ms_copy = 0.0;
        try { run_streams(ctx, D, {0ull}, {n}, Z, tm, ms_copy); } catch (...) { (void)hipStreamSynchronize(s); throw; }
        uint8_t* z = (uint8_t*)malloc((size_t)Z.bytes[0]);
        if (!z) throw StatusError(MVS_ERR_INVALID, "out of host memory");
        memcpy(z, Z.base + Z.begin[0], (size_t)Z.bytes[0]);
        *out = z; *out_bytes = Z.bytes[0];
    });
}

mvs_status mvs_encode_png_rle(const uint8_t* rgb, uint32_t width, uint32_t height, uint8_t** out, uint64_t* out_bytes) {
    if (!out || !out_bytes) return api_fail(MVS_ERR_INVALID, "null argument");
    *out = nullptr; *out_bytes = 0;
    std::vector<uint8_t> v; std::string msg;
    return twin_out(encode_png_rle(rgb, width, height, v, msg), msg, v, out, out_bytes);
}

mvs_status mvs_deflate_rle(const uint8_t* bytes, uint64_t n, uint8_t** out, uint64_t* out_bytes) {
    if (!out || !out_bytes) return api_fail(MVS_ERR_INVALID, "null argument");
    *out = nullptr; *out_bytes = 0;
    std::vector<uint8_t> v; std::string msg;
    return twin_out(deflate_rle(bytes, n, v, msg), msg, v, out, out_bytes);
}

}  // extern "C"
