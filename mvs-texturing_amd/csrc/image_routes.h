// image_routes.h -- what the image routes of rows f9 and f11 share (k_png.hip, k_jpeg.hip and their caller in k_model.hip): the files a route
//   leaves and their hand-over to the ABI, the reader / checker of an image set, the two encoder entry points' body, the host twins'
//   hand-over, and the pass that follows a route's coding pass -- the units' slots packed behind each other and brought to the host
//   (DESIGN.md section 4 "Shared plumbing").  Internal, header-only.
#pragma once
#include "rows.h"

namespace mvs {

// ---- the finished files of a call: file i is data[offsets[i], offsets[i + 1]) ----
struct EncodedFiles {
    uint8_t* data = nullptr; std::vector<uint64_t> offsets;
    EncodedFiles() = default;
    EncodedFiles(const EncodedFiles&) = delete;
    EncodedFiles& operator=(const EncodedFiles&) = delete;
    ~EncodedFiles() { free(data); }
    void resize_data() {   // room for offsets.back() bytes
        free(data);
        data = (uint8_t*)malloc(std::max<size_t>((size_t)offsets.back(), 1));
        if (!data) throw StatusError(MVS_ERR_INVALID, "out of host memory");
    }
};
// k_png.hip / k_jpeg.hip: the files of n images encoded on the device (the entry points after their checks: width, height [n] and pix [n + 1]
// are host arrays that agree, image is 3 bytes per pixel on the host or the device).  JPEG: quality and subsampling are checked again by
// jpeg_base.h's check_params; a side above 65535 throws MVS_ERR_UNSUPPORTED.
void png_encode_images(mvs_ctx* ctx, uint32_t n, const uint32_t* width, const uint32_t* height, const uint64_t* pix, const uint8_t* image, int image_on_device,
                       EncodedFiles& out, mvs_png_stats& st);
void jpeg_encode_images(mvs_ctx* ctx, uint32_t n, const uint32_t* width, const uint32_t* height, const uint64_t* pix, const uint8_t* image, int image_on_device,
                        int quality, int subsampling, EncodedFiles& out, mvs_jpeg_stats& st);

// F's n files as the ABI's set (mvs_png_set_free releases it): the bytes move, the offsets are copied
inline void files_to_set(EncodedFiles& F, uint32_t n, mvs_png_set* out) {
    out->offsets = (uint64_t*)malloc(((size_t)n + 1) * sizeof(uint64_t));
    if (!out->offsets) throw StatusError(MVS_ERR_INVALID, "out of host memory");
    memcpy(out->offsets, F.offsets.data(), ((size_t)n + 1) * sizeof(uint64_t));
    out->n_images = n; out->n_bytes = F.offsets[n]; out->data = F.data; F.data = nullptr;
}

// what a host twin made (status, message, bytes) as its entry point returns it: a malloc'ed copy for mvs_png_free / mvs_jpeg_free
inline mvs_status twin_out(mvs_status st, const std::string& msg, const std::vector<uint8_t>& v, uint8_t** out, uint64_t* out_bytes) {
    if (st != MVS_OK) return api_fail(st, msg);
    uint8_t* p = (uint8_t*)malloc(std::max<size_t>(v.size(), 1));
    if (!p) return api_fail(MVS_ERR_INVALID, "out of host memory");
    if (!v.empty()) memcpy(p, v.data(), v.size());
    *out = p; *out_bytes = v.size();
    return MVS_OK;
}

// ---- an image set's per-image arrays on the host ----
struct ImageSet { std::vector<uint32_t> w, h; std::vector<uint64_t> pix; };   // [n], [n], [n + 1]
// width, height [n], pix_ptr [n + 1] from the host or (in one drain of the stream) the device; an atlas set gives ONE array for both
// sides, which is read once
inline ImageSet read_image_arrays(mvs_ctx* ctx, uint32_t n, const uint32_t* width, const uint32_t* height, const uint64_t* pix_ptr, int on_device) {
    ImageSet S{std::vector<uint32_t>(n), std::vector<uint32_t>(n), std::vector<uint64_t>((size_t)n + 1)};
    const bool square = height == width;
    const struct { void* dst; const void* src; size_t bytes; } part[3] = {{S.w.data(), width, n * sizeof(uint32_t)}, {S.h.data(), height, square ? 0 : n * sizeof(uint32_t)},
                                                                          {S.pix.data(), pix_ptr, ((size_t)n + 1) * sizeof(uint64_t)}};
    for (const auto& q : part) {
        if (!q.bytes) continue;
        if (on_device) MVS_HIP(hipMemcpyAsync(q.dst, q.src, q.bytes, hipMemcpyDeviceToHost, ctx->stream));
        else memcpy(q.dst, q.src, q.bytes);
    }
    if (on_device) MVS_HIP(hipStreamSynchronize(ctx->stream));
    if (square) S.h = S.w;
    return S;
}
// the rules of the encoder entry points: pix starts at 0, no empty frame, every image's pix range is its width x height.  Throws
// MVS_ERR_INVALID, `who` in front.
inline void check_image_set(const ImageSet& S, const char* who) {
    const std::string w = std::string(who) + ": ";
    if (S.pix[0] != 0) throw StatusError(MVS_ERR_INVALID, w + "pix_ptr does not start at 0");
    for (size_t k = 0; k < S.w.size(); ++k)
        if (!S.w[k] || !S.h[k] || S.pix[k + 1] < S.pix[k] || S.pix[k + 1] - S.pix[k] != (uint64_t)S.w[k] * S.h[k])
            throw StatusError(MVS_ERR_INVALID, w + "image " + std::to_string(k) + ": width, height and pix_ptr do not agree");
}
inline ImageSet read_image_set(mvs_ctx* ctx, uint32_t n, const uint32_t* width, const uint32_t* height, const uint64_t* pix_ptr, int on_device, const char* who) {
    ImageSet S = read_image_arrays(ctx, n, width, height, pix_ptr, on_device);
    check_image_set(S, who);
    return S;
}

// ---- the body of mvs_ctx_encode_pngs / mvs_ctx_encode_jpegs behind their null checks: route(S, F, st) encodes the checked set S into F ----
template <class Stats, class Route>
mvs_status encode_entry(mvs_ctx* ctx, uint32_t n, const uint32_t* width, const uint32_t* height, const uint64_t* pix_ptr, const uint8_t* image, int on_device,
                        mvs_png_set* out, Stats* stats, const char* who, Route&& route) {
    *out = mvs_png_set{};
    Stats st{};
    if (stats) *stats = st;
    return api_guard([&] {
        MVS_HIP(hipSetDevice(ctx->device));
        const ImageSet S = read_image_set(ctx, n, width, height, pix_ptr, on_device, who);
        if (S.pix[n] && !image) throw StatusError(MVS_ERR_INVALID, std::string(who) + ": null image");
        run_with_stats(ctx->stream, stats, st, [&] {
            EncodedFiles F;
            route(S, F, st);
            files_to_set(F, n, out);
        });
    });
}

// ---- the gather pass ----
// ptr [K + 1] ascending from 0: the k with ptr[k] <= i < ptr[k + 1]
__device__ inline uint32_t owner_of(const uint32_t* __restrict__ ptr, uint32_t K, uint32_t i) {
    uint32_t lo = 0, hi = K;
    while (hi - lo > 1u) { const uint32_t mid = lo + (hi - lo) / 2u; if (ptr[mid] <= i) lo = mid; else hi = mid; }
    return lo;
}

constexpr uint32_t GATHER_THREADS = 256;
// Slot c (sizes[c] bytes at slots + c * slot) goes behind its predecessors: off [NC + 1] is the scan of the sizes.  ROOM bytes are left in
// front of every image's slots and the image's first byte lies LEAD behind them (unit_ptr [K + 1]: the slots of image k), so slot c of
// image k lands at off[c] + ROOM k + LEAD.  PNG: <16, 2>, the zlib header in front and room for the Adler-32 behind; JPEG: <0, 0>, unit_ptr unread.
template <uint32_t ROOM, uint32_t LEAD>
__global__ void __launch_bounds__(GATHER_THREADS) gather_slots_kernel(const uint32_t* __restrict__ unit_ptr, uint32_t K, uint32_t slot, const uint8_t* __restrict__ slots,
                                                                      const uint32_t* __restrict__ sizes, const unsigned long long* __restrict__ off, uint8_t* __restrict__ out) {
    const uint32_t c = blockIdx.x, nb = sizes[c];
    const uint8_t* src = slots + (unsigned long long)c * slot;
    uint8_t* dst = out + off[c] + LEAD;
    if (ROOM) dst += (unsigned long long)ROOM * owner_of(unit_ptr, K, c);
    const uint32_t lead = (uint32_t)((16u - ((uintptr_t)dst & 15u)) & 15u), head = lead < nb ? lead : nb;   // bytes up to dst's first 16-byte boundary
    for (uint32_t i = threadIdx.x; i < head; i += GATHER_THREADS) dst[i] = src[i];
    const uint32_t words = (nb - head) / 16u;
    for (uint32_t i = threadIdx.x; i < words; i += GATHER_THREADS) {
        uint4 v;
        uint8_t* b = reinterpret_cast<uint8_t*>(&v);
        const uint8_t* s = src + head + 16u * i;
        for (int j = 0; j < 16; ++j) b[j] = s[j];
        reinterpret_cast<uint4*>(dst + head)[i] = v;
    }
    for (uint32_t i = head + 16u * words + threadIdx.x; i < nb; i += GATHER_THREADS) dst[i] = src[i];
}

// What follows a route's coding pass, which left slot c's bytes and sizes[c] for c < NC: the sentinel size zeroed, the scan into off
// [NC + 1], the gather into `out` (room for off[NC] + ROOM K bytes, and 16 more), ONE mark on tm, the stream drained; then off and the
// caller's meta_bytes at d_meta come to the host (h_meta), and the packed bytes into ctx->row_pin.  Returns the host offsets; ms_copy +=
// the host time of the copies alone.
template <uint32_t ROOM, uint32_t LEAD, int N>
std::vector<unsigned long long> pack_slots(mvs_ctx* ctx, const uint32_t* unit_ptr, uint32_t K, uint32_t NC, uint32_t slot, const uint8_t* slots, uint32_t* sizes,
                                           DBuf<unsigned long long>& off, uint8_t* out, const void* d_meta, void* h_meta, size_t meta_bytes, StageTimer<N>& tm, double& ms_copy) {
    typedef unsigned long long u64;
    hipStream_t s = ctx->stream;
    MVS_HIP(hipMemsetAsync(sizes + NC, 0, sizeof(uint32_t), s));
    dev_exclusive_scan(ctx, (const uint32_t*)sizes, off.p, (size_t)NC + 1);
    if (NC) {
        hipLaunchKernelGGL((gather_slots_kernel<ROOM, LEAD>), dim3(NC), dim3(GATHER_THREADS), 0, s, unit_ptr, K, slot, slots, (const uint32_t*)sizes, (const u64*)off.p, out);
        MVS_LAUNCH_CHECK();
    }
    tm.mark();
    MVS_HIP(hipStreamSynchronize(s));   // (so that ms_copy is the copies' time, not the passes')
    const double t0 = now_ms_host();
    const size_t b_off = ((size_t)NC + 1) * sizeof(u64);
    ctx->row_pin.ensure(b_off + meta_bytes + 16);
    MVS_HIP(hipMemcpyAsync(ctx->row_pin.p, off.p, b_off, hipMemcpyDeviceToHost, s));
    if (meta_bytes) MVS_HIP(hipMemcpyAsync(ctx->row_pin.p + b_off, d_meta, meta_bytes, hipMemcpyDeviceToHost, s));
    MVS_HIP(hipStreamSynchronize(s));
    std::vector<u64> h_off((const u64*)ctx->row_pin.p, (const u64*)ctx->row_pin.p + NC + 1);
    if (meta_bytes) memcpy(h_meta, ctx->row_pin.p + b_off, meta_bytes);
    const uint64_t total = h_off[NC] + (uint64_t)ROOM * K;
    ctx->row_pin.ensure((size_t)total + 16);
    if (total) MVS_HIP(hipMemcpyAsync(ctx->row_pin.p, out, (size_t)total, hipMemcpyDeviceToHost, s));
    MVS_HIP(hipStreamSynchronize(s));
    ms_copy += now_ms_host() - t0;
    return h_off;
}

}  // namespace mvs
