// k_lens.hip -- view input: lens undistortion on the device for pixel and JPEG views (DESIGN.md section 4 "View input"; lens.h states the
// arithmetic of row f4 once, for this file, for undistort_kernel of k_prep.hip and for the host twin).
//   The distorted image has to exist whole before it is sampled, so a view with dist0 != 0 goes to a STAGING buffer of the context --
//   host pixels through the pinned upload ring, a JPEG file decoded there by k_jpegdec.hip (decode_view_files) -- and ONE launch of
//   lens_kernel per batch writes the undistorted pixels of all the batch's views into their image buffers.  Staging is bounded by
//   mvs_jpegdec_params.max_scratch_bytes: the 3 w h bytes of a staged file count towards its scratch in the batch cut of the files,
//   pixel views are staged in groups that fit, and a view that does not fit alone is refused.  Views with dist0 == 0 never see staging.
//   lens_kernel: a lane makes 16 bytes of a destination image, aligned to it, and leaves them as one 16-byte store (the head and the tail
//   of an image go out by bytes).  The batch's chunks of 16 bytes are numbered through all views (chunk_ptr, a prefix array); a lane
//   finds its view by binary search, as colour_kernel of k_jpegdec.hip does.  16 bytes are 5 1/3 pixels: they touch at most 6, whose
//   source positions the lane evaluates, keeping only its own bytes -- 1.125 evaluations per pixel against undistort_kernel's one, for
//   one store per 16 bytes against three per pixel.
#include "rows.h"
#include "lens.h"

namespace mvs {

typedef unsigned long long u64;

namespace {

constexpr uint32_t THREADS = 256;
constexpr uint64_t DEFAULT_MAX_SCRATCH = 1ull << 30;   // mvs_jpegdec_default_params

// per view of a batch (host made)
struct LensView {
    const uint8_t* src;   // the distorted image
    uint8_t* dst;         // the undistorted one
    int32_t width, height;
    float flen, d0, d1;   // d0 == 0: a plain copy
    uint32_t pad_;
};

__global__ void __launch_bounds__(THREADS) lens_kernel(const LensView* __restrict__ views, uint32_t n, const u64* __restrict__ chunk_ptr, u64 n_chunks, u64* __restrict__ no_source) {
    const u64 g = (u64)blockIdx.x * THREADS + threadIdx.x;
    uint32_t none = 0;   // pixels without a source among those that START in this lane's bytes
    if (g < n_chunks) {
        uint32_t lo = 0, hi = n;
        while (hi - lo > 1u) { const uint32_t mid = lo + (hi - lo) / 2u; if (chunk_ptr[mid] <= g) lo = mid; else hi = mid; }
        const LensView V = views[lo];
        const u64 bytes = 3ull * (u64)V.width * (u64)V.height, lead = (u64)((uintptr_t)V.dst & 15u), q = g - chunk_ptr[lo];
        const u64 t0 = q * 16u < lead ? 0ull : q * 16u - lead, t1 = min(bytes, (q + 1u) * 16u - lead);   // the image's bytes [t0, t1) of this chunk
        const uint32_t len = (uint32_t)(t1 - t0);
        union { uint8_t b[16]; uint4 w; } o;
        if (V.d0 == 0.0f) {
#pragma unroll
            for (uint32_t s = 0; s < 16u; ++s) o.b[s] = s < len ? V.src[t0 + s] : (uint8_t)0;
        } else {
            // bytes [t0, t1) lie in the pixels p0 .. p0 + 5: m = t0 - 3 p0 < 3 and m + 16 <= 18
            const u64 p0 = t0 / 3u, p_end = (t1 + 2u) / 3u;
            const uint32_t m = (uint32_t)(t0 - 3u * p0);
            const double flen = (double)V.flen, d0 = (double)V.d0, d1 = (double)V.d1;
            int x = (int)(p0 % (u64)V.width), y = (int)(p0 / (u64)V.width);
            uint8_t px[18];
#pragma unroll
            for (uint32_t j = 0; j < 6u; ++j) {
                uint8_t rgb[3] = {0, 0, 0};
                if (p0 + j < p_end) {
                    const bool ok = lens_pixel(V.src, V.width, V.height, x, y, flen, d0, d1, rgb);
                    if (!ok && 3u * j >= m) ++none;
                    if (++x == V.width) { x = 0; ++y; }
                }
                px[3u * j] = rgb[0]; px[3u * j + 1u] = rgb[1]; px[3u * j + 2u] = rgb[2];
            }
#pragma unroll
            for (uint32_t s = 0; s < 16u; ++s) o.b[s] = m == 0u ? px[s] : m == 1u ? px[s + 1u] : px[s + 2u];
        }
        if (len == 16u) *reinterpret_cast<uint4*>(V.dst + t0) = o.w;
        else for (uint32_t s = 0; s < len; ++s) V.dst[t0 + s] = o.b[s];
    }
    // one atomic per wave that found any (every lane of the block arrives here)
    for (int d = warpSize / 2; d > 0; d >>= 1) none += __shfl_xor(none, d);
    if (none && (threadIdx.x & (warpSize - 1)) == 0) atomicAdd(no_source, (u64)none);
}

// View masks under a lens: keep words (mask_stride words per row, bit b of word wx = pixel 32 wx + b, bits beyond the width zero) from the
// staged byte mask in the camera's frame.  A lane evaluates lens.h lens_keep for ONE destination pixel; 32 consecutive lanes are the 32
// bit positions of one word (positions beyond the width evaluate nothing), so a wave's ballot is two finished words.  The batch's words
// are numbered through all views (word_ptr, a prefix array), as lens_kernel numbers its chunks.
__global__ void __launch_bounds__(THREADS) lens_mask_kernel(const LensMaskView* __restrict__ views, uint32_t n, const u64* __restrict__ word_ptr, u64 n_words) {
    const u64 g = ((u64)blockIdx.x * THREADS + threadIdx.x) >> 5;   // the word; THREADS and the wave are multiples of 32
    const int b = (int)(threadIdx.x & 31u);
    bool keep = false;
    uint32_t* dst = nullptr;
    __shared__ uint32_t s_lo;   // the view of the block's first word, searched once per block (k_viewmask.hip mask_pack_kernel)
    if (threadIdx.x == 0) {
        const u64 g0 = ((u64)blockIdx.x * THREADS) >> 5;   // < n_words: the grid has no empty block
        uint32_t lo = 0, hi = n;
        while (hi - lo > 1u) { const uint32_t mid = lo + (hi - lo) / 2u; if (word_ptr[mid] <= g0) lo = mid; else hi = mid; }
        s_lo = lo;
    }
    __syncthreads();
    if (g < n_words) {
        uint32_t lo = s_lo;
        while (word_ptr[lo + 1] <= g) ++lo;                // g < n_words = word_ptr[n]: ends at lo <= n - 1
        const LensMaskView V = views[lo];
        const u64 q = g - word_ptr[lo];
        const uint32_t wpr = ((uint32_t)V.width + 31u) / 32u;
        const uint32_t yq = (q >> 32) ? (uint32_t)(q / wpr) : (uint32_t)q / wpr;
        const int y = (int)yq, x = 32 * (int)(uint32_t)(q - (u64)yq * wpr) + b;
        if (x < V.width) keep = lens_keep(V.src, V.width, V.height, x, y, (double)V.flen, (double)V.d0, (double)V.d1);
        dst = V.keep + q;
    }
    const u64 kept = __ballot(keep);
    if (dst && b == 0) *dst = (uint32_t)(kept >> (threadIdx.x & 32u));
}

uint64_t align16(uint64_t v) { return (v + 15u) & ~15ull; }

}  // namespace

// per-context buffers of the route, allocated on first use
struct LensDev { DBuf<uint8_t> staging, out; DBuf<LensView> table; DBuf<u64> chunk_ptr, words; DBuf<LensMaskView> mask_table; DBuf<u64> mask_word_ptr; };
void lens_release(mvs_ctx* ctx) { delete ctx->lens; ctx->lens = nullptr; }
uint8_t* lens_staging(mvs_ctx* ctx, uint64_t bytes) {
    LensDev& D = row_dev(ctx->lens);
    D.staging.ensure((size_t)bytes + 16);
    return D.staging.p;
}

void lens_mask_run(mvs_ctx* ctx, const std::vector<LensMaskView>& T, float& ms) {
    if (T.empty()) return;
    LensDev& D = row_dev(ctx->lens);
    hipStream_t s = ctx->stream;
    const uint32_t n = (uint32_t)T.size();
    std::vector<u64> word_ptr((size_t)n + 1, 0);
    for (uint32_t k = 0; k < n; ++k) word_ptr[k + 1] = word_ptr[k] + (u64)(((uint32_t)T[k].width + 31u) / 32u) * (u64)T[k].height;
    const u64 n_words = word_ptr[n], blocks = (n_words * 32u + THREADS - 1u) / THREADS;
    if (blocks >= 0x7FFFFFFFull) throw StatusError(MVS_ERR_UNSUPPORTED, "set_view_masks: too many pixels in one batch (lower max_scratch_bytes)");
    upload(D.mask_table, T, s); upload(D.mask_word_ptr, word_ptr, s);
    StageTimer<2> tm(s);
    tm.mark();
    if (blocks) {
        hipLaunchKernelGGL(lens_mask_kernel, dim3((unsigned)blocks), dim3(THREADS), 0, s, (const LensMaskView*)D.mask_table.p, n, (const u64*)D.mask_word_ptr.p, n_words);
        MVS_LAUNCH_CHECK();
    }
    tm.mark();
    MVS_HIP(hipStreamSynchronize(s));   // (T and word_ptr were read by asynchronous copies)
    ms += tm.ms(0, 1);
}

namespace {

// one launch for the views of T; returns with the stream drained
void lens_run(mvs_ctx* ctx, const std::vector<LensView>& T, const char* who, mvs_lens_stats& st) {
    if (T.empty()) return;
    LensDev& D = row_dev(ctx->lens);
    hipStream_t s = ctx->stream;
    const uint32_t n = (uint32_t)T.size();
    std::vector<u64> chunk_ptr((size_t)n + 1, 0);
    for (uint32_t k = 0; k < n; ++k) {
        const uint64_t bytes = 3ull * (uint64_t)T[k].width * (uint64_t)T[k].height;
        chunk_ptr[k + 1] = chunk_ptr[k] + (((uintptr_t)T[k].dst & 15u) + bytes + 15u) / 16u;
        if (T[k].d0 != 0.0f) { st.views_undistorted += 1; st.pixels += bytes / 3u; } else st.views_copied += 1;
    }
    const u64 n_chunks = chunk_ptr[n];
    if (n_chunks >= 0x7FFFFFFFull * THREADS) throw StatusError(MVS_ERR_UNSUPPORTED, std::string(who) + ": too many pixels in one batch (lower max_scratch_bytes)");
    D.words.ensure(2);
    upload(D.table, T, s); upload(D.chunk_ptr, chunk_ptr, s);
    MVS_HIP(hipMemsetAsync(D.words.p, 0, sizeof(u64), s));
    StageTimer<2> tm(s);
    tm.mark();
    if (n_chunks) {
        hipLaunchKernelGGL(lens_kernel, dim3((unsigned)((n_chunks + THREADS - 1u) / THREADS)), dim3(THREADS), 0, s, (const LensView*)D.table.p, n, (const u64*)D.chunk_ptr.p, n_chunks, D.words.p);
        MVS_LAUNCH_CHECK();
    }
    tm.mark();
    u64 none = 0;
    MVS_HIP(hipMemcpyAsync(&none, D.words.p, sizeof(u64), hipMemcpyDeviceToHost, s));
    MVS_HIP(hipStreamSynchronize(s));   // (T and chunk_ptr were read by asynchronous copies)
    st.pixels_no_source += none; st.batches += 1; st.ms_undistort += tm.ms(0, 1);
}

// every view's lens checked: MVS_ERR_INVALID names the first bad view
void check_lenses(const mvs_lens* lens, uint32_t n, const char* who) {
    for (uint32_t j = 0; j < n; ++j) {
        const std::string why = lens_refusal(lens[j]);
        if (!why.empty()) throw StatusError(MVS_ERR_INVALID, std::string(who) + ": view " + std::to_string(j) + ": " + why);
    }
}

// Host images through staging in groups of at most `cap` bytes: image k (src[k], w[k] x h[k], lens[k]) -> dst[k].  `view` names image k in
// a refusal.  An image with dist0 == 0 is copied by the same launch (mvs_ctx_undistort_images; mvs_scene_set_views_lens sends none).
void stage_pixels(mvs_ctx* ctx, const std::vector<const uint8_t*>& src, const std::vector<uint8_t*>& dst, const std::vector<uint32_t>& w, const std::vector<uint32_t>& h,
                  const std::vector<mvs_lens>& lens, const std::vector<uint32_t>& view, uint64_t cap, const char* who, mvs_lens_stats& st) {
    const size_t n = src.size();
    for (size_t k = 0; k < n; ++k) {
        const uint64_t need = align16(3ull * w[k] * h[k]);
        if (need > cap)
            throw StatusError(MVS_ERR_INVALID, std::string(who) + ": view " + std::to_string(view[k]) + " needs " + std::to_string(need) + " bytes of staging, max_scratch_bytes is " + std::to_string(cap));
    }
    std::vector<size_t> cut{0};
    uint64_t most = 0;
    for (size_t a = 0; a < n;) {
        size_t b = a; uint64_t sum = 0;
        while (b < n && (b == a || sum + align16(3ull * w[b] * h[b]) <= cap)) sum += align16(3ull * w[b] * h[b]), ++b;
        most = std::max(most, sum); cut.push_back(b); a = b;
    }
    if (!most) return;
    uint8_t* staging = lens_staging(ctx, most);
    st.staging_bytes = std::max<uint64_t>(st.staging_bytes, most);
    for (size_t g = 0; g + 1 < cut.size(); ++g) {
        std::vector<const uint8_t*> from; std::vector<uint8_t*> to; std::vector<size_t> nb; std::vector<LensView> T;
        uint64_t off = 0;
        for (size_t k = cut[g]; k < cut[g + 1]; ++k) {
            const size_t bytes = (size_t)3 * w[k] * h[k];
            from.push_back(src[k]); to.push_back(staging + off); nb.push_back(bytes);
            T.push_back(LensView{staging + off, dst[k], (int32_t)w[k], (int32_t)h[k], lens[k].flen, lens[k].dist0, lens[k].dist1, 0u});
            off += align16(bytes);
        }
        const double t = now_ms_host();
        upload_pieces_through_ring(ctx, from.data(), to.data(), nb.data(), from.size());
        st.ms_upload += (float)(now_ms_host() - t);
        lens_run(ctx, T, who, st);
    }
}

}  // namespace
}  // namespace mvs

using namespace mvs;

extern "C" {

mvs_status mvs_undistort_image_host(const uint8_t* rgb, int32_t width, int32_t height, float flen, float dist0, float dist1, uint8_t* out) {
    if (!rgb || !out || width < 1 || height < 1) return api_fail(MVS_ERR_INVALID, "bad argument");
    const std::string why = lens_refusal(mvs_lens{flen, dist0, dist1, 0u});
    if (!why.empty()) return api_fail(MVS_ERR_INVALID, why);
    undistort_image_host(rgb, width, height, flen, dist0, dist1, out);
    return MVS_OK;
}

mvs_status mvs_ctx_undistort_images(mvs_ctx* ctx, const uint8_t* const* images, const uint32_t* widths, const uint32_t* heights, const mvs_lens* lens, uint32_t n,
                                    int out_on_device, mvs_rgb_set* out, mvs_lens_stats* stats) {
    if (!ctx || !out || (n && (!images || !widths || !heights || !lens))) return api_fail(MVS_ERR_INVALID, "null argument");
    *out = mvs_rgb_set{};
    mvs_lens_stats st{};
    if (stats) *stats = st;
    return api_guard([&] {
        MVS_HIP(hipSetDevice(ctx->device));
        run_with_stats(ctx->stream, stats, st, [&] {
            const char* who = "undistort_images";
            for (uint32_t k = 0; k < n; ++k)
                if (!images[k] || !widths[k] || !heights[k] || widths[k] > 0x7FFFFFFFu || heights[k] > 0x7FFFFFFFu) throw StatusError(MVS_ERR_INVALID, std::string(who) + ": view " + std::to_string(k) + ": bad image");
            check_lenses(lens, n, who);
            LensDev& D = row_dev(ctx->lens);
            std::vector<uint64_t> off((size_t)n + 1, 0);
            for (uint32_t k = 0; k < n; ++k) off[k + 1] = off[k] + 3ull * widths[k] * heights[k];
            D.out.ensure((size_t)off[n] + 16);
            std::vector<const uint8_t*> src(images, images + n); std::vector<uint8_t*> dst(n); std::vector<uint32_t> view(n);
            for (uint32_t k = 0; k < n; ++k) { dst[k] = D.out.p + off[k]; view[k] = k; }
            stage_pixels(ctx, src, dst, std::vector<uint32_t>(widths, widths + n), std::vector<uint32_t>(heights, heights + n), std::vector<mvs_lens>(lens, lens + n), view,
                         DEFAULT_MAX_SCRATCH, who, st);
            download<mvs_rgb_set>(ctx->stream, out, mvs_rgb_set_free, [&] {
                out->n_images = n; out->on_device = out_on_device ? 1u : 0u; out->n_bytes = off[n];
                out->offsets = (uint64_t*)malloc(((size_t)n + 1) * sizeof(uint64_t)); out->width = (uint32_t*)malloc(std::max<size_t>(n, 1) * sizeof(uint32_t)); out->height = (uint32_t*)malloc(std::max<size_t>(n, 1) * sizeof(uint32_t));
                if (!out->offsets || !out->width || !out->height) throw StatusError(MVS_ERR_INVALID, "out of host memory");
                memcpy(out->offsets, off.data(), ((size_t)n + 1) * sizeof(uint64_t));
                for (uint32_t k = 0; k < n; ++k) { out->width[k] = widths[k]; out->height[k] = heights[k]; }
                out->data = out_on_device ? D.out.p : host_copy(D.out.p, (size_t)off[n], ctx->stream);
            });
        });
    });
}

mvs_status mvs_scene_set_views_lens(mvs_ctx* ctx, const mvs_view* views, uint32_t n_views, const mvs_lens* lens, const uint8_t* const* files, const uint64_t* sizes,
                                    const mvs_jpegdec_params* jpeg_params, mvs_jpegdec_stats* jpeg_stats, mvs_lens_stats* lens_stats) {
    if (!ctx || (n_views && (!views || !lens || (files && !sizes)))) return api_fail(MVS_ERR_INVALID, "null argument");
    const char* who = "set_views_lens";
    for (uint32_t j = 0; j < n_views; ++j)
        if (!(files && files[j]) && !views[j].rgb) return api_fail(MVS_ERR_INVALID, std::string(who) + ": view " + std::to_string(j) + ": neither a file nor pixels");
    mvs_jpegdec_stats jst{}; mvs_lens_stats st{};
    if (jpeg_stats) *jpeg_stats = jst;
    if (lens_stats) *lens_stats = st;
    return api_guard([&] {
        MVS_HIP(hipSetDevice(ctx->device));
        const uint64_t cap = jpeg_params ? jpeg_params->max_scratch_bytes : DEFAULT_MAX_SCRATCH;
        // a refusal leaves the context without views, and says so to the next data-cost pass
        ctx->n_views = 0; ctx->h_views.clear(); ctx->have_costs = false; ctx->dc_phase = 0; ctx->views_refused = true;
        view_masks_clear(ctx); ctx->view_scratch_cap = cap;   // (a view input clears the masks; the masks of these views are staged under the same cap)
        run_with_stats(ctx->stream, jpeg_stats, jst, [&] { run_with_stats(ctx->stream, lens_stats, st, [&] {
            for (uint32_t j = 0; j < n_views; ++j)
                if (views[j].width < 2 || views[j].height < 2) throw StatusError(MVS_ERR_INVALID, std::string(who) + ": view " + std::to_string(j) + ": bad image");
            check_lenses(lens, n_views, who);
            while (ctx->own_rgb.size() > n_views) { delete ctx->own_rgb.back(); ctx->own_rgb.pop_back(); }
            std::vector<ViewParams> hv(n_views, ViewParams{});
            std::vector<uint8_t*> image(n_views); std::vector<uint8_t> staged(n_views, 0);
            std::vector<const uint8_t*> psrc; std::vector<uint8_t*> pdst; std::vector<size_t> pbytes;   // pixels uploaded as they are
            std::vector<const uint8_t*> ssrc; std::vector<uint8_t*> sdst; std::vector<uint32_t> sw, sh, sview; std::vector<mvs_lens> slens;   // pixels through staging
            bool any_file = false;
            for (uint32_t j = 0; j < n_views; ++j) {
                const mvs_view& v = views[j];
                ViewParams& p = hv[j];
                p = view_params_of(v);
                if (ctx->own_rgb.size() <= j) ctx->own_rgb.push_back(new DBuf<uint8_t>());
                ctx->own_rgb[j]->ensure((size_t)v.width * v.height * 3 + 16);
                p.rgb = image[j] = ctx->own_rgb[j]->p;
                staged[j] = lens[j].dist0 != 0.0f ? 1 : 0;
                if (files && files[j]) any_file = true;
                else if (staged[j]) { ssrc.push_back(v.rgb); sdst.push_back(image[j]); sw.push_back((uint32_t)v.width); sh.push_back((uint32_t)v.height); sview.push_back(j); slens.push_back(lens[j]); }
                else { psrc.push_back(v.rgb); pdst.push_back(image[j]); pbytes.push_back((size_t)v.width * v.height * 3); }
            }
            upload_pieces_through_ring(ctx, psrc.data(), pdst.data(), pbytes.data(), psrc.size());
            stage_pixels(ctx, ssrc, sdst, sw, sh, slens, sview, cap, who, st);
            if (any_file) {
                mvs_jpegdec_params P; P.max_scratch_bytes = cap; P.reserved = 0;
                decode_view_files(ctx, views, n_views, files, sizes, image.data(), staged.data(), &P, who, jst, [&](const std::vector<uint32_t>& bv, const std::vector<const uint8_t*>& bp) {
                    std::vector<LensView> T; uint64_t sum = 0;
                    for (size_t k = 0; k < bv.size(); ++k) {
                        const uint32_t j = bv[k];
                        T.push_back(LensView{bp[k], image[j], views[j].width, views[j].height, lens[j].flen, lens[j].dist0, lens[j].dist1, 0u});
                        sum += align16(3ull * views[j].width * views[j].height);
                    }
                    st.staging_bytes = std::max<uint64_t>(st.staging_bytes, sum);
                    lens_run(ctx, T, who, st);
                });
            }
            MVS_HIP(hipStreamSynchronize(ctx->stream));
            ctx->h_views.swap(hv);
            ctx->n_views = n_views; ctx->views_refused = false;
        }); });
    });
}

}  // extern "C"
