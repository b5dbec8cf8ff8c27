// k_lens.hip -- view input: lens undistortion on the device for pixel and JPEG views (DESIGN.md section 4 "View input"; lens.h states the
// arithmetic of row f4 once, for this file, for undistort_kernel of k_prep.hip and for the host twin).
//   The distorted image has to exist whole before it is sampled, so a view with dist0 != 0 goes to the context's STAGING buffer
//   (view_input.h) -- host pixels in groups that fit (stage_in_groups), a JPEG file decoded there by k_jpegdec.hip (decode_view_files),
//   its 3 w h bytes counted towards its scratch -- and ONE span launch of lens_kernel per batch writes the undistorted pixels of all the
//   batch's views into their image buffers.  Views with dist0 == 0 never see staging.  This file also holds the one body of the JPEG and
//   the lens view entries (set_views_files).
//   lens_kernel: a lane makes 16 bytes of a destination image, aligned to it, and leaves them as one 16-byte store (the head and the tail
//   of an image go out by bytes).  The batch's chunks of 16 bytes are numbered through all views (chunk_ptr; span_of finds the lane's
//   view).  16 bytes are 5 1/3 pixels: they touch at most 6, whose source positions the lane evaluates, keeping only its own bytes --
//   1.125 evaluations per pixel against undistort_kernel's one, for one store per 16 bytes against three per pixel.
#include "view_input.h"

namespace mvs {

typedef unsigned long long u64;

namespace {

constexpr uint32_t THREADS = 256;

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
        const uint32_t lo = span_of(chunk_ptr, n, g);
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
// are numbered through all views (word_ptr; block_span_of finds the word's view).
__global__ void __launch_bounds__(THREADS) lens_mask_kernel(const LensMaskView* __restrict__ views, uint32_t n, const u64* __restrict__ word_ptr, u64 n_words) {
    const u64 g = ((u64)blockIdx.x * THREADS + threadIdx.x) >> 5;   // the word; THREADS and the wave are multiples of 32
    const int b = (int)(threadIdx.x & 31u);
    bool keep = false;
    uint32_t* dst = nullptr;
    __shared__ uint32_t s_lo;
    const uint32_t lo = block_span_of(word_ptr, n, ((u64)blockIdx.x * THREADS) >> 5, g, n_words, s_lo);
    if (g < n_words) {
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

}  // namespace

// per-context buffers of the route, allocated on first use
struct LensDev { DBuf<uint8_t> out; DBuf<LensView> table; DBuf<u64> chunk_ptr, words; DBuf<LensMaskView> mask_table; DBuf<u64> mask_word_ptr; };
void lens_release(mvs_ctx* ctx) { delete ctx->lens; ctx->lens = nullptr; }

void lens_mask_run(mvs_ctx* ctx, const std::vector<LensMaskView>& T, float& ms) {
    if (T.empty()) return;
    LensDev& D = row_dev(ctx->lens);
    ms += span_launch(ctx->stream, T, [](const LensMaskView& v) { return keep_words(v.width, v.height); }, 32u, THREADS, false, D.mask_table, D.mask_word_ptr, "set_view_masks", [&](unsigned blocks, uint32_t n, u64 n_words) {
        hipLaunchKernelGGL(lens_mask_kernel, dim3(blocks), dim3(THREADS), 0, ctx->stream, (const LensMaskView*)D.mask_table.p, n, (const u64*)D.mask_word_ptr.p, n_words);
    });
}

namespace {

// one launch for the views of T; returns with the stream drained
void lens_run(mvs_ctx* ctx, const std::vector<LensView>& T, const char* who, mvs_lens_stats& st) {
    if (T.empty()) return;
    LensDev& D = row_dev(ctx->lens);
    hipStream_t s = ctx->stream;
    for (const LensView& v : T) { if (v.d0 != 0.0f) { st.views_undistorted += 1; st.pixels += (uint64_t)v.width * (uint64_t)v.height; } else st.views_copied += 1; }
    auto chunks = [](const LensView& v) { return (((uintptr_t)v.dst & 15u) + 3ull * (uint64_t)v.width * (uint64_t)v.height + 15u) / 16u; };   // of 16 bytes, aligned to dst
    D.words.ensure(2);
    MVS_HIP(hipMemsetAsync(D.words.p, 0, sizeof(u64), s));
    u64 none = 0;
    st.ms_undistort += span_launch(s, T, chunks, 1u, THREADS, true, D.table, D.chunk_ptr, who, [&](unsigned blocks, uint32_t n, u64 n_chunks) {
        hipLaunchKernelGGL(lens_kernel, dim3(blocks), dim3(THREADS), 0, s, (const LensView*)D.table.p, n, (const u64*)D.chunk_ptr.p, n_chunks, D.words.p);
    }, [&] { MVS_HIP(hipMemcpyAsync(&none, D.words.p, sizeof(u64), hipMemcpyDeviceToHost, s)); });
    st.pixels_no_source += none; st.batches += 1;
}

}  // namespace

// host images through staging in groups (ctx.h): level 0 by lens_kernel (an image with dist0 == 0 is copied by the same launch:
// mvs_ctx_undistort_images and mvs_ctx_halve_images; the view entries send none), a level above by level_run of k_level.hip
void stage_pixels(mvs_ctx* ctx, const std::vector<const uint8_t*>& src, const std::vector<uint8_t*>& dst, const std::vector<uint32_t>& w, const std::vector<uint32_t>& h,
                  const std::vector<mvs_lens>& lens, const std::vector<uint32_t>& level, const std::vector<uint32_t>& view, uint64_t cap, const char* who, mvs_lens_stats& st,
                  mvs_level_stats* level_st) {
    std::vector<uint64_t> bytes(src.size());
    for (size_t k = 0; k < src.size(); ++k) bytes[k] = 3ull * w[k] * h[k];
    stage_in_groups(ctx, src, bytes, view, cap, who, st.ms_upload, st.staging_bytes, [&](size_t first, size_t last, const std::vector<uint8_t*>& at) {
        std::vector<LensView> T; std::vector<LevelItem> U;
        for (size_t k = first; k < last; ++k) {
            if (level[k]) U.push_back(LevelItem{at[k - first], dst[k], (int32_t)w[k], (int32_t)h[k], level[k], lens[k].flen, lens[k].dist0, lens[k].dist1});
            else T.push_back(LensView{at[k - first], dst[k], (int32_t)w[k], (int32_t)h[k], lens[k].flen, lens[k].dist0, lens[k].dist1, 0u});
        }
        lens_run(ctx, T, who, st);
        if (!U.empty()) level_run(ctx, U, who, *level_st, st);
    });
}

namespace {

}  // namespace

// mvs_scene_set_views_jpeg (lens == null: no view is undistorted), mvs_scene_set_views_lens and mvs_scene_set_views_files (accept_png: a file
// with the PNG signature takes the route of k_pngdec.hip) behind their argument checks: who_view starts the messages about a view's size
// and source ("" for the JPEG entry), `who` all others
mvs_status set_views_files(mvs_ctx* ctx, const mvs_view* views, uint32_t n_views, const mvs_lens* lens, const uint8_t* const* files, const uint64_t* sizes,
                           const mvs_jpegdec_params* jpeg_params, mvs_jpegdec_stats* jpeg_stats, mvs_lens_stats* lens_stats, const char* who_view, const char* who,
                           bool accept_png, mvs_pngdec_stats* png_stats, const mvs_view_level* levels, mvs_level_stats* level_stats) {
    for (uint32_t j = 0; j < n_views; ++j)
        if (!(files && files[j]) && !views[j].rgb) return api_fail(MVS_ERR_INVALID, view_msg(who_view, j) + "neither a file nor pixels");
    mvs_jpegdec_stats jst{}; mvs_lens_stats st{}; mvs_pngdec_stats pst{}; mvs_level_stats vst{};
    if (level_stats) *level_stats = vst;
    if (jpeg_stats) *jpeg_stats = jst;
    if (lens_stats) *lens_stats = st;
    if (png_stats) *png_stats = pst;
    return api_guard([&] {
        MVS_HIP(hipSetDevice(ctx->device));
        const uint64_t cap = jpeg_params ? jpeg_params->max_scratch_bytes : VIEW_SCRATCH_DEFAULT;
        view_input_begin(ctx, cap);
        run_with_stats(ctx->stream, level_stats, vst, [&] { run_with_stats(ctx->stream, png_stats, pst, [&] { run_with_stats(ctx->stream, jpeg_stats, jst, [&] { run_with_stats(ctx->stream, lens_stats, st, [&] {
            if (levels) check_levels(views, levels, n_views, who);
            check_view_sizes(views, n_views, who_view);
            if (lens) check_lenses(lens, n_views, who);
            // a view with a level comes at its source's size: the files' frames are checked against it, and the staging holds it
            auto level_of = [&](uint32_t j) { return levels ? levels[j].level : 0u; };
            std::vector<mvs_view> src_views(views, views + n_views);
            for (uint32_t j = 0; levels && j < n_views; ++j) { src_views[j].width = levels[j].src_width; src_views[j].height = levels[j].src_height; }
            const mvs_lens no_lens{0.0f, 0.0f, 0.0f, 0u};
            std::vector<ViewParams> hv;
            const std::vector<uint8_t*> image = own_images(ctx, views, n_views, hv);
            std::vector<uint8_t> staged(n_views, 0);
            std::vector<const uint8_t*> psrc; std::vector<uint8_t*> pdst; std::vector<size_t> pbytes;   // pixels uploaded as they are
            std::vector<const uint8_t*> ssrc; std::vector<uint8_t*> sdst; std::vector<uint32_t> sw, sh, sview, slevel; std::vector<mvs_lens> slens;   // pixels through staging
            bool any_file = false;
            for (uint32_t j = 0; j < n_views; ++j) {
                const mvs_view& v = views[j];
                staged[j] = (lens && lens[j].dist0 != 0.0f) || level_of(j) ? 1 : 0;
                if (files && files[j]) any_file = true;
                else if (staged[j]) {
                    ssrc.push_back(v.rgb); sdst.push_back(image[j]); sw.push_back((uint32_t)src_views[j].width); sh.push_back((uint32_t)src_views[j].height); sview.push_back(j);
                    slens.push_back(lens ? lens[j] : no_lens); slevel.push_back(level_of(j));
                }
                else { psrc.push_back(v.rgb); pdst.push_back(image[j]); pbytes.push_back((size_t)v.width * v.height * 3); }
            }
            upload_pieces_through_ring(ctx, psrc.data(), pdst.data(), pbytes.data(), psrc.size());
            stage_pixels(ctx, ssrc, sdst, sw, sh, slens, slevel, sview, cap, who, st, &vst);
            if (any_file)
                decode_view_files(ctx, src_views.data(), n_views, files, sizes, image.data(), staged.data(), jpeg_params, who, jst, [&](const std::vector<uint32_t>& bv, const std::vector<const uint8_t*>& bp) {
                    std::vector<LensView> T; std::vector<LevelItem> U; uint64_t sum = 0;
                    for (size_t k = 0; k < bv.size(); ++k) {
                        const uint32_t j = bv[k];
                        const mvs_view& sv = src_views[j];
                        const mvs_lens& L = lens ? lens[j] : no_lens;
                        if (level_of(j)) U.push_back(LevelItem{bp[k], image[j], sv.width, sv.height, level_of(j), L.flen, L.dist0, L.dist1});
                        else T.push_back(LensView{bp[k], image[j], sv.width, sv.height, L.flen, L.dist0, L.dist1, 0u});
                        sum += align16(3ull * sv.width * sv.height);
                    }
                    st.staging_bytes = std::max<uint64_t>(st.staging_bytes, sum);
                    lens_run(ctx, T, who, st);
                    level_run(ctx, U, who, vst, st);
                }, accept_png ? &pst : nullptr);
            MVS_HIP(hipStreamSynchronize(ctx->stream));
            vst.staging_bytes = st.staging_bytes; vst.ms_upload = st.ms_upload;
            view_input_commit(ctx, hv, n_views);
            if (levels) ctx->view_levels.assign(levels, levels + n_views);
        }); }); }); });
    });
}

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
                if (!images[k] || !widths[k] || !heights[k] || widths[k] > 0x7FFFFFFFu || heights[k] > 0x7FFFFFFFu) throw StatusError(MVS_ERR_INVALID, view_msg(who, k) + "bad image");
            check_lenses(lens, n, who);
            LensDev& D = row_dev(ctx->lens);
            const std::vector<uint32_t> w(widths, widths + n), h(heights, heights + n);
            const RgbRoom R = rgb_set_room(D.out, w, h);
            std::vector<uint32_t> view(n);
            for (uint32_t k = 0; k < n; ++k) view[k] = k;
            stage_pixels(ctx, std::vector<const uint8_t*>(images, images + n), R.dst, w, h, std::vector<mvs_lens>(lens, lens + n), std::vector<uint32_t>(n, 0u), view, VIEW_SCRATCH_DEFAULT, who, st, nullptr);
            rgb_set_out(ctx, D.out, R, w, h, out_on_device, out);
        });
    });
}

mvs_status mvs_scene_set_views_lens(mvs_ctx* ctx, const mvs_view* views, uint32_t n_views, const mvs_lens* lens, const uint8_t* const* files, const uint64_t* sizes,
                                    const mvs_jpegdec_params* jpeg_params, mvs_jpegdec_stats* jpeg_stats, mvs_lens_stats* lens_stats) {
    if (!ctx || (n_views && (!views || !lens || (files && !sizes)))) return api_fail(MVS_ERR_INVALID, "null argument");
    return set_views_files(ctx, views, n_views, lens, files, sizes, jpeg_params, jpeg_stats, lens_stats, "set_views_lens", "set_views_lens");
}

}  // extern "C"
