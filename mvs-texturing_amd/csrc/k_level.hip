// k_level.hip -- view input: pyramid levels, views halved on the device on their way in (DESIGN.md section 4 "View input" item 14; level.h
// states `half` once for this file and the host twin).
//   A view with level k > 0 is a STAGED view exactly as one with dist0 != 0 is (k_lens.hip): its full-size pixels lie in the context's
//   staging buffer for the length of one batch, and ONE span launch of level_kernel per batch writes the level images of all the batch's
//   views, of any sizes and levels, into their image buffers.  Only the level image stays resident.
//   level_kernel: a block makes one SEGMENT of one destination row -- at most SEG_PX[k] level pixels, i.e. a window of 2^k source rows by
//   at most seg << k source pixels -- in three steps.  (1) The window's source rows come into LDS as they lie in memory: rows of an RGB8
//   image start at every residue modulo 16, so a lane copies one ALIGNED 16-byte piece of a row, as one 16-byte load where the piece lies
//   inside the image and byte by byte where it does not (the head of the first row, the tail of the last): no load leaves the image, and
//   every source byte is fetched once but for the pieces two neighbouring segments share.  Under a lens the window's pixels are
//   lens.h lens_pixel of the staged image instead -- the two are FUSED, no second full-size buffer exists -- and a pixel without a source
//   is black before it is averaged.  (2) k times level.h half_sample from one LDS window into the next; the bytes are rounded at every
//   level, the intermediate levels never leave LDS.  (3) The row segment leaves as 16-byte stores aligned to the destination, its head
//   and tail by bytes.
//   keep_level_kernel: a lane makes one keep word of the level from the full-size keep words of the mask kernels: the AND of the 2^k
//   source rows, bits beyond the source's width set (the clamped column is x1 = x0, not "masked"), then k times level.h keep_half_pair.
#include "view_input.h"
#include "level.h"

namespace mvs {

typedef unsigned long long u64;

namespace {

constexpr uint32_t THREADS = 256;
// the level pixels of one segment: the source window is 2^k rows of 3 * (seg << k) + 32 bytes, at most RAW_BYTES
constexpr uint32_t SEG_PX[LEVEL_MAX + 1] = {0u, 1024u, 512u, 128u, 32u};
constexpr uint32_t RAW_BYTES = 25088u, A_BYTES = 6144u, B_BYTES = 1536u, OUT_BYTES = 3072u + 32u;
constexpr bool seg_fits(uint32_t k) {
    return (3u * (SEG_PX[k] << k) + 32u) * (1u << k) <= RAW_BYTES && (k < 2u || 3u * (SEG_PX[k] << (k - 1u)) * (1u << (k - 1u)) <= A_BYTES) &&
           (k < 3u || 3u * (SEG_PX[k] << (k - 2u)) * (1u << (k - 2u)) <= B_BYTES) && 3u * SEG_PX[k] + 32u <= OUT_BYTES && (3u * (SEG_PX[k] << k)) % 16u == 0u;
}
static_assert(seg_fits(1) && seg_fits(2) && seg_fits(3) && seg_fits(4), "a segment's windows fit their LDS buffers");

// per view of a batch (host made)
struct LevelView {
    const uint8_t* src;      // the full-size image (as the camera took it where d0 != 0)
    uint8_t* dst;            // the level image
    int32_t width, height;   // of the source
    uint32_t level;          // 1 .. LEVEL_MAX
    uint32_t seg, n_seg;     // level pixels per segment, segments per level row
    float flen, d0, d1;
};

__global__ void __launch_bounds__(THREADS) level_kernel(const LevelView* __restrict__ views, uint32_t n, const u64* __restrict__ unit_ptr, u64 n_units, u64* __restrict__ no_source) {
    __shared__ __attribute__((aligned(16))) uint8_t s_raw[RAW_BYTES];
    __shared__ __attribute__((aligned(16))) uint8_t s_a[A_BYTES];
    __shared__ __attribute__((aligned(16))) uint8_t s_b[B_BYTES];
    __shared__ __attribute__((aligned(16))) uint8_t s_out[OUT_BYTES];
    __shared__ uint32_t s_lo;
    const u64 g = blockIdx.x;   // the unit: the grid has exactly n_units blocks
    if (threadIdx.x == 0) s_lo = span_of(unit_ptr, n, g);
    __syncthreads();
    const LevelView V = views[s_lo];
    const uint32_t k = V.level;
    const u64 q = g - unit_ptr[s_lo];
    const int wl = level_dim(V.width, k);
    const uint32_t y = (q >> 32) ? (uint32_t)(q / V.n_seg) : (uint32_t)q / V.n_seg;   // the level row, and the segment [xa, xb) of it
    const int xa = (int)((uint32_t)(q - (u64)y * V.n_seg) * V.seg), xb = min(xa + (int)V.seg, wl);
    // the source window: columns [xs, xs + nw0), rows [ys, ys + nh0); row r lies at s_raw + r * pitch + off(r), as aligned as in memory
    const int xs = xa << k, ys = (int)(y << k), nw0 = min(xb << k, V.width) - xs, nh0 = min((int)((y + 1u) << k), V.height) - ys;
    const uint32_t pitch = ((3u * (V.seg << k) + 15u) & ~15u) + 32u;
    const uintptr_t base = (uintptr_t)V.src, end = base + 3u * (uintptr_t)V.width * (uintptr_t)V.height;
    auto row_addr = [&](int r) { return base + 3u * ((uintptr_t)(ys + r) * (uintptr_t)V.width + (uintptr_t)xs); };
    uint32_t none = 0;
    if (V.d0 == 0.0f) {
        const uint32_t row_bytes = 3u * (uint32_t)nw0, ppr = (row_bytes + 15u) / 16u + 1u;   // aligned pieces that cover a row, at most
        for (uint32_t i = threadIdx.x; i < ppr * (uint32_t)nh0; i += THREADS) {
            const uint32_t r = i / ppr, p = i - r * ppr;
            const uintptr_t a = row_addr((int)r), c = (a & ~(uintptr_t)15) + 16u * p;
            if (c >= a + row_bytes) continue;
            uint8_t* to = s_raw + r * pitch + 16u * p;
            if (c >= base && c + 16u <= end) *reinterpret_cast<uint4*>(to) = *reinterpret_cast<const uint4*>(c);
            else for (uint32_t b = 0; b < 16u; ++b) if (c + b >= a && c + b < a + row_bytes) to[b] = *reinterpret_cast<const uint8_t*>(c + b);
        }
    } else {
        const double flen = (double)V.flen, d0 = (double)V.d0, d1 = (double)V.d1;
        for (uint32_t i = threadIdx.x; i < (uint32_t)nw0 * (uint32_t)nh0; i += THREADS) {
            const uint32_t r = i / (uint32_t)nw0, x = i - r * (uint32_t)nw0;
            uint8_t rgb[3];
            if (!lens_pixel(V.src, V.width, V.height, xs + (int)x, ys + (int)r, flen, d0, d1, rgb)) ++none;
            uint8_t* to = s_raw + r * pitch + (uint32_t)(row_addr((int)r) & 15u) + 3u * x;
            to[0] = rgb[0]; to[1] = rgb[1]; to[2] = rgb[2];
        }
    }
    __syncthreads();
    // level j from level j - 1, j = 1 .. k: windows of nw x nh pixels, dense from level 1 on; the last one lies in s_out as the
    // destination is aligned
    const uintptr_t D = (uintptr_t)V.dst + 3u * ((uintptr_t)y * (uintptr_t)wl + (uintptr_t)xa);
    const uint32_t lead = (uint32_t)(D & 15u);
    int nw = nw0, nh = nh0;
    const uint8_t* in = s_raw;
    for (uint32_t j = 1; j <= k; ++j) {
        const int nwj = (nw + 1) >> 1, nhj = (nh + 1) >> 1;
        uint8_t* out = j == k ? s_out + lead : (j & 1u) ? s_a : s_b;
        const uint32_t spr = 3u * (uint32_t)nwj;   // samples per row
        for (uint32_t i = threadIdx.x; i < spr * (uint32_t)nhj; i += THREADS) {
            const uint32_t yy = i / spr, s = i - yy * spr, x = s / 3u, c = s - 3u * x;
            const int y0 = half_row0((int)yy), y1 = half_row1((int)yy, nh);
            const uint8_t* r0 = j == 1u ? s_raw + (uint32_t)y0 * pitch + (uint32_t)(row_addr(y0) & 15u) : in + (size_t)y0 * 3u * (uint32_t)nw;
            const uint8_t* r1 = j == 1u ? s_raw + (uint32_t)y1 * pitch + (uint32_t)(row_addr(y1) & 15u) : in + (size_t)y1 * 3u * (uint32_t)nw;
            out[i] = half_sample(r0, r1, nw, 3, (int)x, (int)c);
        }
        __syncthreads();
        in = out; nw = nwj; nh = nhj;
    }
    // the segment's bytes [D, D + len) in aligned pieces
    const uint32_t len = 3u * (uint32_t)(xb - xa);
    for (uint32_t p = threadIdx.x; p < (lead + len + 15u) / 16u; p += THREADS) {
        const uintptr_t c = (D & ~(uintptr_t)15) + 16u * p;
        if (c >= D && c + 16u <= D + len) *reinterpret_cast<uint4*>(c) = *reinterpret_cast<const uint4*>(s_out + 16u * p);
        else for (uint32_t b = 0; b < 16u; ++b) if (c + b >= D && c + b < D + len) *reinterpret_cast<uint8_t*>(c + b) = s_out[16u * p + b];
    }
    // one atomic per wave that found any (every lane of the block arrives here)
    for (int d = warpSize / 2; d > 0; d >>= 1) none += __shfl_xor(none, d);
    if (none && (threadIdx.x & (warpSize - 1)) == 0) atomicAdd(no_source, (u64)none);
}

struct KeepView { const uint32_t* src; uint32_t* keep; int32_t width, height; uint32_t level, pad_; };

__global__ void __launch_bounds__(THREADS) keep_level_kernel(const KeepView* __restrict__ views, uint32_t n, const u64* __restrict__ word_ptr, u64 n_words) {
    const u64 g = (u64)blockIdx.x * THREADS + threadIdx.x;
    __shared__ uint32_t s_lo;
    const uint32_t lo = block_span_of(word_ptr, n, (u64)blockIdx.x * THREADS, g, n_words, s_lo);
    if (g >= n_words) return;
    const KeepView V = views[lo];
    const uint32_t k = V.level, nk = 1u << k;
    const u64 q = g - word_ptr[lo];
    const int wl = level_dim(V.width, k);
    const uint32_t wpr = ((uint32_t)wl + 31u) / 32u, wpr_s = ((uint32_t)V.width + 31u) / 32u;
    const uint32_t y = (q >> 32) ? (uint32_t)(q / wpr) : (uint32_t)q / wpr;
    const uint32_t wx = (uint32_t)(q - (u64)y * wpr);
    const uint32_t r0 = y << k, r1 = min((y + 1u) << k, (uint32_t)V.height);   // the source rows
    uint32_t v[1u << LEVEL_MAX];
#pragma unroll
    for (uint32_t i = 0; i < (1u << LEVEL_MAX); ++i) {
        v[i] = 0xFFFFFFFFu;
        const uint32_t sw = (wx << k) + i;   // the source word; one that does not exist is all ones, as the bits beyond the width
        if (i < nk && sw < wpr_s) {
            for (uint32_t r = r0; r < r1; ++r) v[i] &= V.src[(size_t)r * wpr_s + sw];
            if (sw == wpr_s - 1u && ((uint32_t)V.width & 31u)) v[i] |= ~((1u << ((uint32_t)V.width & 31u)) - 1u);
        }
    }
#pragma unroll
    for (uint32_t m = (1u << LEVEL_MAX) / 2u; m >= 1u; m >>= 1) {   // 2 m words -> m words, where the level has that many
        if (2u * m <= nk) {
#pragma unroll
            for (uint32_t i = 0; i < m; ++i) v[i] = keep_half_pair(v[2u * i], v[2u * i + 1u]);
        }
    }
    const int nb = min(32, wl - 32 * (int)wx);
    V.keep[q] = nb < 32 ? v[0] & ((1u << nb) - 1u) : v[0];
}

}  // namespace

// per-context buffers of the route, allocated on first use
struct LevelDev { DBuf<uint8_t> out; DBuf<LevelView> table; DBuf<u64> unit_ptr, words; DBuf<KeepView> keep_table; DBuf<u64> keep_word_ptr; };
void level_release(mvs_ctx* ctx) { delete ctx->level; ctx->level = nullptr; }

void level_run(mvs_ctx* ctx, const std::vector<LevelItem>& items, const char* who, mvs_level_stats& st, mvs_lens_stats& lens_st) {
    if (items.empty()) return;
    LevelDev& D = row_dev(ctx->level);
    hipStream_t s = ctx->stream;
    std::vector<LevelView> T;
    for (const LevelItem& v : items) {
        const uint32_t wl = (uint32_t)level_dim(v.width, v.level), hl = (uint32_t)level_dim(v.height, v.level);
        const uint32_t n_seg = (wl + SEG_PX[v.level] - 1u) / SEG_PX[v.level], seg = (wl + n_seg - 1u) / n_seg;   // the row in equal segments
        T.push_back(LevelView{v.src, v.dst, v.width, v.height, v.level, seg, n_seg, v.flen, v.d0, v.d1});
        st.views_halved += 1; st.pixels_in += (uint64_t)v.width * (uint64_t)v.height; st.pixels_out += (uint64_t)wl * hl;
        if (v.d0 != 0.0f) { lens_st.views_undistorted += 1; lens_st.pixels += (uint64_t)v.width * (uint64_t)v.height; }
    }
    D.words.ensure(2);
    MVS_HIP(hipMemsetAsync(D.words.p, 0, sizeof(u64), s));
    u64 none = 0;
    st.ms_halve += span_launch(s, T, [](const LevelView& v) { return (uint64_t)v.n_seg * (uint64_t)level_dim(v.height, v.level); }, THREADS, THREADS, false, D.table, D.unit_ptr, who,
                               [&](unsigned blocks, uint32_t n, u64 n_units) {
        hipLaunchKernelGGL(level_kernel, dim3(blocks), dim3(THREADS), 0, s, (const LevelView*)D.table.p, n, (const u64*)D.unit_ptr.p, n_units, D.words.p);
    }, [&] { MVS_HIP(hipMemcpyAsync(&none, D.words.p, sizeof(u64), hipMemcpyDeviceToHost, s)); });
    lens_st.pixels_no_source += none; st.pixels_no_source += none; st.batches += 1;
}

void keep_level_run(mvs_ctx* ctx, const std::vector<KeepLevelItem>& items, float& ms) {
    if (items.empty()) return;
    LevelDev& D = row_dev(ctx->level);
    std::vector<KeepView> T;
    for (const KeepLevelItem& v : items) T.push_back(KeepView{v.src, v.keep, v.width, v.height, v.level, 0u});
    ms += span_launch(ctx->stream, T, [](const KeepView& v) { return keep_words(level_dim(v.width, v.level), level_dim(v.height, v.level)); }, 1u, THREADS, false, D.keep_table, D.keep_word_ptr,
                      "set_view_masks", [&](unsigned blocks, uint32_t n, u64 n_words) {
        hipLaunchKernelGGL(keep_level_kernel, dim3(blocks), dim3(THREADS), 0, ctx->stream, (const KeepView*)D.keep_table.p, n, (const u64*)D.keep_word_ptr.p, n_words);
    });
}

void check_levels(const mvs_view* views, const mvs_view_level* levels, uint32_t n, const char* who) {
    for (uint32_t j = 0; j < n; ++j) {
        const mvs_view_level& L = levels[j];
        const std::string w = view_msg(who, j);
        if (L.level > LEVEL_MAX) throw StatusError(MVS_ERR_INVALID, w + "level: " + std::to_string(L.level) + " is above " + std::to_string(LEVEL_MAX));
        if (L.reserved != 0u) throw StatusError(MVS_ERR_INVALID, w + "level: reserved must be 0");
        if (L.src_width < 1 || L.src_height < 1) throw StatusError(MVS_ERR_INVALID, w + "level: bad source size");
        const int wl = level_dim(L.src_width, L.level), hl = level_dim(L.src_height, L.level);
        if (wl != views[j].width || hl != views[j].height)
            throw StatusError(MVS_ERR_INVALID, w + "level: " + std::to_string(L.src_width) + " x " + std::to_string(L.src_height) + " at level " + std::to_string(L.level) + " is " +
                                                   std::to_string(wl) + " x " + std::to_string(hl) + ", the view " + std::to_string(views[j].width) + " x " + std::to_string(views[j].height));
        if (wl < 2 || hl < 2) throw StatusError(MVS_ERR_INVALID, w + "level: the level image is below 2 x 2");
    }
}

}  // namespace mvs

using namespace mvs;

extern "C" {

mvs_status mvs_level_size(int32_t width, int32_t height, uint32_t level, int32_t* level_width, int32_t* level_height) {
    if (width < 1 || height < 1 || level > LEVEL_MAX || !level_width || !level_height) return api_fail(MVS_ERR_INVALID, "level_size: bad argument");
    *level_width = level_dim(width, level); *level_height = level_dim(height, level);
    return MVS_OK;
}

mvs_status mvs_halve_image_host(const uint8_t* rgb, int32_t width, int32_t height, uint32_t level, uint8_t* out) {
    if (!rgb || !out || width < 1 || height < 1 || level > LEVEL_MAX) return api_fail(MVS_ERR_INVALID, "halve_image_host: bad argument");
    halve_image_host(rgb, width, height, 3, level, out);
    return MVS_OK;
}

mvs_status mvs_ctx_halve_images(mvs_ctx* ctx, const uint8_t* const* images, const uint32_t* widths, const uint32_t* heights, const uint32_t* levels, const mvs_lens* lens, uint32_t n,
                                int out_on_device, mvs_rgb_set* out, mvs_level_stats* stats) {
    if (!ctx || !out || (n && (!images || !widths || !heights || !levels))) return api_fail(MVS_ERR_INVALID, "null argument");
    *out = mvs_rgb_set{};
    mvs_level_stats st{};
    if (stats) *stats = st;
    return api_guard([&] {
        MVS_HIP(hipSetDevice(ctx->device));
        run_with_stats(ctx->stream, stats, st, [&] {
            const char* who = "halve_images";
            for (uint32_t k = 0; k < n; ++k) {
                if (!images[k] || !widths[k] || !heights[k] || widths[k] > 0x7FFFFFFFu || heights[k] > 0x7FFFFFFFu) throw StatusError(MVS_ERR_INVALID, view_msg(who, k) + "bad image");
                if (levels[k] > LEVEL_MAX) throw StatusError(MVS_ERR_INVALID, view_msg(who, k) + "level: " + std::to_string(levels[k]) + " is above " + std::to_string(LEVEL_MAX));
            }
            if (lens) check_lenses(lens, n, who);
            LevelDev& D = row_dev(ctx->level);
            const std::vector<uint32_t> w(widths, widths + n), h(heights, heights + n), lv(levels, levels + n);
            std::vector<uint32_t> wl(n), hl(n), view(n);
            for (uint32_t k = 0; k < n; ++k) { wl[k] = (uint32_t)level_dim((int)w[k], lv[k]); hl[k] = (uint32_t)level_dim((int)h[k], lv[k]); view[k] = k; }
            const RgbRoom R = rgb_set_room(D.out, wl, hl);
            mvs_lens_stats lst{};
            stage_pixels(ctx, std::vector<const uint8_t*>(images, images + n), R.dst, w, h, lens ? std::vector<mvs_lens>(lens, lens + n) : std::vector<mvs_lens>(n, mvs_lens{0.0f, 0.0f, 0.0f, 0u}), lv, view,
                         VIEW_SCRATCH_DEFAULT, who, lst, &st);
            st.staging_bytes = lst.staging_bytes; st.ms_upload = lst.ms_upload; st.pixels_no_source = lst.pixels_no_source;
            rgb_set_out(ctx, D.out, R, wl, hl, out_on_device, out);
        });
    });
}

mvs_status mvs_scene_set_views_levels(mvs_ctx* ctx, const mvs_view* views, uint32_t n_views, const mvs_view_level* levels, const mvs_lens* lens, const uint8_t* const* files,
                                      const uint64_t* sizes, const mvs_jpegdec_params* jpeg_params, mvs_jpegdec_stats* jpeg_stats, mvs_lens_stats* lens_stats, mvs_pngdec_stats* png_stats,
                                      mvs_level_stats* level_stats) {
    if (!ctx || (n_views && (!views || !levels || (files && !sizes)))) return api_fail(MVS_ERR_INVALID, "null argument");
    return set_views_files(ctx, views, n_views, lens, files, sizes, jpeg_params, jpeg_stats, lens_stats, "set_views_levels", "set_views_levels", true, png_stats, levels, level_stats);
}

}  // extern "C"
