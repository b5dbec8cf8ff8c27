// k_viewmask.hip -- view input: view masks (DESIGN.md section 4 "View input" item 10; include/mvs_viewsel.h mvs_scene_set_view_masks).
//   A masked pixel is an invalid pixel, and nothing else changes.  A view's byte mask [height][width] (0 = leave out) becomes KEEP WORDS in the
//   layout of the validity mask -- mask_stride words per row, bit b of word wx = pixel 32 wx + b, bits beyond the width zero -- which
//   mask_final_kernel (k_prep.hip) ANDs into the flood-fill validity in front of the erosion.  Keep words exist for masked views only.
//   Host masks go through the context's staging buffer in groups of at most ctx->view_scratch_cap bytes (view_input.h stage_in_groups);
//   device masks are read where they lie.  Per batch ONE span launch of mask_pack_kernel packs the masks that are used as they are, and
//   one of lens_mask_kernel (k_lens.hip) undistorts those that come in the camera's frame.
//   mask_pack_kernel: a lane makes one word from up to 32 bytes of one row.  Rows of a [h][w] byte image start at every residue modulo 16,
//   so the lane reads the (at most three) ALIGNED 16-byte pieces that cover its bytes, each as one 16-byte load where the piece lies inside
//   the image and byte by byte where it does not (the head of the first row, the tail of the last): no load leaves the image.
#include "view_input.h"

namespace mvs {

typedef unsigned long long u64;

namespace {

constexpr uint32_t THREADS = 256;

struct PackView { const uint8_t* src; uint32_t* keep; int32_t width, height; };

// bit k = byte k of w is not zero
__device__ __forceinline__ uint32_t nonzero4(uint32_t w) {
    const uint32_t t = (((w & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | w) & 0x80808080u;   // bit 7 of every byte that is not zero
    return ((t >> 7) * 0x01020408u) >> 24;                                        // bits 0, 8, 16, 24 -> bits 24 .. 27 (no two products meet)
}

__global__ void __launch_bounds__(THREADS) mask_pack_kernel(const PackView* __restrict__ views, uint32_t n, const u64* __restrict__ word_ptr, u64 n_words) {
    const u64 g = (u64)blockIdx.x * THREADS + threadIdx.x;
    __shared__ uint32_t s_lo;
    const uint32_t lo = block_span_of(word_ptr, n, (u64)blockIdx.x * THREADS, g, n_words, s_lo);
    if (g < n_words) {
        const PackView V = views[lo];
        const u64 q = g - word_ptr[lo];
        const uint32_t wpr = ((uint32_t)V.width + 31u) / 32u;
        const uint32_t y = (q >> 32) ? (uint32_t)(q / wpr) : (uint32_t)q / wpr;          // (a 64-bit division is a subroutine)
        const uint32_t wx = (uint32_t)(q - (u64)y * wpr);
        const int nb = min(32, V.width - 32 * (int)wx);                                   // 1 .. 32 real pixels
        const uintptr_t base = (uintptr_t)V.src, end = base + (uintptr_t)V.width * (uintptr_t)V.height;
        const uintptr_t p = base + (uintptr_t)y * (uintptr_t)V.width + 32u * wx;         // the word's bytes are [p, p + nb)
        uintptr_t c = p & ~(uintptr_t)15;
        uint32_t bits = 0;
#pragma unroll
        for (int k = 0; k < 3; ++k, c += 16) {
            const int d = (int)((long long)c - (long long)p);                            // -15 .. 0, 1 .. 16, 17 .. 32
            if (d >= nb) break;
            uint32_t m = 0;   // bit i: byte c[i] is not zero; what lies outside [p, p + nb) is shifted or masked away below
            if (c >= base && c + 16 <= end) {
                const uint4 v = *reinterpret_cast<const uint4*>(c);
                m = nonzero4(v.x) | (nonzero4(v.y) << 4) | (nonzero4(v.z) << 8) | (nonzero4(v.w) << 12);
            } else {
                for (int i = 0; i < 16; ++i) {
                    const uintptr_t a = c + (uintptr_t)i;
                    if (a >= p && a < p + (uintptr_t)nb && *reinterpret_cast<const uint8_t*>(a)) m |= 1u << i;
                }
            }
            bits |= d >= 0 ? m << d : m >> -d;
        }
        if (nb < 32) bits &= (1u << nb) - 1u;
        V.keep[q] = bits;
    }
}

// the kept pixels of all masked views: the set bits of their keep words (bits beyond a row's width are zero), one atomic per block of a
// grid-stride loop.  The pack and lens kernels do not count: one atomic per wave that left a pixel out was a million atomics on one
// address at config 3 with a disc on every view, and the lens launch took 14.5 ms of which the arithmetic needs a third.
__global__ void __launch_bounds__(THREADS) keep_count_kernel(const uint32_t* __restrict__ keep, u64 n_words, u64* __restrict__ kept) {
    u64 sum = 0;
    for (u64 i = (u64)blockIdx.x * THREADS + threadIdx.x; i < n_words; i += (u64)gridDim.x * THREADS) sum += (u64)__popc(keep[i]);
    for (int d = warpSize / 2; d > 0; d >>= 1) sum += __shfl_xor(sum, d);
    __shared__ u64 s_sum[THREADS / 64];
    if ((threadIdx.x & (warpSize - 1)) == 0) s_sum[threadIdx.x / warpSize] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        u64 t = 0;
        for (uint32_t k = 0; k < THREADS / warpSize; ++k) t += s_sum[k];
        if (t) atomicAdd(kept, t);
    }
}

}  // namespace

// per-context state of the masks: the keep words of the masked views back to back, the table of every view's keep pointer (null: no
// mask) and the list of the masked views as prepare_views hands them to its kernels, and the launch tables of the pack kernel
struct ViewMaskDev {
    DBuf<uint32_t> keep, list, full; DBuf<const uint32_t*> table; DBuf<PackView> pack_table; DBuf<u64> word_ptr, counter;
    uint32_t n_masked = 0;
};
void viewmask_release(mvs_ctx* ctx) { delete ctx->viewmask; ctx->viewmask = nullptr; }
void view_masks_clear(mvs_ctx* ctx) { if (ctx->viewmask) ctx->viewmask->n_masked = 0; }
ViewKeep view_keep(mvs_ctx* ctx) {
    const ViewMaskDev* D = ctx->viewmask;
    if (!D || !D->n_masked) return ViewKeep{nullptr, nullptr, 0u};
    return ViewKeep{D->table.p, D->list.p, D->n_masked};
}
const uint32_t* view_keep_words(mvs_ctx* ctx, uint32_t view, std::vector<const uint32_t*>& host_table) {
    const ViewMaskDev* D = ctx->viewmask;
    if (!D || !D->n_masked) return nullptr;
    host_table.assign(ctx->n_views, nullptr);
    MVS_HIP(hipMemcpyAsync(host_table.data(), D->table.p, (size_t)ctx->n_views * sizeof(const uint32_t*), hipMemcpyDeviceToHost, ctx->stream));
    MVS_HIP(hipStreamSynchronize(ctx->stream));
    return host_table[view];
}

namespace {

// one launch of the pack kernel for the views of T; returns with the stream drained; the launch's device time is added to ms
void pack_run(mvs_ctx* ctx, ViewMaskDev& D, const std::vector<PackView>& T, float& ms) {
    ms += span_launch(ctx->stream, T, [](const PackView& v) { return keep_words(v.width, v.height); }, 1u, THREADS, false, D.pack_table, D.word_ptr, "set_view_masks", [&](unsigned blocks, uint32_t n, u64 n_words) {
        hipLaunchKernelGGL(mask_pack_kernel, dim3(blocks), dim3(THREADS), 0, ctx->stream, (const PackView*)D.pack_table.p, n, (const u64*)D.word_ptr.p, n_words);
    });
}

}  // namespace
}  // namespace mvs

using namespace mvs;

extern "C" {

mvs_status mvs_scene_set_view_masks(mvs_ctx* ctx, const uint8_t* const* masks, uint32_t n_views, int on_device, const mvs_lens* lens, mvs_mask_stats* stats) {
    if (!ctx) return api_fail(MVS_ERR_INVALID, "ctx is null");
    const char* who = "set_view_masks";
    mvs_mask_stats st{};
    if (stats) *stats = st;
    return api_guard([&] {
        MVS_HIP(hipSetDevice(ctx->device));
        // a refusal leaves the context without masks; the table of an earlier pass was made of other validity masks
        view_masks_clear(ctx); ctx->have_costs = false; ctx->dc_phase = 0;
        run_with_stats(ctx->stream, stats, st, [&] {
            if (ctx->n_views == 0) throw StatusError(MVS_ERR_STATE, std::string(who) + ": the context has no views (a view input comes first)");
            if (n_views != ctx->n_views)
                throw StatusError(MVS_ERR_INVALID, std::string(who) + ": n_views is " + std::to_string(n_views) + ", the context has " + std::to_string(ctx->n_views) + " views");
            if (lens) check_lenses(lens, n_views, who);
            std::vector<uint32_t> mv;   // the views that carry a mask
            for (uint32_t j = 0; masks && j < n_views; ++j) if (masks[j]) mv.push_back(j);
            if (mv.empty()) return;
            const size_t n = mv.size();
            const uint64_t cap = ctx->view_scratch_cap;
            // a view with a pyramid level (k_level.hip) brings its mask at the SOURCE's size: sw x sh, level lv (0: the view's own size)
            std::vector<uint64_t> off(n + 1, 0), bytes(n), need(n), px(n);
            std::vector<const uint8_t*> src(n);
            std::vector<int32_t> sw(n), sh(n); std::vector<uint32_t> lv(n, 0u);
            for (size_t k = 0; k < n; ++k) {
                const ViewParams& v = ctx->h_views[mv[k]];
                src[k] = masks[mv[k]];
                sw[k] = v.width; sh[k] = v.height;
                if (!ctx->view_levels.empty() && ctx->view_levels[mv[k]].level) { const mvs_view_level& L = ctx->view_levels[mv[k]]; lv[k] = L.level; sw[k] = L.src_width; sh[k] = L.src_height; }
                bytes[k] = (uint64_t)sw[k] * (uint64_t)sh[k]; need[k] = align16(bytes[k]); px[k] = (uint64_t)v.width * (uint64_t)v.height;
                off[k + 1] = off[k] + keep_words(v.width, v.height);
            }
            const size_t counted = on_device ? n : std::min(n, first_over_cap(need.data(), n, cap) + 1);   // (a refusal reports the pixels up to the refused view)
            for (size_t k = 0; k < counted; ++k) st.pixels += px[k];
            if (!on_device) refuse_over_cap(need, cap, mv.data(), who, "staging");
            ViewMaskDev& D = row_dev(ctx->viewmask);
            D.keep.ensure((size_t)off[n] + 4); D.counter.ensure(2);
            MVS_HIP(hipMemsetAsync(D.counter.p, 0, sizeof(u64), ctx->stream));
            // items [first, last) of mv with their bytes at at[k - first]: one launch packs the masks that are used as they are, one undistorts the others
            auto batch = [&](size_t first, size_t last, const auto& at) {
                std::vector<PackView> P; std::vector<LensMaskView> Q; std::vector<KeepLevelItem> R;
                uint64_t full = 0;   // the full-size keep words of the batch's views with a level: a scratch of this batch
                for (size_t k = first; k < last; ++k) if (lv[k]) full += keep_words(sw[k], sh[k]);
                D.full.ensure((size_t)full + 4);
                full = 0;
                for (size_t k = first; k < last; ++k) {
                    const uint32_t j = mv[k];
                    uint32_t* keep = D.keep.p + off[k];
                    if (lv[k]) { R.push_back(KeepLevelItem{D.full.p + full, keep, sw[k], sh[k], lv[k], 0u}); keep = D.full.p + full; full += keep_words(sw[k], sh[k]); }
                    if (lens && lens[j].dist0 != 0.0f) Q.push_back(LensMaskView{at[k - first], keep, sw[k], sh[k], lens[j].flen, lens[j].dist0, lens[j].dist1, 0u});
                    else P.push_back(PackView{at[k - first], keep, sw[k], sh[k]});
                }
                pack_run(ctx, D, P, st.ms_pack);                      // (all three return with the stream drained: the staging is free for the next batch)
                lens_mask_run(ctx, Q, st.ms_undistort);
                keep_level_run(ctx, R, st.ms_pack);
                st.batches += 1; st.views_undistorted += Q.size();
            };
            // device masks are read where they lie, all in one batch; host masks in groups whose staged bytes fit the cap
            if (on_device) batch(0, n, src);
            else stage_in_groups(ctx, src, bytes, mv, cap, who, st.ms_upload, st.staging_bytes, batch);
            std::vector<const uint32_t*> table(n_views, nullptr);
            for (size_t k = 0; k < n; ++k) table[mv[k]] = D.keep.p + off[k];
            upload(D.table, table, ctx->stream); upload(D.list, mv, ctx->stream);
            u64 kept = 0;
            hipLaunchKernelGGL(keep_count_kernel, dim3((unsigned)std::min<uint64_t>((off[n] + THREADS - 1) / THREADS, 2048)), dim3(THREADS), 0, ctx->stream, (const uint32_t*)D.keep.p, (u64)off[n], D.counter.p);
            MVS_LAUNCH_CHECK();
            MVS_HIP(hipMemcpyAsync(&kept, D.counter.p, sizeof(u64), hipMemcpyDeviceToHost, ctx->stream));
            MVS_HIP(hipStreamSynchronize(ctx->stream));
            st.views_masked = n; st.pixels_masked_out = st.pixels - kept; st.device_bytes = off[n] * sizeof(uint32_t);
            D.n_masked = (uint32_t)n;
        });
    });
}

}  // extern "C"
