// k_viewmask.hip -- view input: view masks (DESIGN.md section 4 "View input" item 10; include/mvs_viewsel.h mvs_scene_set_view_masks).
//   A masked pixel is an invalid pixel, and nothing else changes.  A view's byte mask [height][width] (0 = leave out) becomes KEEP WORDS in the
//   layout of the validity mask -- mask_stride words per row, bit b of word wx = pixel 32 wx + b, bits beyond the width zero -- which
//   mask_final_kernel (k_prep.hip) ANDs into the flood-fill validity in front of the erosion.  Keep words exist for masked views only.
//   Host masks go through the pinned upload ring into the context's staging buffer (k_lens.hip lens_staging) in batches of at most
//   ctx->view_scratch_cap bytes; device masks are read where they lie.  Per batch ONE launch of mask_pack_kernel packs the masks that are used
//   as they are, and one of lens_mask_kernel (k_lens.hip) undistorts those that come in the camera's frame.
//   mask_pack_kernel: a lane makes one word from up to 32 bytes of one row.  Rows of a [h][w] byte image start at every residue modulo 16,
//   so the lane reads the (at most three) ALIGNED 16-byte pieces that cover its bytes, each as one 16-byte load where the piece lies inside
//   the image and byte by byte where it does not (the head of the first row, the tail of the last): no load leaves the image.
#include "rows.h"
#include "lens.h"

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
    // the view of the block's first word by binary search, once per block; a lane walks on from there (a block seldom spans two views).
    // With the search in every lane the kernel ran at 405 GB/s at config 3: eight dependent loads in front of two independent ones.
    __shared__ uint32_t s_lo;
    if (threadIdx.x == 0) {
        const u64 g0 = (u64)blockIdx.x * THREADS;   // < n_words: the grid has no empty block
        uint32_t lo = 0, hi = n;
        while (hi - lo > 1u) { const uint32_t mid = lo + (hi - lo) / 2u; if (word_ptr[mid] <= g0) lo = mid; else hi = mid; }
        s_lo = lo;
    }
    __syncthreads();
    if (g < n_words) {
        uint32_t lo = s_lo;
        while (word_ptr[lo + 1] <= g) ++lo;         // g < n_words = word_ptr[n]: ends at lo <= n - 1
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

uint64_t align16(uint64_t v) { return (v + 15u) & ~15ull; }

}  // namespace

// per-context state of the masks: the keep words of the masked views back to back, the table of every view's keep pointer (null: no
// mask) and the list of the masked views as prepare_views hands them to its kernels, and the launch tables of the pack kernel
struct ViewMaskDev {
    DBuf<uint32_t> keep, list; DBuf<const uint32_t*> table; DBuf<PackView> pack_table; DBuf<u64> word_ptr, counter;
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
    if (T.empty()) return;
    std::vector<u64> word_ptr;
    const uint32_t n = (uint32_t)T.size();
    word_ptr.assign((size_t)n + 1, 0);
    for (uint32_t k = 0; k < n; ++k) word_ptr[k + 1] = word_ptr[k] + (u64)(((uint32_t)T[k].width + 31u) / 32u) * (u64)T[k].height;
    const u64 n_words = word_ptr[n], blocks = (n_words + THREADS - 1u) / THREADS;
    if (blocks >= 0x7FFFFFFFull) throw StatusError(MVS_ERR_UNSUPPORTED, "set_view_masks: too many pixels in one batch (lower max_scratch_bytes)");
    upload(D.pack_table, T, ctx->stream); upload(D.word_ptr, word_ptr, ctx->stream);
    StageTimer<2> tm(ctx->stream);
    tm.mark();
    if (blocks) {
        hipLaunchKernelGGL(mask_pack_kernel, dim3((unsigned)blocks), dim3(THREADS), 0, ctx->stream, (const PackView*)D.pack_table.p, n, (const u64*)D.word_ptr.p, n_words);
        MVS_LAUNCH_CHECK();
    }
    tm.mark();
    MVS_HIP(hipStreamSynchronize(ctx->stream));   // (T and word_ptr were read by asynchronous copies)
    ms += tm.ms(0, 1);
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
            if (ctx->n_views == 0 || ctx->h_views.size() != ctx->n_views) throw StatusError(MVS_ERR_STATE, std::string(who) + ": the context has no views (a view input comes first)");
            if (n_views != ctx->n_views)
                throw StatusError(MVS_ERR_INVALID, std::string(who) + ": n_views is " + std::to_string(n_views) + ", the context has " + std::to_string(ctx->n_views) + " views");
            if (lens)
                for (uint32_t j = 0; j < n_views; ++j) {
                    const std::string why = lens_refusal(lens[j]);
                    if (!why.empty()) throw StatusError(MVS_ERR_INVALID, std::string(who) + ": view " + std::to_string(j) + ": " + why);
                }
            std::vector<uint32_t> mv;   // the views that carry a mask
            for (uint32_t j = 0; masks && j < n_views; ++j) if (masks[j]) mv.push_back(j);
            if (mv.empty()) return;
            const size_t n = mv.size();
            const uint64_t cap = ctx->view_scratch_cap;
            std::vector<uint64_t> off(n + 1, 0), bytes(n);
            for (size_t k = 0; k < n; ++k) {
                const ViewParams& v = ctx->h_views[mv[k]];
                bytes[k] = (uint64_t)v.width * (uint64_t)v.height;
                off[k + 1] = off[k] + (uint64_t)((v.width + 31) / 32) * (uint64_t)v.height;
                st.pixels += bytes[k];
                if (!on_device && align16(bytes[k]) > cap)
                    throw StatusError(MVS_ERR_INVALID, std::string(who) + ": view " + std::to_string(mv[k]) + " needs " + std::to_string(align16(bytes[k])) + " bytes of staging, max_scratch_bytes is " + std::to_string(cap));
            }
            ViewMaskDev& D = row_dev(ctx->viewmask);
            D.keep.ensure((size_t)off[n] + 4); D.counter.ensure(2);
            MVS_HIP(hipMemsetAsync(D.counter.p, 0, sizeof(u64), ctx->stream));
            // batches: device masks are read where they lie, all in one; host masks in groups whose staged bytes fit the cap
            std::vector<size_t> cut{0};
            uint64_t most = 0;
            if (on_device) cut.push_back(n);
            else
                for (size_t a = 0; a < n;) {
                    size_t b = a; uint64_t sum = 0;
                    while (b < n && (b == a || sum + align16(bytes[b]) <= cap)) sum += align16(bytes[b]), ++b;
                    most = std::max(most, sum); cut.push_back(b); a = b;
                }
            uint8_t* staging = most ? lens_staging(ctx, most) : nullptr;
            st.staging_bytes = most;
            for (size_t g = 0; g + 1 < cut.size(); ++g) {
                std::vector<const uint8_t*> from; std::vector<uint8_t*> to; std::vector<size_t> nb;
                std::vector<PackView> P; std::vector<LensMaskView> Q;
                uint64_t so = 0;
                for (size_t k = cut[g]; k < cut[g + 1]; ++k) {
                    const uint32_t j = mv[k];
                    const ViewParams& v = ctx->h_views[j];
                    const uint8_t* src = masks[j];
                    if (!on_device) { from.push_back(masks[j]); to.push_back(staging + so); nb.push_back((size_t)bytes[k]); src = staging + so; so += align16(bytes[k]); }
                    uint32_t* keep = D.keep.p + off[k];
                    if (lens && lens[j].dist0 != 0.0f) Q.push_back(LensMaskView{src, keep, v.width, v.height, lens[j].flen, lens[j].dist0, lens[j].dist1, 0u});
                    else P.push_back(PackView{src, keep, v.width, v.height});
                }
                if (!from.empty()) {
                    const double t = now_ms_host();
                    upload_pieces_through_ring(ctx, from.data(), to.data(), nb.data(), from.size());
                    st.ms_upload += (float)(now_ms_host() - t);
                }
                pack_run(ctx, D, P, st.ms_pack);                      // (both return with the stream drained: the staging is free for the next batch)
                lens_mask_run(ctx, Q, st.ms_undistort);
                st.batches += 1; st.views_undistorted += Q.size();
            }
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
