// view_input.h -- the plumbing the view inputs share (api.hip set_views_impl, k_jpegdec.hip, k_lens.hip, k_viewmask.hip; DESIGN.md section 4
//   "Shared plumbing of the view input"): what a refused view input leaves behind (begin / commit), the context's image buffers, the checks,
//   the views that come as files, the hand-over of an mvs_rgb_set, the staging buffer and host items through it in groups, the span launch
//   and its two device-side searches.  view_batches.h holds the arithmetic.  Internal, header-only.
#pragma once
#include "rows.h"
#include "view_batches.h"
#include "lens.h"

namespace mvs {

// ---- one rule for every entry: after a refused view input the context has no views, and a data-cost pass is MVS_ERR_STATE until a
// view input succeeds.  begin() leaves exactly that state behind (a view input also clears the masks, and the masks of its views are
// staged under its cap); commit() hands over the finished views.  Nothing of the context's views is written in between.
inline void view_input_begin(mvs_ctx* ctx, uint64_t cap) {
    ctx->n_views = 0; ctx->h_views.clear(); ctx->have_costs = false; ctx->dc_phase = 0; ctx->views_refused = true;
    view_masks_clear(ctx); ctx->view_scratch_cap = cap; ctx->view_levels.clear();
}
inline void view_input_commit(mvs_ctx* ctx, std::vector<ViewParams>& hv, uint32_t n_views) { ctx->h_views.swap(hv); ctx->n_views = n_views; ctx->views_refused = false; }

// ---- the context's image buffers: those of an earlier call are reused (a context that serves one scene after another allocates once) ----
inline void own_images_keep(mvs_ctx* ctx, uint32_t n) { while (ctx->own_rgb.size() > n) { delete ctx->own_rgb.back(); ctx->own_rgb.pop_back(); } }
inline uint8_t* own_image(mvs_ctx* ctx, uint32_t j, const mvs_view& v) {   // view j's, with room for v (views come in order)
    if (ctx->own_rgb.size() <= j) ctx->own_rgb.push_back(new DBuf<uint8_t>());
    ctx->own_rgb[j]->ensure((size_t)v.width * v.height * 3 + 16);
    return ctx->own_rgb[j]->p;
}
// all views': hv[j] = view j as the kernels read it, its rgb the returned image[j]
inline std::vector<uint8_t*> own_images(mvs_ctx* ctx, const mvs_view* views, uint32_t n_views, std::vector<ViewParams>& hv) {
    own_images_keep(ctx, n_views);
    hv.assign(n_views, ViewParams{});
    std::vector<uint8_t*> image(n_views);
    for (uint32_t j = 0; j < n_views; ++j) { hv[j] = view_params_of(views[j]); hv[j].rgb = image[j] = own_image(ctx, j, views[j]); }
    return image;
}

// ---- checks; `who` starts the message where the entry has one ("" : the message starts with the view) ----
inline std::string view_msg(const char* who, uint32_t j) { return (*who ? std::string(who) + ": " : std::string()) + "view " + std::to_string(j) + ": "; }
inline void check_view_sizes(const mvs_view* views, uint32_t n, const char* who) {
    for (uint32_t j = 0; j < n; ++j) if (views[j].width < 2 || views[j].height < 2) throw StatusError(MVS_ERR_INVALID, view_msg(who, j) + "bad image");
}
inline void check_lenses(const mvs_lens* lens, uint32_t n, const char* who) {
    for (uint32_t j = 0; j < n; ++j) {
        const std::string why = lens_refusal(lens[j]);
        if (!why.empty()) throw StatusError(MVS_ERR_INVALID, view_msg(who, j) + why);
    }
}
// item k (view[k] of the caller's list) does not fit alone: "... needs N bytes of <what>, max_scratch_bytes is <cap>"
inline void refuse_over_cap(const std::vector<uint64_t>& need, uint64_t cap, const uint32_t* view, const char* who, const char* what) {
    const size_t k = first_over_cap(need.data(), need.size(), cap);
    if (k < need.size())
        throw StatusError(MVS_ERR_INVALID, std::string(who) + ": view " + std::to_string(view[k]) + " needs " + std::to_string(need[k]) + " bytes of " + what + ", max_scratch_bytes is " + std::to_string(cap));
}

// ---- the views that come as files: file k is view view[k] of the caller's list ----
struct FileViews { std::vector<const uint8_t*> files; std::vector<uint64_t> sizes; std::vector<uint32_t> view; };
inline FileViews file_views(const uint8_t* const* files, const uint64_t* sizes, uint32_t n_views) {
    FileViews f;
    for (uint32_t j = 0; files && j < n_views; ++j) if (files[j]) { f.files.push_back(files[j]); f.sizes.push_back(sizes[j]); f.view.push_back(j); }
    return f;
}

// ---- the routes on their own: n images back to back in `buf`, handed over as an mvs_rgb_set ----
struct RgbRoom { std::vector<uint64_t> off; std::vector<uint8_t*> dst; };   // offsets [n + 1], where image k starts
inline RgbRoom rgb_set_room(DBuf<uint8_t>& buf, const std::vector<uint32_t>& w, const std::vector<uint32_t>& h) {
    const size_t n = w.size();
    RgbRoom R{std::vector<uint64_t>(n + 1, 0), std::vector<uint8_t*>(n)};
    for (size_t k = 0; k < n; ++k) R.off[k + 1] = R.off[k] + 3ull * w[k] * h[k];
    buf.ensure((size_t)R.off[n] + 16);
    for (size_t k = 0; k < n; ++k) R.dst[k] = buf.p + R.off[k];
    return R;
}
inline void rgb_set_out(mvs_ctx* ctx, DBuf<uint8_t>& buf, const RgbRoom& R, const std::vector<uint32_t>& w, const std::vector<uint32_t>& h, int out_on_device, mvs_rgb_set* out) {
    const size_t n = w.size();
    download<mvs_rgb_set>(ctx->stream, out, mvs_rgb_set_free, [&] {
        out->n_images = (uint32_t)n; out->on_device = out_on_device ? 1u : 0u; out->n_bytes = R.off[n];
        out->offsets = (uint64_t*)malloc((n + 1) * sizeof(uint64_t)); out->width = (uint32_t*)malloc(std::max<size_t>(n, 1) * sizeof(uint32_t)); out->height = (uint32_t*)malloc(std::max<size_t>(n, 1) * sizeof(uint32_t));
        if (!out->offsets || !out->width || !out->height) throw StatusError(MVS_ERR_INVALID, "out of host memory");
        memcpy(out->offsets, R.off.data(), (n + 1) * sizeof(uint64_t));
        if (n) { memcpy(out->width, w.data(), n * sizeof(uint32_t)); memcpy(out->height, h.data(), n * sizeof(uint32_t)); }
        out->data = out_on_device ? buf.p : host_copy(buf.p, (size_t)R.off[n], ctx->stream);
    });
}

// ---- the staging buffer: what has to exist whole on the device before a kernel reads it -- a distorted image, a host mask -- lies
// here for the length of one batch.  Room for `bytes`, 16-byte aligned; growing it loses what it held.
inline uint8_t* view_staging(mvs_ctx* ctx, uint64_t bytes) { ctx->view_staging.ensure((size_t)bytes + 16); return ctx->view_staging.p; }
// Host items through the staging in groups whose bytes fit `cap`: item k is src[k][0, bytes[k]), view[k] of the caller's list; one that
// does not fit alone is refused.  Per group the items go up through the pinned ring (its time is added to ms_upload) and
// per_batch(first, last, at) finds item k at at[k - first]; it returns with the stream drained: the staging is free for the next
// group.  staging_bytes is raised to the bytes of the largest group before the first one goes up.
template <class PerBatch>
void stage_in_groups(mvs_ctx* ctx, const std::vector<const uint8_t*>& src, const std::vector<uint64_t>& bytes, const std::vector<uint32_t>& view, uint64_t cap,
                     const char* who, float& ms_upload, uint64_t& staging_bytes, PerBatch&& per_batch) {
    const size_t n = src.size();
    std::vector<uint64_t> need(n);
    for (size_t k = 0; k < n; ++k) need[k] = align16(bytes[k]);
    refuse_over_cap(need, cap, view.data(), who, "staging");
    const std::vector<size_t> cut = cut_batches(need.data(), n, cap);
    const BatchLayout L = batch_layout(bytes.data(), n, cut);
    if (!L.most) return;
    uint8_t* staging = view_staging(ctx, L.most);
    staging_bytes = std::max(staging_bytes, L.most);
    for (size_t g = 0; g + 1 < cut.size(); ++g) {
        std::vector<uint8_t*> at; std::vector<size_t> nb;
        for (size_t k = cut[g]; k < cut[g + 1]; ++k) { at.push_back(staging + L.off[k]); nb.push_back((size_t)bytes[k]); }
        const double t = now_ms_host();
        upload_pieces_through_ring(ctx, src.data() + cut[g], at.data(), nb.data(), at.size());
        ms_upload += (float)(now_ms_host() - t);
        per_batch(cut[g], cut[g + 1], at);
    }
}

// ---- the span launch: ONE launch for all items of a batch.  T is the per-item table; its prefix array ptr (view_batches.h span_prefix)
// numbers the count(T[k]) pieces of work of every item, lanes_per_item lanes each.  Uploads both, launch(blocks, n, ptr[n]) between two
// timing marks, then after() (a read-back that wants the same drain), and drains the stream: T and ptr were read by asynchronous copies.
// Returns the launch's device time; nothing happens for an empty T.
inline uint64_t keep_words(int32_t width, int32_t height) { return (uint64_t)(((uint32_t)width + 31u) / 32u) * (uint64_t)height; }   // of a view's keep words
template <class V, class Count, class Launch>
float span_launch(hipStream_t s, const std::vector<V>& T, Count&& count, uint32_t lanes_per_item, uint32_t threads, bool bound_on_lanes,
                  DBuf<V>& d_table, DBuf<unsigned long long>& d_ptr, const char* who, Launch&& launch, const std::function<void()>& after = {}) {
    if (T.empty()) return 0.0f;
    std::vector<uint64_t> counts(T.size());
    for (size_t k = 0; k < T.size(); ++k) counts[k] = count(T[k]);
    const std::vector<unsigned long long> ptr = span_prefix(counts);
    uint64_t blocks = 0;
    if (!span_blocks(ptr.back() * lanes_per_item, threads, bound_on_lanes, blocks)) throw StatusError(MVS_ERR_UNSUPPORTED, std::string(who) + ": too many pixels in one batch (lower max_scratch_bytes)");
    upload(d_table, T, s); upload(d_ptr, ptr, s);
    StageTimer<2> tm(s);
    tm.mark();
    if (blocks) { launch((unsigned)blocks, (uint32_t)T.size(), ptr.back()); MVS_LAUNCH_CHECK(); }
    tm.mark();
    if (after) after();
    MVS_HIP(hipStreamSynchronize(s));
    return tm.ms(0, 1);
}

// ---- on the device: the item that owns g, lo with ptr[lo] <= g < ptr[lo + 1] (g < ptr[n]): by binary search in every lane ... ----
__device__ __forceinline__ uint32_t span_of(const unsigned long long* __restrict__ ptr, uint32_t n, unsigned long long g) {
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1u) { const uint32_t mid = lo + (hi - lo) / 2u; if (ptr[mid] <= g) lo = mid; else hi = mid; }
    return lo;
}
// ... or for the block's first g (g0 < ptr[n]: the grid has no empty block) once per block, a lane walks on from there (a block seldom
// spans two items).  With the search in every lane mask_pack_kernel ran at 405 GB/s at config 3: eight dependent loads in front of two
// independent ones.  Every lane of the block calls it (s_lo: the block's __shared__ word; a barrier inside); g >= total = ptr[n] gets n.
__device__ __forceinline__ uint32_t block_span_of(const unsigned long long* __restrict__ ptr, uint32_t n, unsigned long long g0, unsigned long long g, unsigned long long total,
                                                  uint32_t& s_lo) {
    if (threadIdx.x == 0) s_lo = span_of(ptr, n, g0);
    __syncthreads();
    if (g >= total) return n;
    uint32_t lo = s_lo;
    while (ptr[lo + 1] <= g) ++lo;   // g < ptr[n]: ends at lo <= n - 1
    return lo;
}

}  // namespace mvs
