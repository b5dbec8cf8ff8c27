// mgpu.hip -- libmvs_blocks.so: the building blocks of include/mvs_viewsel_blocks.h (per-phase sweeps of a node range, gather /
// scatter of halo elements, the data-cost reduce hooks).  NOT in the product library: the product's sharded driver is csrc/shard.hip.
// The collectives themselves are issued by whoever drives these blocks (the test harness tests/tools/multigpu.py) on its own
// device buffers; these entry points only move data between those buffers and the solver's arrays and run the per-range kernels.
#include "ctx.h"
#include "../../include/mvs_viewsel_blocks.h"
#include <vector>

namespace mvs {
namespace {
// st != null: the array is the CURRENT decode buffer, i.e. offset st->w * buf_stride (the step kernel flips w on the device)
__global__ void gather_kernel(const uint32_t* __restrict__ src, const mvs_mrf_progress* __restrict__ st, uint32_t buf_stride, const uint32_t* __restrict__ idx, uint64_t n, uint32_t* __restrict__ dst) {
    if (st) src += (size_t)st->w * buf_stride;
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (uint64_t)gridDim.x * blockDim.x) dst[k] = src[idx[k]];
}
__global__ void scatter_kernel(uint32_t* __restrict__ dst, const mvs_mrf_progress* __restrict__ st, uint32_t buf_stride, const uint32_t* __restrict__ idx, uint64_t n, const uint32_t* __restrict__ src) {
    if (st) dst += (size_t)st->w * buf_stride;
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (uint64_t)gridDim.x * blockDim.x) dst[idx[k]] = src[k];
}
// combined addressing: index < 2^31 -> array a (messages), else array b[index & 0x7FFFFFFF] (labels):
// one gather / scatter per sweep moves cut-edge messages AND boundary labels
// message elements are 8-bit codes: moved zero-extended in 4-byte exchange words
__global__ void gather_msg_kernel(const uint8_t* __restrict__ src, const uint32_t* __restrict__ idx, uint64_t n, uint32_t* __restrict__ dst) {
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (uint64_t)gridDim.x * blockDim.x) dst[k] = src[idx[k]];
}
__global__ void scatter_msg_kernel(uint8_t* __restrict__ dst, const uint32_t* __restrict__ idx, uint64_t n, const uint32_t* __restrict__ src) {
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (uint64_t)gridDim.x * blockDim.x) dst[idx[k]] = (uint8_t)src[k];
}
__global__ void gather2_kernel(const uint8_t* __restrict__ a, const uint32_t* __restrict__ b, const mvs_mrf_progress* __restrict__ st, uint32_t buf_stride, const uint32_t* __restrict__ idx, uint64_t n, uint32_t* __restrict__ dst) {
    b += (size_t)st->w * buf_stride;
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t i = idx[k];
        dst[k] = (i & 0x80000000u) ? b[i & 0x7FFFFFFFu] : a[i];
    }
}
__global__ void scatter2_kernel(uint8_t* __restrict__ a, uint32_t* __restrict__ b, const mvs_mrf_progress* __restrict__ st, uint32_t buf_stride, const uint32_t* __restrict__ idx, uint64_t n, const uint32_t* __restrict__ src) {
    b += (size_t)st->w * buf_stride;
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t i = idx[k];
        if (i & 0x80000000u) b[i & 0x7FFFFFFFu] = src[k]; else a[i] = (uint8_t)src[k];
    }
}
__global__ void counts_kernel(const uint32_t* __restrict__ col_ptr, uint32_t n, uint32_t* __restrict__ counts) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) counts[i] = col_ptr[i + 1] - col_ptr[i];
}
}  // namespace

static uint8_t* mrf_msg(mvs_ctx* ctx) { return ctx->m_msg_a.p; }  // one buffer, updated in place
// LAB = the current decode buffer (resolved on the device through the solver state), BEST_LAB = the best labeling's buffer
static uint32_t* mrf_array(mvs_ctx* ctx, int which, const mvs_mrf_progress** st) {
    *st = nullptr;
    switch (which) {
        case MVS_MRF_LAB: *st = ctx->m_state.p; return ctx->m_lab.p;
        case MVS_MRF_GAIN: return (uint32_t*)ctx->m_gain.p;
        case MVS_MRF_BEST_LAB: resolve_best(ctx); return ctx->b_lab;
    }
    throw StatusError(MVS_ERR_INVALID, "bad array selector");
}
}  // namespace mvs

using namespace mvs;

extern "C" {

mvs_status mvs_ctx_dc_get_max(mvs_ctx* ctx, float* dst) {
    if (!ctx || !dst) return api_fail(MVS_ERR_INVALID, "null argument");
    if (ctx->dc_phase < 1) return api_fail(MVS_ERR_STATE, "dc_phase1 first");
    MVS_CTX_API_BEGIN
    MVS_HIP(hipMemcpyAsync(dst, ctx->max_q.p, sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
    MVS_API_END
}
mvs_status mvs_ctx_dc_set_max(mvs_ctx* ctx, const float* src) {
    if (!ctx || !src) return api_fail(MVS_ERR_INVALID, "null argument");
    if (ctx->dc_phase < 1) return api_fail(MVS_ERR_STATE, "dc_phase1 first");
    MVS_CTX_API_BEGIN
    MVS_HIP(hipMemcpyAsync(ctx->max_q.p, src, sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
    MVS_API_END
}
mvs_status mvs_ctx_dc_get_histogram(mvs_ctx* ctx, uint32_t* dst) {
    if (!ctx || !dst) return api_fail(MVS_ERR_INVALID, "null argument");
    if (ctx->dc_phase < 2) return api_fail(MVS_ERR_STATE, "dc_phase2 first");
    MVS_CTX_API_BEGIN
    MVS_HIP(hipMemcpyAsync(dst, ctx->hist.p, MVS_HIST_WORDS * sizeof(uint32_t), hipMemcpyDeviceToDevice, ctx->stream));
    MVS_API_END
}
mvs_status mvs_ctx_dc_set_histogram(mvs_ctx* ctx, const uint32_t* src) {
    if (!ctx || !src) return api_fail(MVS_ERR_INVALID, "null argument");
    if (ctx->dc_phase < 2) return api_fail(MVS_ERR_STATE, "dc_phase2 first");
    MVS_CTX_API_BEGIN
    MVS_HIP(hipMemcpyAsync(ctx->hist.p, src, MVS_HIST_WORDS * sizeof(uint32_t), hipMemcpyDeviceToDevice, ctx->stream));
    MVS_API_END
}

mvs_status mvs_ctx_costs_export(mvs_ctx* ctx, uint32_t* counts, uint16_t* view_id, float* cost) {
    if (!ctx || !counts) return api_fail(MVS_ERR_INVALID, "null argument");
    if (!ctx->have_costs) return api_fail(MVS_ERR_STATE, "no data costs on the device");
    MVS_CTX_API_BEGIN
    const uint32_t F = ctx->csr_faces;
    if (F) { hipLaunchKernelGGL(counts_kernel, dim3((F + 255) / 256), dim3(256), 0, ctx->stream, ctx->r_ptr, F, counts); MVS_LAUNCH_CHECK(); }
    if (ctx->csr_nnz && view_id) MVS_HIP(hipMemcpyAsync(view_id, ctx->r_view, ctx->csr_nnz * sizeof(uint16_t), hipMemcpyDeviceToDevice, ctx->stream));
    if (ctx->csr_nnz && cost) MVS_HIP(hipMemcpyAsync(cost, ctx->r_cost, ctx->csr_nnz * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
    MVS_API_END
}

// harness only: need / occluded bits of the last data-cost pass (k_dc.hip dc_phase1 -> k_bvh.hip trace_rays), device rows in curve order ->
// host rows in the caller's vertex numbering through vperm (position s of the curve = the caller's vertex vperm[s])
mvs_status mvs_ctx_ray_bits(mvs_ctx* ctx, int which, void* out_host, uint64_t cap_bytes, uint64_t* n_bytes) {
    if (!ctx || !n_bytes || which < 0 || which > 2) return api_fail(MVS_ERR_INVALID, "bad argument");
    // dc_stats.pairs: set by the pass over the scene (faces of the range x views), zero after mvs_postprocess_face_infos
    const uint64_t whole = (uint64_t)ctx->n_faces * ctx->n_views;
    if (ctx->dc_phase < 1 || !ctx->dc_settings.geometric_visibility_test || whole == 0 || ctx->n_verts == 0 || ctx->dc_stats.pairs != whole ||
        ctx->face_begin != 0 || ctx->face_end != ctx->n_faces || !ctx->need_bits.p || !ctx->occl_bits.p || !ctx->vperm.p)
        return api_fail(MVS_ERR_STATE, "ray bits: needs a data-cost pass with the visibility test over the whole mesh");
    // after a ranged pass (k_dc.hip dc_ranged) the matrices hold the LAST range's rays only
    if (which < 2 && ctx->dc_n_ranges > 1)
        return api_fail(MVS_ERR_STATE, "ray bits: the last data-cost pass evaluated the faces in " + std::to_string(ctx->dc_n_ranges) + " ranges (option dc_range_pairs); the matrices hold the last range only");
    MVS_CTX_API_BEGIN
    const uint32_t NV = ctx->n_verts, V = ctx->n_views, vwords = (NV + 63) / 64;
    const uint64_t words = (uint64_t)V * vwords, n = which == 2 ? (uint64_t)NV * sizeof(uint32_t) : words * sizeof(unsigned long long);
    *n_bytes = n;
    if (out_host && cap_bytes < n) throw StatusError(MVS_ERR_INVALID, "ray bits: buffer too small");
    if (out_host && which == 2) {
        MVS_HIP(hipMemcpyAsync(out_host, ctx->vperm.p, n, hipMemcpyDeviceToHost, ctx->stream));
        MVS_HIP(hipStreamSynchronize(ctx->stream));
    } else if (out_host) {
        std::vector<unsigned long long> dev(words);
        std::vector<uint32_t> vperm(NV);
        MVS_HIP(hipMemcpyAsync(dev.data(), which == 0 ? ctx->need_bits.p : ctx->occl_bits.p, n, hipMemcpyDeviceToHost, ctx->stream));
        MVS_HIP(hipMemcpyAsync(vperm.data(), ctx->vperm.p, (size_t)NV * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
        MVS_HIP(hipStreamSynchronize(ctx->stream));
        unsigned long long* out = (unsigned long long*)out_host;
        memset(out, 0, n);
        for (uint32_t j = 0; j < V; ++j)
            for (uint32_t s = 0; s < NV; ++s)
                if ((dev[(size_t)j * vwords + (s >> 6)] >> (s & 63u)) & 1ull) {
                    const uint32_t v = vperm[s];
                    if (v >= NV) throw StatusError(MVS_ERR_STATE, "ray bits: vertex order is not a permutation");
                    out[(size_t)j * vwords + (v >> 6)] |= 1ull << (v & 63u);
                }
        // lanes behind the last vertex of a row must be clear on the device: they have no vertex to be mapped to
        if (NV & 63u)
            for (uint32_t j = 0; j < V; ++j)
                if (dev[(size_t)j * vwords + vwords - 1] >> (NV & 63u)) throw StatusError(MVS_ERR_STATE, "ray bits: a bit behind the last vertex is set");
    }
    MVS_API_END
}

// harness only: what the image preparation of the last data-cost pass (k_prep.hip prepare_views) left on the device, copied out as it lies:
// nothing is launched.  The pass that ran the preparation is the last one that evaluated (face, view) pairs -- a ranged pass prepares in its
// first range and keeps the products resident for the others, a rank of the sharded driver prepares for itself -- so every such state is served.
mvs_status mvs_ctx_prep_products(mvs_ctx* ctx, int which, uint32_t view, void* out_host, uint64_t cap_bytes, uint64_t* n_bytes) {
    if (!ctx || !n_bytes || which < 0 || which > 3) return api_fail(MVS_ERR_INVALID, "bad argument");
    const uint32_t V = ctx->n_views;
    // dc_stats.pairs: set by a pass over the scene, zero after mvs_postprocess_face_infos and for a pass with nothing to evaluate (no preparation either)
    if (ctx->dc_phase < 1 || V == 0 || ctx->dc_stats.pairs == 0 || ctx->h_views.size() != V || ctx->mask_off.size() != (size_t)V + 1 ||
        ctx->gmi_off.size() != (size_t)V + 1 || ctx->msum_off.size() != (size_t)V + 1 || !ctx->d_views.p || !ctx->mask_all.p || !ctx->msum_all.p)
        return api_fail(MVS_ERR_STATE, "prep products: needs a data-cost pass that evaluated the scene's views");
    const bool have_gmi = ctx->dc_settings.data_term == MVS_DATA_TERM_GMI;
    if (which == 0 && !have_gmi) return api_fail(MVS_ERR_STATE, "prep products: the last data-cost pass ran the area term: there is no gradient-magnitude image");
    if (which != 3 && view >= V) return api_fail(MVS_ERR_INVALID, "prep products: view " + std::to_string(view) + " of " + std::to_string(V));
    MVS_CTX_API_BEGIN
    const ViewParams& hv = ctx->h_views[which == 3 ? 0 : view];
    const void* src = nullptr; uint64_t n = 0;
    if (which == 0) { src = ctx->gmi_all.p + ctx->gmi_off[view]; n = (uint64_t)hv.width * hv.height; }
    else if (which == 1) { src = ctx->mask_all.p + ctx->mask_off[view]; n = (uint64_t)hv.height * hv.mask_stride * sizeof(uint32_t); }
    else if (which == 2) { src = ctx->msum_all.p + ctx->msum_off[view]; n = (uint64_t)((hv.height + 31) / 32) * hv.msum_stride * sizeof(uint32_t); }
    else n = V;
    *n_bytes = n;
    if (out_host && cap_bytes < n) throw StatusError(MVS_ERR_INVALID, "prep products: buffer too small");
    if (out_host && which == 3) {   // the DEVICE copy of the view table: the host copy keeps every mask pointer
        std::vector<ViewParams> dv(V);
        MVS_HIP(hipMemcpyAsync(dv.data(), ctx->d_views.p, (size_t)V * sizeof(ViewParams), hipMemcpyDeviceToHost, ctx->stream));
        MVS_HIP(hipStreamSynchronize(ctx->stream));
        for (uint32_t j = 0; j < V; ++j) ((uint8_t*)out_host)[j] = dv[j].mask ? 1 : 0;
    } else if (out_host) {
        MVS_HIP(hipMemcpyAsync(out_host, src, n, hipMemcpyDeviceToHost, ctx->stream));
        MVS_HIP(hipStreamSynchronize(ctx->stream));
    }
    MVS_API_END
}

// harness only: a host table in position order + the order itself -> the state name_table_order (k_dc.hip) leaves behind a pass over the
// whole mesh.  f_perm / f_pos carry it: they no longer describe the resident mesh (mesh_ordered = false; every data-cost pass derives the
// mesh's order again before it reads them), and a shard that pinned them keeps them.
mvs_status mvs_ctx_costs_upload_ordered(mvs_ctx* ctx, const mvs_csr* csr, const uint32_t* order) {
    if (!ctx || !csr || !csr->col_ptr || (!order && csr->n_faces)) return api_fail(MVS_ERR_INVALID, "null argument");
    if (ctx->order_pinned) return api_fail(MVS_ERR_STATE, "ordered upload: a shard owns this context's face order");
    const uint32_t F = csr->n_faces;
    std::vector<uint32_t> pos(F, 0xFFFFFFFFu);
    for (uint32_t p = 0; p < F; ++p) {
        const uint32_t id = order[p];
        if (id >= F) return api_fail(MVS_ERR_INVALID, "ordered upload: order[" + std::to_string(p) + "] = " + std::to_string(id) + " is no face id (n_faces = " + std::to_string(F) + ")");
        if (pos[id] != 0xFFFFFFFFu) return api_fail(MVS_ERR_INVALID, "ordered upload: face " + std::to_string(id) + " stands at positions " + std::to_string(pos[id]) + " and " + std::to_string(p) + ": not a permutation");
        pos[id] = p;
    }
    const mvs_status st = mvs_ctx_costs_upload(ctx, csr, 0);
    if (st != MVS_OK) return st;
    MVS_CTX_API_BEGIN
    ctx->mesh_ordered = false;
    ctx->f_perm.ensure((size_t)F + 1); ctx->f_pos.ensure((size_t)F + 1);
    if (F) {
        MVS_HIP(hipMemcpyAsync(ctx->f_perm.p, order, (size_t)F * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
        MVS_HIP(hipMemcpyAsync(ctx->f_pos.p, pos.data(), (size_t)F * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
        MVS_HIP(hipStreamSynchronize(ctx->stream));
    }
    ctx->t_perm = ctx->f_perm.p; ctx->t_pos = ctx->f_pos.p;
    MVS_API_END
}

// harness only: the texel table tone mapping `gamma` reads in rows f5, f6 and f10 (k_tone.hip); null = the gamma table of tone.h again
mvs_status mvs_ctx_tone_table(mvs_ctx* ctx, const float* table256) {
    if (!ctx) return api_fail(MVS_ERR_INVALID, "null argument");
    MVS_CTX_API_BEGIN
    tone_table_set(ctx, table256);
    MVS_API_END
}

// harness only: the context's image of one view as it lies on the device
// harness only: the keep words of view `view` as mvs_scene_set_view_masks left them (height * mask_stride words); *n_bytes == 0: the view has no mask
mvs_status mvs_ctx_view_keep_words(mvs_ctx* ctx, uint32_t view, void* out_host, uint64_t cap_bytes, uint64_t* n_bytes) {
    if (!ctx || !n_bytes) return api_fail(MVS_ERR_INVALID, "null argument");
    if (ctx->n_views == 0) return api_fail(MVS_ERR_STATE, "view keep words: the context has no views");
    if (view >= ctx->n_views) return api_fail(MVS_ERR_INVALID, "view keep words: view " + std::to_string(view) + " of " + std::to_string(ctx->n_views));
    MVS_CTX_API_BEGIN
    std::vector<const uint32_t*> table;
    const uint32_t* src = view_keep_words(ctx, view, table);
    const ViewParams& hv = ctx->h_views[view];
    const uint64_t n = src ? (uint64_t)hv.height * (uint64_t)((hv.width + 31) / 32) * sizeof(uint32_t) : 0;
    *n_bytes = n;
    if (out_host && cap_bytes < n) throw StatusError(MVS_ERR_INVALID, "view keep words: buffer too small");
    if (out_host && n) {
        MVS_HIP(hipMemcpyAsync(out_host, src, n, hipMemcpyDeviceToHost, ctx->stream));
        MVS_HIP(hipStreamSynchronize(ctx->stream));
    }
    MVS_API_END
}

mvs_status mvs_ctx_view_image(mvs_ctx* ctx, uint32_t view, void* out_host, uint64_t cap_bytes, uint64_t* n_bytes) {
    if (!ctx || !n_bytes) return api_fail(MVS_ERR_INVALID, "null argument");
    if (ctx->n_views == 0) return api_fail(MVS_ERR_STATE, "view image: the context has no views");
    if (view >= ctx->n_views) return api_fail(MVS_ERR_INVALID, "view image: view " + std::to_string(view) + " of " + std::to_string(ctx->n_views));
    MVS_CTX_API_BEGIN
    const ViewParams& hv = ctx->h_views[view];
    const uint64_t n = (uint64_t)hv.width * hv.height * 3;
    *n_bytes = n;
    if (out_host && cap_bytes < n) throw StatusError(MVS_ERR_INVALID, "view image: buffer too small");
    if (out_host) {
        MVS_HIP(hipMemcpyAsync(out_host, hv.rgb, n, hipMemcpyDeviceToHost, ctx->stream));
        MVS_HIP(hipStreamSynchronize(ctx->stream));
    }
    MVS_API_END
}

mvs_status mvs_ctx_mrf_setup(mvs_ctx* ctx, const uint32_t* adj_ptr, const uint32_t* adj, int adj_on_device, const mvs_mrf_params* params) {
    if (!ctx || !adj_ptr || !adj) return api_fail(MVS_ERR_INVALID, "null argument");
    if (!ctx->have_costs) return api_fail(MVS_ERR_STATE, "mrf setup needs data costs");
    MVS_CTX_API_BEGIN
    mvs_mrf_params P; if (params) P = *params; else mvs_mrf_default_params(&P);
    set_adjacency(ctx, adj_ptr, adj, adj_on_device, false);
    mrf_setup(ctx, &P);
    MVS_API_END
}

mvs_status mvs_ctx_mrf_sweep(mvs_ctx* ctx, uint32_t nb0, uint32_t ne0) {
    if (!ctx || nb0 > ne0 || ne0 > ctx->csr_faces) return api_fail(MVS_ERR_INVALID, "bad node range");
    MVS_CTX_API_BEGIN
    Prof pr(ctx, "mrf_sweep");
    mrf_sweep(ctx, nb0, ne0);
    MVS_API_END
}

mvs_status mvs_ctx_mrf_sweep_phase(mvs_ctx* ctx, uint32_t phase, uint32_t nb0, uint32_t ne0) {
    if (!ctx || nb0 > ne0 || ne0 > ctx->csr_faces || phase >= ctx->m_colours) return api_fail(MVS_ERR_INVALID, "bad phase or node range");
    MVS_CTX_API_BEGIN
    Prof pr(ctx, "mrf_sweep");
    mrf_sweep_phase(ctx, phase, nb0, ne0);
    MVS_API_END
}
/* the set-up with BOUNDARY MARKS (marks_device[i] != 0: node i goes to the boundary zone of its colour class, see mrf.h "zones") and one
 * zone of a colour phase: what csrc/shard.hip does per rank, for drivers / measuring scripts one level below it */
mvs_status mvs_ctx_mrf_setup_marked(mvs_ctx* ctx, const uint32_t* adj_ptr, const uint32_t* adj, int adj_on_device, const mvs_mrf_params* params, const uint8_t* marks_device) {
    if (!ctx || !adj_ptr || !adj) return api_fail(MVS_ERR_INVALID, "null argument");
    if (!ctx->have_costs) return api_fail(MVS_ERR_STATE, "mrf setup needs data costs");
    MVS_CTX_API_BEGIN
    mvs_mrf_params P; if (params) P = *params; else mvs_mrf_default_params(&P);
    set_adjacency(ctx, adj_ptr, adj, adj_on_device, false);
    struct Marks { mvs_ctx* c; ~Marks() { c->m_bnd = nullptr; } } marks{ctx};
    ctx->m_bnd = marks_device;
    mrf_setup(ctx, &P);
    MVS_API_END
}
mvs_status mvs_ctx_mrf_sweep_phase_part(mvs_ctx* ctx, uint32_t phase, uint32_t nb0, uint32_t ne0, int part) {
    if (!ctx || nb0 > ne0 || ne0 > ctx->csr_faces || phase >= ctx->m_colours || part < 0 || part > 2) return api_fail(MVS_ERR_INVALID, "bad phase, node range or part");
    MVS_CTX_API_BEGIN
    Prof pr(ctx, part == MRF_PART_BOUNDARY ? "mrf_sweep_boundary" : "mrf_sweep");
    mrf_sweep_phase(ctx, phase, nb0, ne0, part);
    MVS_API_END
}
mvs_status mvs_ctx_mrf_setup_tables(mvs_ctx* ctx, int which, void* out_host, uint64_t cap_bytes, uint64_t* n_bytes) {
    if (!ctx || !n_bytes || which < 0 || which > 3) return api_fail(MVS_ERR_INVALID, "bad argument");
    if (!ctx->m_state.p) return api_fail(MVS_ERR_STATE, "mrf setup first");
    MVS_CTX_API_BEGIN
    const uint32_t F = ctx->csr_faces, n_fast = ctx->m_n_fast;
    const void* src = nullptr; uint64_t n = 0, route = ctx->m_bitmaps ? 1u : 0u;
    if (which == 0) { n = sizeof(route); }
    else if (which == 1 && n_fast) {   // roff[F] = words of all records, still where the set-up's scan left it
        uint32_t words = 0;
        MVS_HIP(hipMemcpyAsync(&words, ctx->m_tmp_b.p + F, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
        MVS_HIP(hipStreamSynchronize(ctx->stream));
        src = ctx->m_rec.p; n = ((uint64_t)MRF_REC_BASE + words) * sizeof(uint32_t);
    }
    else if (which == 2 && n_fast) { src = ctx->m_desc.p; n = (uint64_t)n_fast * sizeof(NodeDesc); }
    else if (which == 3) { src = ctx->m_ident.p; n = ctx->m_n_adj; }
    *n_bytes = n;
    if (out_host && n) {
        if (cap_bytes < n) throw StatusError(MVS_ERR_INVALID, "setup tables: buffer too small");
        if (which == 0) memcpy(out_host, &route, sizeof(route));
        else { MVS_HIP(hipMemcpyAsync(out_host, src, n, hipMemcpyDeviceToHost, ctx->stream)); MVS_HIP(hipStreamSynchronize(ctx->stream)); }
    }
    MVS_API_END
}
mvs_status mvs_ctx_mrf_layout(mvs_ctx* ctx, uint32_t* in_off_host, uint64_t n_edges) {
    if (!ctx || (n_edges && !in_off_host)) return api_fail(MVS_ERR_INVALID, "null argument");
    MVS_CTX_API_BEGIN
    // MrfEdge = {in_off, out_off, kj}: strided copy of the first member
    if (n_edges) MVS_HIP(hipMemcpy2DAsync(in_off_host, sizeof(uint32_t), ctx->m_edge.p, sizeof(MrfEdge), sizeof(uint32_t), n_edges, hipMemcpyDeviceToHost, ctx->stream));
    MVS_HIP(hipStreamSynchronize(ctx->stream));
    MVS_API_END
}

mvs_status mvs_ctx_mrf_gather(mvs_ctx* ctx, int which, const uint32_t* idx, uint64_t n, void* dst) {
    if (!ctx || (n && (!idx || !dst))) return api_fail(MVS_ERR_INVALID, "null argument");
    MVS_CTX_API_BEGIN
    if (n && which == MVS_MRF_MSG_LAB) {
        if (ctx->m_total >= 0x80000000ull) throw StatusError(MVS_ERR_UNSUPPORTED, "combined addressing needs < 2^31 message words");
        hipLaunchKernelGGL(gather2_kernel, dim3((unsigned)std::min<uint64_t>((n + 255) / 256, 4096)), dim3(256), 0, ctx->stream, mrf_msg(ctx), ctx->m_lab.p, ctx->m_state.p, ctx->m_stride, idx, n, (uint32_t*)dst);
        MVS_LAUNCH_CHECK();
    } else if (n && which == MVS_MRF_MSG) {
        hipLaunchKernelGGL(gather_msg_kernel, dim3((unsigned)std::min<uint64_t>((n + 255) / 256, 4096)), dim3(256), 0, ctx->stream, mrf_msg(ctx), idx, n, (uint32_t*)dst);
        MVS_LAUNCH_CHECK();
    } else if (n) {
        const mvs_mrf_progress* st; const uint32_t* arr = mrf_array(ctx, which, &st);
        hipLaunchKernelGGL(gather_kernel, dim3((unsigned)std::min<uint64_t>((n + 255) / 256, 4096)), dim3(256), 0, ctx->stream, arr, st, ctx->m_stride, idx, n, (uint32_t*)dst);
        MVS_LAUNCH_CHECK();
    }
    MVS_API_END
}
mvs_status mvs_ctx_mrf_scatter(mvs_ctx* ctx, int which, const uint32_t* idx, uint64_t n, const void* src) {
    if (!ctx || (n && (!idx || !src))) return api_fail(MVS_ERR_INVALID, "null argument");
    MVS_CTX_API_BEGIN
    if (n) { ctx->icm_dirty_valid = false; ctx->exact_valid = false; }   // labels changed behind the ICM active set
    if (n && which == MVS_MRF_MSG_LAB) {
        hipLaunchKernelGGL(scatter2_kernel, dim3((unsigned)std::min<uint64_t>((n + 255) / 256, 4096)), dim3(256), 0, ctx->stream, mrf_msg(ctx), ctx->m_lab.p, ctx->m_state.p, ctx->m_stride, idx, n, (const uint32_t*)src);
        MVS_LAUNCH_CHECK();
    } else if (n && which == MVS_MRF_MSG) {
        hipLaunchKernelGGL(scatter_msg_kernel, dim3((unsigned)std::min<uint64_t>((n + 255) / 256, 4096)), dim3(256), 0, ctx->stream, mrf_msg(ctx), idx, n, (const uint32_t*)src);
        MVS_LAUNCH_CHECK();
    } else if (n) {
        const mvs_mrf_progress* st; uint32_t* arr = mrf_array(ctx, which, &st);
        hipLaunchKernelGGL(scatter_kernel, dim3((unsigned)std::min<uint64_t>((n + 255) / 256, 4096)), dim3(256), 0, ctx->stream, arr, st, ctx->m_stride, idx, n, (const uint32_t*)src);
        MVS_LAUNCH_CHECK();
    }
    MVS_API_END
}

mvs_status mvs_ctx_mrf_energy(mvs_ctx* ctx, int which_sel, uint32_t nb0, uint32_t ne0, uint64_t* dst) {
    if (!ctx || !dst || nb0 > ne0 || ne0 > ctx->csr_faces) return api_fail(MVS_ERR_INVALID, "bad argument");
    if (which_sel != MVS_MRF_LAB && which_sel != MVS_MRF_BEST_LAB) return api_fail(MVS_ERR_INVALID, "energy: LAB or BEST_LAB");
    MVS_CTX_API_BEGIN
    mrf_energy(ctx, which_sel == MVS_MRF_BEST_LAB, nb0, ne0);
    MVS_HIP(hipMemcpyAsync(dst, ctx->m_energy.p, 2 * sizeof(uint64_t), hipMemcpyDeviceToDevice, ctx->stream));
    MVS_API_END
}

mvs_status mvs_ctx_mrf_keep_best(mvs_ctx* ctx) {
    if (!ctx) return api_fail(MVS_ERR_INVALID, "ctx is null");
    MVS_CTX_API_BEGIN
    mrf_keep_best(ctx);
    MVS_API_END
}

mvs_status mvs_ctx_mrf_step(mvs_ctx* ctx, const uint64_t* energy_device) {
    if (!ctx) return api_fail(MVS_ERR_INVALID, "ctx is null");
    MVS_CTX_API_BEGIN
    mrf_step(ctx, (const unsigned long long*)energy_device);
    MVS_API_END
}
mvs_status mvs_ctx_mrf_poll(mvs_ctx* ctx, uint32_t step, mvs_mrf_progress* out) {
    if (!ctx || !out) return api_fail(MVS_ERR_INVALID, "null argument");
    MVS_CTX_API_BEGIN
    mrf_poll(ctx, step, out);
    MVS_API_END
}

mvs_status mvs_ctx_mrf_icm_gain(mvs_ctx* ctx, uint32_t nb0, uint32_t ne0) {
    if (!ctx || nb0 > ne0 || ne0 > ctx->csr_faces) return api_fail(MVS_ERR_INVALID, "bad node range");
    MVS_CTX_API_BEGIN
    mrf_icm_gain(ctx, nb0, ne0);
    MVS_API_END
}
mvs_status mvs_ctx_mrf_icm_apply(mvs_ctx* ctx, uint32_t nb0, uint32_t ne0, uint32_t* moved) {
    if (!ctx || !moved || nb0 > ne0 || ne0 > ctx->csr_faces) return api_fail(MVS_ERR_INVALID, "bad argument");
    MVS_CTX_API_BEGIN
    mrf_icm_apply(ctx, nb0, ne0);  // in place: winners form an independent set
    MVS_HIP(hipMemcpyAsync(moved, &ctx->words->icm_n_moved, sizeof(uint32_t), hipMemcpyDeviceToDevice, ctx->stream));
    MVS_API_END
}

mvs_status mvs_ctx_mrf_labels(mvs_ctx* ctx, uint32_t nb0, uint32_t ne0, uint32_t* labels, uint32_t* unseen_out) {
    if (!ctx || !labels || nb0 > ne0 || ne0 > ctx->csr_faces) return api_fail(MVS_ERR_INVALID, "bad argument");
    MVS_CTX_API_BEGIN
    uint32_t bu[2];
    mrf_labels(ctx, nb0, ne0, labels, bu);
    if (unseen_out) *unseen_out = bu[1];
    if (bu[0]) throw StatusError(MVS_ERR_LABELING, "Incorrect labeling");
    MVS_API_END
}

}  // extern "C"
