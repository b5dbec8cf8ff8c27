// k_debug.hip -- row f10: the view-selection debug model (texrecon.cpp:216-236, generate_debug_embeddings.cpp): every view's image
//   replaced by a flat colour of its own stamped with its id, then rows f6 (without adjust_colors), f8 and f9 on those images.  The
//   definition is DESIGN.md section 4 "Debug model"; the embedding itself is debug_embed.h, shared with the host.
//   debug_views_kernel materialises n images packed back to back (a pure store stream: 16 bytes per thread, one 16-byte store);
//   debug_patch_kernel writes the patch pixels of the debug path straight from the rule -- the debug images never exist -- on the
//   patch geometry and chunk tables of row f6 (texpatch_geometry, the same device functions): four pixels per thread, 48 bytes of
//   image as three 16-byte stores, validity 255 and blending 0 as TexturePatch's constructor leaves them.  Instantiated on the tone
//   mapping: under `gamma` the bytes of the rule (and the crop's fill) go through the context's texel table (tone.h), and row f8's
//   correction brings every one of them back to its byte -- the files do not depend on the mode.
#include "rows.h"
#include "debug_embed.h"
#include "tone.h"

namespace mvs {

// per-context buffers of row f10, allocated on first use, freed with the context (debug_release)
struct DebugDev {
    DBuf<uint32_t> style; bool style_set = false;
    DBuf<DebugView> views; DBuf<unsigned long long> pix_off; DBuf<uint8_t> rgb;
};
void debug_release(mvs_ctx* ctx) { delete ctx->debug; ctx->debug = nullptr; }

namespace {
constexpr uint32_t VEC = 16;   // bytes per thread of debug_views_kernel

// where byte `b` of the packed images lies: the last image that starts at or before it (images without pixels are stepped over: of
// equal starts the last one wins) among [lo, hi], and its pixel and channel there -- the one division by the width
struct Cursor { uint32_t i; int x, y, c, w, h; uint32_t style; uint64_t glyphs; bool on; };
__device__ inline void cursor_load(Cursor& k, const DebugView* __restrict__ views, const uint32_t* __restrict__ style) {
    const DebugView v = views[k.i];
    k.w = v.width; k.h = v.height; k.style = style[v.colour]; k.glyphs = debug_id_glyphs(v.id);
}
__device__ inline Cursor cursor_at(unsigned long long b, uint32_t lo, uint32_t hi, const unsigned long long* __restrict__ pix_off,
                                   const DebugView* __restrict__ views, const uint32_t* __restrict__ style) {
    while (lo < hi) { const uint32_t mid = (lo + hi + 1) >> 1; if (3ull * pix_off[mid] <= b) lo = mid; else hi = mid - 1; }
    Cursor k;
    k.i = lo;
    cursor_load(k, views, style);
    const unsigned long long rel = b - 3ull * pix_off[lo];
    const uint32_t p = (uint32_t)(rel / 3ull);   // < width * height < 2^32
    k.c = (int)(rel - 3ull * p);
    k.y = (int)(p / (uint32_t)k.w); k.x = (int)(p - (uint32_t)k.y * (uint32_t)k.w);
    k.on = debug_pixel_glyphs(k.x, k.y, k.w, k.h, k.glyphs);
    return k;
}
__device__ inline uint32_t cursor_byte(const Cursor& k) { return k.on ? k.style >> 24 : (k.style >> (8 * k.c)) & 255u; }
// one byte on; b_next = the index of the byte stepped to (only read when an image ends)
__device__ inline void cursor_step(Cursor& k, unsigned long long b_next, unsigned long long total, const unsigned long long* __restrict__ pix_off,
                                   const DebugView* __restrict__ views, const uint32_t* __restrict__ style) {
    if (++k.c < 3) return;
    k.c = 0;
    if (++k.x == k.w) {
        k.x = 0;
        if (++k.y == k.h) {
            if (b_next >= total) return;
            k.y = 0;
            do ++k.i; while (3ull * pix_off[k.i + 1] <= b_next);   // ends: b_next < total = 3 pix_off[n]
            cursor_load(k, views, style);
        }
    }
    k.on = debug_pixel_glyphs(k.x, k.y, k.w, k.h, k.glyphs);
}

// out[0, total): the images back to back.  Threads [0, nvec) write bytes [head + 16 t, head + 16 t + 16) with one aligned 16-byte store
// (head = the bytes in front of the first 16-byte boundary of `out`); the threads after them write one byte each of the head and of
// the tail behind the last full vector.  The block looks its first and last image up once, its threads search between the two.
__global__ void __launch_bounds__(256) debug_views_kernel(uint8_t* __restrict__ out, unsigned long long total, uint32_t head, unsigned long long nvec,
                                                          const DebugView* __restrict__ views, const unsigned long long* __restrict__ pix_off, uint32_t n,
                                                          const uint32_t* __restrict__ style) {
    __shared__ uint32_t s_img[2];
    const unsigned long long t0 = (unsigned long long)blockIdx.x * 256ull, t = t0 + threadIdx.x;
    if (threadIdx.x < 2 && t0 < nvec) {
        const unsigned long long t1 = t0 + 255ull < nvec ? t0 + 255ull : nvec - 1ull;
        const unsigned long long b = threadIdx.x == 0 ? head + VEC * t0 : head + VEC * t1 + (VEC - 1);
        uint32_t lo = 0, hi = n - 1;
        while (lo < hi) { const uint32_t mid = (lo + hi + 1) >> 1; if (3ull * pix_off[mid] <= b) lo = mid; else hi = mid - 1; }
        s_img[threadIdx.x] = lo;
    }
    __syncthreads();
    if (t < nvec) {
        const unsigned long long b0 = head + VEC * t;
        Cursor k = cursor_at(b0, s_img[0], s_img[1], pix_off, views, style);
        uint32_t word[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (uint32_t j = 0; j < VEC; ++j) {
            word[j >> 2] |= cursor_byte(k) << (8 * (j & 3));
            cursor_step(k, b0 + j + 1, total, pix_off, views, style);
        }
        *reinterpret_cast<uint4*>(out + b0) = make_uint4(word[0], word[1], word[2], word[3]);
        return;
    }
    unsigned long long e = t - nvec;                    // the byte stores: head first, then the tail
    const unsigned long long b = e < head ? e : head + VEC * nvec + (e - head);
    if (b >= total) return;
    const Cursor k = cursor_at(b, 0, n - 1, pix_off, views, style);
    out[b] = (uint8_t)cursor_byte(k);
}

// one block per chunk of TEXPATCH_CHUNK pixels of one patch (row f6's chunk_ptr).  The pixel arrays are cut into groups of four pixels
// by their GLOBAL index, so that a group's 48 bytes of image and 4 + 4 mask bytes are aligned; thread g of the block owns the g-th
// group that overlaps the chunk (a chunk that does not start on a group boundary has a 257th, thread 0's), clipped to the chunk.  A
// whole group is three 16-byte stores and two 4-byte ones, a clipped one goes element by element.
template <int TONE>
__global__ void __launch_bounds__(256) debug_patch_kernel(const float* __restrict__ tone, uint32_t P, const uint32_t* __restrict__ chunk_ptr, const uint32_t* __restrict__ label,
                                                          const int4* __restrict__ box, const unsigned long long* __restrict__ pix_ptr,
                                                          const DebugView* __restrict__ views, const uint32_t* __restrict__ style,
                                                          float* __restrict__ image, uint8_t* __restrict__ validity, uint8_t* __restrict__ blending) {
    uint32_t lo = 0, hi = P;   // the last patch whose chunks start at or before this one
    while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (chunk_ptr[mid] <= blockIdx.x) lo = mid; else hi = mid; }
    const uint32_t p = lo;
    const int4 b = box[p];
    const unsigned long long base = pix_ptr[p], n = (unsigned long long)b.z * (unsigned long long)b.w;
    const unsigned long long j0 = (unsigned long long)(blockIdx.x - chunk_ptr[p]) * TEXPATCH_CHUNK;
    const unsigned long long i_begin = base + j0, i_end = base + (j0 + TEXPATCH_CHUNK < n ? j0 + TEXPATCH_CHUNK : n);
    const unsigned long long g_base = i_begin & ~3ull;
    const DebugView vw = views[label[p] - 1];
    const uint32_t st = style[vw.colour];
    const uint64_t glyphs = debug_id_glyphs(vw.id);
    float bg[3], font, fill1, fill0;   // the four values of the view, and the crop's fill (255, 0, 255)
    if (TONE == TONE_GAMMA) {
        bg[0] = tone[st & 255u]; bg[1] = tone[(st >> 8) & 255u]; bg[2] = tone[(st >> 16) & 255u]; font = tone[st >> 24];
        fill1 = tone[255]; fill0 = tone[0];
    } else {
        bg[0] = (float)(st & 255u) / 255.0f; bg[1] = (float)((st >> 8) & 255u) / 255.0f; bg[2] = (float)((st >> 16) & 255u) / 255.0f;
        font = (float)(st >> 24) / 255.0f;
        fill1 = 1.0f; fill0 = 0.0f;
    }
    for (unsigned long long i0 = g_base + 4ull * threadIdx.x; i0 < i_end; i0 += 1024ull) {
        const unsigned long long a = i0 > i_begin ? i0 : i_begin, e = i0 + 4ull < i_end ? i0 + 4ull : i_end;
        const unsigned long long j = a - base;
        int y = (j >> 32) ? (int)(j / (unsigned long long)b.z) : (int)((uint32_t)j / (uint32_t)b.z);   // the thread's one division
        int x = (int)(j - (unsigned long long)y * (unsigned long long)b.z);
        float px[12];
        const uint32_t cnt = (uint32_t)(e - a);
#pragma unroll
        for (uint32_t q = 0; q < 4; ++q) {
            if (q < cnt) {
                const int vx = b.x + x, vy = b.y + y;
                const bool in_view = vx >= 0 && vy >= 0 && vx < vw.width && vy < vw.height;
                const bool on = in_view && debug_pixel_glyphs(vx, vy, vw.width, vw.height, glyphs);
                px[3 * q] = in_view ? (on ? font : bg[0]) : fill1;      // outside: the crop's fill (255, 0, 255)
                px[3 * q + 1] = in_view ? (on ? font : bg[1]) : fill0;
                px[3 * q + 2] = in_view ? (on ? font : bg[2]) : fill1;
                if (++x == b.z) { x = 0; ++y; }
            } else {
                px[3 * q] = 0.0f; px[3 * q + 1] = 0.0f; px[3 * q + 2] = 0.0f;
            }
        }
        if (cnt == 4) {
            float4* im = reinterpret_cast<float4*>(image + 3ull * i0);
            im[0] = make_float4(px[0], px[1], px[2], px[3]); im[1] = make_float4(px[4], px[5], px[6], px[7]); im[2] = make_float4(px[8], px[9], px[10], px[11]);
            *reinterpret_cast<uint32_t*>(validity + i0) = 0xFFFFFFFFu;
            *reinterpret_cast<uint32_t*>(blending + i0) = 0u;
        } else {
#pragma unroll
            for (uint32_t q = 0; q < 3; ++q) {   // a clipped group has at most three pixels
                if (q >= cnt) break;
                const unsigned long long i = a + q;
                image[3 * i] = px[3 * q]; image[3 * i + 1] = px[3 * q + 1]; image[3 * i + 2] = px[3 * q + 2];
                validity[i] = 255; blending[i] = 0;
            }
        }
    }
}

DebugDev& debug_dev(mvs_ctx* ctx) {
    DebugDev& G = row_dev(ctx->debug);
    if (!G.style_set) {   // the table is data: built on the host (debug_embed.h), uploaded once per context
        uint32_t h_style[DEBUG_COLOURS];
        debug_style_table(h_style);
        G.style.ensure(DEBUG_COLOURS);
        MVS_HIP(hipMemcpy(G.style.p, h_style, sizeof(h_style), hipMemcpyHostToDevice));
        G.style_set = true;
    }
    return G;
}
// the headers of n images: sizes, ids (view_ids, or the position), colours
std::vector<DebugView> debug_headers(uint32_t n, const int32_t* width, const int32_t* height, const uint32_t* view_ids, uint32_t first_position, const char* who) {
    std::vector<DebugView> v(n);
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t pos = first_position + i, id = view_ids ? view_ids[i] : pos;
        if (id > DEBUG_MAX_ID) throw StatusError(MVS_ERR_UNSUPPORTED, std::string(who) + ": view id " + std::to_string(id) + " has more than three digits");
        v[i] = DebugView{width[i], height[i], id, pos % (uint32_t)DEBUG_COLOURS};
    }
    return v;
}
}  // namespace
}  // namespace mvs

using namespace mvs;

extern "C" {

mvs_status mvs_debug_view_style(uint32_t position, uint8_t bg[3], uint8_t fg[3]) {
    if (!bg || !fg) return api_fail(MVS_ERR_INVALID, "null argument");
    uint32_t style[DEBUG_COLOURS];
    debug_style_table(style);
    const uint32_t st = style[position % (uint32_t)DEBUG_COLOURS];
    for (int c = 0; c < 3; ++c) { bg[c] = (uint8_t)(st >> (8 * c)); fg[c] = (uint8_t)(st >> 24); }
    return MVS_OK;
}

mvs_status mvs_ctx_debug_embeddings(mvs_ctx* ctx, uint32_t n, const int32_t* width, const int32_t* height, const uint32_t* view_ids, uint32_t first_position,
                                    uint8_t* rgb_out, int out_on_device) {
    if (!ctx || (n && (!width || !height))) return api_fail(MVS_ERR_INVALID, "null argument");
    return api_guard([&] {
        MVS_HIP(hipSetDevice(ctx->device));
        hipStream_t s = ctx->stream;
        std::vector<unsigned long long> off((size_t)n + 1, 0ull);
        for (uint32_t i = 0; i < n; ++i) {
            if (width[i] < 0 || height[i] < 0) throw StatusError(MVS_ERR_INVALID, "debug_embeddings: negative image size");
            if (width[i] > 65535 || height[i] > 65535) throw StatusError(MVS_ERR_UNSUPPORTED, "debug_embeddings: an image side above 65535");
            off[i + 1] = off[i] + (unsigned long long)width[i] * (unsigned long long)height[i];
        }
        const std::vector<DebugView> hv = debug_headers(n, width, height, view_ids, first_position, "debug_embeddings");
        const unsigned long long total = 3ull * off[n];
        if (!total) return;
        if (!rgb_out) throw StatusError(MVS_ERR_INVALID, "debug_embeddings: null output");
        DebugDev& G = debug_dev(ctx);
        upload(G.views, hv, s); upload(G.pix_off, off, s);
        uint8_t* d_out = rgb_out;
        if (!out_on_device) { G.rgb.ensure((size_t)total + VEC); d_out = G.rgb.p; }
        const uint32_t head = (uint32_t)std::min<unsigned long long>((VEC - ((uintptr_t)d_out & (VEC - 1))) & (VEC - 1), total);
        const unsigned long long nvec = (total - head) / VEC, threads = nvec + head + (total - head - VEC * nvec);
        if ((threads + 255) / 256 >= 0x7FFFFFFFull) throw StatusError(MVS_ERR_UNSUPPORTED, "debug_embeddings: too many pixels for one call");
        {
            Prof pr(ctx, "debug_views");   // option "profile": the kernel's device time (mvs_ctx_get_profile)
            hipLaunchKernelGGL(debug_views_kernel, dim3(grid((size_t)threads)), dim3(256), 0, s, d_out, total, head, nvec, (const DebugView*)G.views.p,
                               (const unsigned long long*)G.pix_off.p, n, (const uint32_t*)G.style.p);
            MVS_LAUNCH_CHECK();
        }
        if (!out_on_device) MVS_HIP(hipMemcpyAsync(rgb_out, d_out, (size_t)total, hipMemcpyDeviceToHost, s));
        MVS_HIP(hipStreamSynchronize(s));   // hv and off are borrowed by the uploads
    });
}

mvs_status mvs_ctx_debug_patches(mvs_ctx* ctx, const uint32_t* adj_ptr, const uint32_t* adj, int adj_on_device, const uint32_t* labels,
                                 int labels_on_device, const uint32_t* view_ids, const mvs_patch_params* params, mvs_patch_set* out, int out_on_device,
                                 mvs_patch_stats* stats) {
    if (!ctx || !out) return api_fail(MVS_ERR_INVALID, "null argument");
    if (!ctx->d_verts || !ctx->d_faces || ctx->n_views == 0 || ctx->h_views.size() < ctx->n_views)
        return api_fail(MVS_ERR_STATE, "debug patches need the mesh and the views (mvs_scene_set_mesh, mvs_scene_set_views)");
    const uint32_t F = ctx->n_faces;
    if (F && (!adj_ptr || !adj || !labels)) return api_fail(MVS_ERR_INVALID, "null argument");
    *out = mvs_patch_set{};
    mvs_patch_stats S{};
    return api_guard([&] {
        MVS_HIP(hipSetDevice(ctx->device));
        hipStream_t s = ctx->stream;
        const uint32_t V = ctx->n_views;
        std::vector<int32_t> w(V), h(V);
        for (uint32_t v = 0; v < V; ++v) { w[v] = ctx->h_views[v].width; h[v] = ctx->h_views[v].height; }
        const std::vector<DebugView> hv = debug_headers(V, w.data(), h.data(), view_ids, 0, "debug_patches");
        TexPatchDev& D = row_dev(ctx->texpatch);
        DebugDev& G = debug_dev(ctx);
        mvs_patch_params P;
        if (params) P = *params; else mvs_patch_default_params(&P);
        const uint32_t tone = tone_mode(P.tone_mapping, "debug_patches");
        const float* d_tone = tone == TONE_GAMMA ? tone_table_dev(ctx) : nullptr;
        const RowGraph g = stage_graph(ctx, adj_ptr, adj, adj_on_device, labels, labels_on_device);
        upload(G.views, hv, s);
        MVS_HIP(hipStreamSynchronize(s));   // host buffers are borrowed for the call only
        uint32_t n_listed = 0; uint64_t n_pixels = 0;
        run_with_stats(s, stats, S, [&] {
            StageTimer<5> tm(s);   // marks: begin, tables, lists, pixels
            uint32_t n_chunks = 0;
            texpatch_geometry(ctx, D, g.adj_ptr, g.adj, g.labels, P, S, n_listed, n_pixels, &n_chunks, tm, "debug_patches");
            MVS_HIP(hipStreamSynchronize(s));   // n_chunks
            if (n_chunks) {
                auto* pixels = tone == TONE_GAMMA ? debug_patch_kernel<TONE_GAMMA> : debug_patch_kernel<TONE_NONE>;
                hipLaunchKernelGGL(pixels, dim3(n_chunks), dim3(256), 0, s, d_tone, D.pt.n_patches, (const uint32_t*)D.chunk_ptr.p, (const uint32_t*)D.label.p,
                                   (const int4*)D.box.p, (const unsigned long long*)D.pix_ptr.p, (const DebugView*)G.views.p, (const uint32_t*)G.style.p,
                                   D.image.p, D.validity.p, D.blending.p);
                MVS_LAUNCH_CHECK();
            }
            tm.mark();
            MVS_HIP(hipStreamSynchronize(s));
            S.valid_pixels = n_pixels; S.near_pixels = 0; S.degenerate_faces = 0;
            S.ms_tables = tm.ms(0, 1); S.ms_lists = tm.ms(1, 2); S.ms_mark = 0.0f; S.ms_resolve = tm.ms(2, 3); S.ms_total = tm.ms(0, 3);
        });
        texpatch_output(ctx, D, n_listed, n_pixels, out, out_on_device);
    });
}

mvs_status mvs_ctx_view_selection_model(mvs_ctx* ctx, const uint32_t* adj_ptr, const uint32_t* adj, int adj_on_device, const uint32_t* labels,
                                        int labels_on_device, const uint32_t* view_ids, const float* vertex_normals, int normals_on_device, const char* prefix,
                                        const mvs_patch_params* patch_params, const mvs_atlas_params* atlas_params, const mvs_model_params* model_params,
                                        mvs_patch_stats* patch_stats, mvs_atlas_stats* atlas_stats, mvs_model_stats* model_stats) {
    if (!ctx || !prefix) return api_fail(MVS_ERR_INVALID, "null argument");
    mvs_patch_set patches{}; mvs_atlas_set atlases{};
    mvs_status rc = mvs_ctx_debug_patches(ctx, adj_ptr, adj, adj_on_device, labels, labels_on_device, view_ids, patch_params, &patches, 1, patch_stats);
    if (rc != MVS_OK) return rc;
    rc = mvs_ctx_texture_atlases(ctx, &patches, 1, atlas_params, &atlases, 1, atlas_stats);
    if (rc != MVS_OK) return rc;
    const std::string pre = std::string(prefix) + "_view_selection";
    return mvs_ctx_save_model(ctx, &atlases, 1, vertex_normals, normals_on_device, pre.c_str(), model_params, model_stats);
}

}  // extern "C"
