// ctx.h -- context object, device buffers and launch helpers (internal).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <functional>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/mvs_viewsel.h"
#include "dmath.h"
#include "view_batches.h"

namespace mvs {

struct HipError : std::runtime_error {
    explicit HipError(const std::string& m) : std::runtime_error(m) {}
};
struct StatusError : std::runtime_error {
    mvs_status st;
    StatusError(mvs_status s, const std::string& m) : std::runtime_error(m), st(s) {}
};

#define MVS_HIP(expr)                                                                          \
    do {                                                                                       \
        hipError_t _e = (expr);                                                                \
        if (_e != hipSuccess)                                                                  \
            throw mvs::HipError(std::string(#expr) + ": " + hipGetErrorString(_e) + " (" +     \
                                __FILE__ + ":" + std::to_string(__LINE__) + ")");              \
    } while (0)

#define MVS_LAUNCH_CHECK() MVS_HIP(hipGetLastError())

// Growable device buffer; capacity persists across calls so that a steady-state
// step performs no hipMalloc.
template <class T>
struct DBuf {
    T* p = nullptr;
    size_t cap = 0;
    void ensure(size_t n) {
        if (n <= cap) return;
        if (p) MVS_HIP(hipFree(p));
        p = nullptr; cap = 0;
        size_t want = n + n / 8 + 64;
        MVS_HIP(hipMalloc((void**)&p, want * sizeof(T)));
        cap = want;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
    ~DBuf() { release(); }
    DBuf() = default;
    DBuf(const DBuf&) = delete;
    DBuf& operator=(const DBuf&) = delete;
};

// Growable PINNED host buffer (device-to-host staging of the streamed table download, oneshot.hip)
template <class T>
struct HBuf {
    T* p = nullptr;
    size_t cap = 0;
    void ensure(size_t n) {
        if (n <= cap) return;
        if (p) MVS_HIP(hipHostFree(p));
        p = nullptr; cap = 0;
        size_t want = n + n / 8 + 64;
        MVS_HIP(hipHostMalloc((void**)&p, want * sizeof(T), hipHostMallocDefault));
        cap = want;
    }
    ~HBuf() { if (p) (void)hipHostFree(p); }
    HBuf() = default;
    HBuf(const HBuf&) = delete;
    HBuf& operator=(const HBuf&) = delete;
};

// ---- implicit 4-ary BVH over Hilbert-sorted triangles (k_bvh.hip) ----
struct alignas(128) Node4 {
    float b[4][6];            // child c: lo.x lo.y lo.z hi.x hi.y hi.z -- child-major, so that (lo.x, lo.y) (lo.z, hi.x) (hi.y, hi.z) are
                              // the aligned SGPR pairs of three v_pk_fma_f32 per child; absent children are far-away points
    uint32_t nchild;
    uint32_t pad_[7];
    __host__ __device__ float lo(int a, int c) const { return b[c][a]; }
    __host__ __device__ float hi(int a, int c) const { return b[c][3 + a]; }
};
static_assert(sizeof(Node4) == 128, "Node4 must be one 128-byte line");

struct BvhDev {
    const Node4* nodes;       // all levels, level L at nodes + level_off[L]
    const float4* tris;       // 4 float4 per triangle: {a, lo.x} {e1 = b - a, lo.y} {e2 = c - a, lo.z} {hi, 0}  (curve order, zero padded)
    uint32_t level_off[16];
    uint32_t level_cnt[16];
    int32_t top;              // index of the root level (level_cnt[top] == 1)
    uint32_t n_leaves;
};

// Stage profiler: hipEvent pairs recorded on the context's stream (enabled by
// mvs_set_option("profile", 1)); read back with mvs_ctx_get_profile.
struct ProfSpan { std::string name; hipEvent_t a, b; bool owns_a; };   // owns_a = false: `a` is the previous span's `b` (ProfChain)

struct MrfEdge {      // per directed edge e = (i <- j) in adjacency-CSR order
    uint32_t in_off;  // offset of the message INTO i over e (K_i floats, aligned with i's labels)
    uint32_t out_off; // offset of the message i sends over e, i.e. in_off of the reverse edge (K_j floats)
    uint32_t kj;      // K_j if the edge is valid (both columns non-empty), else 0
};

// Fast-path (degree <= 3, every column <= 255 labels) per-node descriptor: 48 bytes = 3 x 16-byte loads, stored in
// (colour, id) order.  Offsets of message runs are multiples of 4 elements, which frees their low bits for flags.
struct alignas(16) NodeDesc {
    uint32_t rec;         // first 32-bit word of the node's RECORD in m_rec: ceil4(k) label words {cost code << 16 | view id},
                          // then, for every out-edge whose two label lists differ, ceil4(kj) one-byte re-alignment map entries
    uint32_t id;          // the node (face) this descriptor belongs to
    uint32_t in_off[3];   // incoming message offsets; bit 0: that neighbour has a LOWER colour (its label of this sweep is final when this node is swept)
    uint32_t out_off[3];  // outgoing message offsets (= in_off of the reverse edges); bit 0: identical label lists (map = identity, not stored)
    uint32_t kk;          // k | kj[0] << 8 | kj[1] << 16 | kj[2] << 24   (kj = 0: edge not in the model)
    uint32_t nbr[3];      // neighbour node ids (0xFFFFFFFF = none)
};
static_assert(sizeof(NodeDesc) == 48, "NodeDesc must be 48 bytes");

// The single words the solver's stages (and the rows that borrow a context) count in and read back: one named field per purpose, in one
// device allocation made with the context and never re-allocated.  A stage clears its own fields before it counts in them and touches
// nobody else's.  Fields on one line travel together (a kernel indexes them from the first, or one copy / read_words fetches them).
struct SolverWords {
    uint32_t icm_n_moved, icm_cursor;                                // mrf_icm_apply: nodes moved, length of the active list (the kernels' moved[0], moved[1])
    uint32_t labels_bad, labels_unseen;                            // mrf_labels: labels above the number of views (+ foreign ones), faces left with label 0
    uint32_t colour_pending, colour_full;                          // mrf_setup's colouring: a node is still waiting, a node saw all 64 colours around it
    uint32_t setup_kmax, setup_degmax, setup_total, setup_unsorted;   // mrf_setup: largest column, largest degree, message elements, "a column is not strictly ascending"
    uint32_t exact_foreign;                                        // mrf_exact_costs: labels that are no entry of their node's column (mrf_labels adds them to "bad")
    uint32_t adj_overflow, adj_self;                               // k_mesh.hip build_adjacency: a neighbour list overflowed, faces with a repeated vertex
    uint32_t patch_bad;                                            // k_patch.hip get_subgraphs: a label >= n_labels
    uint32_t region_moved;                                         // k_region.hip mrf_region_round: regions that moved
};
static_assert(sizeof(SolverWords) <= 64 * sizeof(uint32_t), "SolverWords must fit one read_words");
static_assert(offsetof(SolverWords, setup_unsorted) - offsetof(SolverWords, colour_pending) == 5 * sizeof(uint32_t), "mrf_setup clears colour_pending .. setup_unsorted with one memset");

struct GslDev;   // row f5 (k_seam.hip)
struct TexPatchDev;   // row f6 (k_texpatch.hip)
struct LslDev;   // row f7 (k_localseam.hip)
struct AtlasDev; // row f8 (k_atlas.hip)
struct ModelDev; // row f9 (k_model.hip)
struct DebugDev; // row f10 (k_debug.hip)
struct GlbDev;   // row f11 (k_glb.hip)
struct PngDev;   // row f9's compressed PNGs (k_png.hip)
struct JpegDev;  // rows f9 / f11: JPEG images (k_jpeg.hip)
struct JpegDecDev;   // view input: JPEG files decoded on the device (k_jpegdec.hip)
struct LensDev;      // view input: lens undistortion on the device (k_lens.hip)
struct PngDecDev;    // view input: PNG files inflated and unfiltered on the device (k_pngdec.hip)
struct LevelDev;     // view input: the tables and the output of the level route (k_level.hip)
struct ViewMaskDev;  // view input: the keep words of the views that carry a mask (k_viewmask.hip)

// The tables of generate_texture_patches both rows build (DESIGN.md section 4 "Global seam leveling" items 3-4; k_texpatch.hip
// build_patch_tables): per candidate (component of a label, label-major) its frame box = (min_x - 1, min_y - 1, max_x, max_y), the
// candidate that absorbed it (parent, NONE for a survivor), where its list starts in that one's list (off), the list length after the
// merges (len), alive, the patch id of a survivor (pscan) and of the chain's root (cand_pid) with the list position of the
// candidate's first face there (cand_pos); per face its candidate and place in it (fcand, fidx), its patch and list position (fpid,
// fpos) and its corners' pixel coordinates in its view (pc).
struct PatchTables {
    DBuf<int4> box; DBuf<float2> pc;
    DBuf<uint32_t> fcand, fidx, parent, off, len, alive, pscan, cand_pid, cand_pos, fpid, fpos, flags;
    DBuf<unsigned long long> merged; DBuf<ViewParams> views;
    uint32_t C = 0, n_patches = 0; uint64_t n_merged = 0;   // of the last build_patch_tables
};

}  // namespace mvs

struct mvs_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    bool verbose = false;
    bool profile = false;
    std::vector<mvs::ProfSpan> prof_spans; std::vector<hipEvent_t> prof_pool;
    bool prep_fused = true;  // image prep: luminance + Sobel in one pass through LDS (false: the two-pass kernels; identical output)
    bool stats = false;      // fill the cull-reason counters of mvs_dc_stats (diagnostics; costs atomics)
    bool count_rays = false;
    uint32_t* h_kd_flags = nullptr; int kd_pending = 0; bool kd_disabled = false;   // k_kdorder.hip: per-level overflow words (pinned), levels awaiting scene_order_commit, "this mesh keeps the curve order"
    uint32_t* h_rb = nullptr; uint32_t* d_rb = nullptr; uint32_t rb_seq = 0;   // read_words() / read_block(): 64 data words, the sequence number, 4 KB of staging -- pinned
    hipStream_t aux_stream = nullptr; hipEvent_t ev_fork = nullptr, ev_join = nullptr;   // the image preparation runs beside the face order + BVH build (k_dc.hip dc_phase1)
    uint32_t bvh_upper_min_faces = 1000000;   // meshes below this many faces keep the Hilbert order above the LDS window (k_bvh.hip build_scene_order)
    uint32_t bvh_window = 262144;    // upper levels of the face order: exact top-down median cuts inside aligned windows of this many positions of the Hilbert order (k_kdorder.hip); 0 = the whole mesh, 1 = none
    mvs::DBuf<float> kd_c[2][3]; mvs::DBuf<uint32_t> kd_id[2], kd_hist, kd_cursor, kd_tie, kd_pivot, kd_box;   // k_kdorder.hip work buffers
    int ray_xcd = 1;         // XCD-aware block order in the packet ray kernel
    int info_wave_area = 32;   // footprints (sampled ones) above this many pixels go to the wave-per-footprint kernel (k_dc.hip wave_info_kernel); 0 = every footprint serial = bit-exact with the reference's fp64 scan order
    int info_wave_area_words = 384;   // the same threshold where info_kernel walks a footprint four pixels per load as integers ("info_words": gradient term, no outlier removal): one lane
                                      // keeps up with the lane group up to a few hundred pixels (real-like scene, threshold 32 / 128 / 256 / 512 / 1024 / 2048: dc_face_info 1.38 / 1.13 / 1.04 / 1.04 / 1.17 / 1.39 ms)
    bool info_words = true;    // small footprints of the gradient term: integer word walk + certificate in info_kernel (option "info_words"; 0: serial fp64 walk)
    int info_cert_shift = 0;   // test hook: widens the exactness certificate of wave_info_kernel by this many bits (forces its serial fallback)
    uint32_t dc_stats_deferred = 0;
    int max_labels = 0;      // > 0: label-space compression after the data costs (k_dc.hip prune_write_kernel); 0 = the reference's model
    float cos_limit = 0.0f;  // see dmath.h cull_pair

    // ---- scene ----
    uint32_t n_verts = 0, n_faces = 0, n_views = 0;
    uint32_t face_begin = 0, face_end = 0;
    const float* d_verts = nullptr; const uint32_t* d_faces = nullptr; const float* d_normals = nullptr;
    mvs::DBuf<float> own_verts, own_normals; mvs::DBuf<uint32_t> own_faces;
    std::vector<mvs::ViewParams> h_views;
    mvs::DBuf<mvs::ViewParams> d_views;
    std::vector<mvs::DBuf<uint8_t>*> own_rgb;
    mvs::DBuf<uint8_t> gmi_all;      // all views' gradient-magnitude planes
    mvs::DBuf<uint8_t> lum_all;      // luminance planes (vectorised prep path)
    mvs::DBuf<uint32_t> mask_all;    // all views' bit-packed validity masks
    mvs::DBuf<uint32_t> mask_zero, mask_tmp;
    mvs::DBuf<uint32_t> msum_all;    // all views' mask tile summaries (dmath.h ViewParams::msum)
    std::vector<size_t> gmi_off, mask_off, msum_off;
    mvs::DBuf<size_t> view_off;
    bool mesh_dirty = true, views_dirty = true;
    bool views_refused = false;      // the last view input was refused (view_input.h view_input_begin): a data-cost pass is MVS_ERR_STATE

    // ---- the library's own mesh layout (k_bvh.hip build_scene_order; DESIGN.md "Face order") ----
    // The caller's mesh arrives in file order (calculate_data_costs.cpp:136-138); nothing about it is assumed.  Every data-cost pass
    // first lays the mesh out along a Hilbert curve: vertices by their position, faces by their centroid (refined by median splits
    // inside 512-face windows: the BVH's leaf order).  i_verts / i_faces / i_normals are that copy -- vertex s of the copy is the
    // s-th vertex of the curve, face p the p-th face -- and everything downstream (culls, rays, footprints, the cost table, the
    // solver's nodes, the parts of the sharded path) is indexed by those positions.  f_perm[p] = the caller's id of face p, f_pos its
    // inverse; results cross the ABI in the caller's numbering.  Option "face_order" = 0 keeps the caller's face numbering (a caller
    // that laid the faces out itself; the building-block API of mgpu.hip); vertices are renumbered either way (invisible outside).
    int face_order = 1;
    mvs::DBuf<float> i_verts, i_normals; mvs::DBuf<uint32_t> i_faces, f_perm, f_pos, f_tmp;
    const float* iv = nullptr; const uint32_t* ifc = nullptr; const float* inr = nullptr;   // the arrays the kernels read (i_* or the caller's)
    bool mesh_ordered = false;        // f_perm / f_pos describe the resident mesh (set by build_scene_order when face_order != 0)
    bool order_pinned = false;        // a shard was made of this mesh (mvs_shard_create): its parts, its renumbered adjacency and its halo plan ARE this
                                      // layout, so the data-cost passes of the sharded path keep it instead of deriving it again (mvs_scene_set_mesh un-pins)
    // order of the ACTIVE cost table (r_ptr ...): t_perm[p] = caller's id of column p (null: the table is in the caller's order)
    const uint32_t* t_perm = nullptr; const uint32_t* t_pos = nullptr;
    mvs::DBuf<uint32_t> u_ptr, u_cnt; mvs::DBuf<uint16_t> u_view; mvs::DBuf<float> u_cost, u_q;   // the table in the caller's order (built on demand)
    bool u_valid = false, u_q_valid = false;
    mvs::DBuf<unsigned long long> fp_acc;   // device-side fingerprint of the table handed out (oneshot.hip mvs_data_costs_stream)
    mvs::HBuf<uint32_t> stage_ptr; mvs::HBuf<uint16_t> stage_view[2]; mvs::HBuf<float> stage_cost[2];   // pinned staging of the chunked download

    // ---- BVH + incidence ----
    mvs::DBuf<mvs::Node4> bvh_nodes; mvs::DBuf<float4> bvh_tris;
    mvs::DBuf<uint32_t> sort_k, sort_k2, sort_v, sort_v2; mvs::DBuf<char> sort_tmp;
    mvs::DBuf<float> lvl_box_a, lvl_box_b; mvs::DBuf<float> scene_box;
    mvs::BvhDev bvh{};
    mvs::DBuf<uint32_t> vf_ptr, vf_cursor, vf;
    mvs::DBuf<uint32_t> vperm, vpos;   // vertices in Hilbert order and the inverse map (caller's vertex ids; used to build i_verts / i_faces only)
    const uint32_t* tri_order = nullptr;   // BVH triangle slot -> face position (null: identity, the faces ARE in curve order)

    // ---- data costs work buffers ----
    mvs::DBuf<unsigned long long> pass_bits, need_bits, occl_bits, surv_bits;
    mvs::DBuf<uint32_t> pass_base;      // exclusive scan of popc(pass words)
    mvs::DBuf<uint32_t> pass_face;      // [view chunk][face] the chunk's pass bits of a face (face-major copy read by need_kernel)
    mvs::DBuf<unsigned long long> defer_bits; mvs::DBuf<uint32_t> defer_base; mvs::DBuf<uint2> defer_list; mvs::DBuf<uint32_t> rewalk_list;   // large footprints left to the wave-per-footprint kernel
    mvs::DBuf<float> pq;                // quality per passing pair
    mvs::DBuf<float> pcol;              // 3 floats per passing pair (outlier removal only)
    mvs::DBuf<uint32_t> face_cnt, scan_tmp;
    mvs::DBuf<unsigned long long> counters;  // 64 slots, named in dc_counters.h
    mvs::DBuf<float> max_q; mvs::DBuf<uint32_t> hist; mvs::DBuf<float> pctl;
    // pre-outlier CSR (only when outlier removal is on)
    mvs::DBuf<uint32_t> pre_ptr; mvs::DBuf<uint16_t> pre_view; mvs::DBuf<float> pre_q; mvs::DBuf<float> pre_col;
    mvs::DBuf<uint8_t> pre_inl;
    // result CSR
    mvs::DBuf<uint32_t> csr_ptr; mvs::DBuf<uint16_t> csr_view; mvs::DBuf<float> csr_cost; mvs::DBuf<float> csr_q;
    uint32_t csr_faces = 0, csr_views = 0; uint64_t csr_nnz = 0;
    const uint32_t* r_ptr = nullptr; const uint16_t* r_view = nullptr; const float* r_cost = nullptr;  // active CSR
    bool csr_q_valid = false;   // csr_q holds the qualities of the active CSR (set by the data-cost stage)
    bool have_costs = false;
    mvs_settings dc_settings{}; mvs_dc_stats dc_stats{}; int dc_phase = 0;
    // ranged data-cost pass (k_dc.hip dc_ranged; planner and accounting in dc_ranges.h): option "dc_range_pairs", what the last pass did
    // (mvs_ctx_dc_ranges), "the order, the BVH and the prepared views of this call are resident" for the ranges after the first, and the
    // (col_ptr, view_id, quality) every range leaves behind until the percentile is known -- back to back, 64-bit bases on the host
    uint64_t dc_range_pairs = 0; uint32_t dc_n_ranges = 1, dc_range_faces = 0; bool dc_walk_resident = false;
    mvs::DBuf<uint32_t> k_ptr, k_max; mvs::DBuf<uint16_t> k_view; mvs::DBuf<float> k_q;

    // ---- row f1: mesh preparation + adjacency graph (k_mesh.hip) ----
    mvs::DBuf<unsigned long long> g_keys, g_keys2; mvs::DBuf<uint32_t> g_vals, g_vals2, g_pos, g_cnt, g_adj_ptr, g_adj, g_faces; mvs::DBuf<float> g_normals;
    uint64_t g_adj_entries = 0; bool have_adj = false;

    // ---- row f3: patch components (k_patch.hip) ----
    mvs::DBuf<uint32_t> p_label_ptr, p_comp_ptr, p_comp_faces, p_parent, p_root, p_state, p_flag, p_pos, p_roots, p_roots2, p_rlab, p_rlab2, p_adj_ptr, p_adj, p_labels;

    // ---- rows f5 - f11 and the image routes: per-row buffers allocated on first use (rows.h row_dev); the caller's adjacency and labels where they
    // arrive as host arrays and the pinned read-back of a patch set's frames and of an image route's bytes are shared (rows.h stage_graph,
    // read_patch_set; image_routes.h pack_slots) ----
    mvs::DBuf<uint32_t> row_adj_ptr, row_adj, row_labels; mvs::HBuf<char> row_pin;
    mvs::GslDev* gsl = nullptr; mvs::TexPatchDev* texpatch = nullptr; mvs::LslDev* lsl = nullptr; mvs::AtlasDev* atlas = nullptr;
    mvs::ModelDev* model = nullptr;   // row f9 (k_model.hip)
    mvs::DebugDev* debug = nullptr;   // row f10 (k_debug.hip)
    mvs::GlbDev* glb = nullptr;       // row f11 (k_glb.hip)
    mvs::PngDev* png = nullptr;       // row f9's compressed PNGs (k_png.hip)
    mvs::JpegDev* jpeg = nullptr;     // rows f9 / f11: JPEG images (k_jpeg.hip)
    mvs::JpegDecDev* jpegdec = nullptr; uint32_t jpegdec_subseq = 128;   // view input (k_jpegdec.hip); option "jpegdec_subseq_bytes": bytes of entropy data one lane owns
    mvs::PngDecDev* pngdec = nullptr; // view input: the PNG route's buffers (k_pngdec.hip)
    mvs::LensDev* lens = nullptr;     // view input: the per-view tables and the output of the lens route (k_lens.hip)
    mvs::ViewMaskDev* viewmask = nullptr; uint64_t view_scratch_cap = mvs::VIEW_SCRATCH_DEFAULT;   // view masks (k_viewmask.hip): the keep words; max_scratch_bytes of the last view input (mask staging is cut by it)
    mvs::DBuf<uint8_t> view_staging;  // view input: the staging buffer of all routes (view_input.h view_staging)
    mvs::LevelDev* level = nullptr; std::vector<mvs_view_level> view_levels;   // view input: pyramid levels (k_level.hip); every view's level and source size as the last view input left them (empty: all at level 0)
    mvs::DBuf<float> tone_table; bool tone_table_valid = false;   // the 256 texel values tone mapping `gamma` reads (k_tone.hip tone_table_dev), uploaded on first use

    // ---- region moves (k_region.hip) ----
    mvs::DBuf<uint32_t> rg_parent, rg_root, rg_size, rg_bestl, rg_lose, rg_flag, rg_pos, rg_cstart, rg_have, rg_cfirst, rg_name;
    mvs::DBuf<unsigned long long> rg_gain, rg_cur, rg_key, rg_key2, rg_ck, rg_sum; mvs::DBuf<long long> rg_cgain; mvs::DBuf<uint2> rg_cut;

    // ---- MRF ----
    mvs::DBuf<uint32_t> m_adj_ptr, m_adj, a_stage_ptr, a_stage; const uint32_t* r_adj_ptr = nullptr; const uint32_t* r_adj = nullptr;   // a_stage*: host lists on their way into the table's order
    uint32_t r_adj_edges = 0; bool r_adj_edges_known = false;   // length of r_adj where set_adjacency learned it (host lists, renumbered lists)
    mvs::DBuf<mvs::NodeDesc> m_desc; mvs::DBuf<uint8_t> m_ident; mvs::DBuf<uint32_t> m_rec; uint64_t m_rec_words = 0; int mrf_blocks_per_cu = 0 /* 0 = resident count from the occupancy API */, mrf_xcd = 1;
    mvs::DBuf<mvs::MrfEdge> m_edge; mvs::DBuf<uint32_t> m_size, m_rev /* reverse directed edge of every in-edge */; mvs::DBuf<uint16_t> m_map;
    mvs::DBuf<uint8_t> m_msg_a;    // messages as 8-bit fixed point over [0, 1/rho], updated in place (one colour class at a time)
    // decode of a sweep = position in the column (sel), label (view + 1) and the unary of that label as the sweeps see it.
    // TWO buffers of F + 1 entries each: the sweeps write buffer m_state->w, the best labeling so far is buffer
    // m_state->best_w; "keep the best" is a flip of those two indices by the step kernel, never a copy.
    mvs::DBuf<uint32_t> m_sel, m_sel2, m_cand; mvs::DBuf<float> m_gain;
    mvs::DBuf<uint32_t> m_lab; mvs::DBuf<float> m_cost;
    uint32_t m_stride = 0;      // F + 1: offset of the second buffer
    bool exact_valid = false; uint32_t exact_nb = 0, exact_ne = 0;   // b_sel / b_cost of nodes [exact_nb, exact_ne) are derived from b_lab (k_mrf_polish.hip mrf_exact_costs)
    uint32_t* b_sel = nullptr; uint32_t* b_lab = nullptr; float* b_cost = nullptr; bool best_resolved = false;   // the best buffer, once the host knows which one it is (resolve_best)
    mvs::DBuf<unsigned long long> m_energy; mvs::SolverWords* words = nullptr /* allocated by mvs_ctx_create */; mvs::DBuf<uint32_t> m_alist; bool icm_dirty_valid = false;   // ICM active set: nodes whose gain the next pass re-evaluates
    uint32_t m_n_adj = 0;      // directed edges of the adjacency given to mrf_setup
    uint32_t m_energy_blocks = 0;   // per-block partial pairs the last mrf_energy left behind m_energy.p + 4
    bool m_energy_from_sweep = false;   // ... or the last sweep's own kernels did (fast path: the energy is accumulated while sweeping)
    uint64_t m_total = 0; uint32_t m_kmax = 0, m_degmax = 0;
    // colour-phased schedule: colours of the adjacency graph and per-node classes (k_mrf_setup.hip mrf_node_class); nodes in SCHEDULE order =
    // sorted by sub-class key (fast nodes by (colour, class, id), then generic nodes by (colour, id)); m_sub_begin[key] = first position
    // of a key >= `key` (host copy of m_sub); positions [0, m_n_fast) are the fast nodes
    mvs::DBuf<uint32_t> m_colour, m_perm, m_tmp_a, m_tmp_b, m_tmp_c, m_sub; mvs::DBuf<uint8_t> m_cls; uint32_t m_colours = 0, m_n_fast = 0; std::vector<uint32_t> m_sub_begin;
    const uint32_t* m_colour_in = nullptr;   // colours of all nodes kept by a sharded caller (null: mrf_setup colours the graph)
    const uint8_t* m_bnd = nullptr;   // per node: 1 = boundary node of a sharded caller (own node with an edge into another rank's part) -> zone 0 of the schedule (mrf.h); null: no marks
    int mrf_force_generic = 0;   // test hook: every node takes the generic sweep kernel
    // view-set bitmaps of the active table, F x ceil(csr_views / 64) words, rebuilt by every mrf_setup (k_mrf_setup.hip mrf_bitmap_kernel); m_bitmaps:
    // the last set-up took the bitmap route (not: more than 1024 views, a column that is not strictly ascending, the hook below)
    mvs::DBuf<unsigned long long> m_bits; bool m_bitmaps = false;
    int mrf_force_lists = 0;     // test hook: the set-up compares and searches the neighbours' view lists at any number of views
    uint32_t m_range_nb = 0, m_range_ne = 0; std::vector<uint32_t> m_range_q;   // cached own share of every sub-class
    uint32_t m_sweep_no = 0;   // sweeps started since mrf_setup (1-based inside a sweep): sweeps 1, 5, 9, ... are damped
    uint32_t m_last_phase = 0xFFFFFFFFu;   // colour phase of the last mrf_sweep_phase since mrf_setup (none yet: 0xFFFFFFFF): a smaller phase number starts a sweep
    mvs_mrf_params m_params{};
    // device-side stop rule (k_mrf_polish.hip mrf_step): solver state in HBM, per-step reports through a pinned ring
    static constexpr uint32_t RING = 16;
    static constexpr uint32_t ICM_RING = 8;
    uint32_t* h_icm = nullptr; uint32_t* d_icm = nullptr; uint32_t icm_seq = 0;   // pinned "moved" counts of the ICM rounds, read a few rounds late
    mvs::DBuf<mvs_mrf_progress> m_state; mvs::DBuf<unsigned long long> m_hist; mvs::DBuf<uint32_t> m_ctl;   // m_ctl: {steps of the solve, sequence base} read by the step kernel
    // the sweep loop as a replayed hipGraph (solve.hip): one damping period, MRF_DAMP_PERIOD sweeps + their bookkeeping steps, captured on a
    // private stream, launched on the context's stream; re-captured per solve and pushed into the instantiated graph with hipGraphExecUpdate
    int mrf_graph = 1; hipStream_t cap_stream = nullptr; hipGraphExec_t sweep_exec = nullptr; uint32_t graph_launches = 0, graph_updates = 0, graph_instantiations = 0;
    mvs_mrf_progress* h_ring = nullptr; mvs_mrf_progress* d_ring = nullptr /* the same pinned slots as the device addresses them */; uint32_t steps_issued = 0; int mrf_lag = 1;
    // arrival of a report = its sequence number in the pinned word next to it (written after a system-scope fence): the host polls
    // memory, no event is recorded in the stream.  Sequence numbers never repeat within a context.
    uint32_t* h_seq = nullptr; uint32_t* d_seq = nullptr; uint32_t seq_base = 0;   // [0, RING): solver steps; [RING, RING + ICM_RING): ICM rounds
};

namespace mvs {
// a caller's view as the kernels read it: the camera and the size (every view input fills in rgb itself)
inline ViewParams view_params_of(const mvs_view& v) {
    ViewParams p{};
    memcpy(p.pos, v.pos, sizeof(p.pos)); memcpy(p.viewdir, v.viewdir, sizeof(p.viewdir));
    memcpy(p.K, v.K, sizeof(p.K)); memcpy(p.w2c, v.w2c, sizeof(p.w2c));
    p.width = v.width; p.height = v.height;
    return p;
}
// RAII stage marker; no-op unless ctx->profile
struct Prof {
    mvs_ctx* c; size_t idx; bool on;
    Prof(mvs_ctx* ctx, const char* name) : c(ctx), idx(0), on(ctx->profile) {
        if (!on) return;
        auto get = [&]() { hipEvent_t e; if (!c->prof_pool.empty()) { e = c->prof_pool.back(); c->prof_pool.pop_back(); } else { MVS_HIP(hipEventCreate(&e)); } return e; };
        ProfSpan sp{name, get(), get(), true};
        MVS_HIP(hipEventRecord(sp.a, c->stream));
        idx = c->prof_spans.size(); c->prof_spans.push_back(sp);
    }
    void end() { if (on) { MVS_HIP(hipEventRecord(c->prof_spans[idx].b, c->stream)); on = false; } }
    ~Prof() { if (on) (void)hipEventRecord(c->prof_spans[idx].b, c->stream); }
};
// Adjacent spans that share their boundary events: one hipEventRecord per mark instead of two per span (an event record costs
// ~5 us of stream time; the solver loop alternates two short stages 42 times).
struct ProfChain {
    mvs_ctx* c; hipEvent_t prev; bool on;
    static hipEvent_t get(mvs_ctx* c) { hipEvent_t e; if (!c->prof_pool.empty()) { e = c->prof_pool.back(); c->prof_pool.pop_back(); } else { MVS_HIP(hipEventCreate(&e)); } return e; }
    explicit ProfChain(mvs_ctx* ctx) : c(ctx), prev(nullptr), on(ctx->profile) {}
    void begin() { if (on && !prev) { prev = get(c); MVS_HIP(hipEventRecord(prev, c->stream)); first = true; } }
    void mark(const char* name) {       // closes the span [previous mark, now)
        if (!on) return;
        begin();
        hipEvent_t e = get(c);
        MVS_HIP(hipEventRecord(e, c->stream));
        c->prof_spans.push_back(ProfSpan{name, prev, e, first});
        first = false; prev = e;
    }
    bool first = false;
};
// roctx range around the two windows the reference times (apps/texrecon/texrecon.cpp:118 "Calculating data costs", :126 "Running MRF
// optimization"): visible to rocprofv3 --marker-trace; libroctx64 is resolved at run time (no link-time dependency), absent = no-op
struct RoctxRange { explicit RoctxRange(const char* name); ~RoctxRange(); bool on; };
// device for the one-shot host entry points (mvs_data_costs, mvs_view_selection, ...): environment MVS_DEVICE, default 0
int default_device();
// option "dc_range_pairs" as the environment sets it (MVS_DC_RANGE_PAIRS, 0 when unset): for a new context and for every one-shot call
uint64_t env_dc_range_pairs();
// which zone(s) of a colour phase mrf_sweep_phase sweeps (k_mrf_sweep.hip)
enum { MRF_PART_ALL = 0, MRF_PART_BOUNDARY = 1, MRF_PART_INTERIOR = 2 };
// reports through pinned host memory (readback.hip)
void ensure_report_ring(mvs_ctx* ctx);
void report_u32(mvs_ctx* ctx, const uint32_t* d_src, uint32_t* d_dst, uint32_t seq_slot, uint32_t seq);
void wait_report(mvs_ctx* ctx, uint32_t seq_slot, uint32_t seq);
// ICM polish rounds until one moves nothing or max_rounds ran (k_mrf_polish.hip): round(k) queues round k, which leaves its "moved" count in
// the device word d_moved.  Returns the index of the round that moved nothing (max_rounds if none did) -- the oracle's loop counter.
int icm_rounds(mvs_ctx* ctx, int max_rounds, const uint32_t* d_moved, const std::function<void(int)>& round);
constexpr uint32_t MRF_REC_BASE = 256;   // the first record starts at this word of m_rec (k_mrf_setup.hip REC_BASE)
// damped sweeps: 1, 5, 9, ... -- part of the solver's definition, restated in oracle/oracle.cpp (MRF_DAMP_PERIOD)
constexpr uint32_t MRF_DAMP_PERIOD = 4;
// up to 64 words from device memory to the host between two launches of ctx->stream: a one-block kernel stores them into a pinned buffer and
// announces them with a sequence number the host spins on (readback.hip).  A 4-byte hipMemcpyAsync into pageable memory + hipStreamSynchronize
// holds the device idle for 22 us, this for 9 (scripts/probe/readback_cost.hip) -- a step has a dozen of them on its critical path.
void read_words(mvs_ctx* ctx, const void* d_src, void* out, uint32_t n_words);
// one word the plain way: a 4-byte copy into pageable memory and a drain of ctx->stream (where that drain is wanted anyway, or off the hot path)
inline uint32_t read_u32(mvs_ctx* ctx, const uint32_t* d) {
    uint32_t h = 0;
    MVS_HIP(hipMemcpyAsync(&h, d, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    MVS_HIP(hipStreamSynchronize(ctx->stream));
    return h;
}
// one word through the pinned route of read_words: between two launches of a pass, where read_u32's drain would hold the device idle
inline uint32_t read_word(mvs_ctx* ctx, const uint32_t* d) { uint32_t h = 0; read_words(ctx, d, &h, 1); return h; }
void read_block(mvs_ctx* ctx, const void* d_src, void* out, size_t bytes);   // up to 4 KB, through pinned staging (readback.hip)
// generic device exclusive scan (scan.hip): out[i] = sum_{k<i} in[i]; returns total via d_total (device, may be null)
void exclusive_scan_u32(mvs_ctx* ctx, const uint32_t* in, uint32_t* out, size_t n, uint32_t* d_total);
// exact 64-bit total of a u32 array (blocking): the guard in front of scans whose total may pass 2^32
uint64_t sum_u32(mvs_ctx* ctx, const uint32_t* in, size_t n);
// frees the buffers of row f5 (k_seam.hip)
void gsl_release(mvs_ctx* ctx);
// frees the buffers of row f6 (k_texpatch.hip)
void texpatch_release(mvs_ctx* ctx);
// frees the buffers of row f7 (k_localseam.hip)
void lsl_release(mvs_ctx* ctx);
void atlas_release(mvs_ctx* ctx);
// frees the buffers of row f9 (k_model.hip)
void model_release(mvs_ctx* ctx);
// k_model.hip, shared with row f11 (k_glb.hip); `who` starts every message:
//   model_check_set: the host-side rules of "Model output" item 6 -- throws MVS_ERR_STATE without a mesh, MVS_ERR_INVALID for a null array or
//     a face_ptr / tc_ptr that does not run from 0 to the totals or descends; leaves both arrays ([n_atlases + 1]) on the host
//   model_refuse_bad_ids: MVS_ERR_INVALID for the counts the device pass made of model_corner.h's two id rules
//   model_check_image_params: image_format, png_level / png_device or jpeg_quality / jpeg_subsampling and the arrays the images need, as
//     mvs_ctx_save_model refuses them
//   model_for_each_image: the image file (PNG or JPEG) of every atlas by the route params chooses (png_io.h on up to 16 host threads, k_png.hip or
//     k_jpeg.hip), handed to `sink` (atlas, bytes, count, message) on the thread that holds it; the bytes are valid during the call only
//   device_to_stream: a device range into an open file through the context's pinned buffer, 32 MB at a time (false: write error);
//     ms_copy: the time spent waiting for the copies
void model_check_set(mvs_ctx* ctx, const mvs_atlas_set& in, int on_device, const char* who, std::vector<uint32_t>& face_ptr, std::vector<uint32_t>& tc_ptr);
void model_refuse_bad_ids(uint64_t bad_faces, uint64_t bad_ids, const char* who);
void model_check_image_params(const mvs_model_params& P, const mvs_atlas_set& in, const char* who);
typedef std::function<mvs_status(uint32_t, const uint8_t*, size_t, std::string&)> ModelImageSink;
void model_for_each_image(mvs_ctx* ctx, const mvs_atlas_set& in, int atlases_on_device, const mvs_model_params& P, const char* who, const ModelImageSink& sink);
bool device_to_stream(mvs_ctx* ctx, const char* d, uint64_t bytes, FILE* f, double& ms_copy);
std::string model_filled4(uint32_t a);   // util::string::get_filled(a, 4)
// frees the buffers of row f11 (k_glb.hip)
void glb_release(mvs_ctx* ctx);
// frees the buffers of row f10 (k_debug.hip)
void debug_release(mvs_ctx* ctx);
// k_png.hip, k_jpeg.hip: free their buffers (the routes themselves: image_routes.h)
void png_release(mvs_ctx* ctx);
void jpeg_release(mvs_ctx* ctx);
void jpegdec_release(mvs_ctx* ctx);   // k_jpegdec.hip
void pngdec_release(mvs_ctx* ctx);    // k_pngdec.hip
void lens_release(mvs_ctx* ctx);      // k_lens.hip
// k_lens.hip: byte masks in the camera's frame -> keep words in the undistorted frame, one span launch (view_input.h) for the n views of T
// (DESIGN.md section 4 "View input" item 10); adds the launch's device time to ms.  Returns with the stream drained.
struct LensMaskView { const uint8_t* src; uint32_t* keep; int32_t width, height; float flen, d0, d1; uint32_t pad_; };
void lens_mask_run(mvs_ctx* ctx, const std::vector<LensMaskView>& T, float& ms);
// k_viewmask.hip: what prepare_views hands to its kernels -- the device table of every view's keep words (null entries: views without a
// mask) and the device list of the n_masked views that carry one; table == null: the scene has no masks.  view_keep_words: one view's
// keep words on the device (null: none; the harness read-back of mgpu.hip).  view_masks_clear forgets the masks (every view input calls
// it), viewmask_release frees them.
struct ViewKeep { const uint32_t* const* table; const uint32_t* list; uint32_t n_masked; };
ViewKeep view_keep(mvs_ctx* ctx);
const uint32_t* view_keep_words(mvs_ctx* ctx, uint32_t view, std::vector<const uint32_t*>& host_table);
void view_masks_clear(mvs_ctx* ctx);
void viewmask_release(mvs_ctx* ctx);
// k_jpegdec.hip: the views whose files[j] is not null, decoded in batches whose scratch fits params->max_scratch_bytes (null: the default) --
// view j into dst[j], or, where staged[j] is not 0, into the context's staging (view_input.h view_staging), whose 3 * width * height bytes
// count towards the view's scratch.  After every batch that staged views, after_batch(views, pixels) gets their numbers and where their decoded
// pixels lie (valid until it returns).  `who` starts the messages; throws as mvs_scene_set_views_jpeg refuses.
typedef std::function<void(const std::vector<uint32_t>& views, const std::vector<const uint8_t*>& pixels)> StagedBatchFn;
// png_stats (null: the entries that refuse a PNG as any file that is no baseline JPEG): a file that starts with the PNG signature takes the
// PNG route (decode_view_pngs) under the same rules, its batches cut on their own.
void decode_view_files(mvs_ctx* ctx, const mvs_view* views, uint32_t n_views, const uint8_t* const* files, const uint64_t* sizes, uint8_t* const* dst, const uint8_t* staged,
                       const mvs_jpegdec_params* params, const char* who, mvs_jpegdec_stats& st, const StagedBatchFn& after_batch, mvs_pngdec_stats* png_stats = nullptr);
// k_pngdec.hip: decode_view_files for the PNG files fv of a scene (view_input.h FileViews; dst and staged are indexed by the view)
struct FileViews;
void decode_view_pngs(mvs_ctx* ctx, const mvs_view* views, const FileViews& fv, uint8_t* const* dst, const uint8_t* staged, const mvs_jpegdec_params* params, const char* who,
                      mvs_pngdec_stats& st, const StagedBatchFn& after_batch);
// k_lens.hip: the body of mvs_scene_set_views_jpeg (lens == null), mvs_scene_set_views_lens and mvs_scene_set_views_files (accept_png) behind their argument checks
mvs_status set_views_files(mvs_ctx* ctx, const mvs_view* views, uint32_t n_views, const mvs_lens* lens, const uint8_t* const* files, const uint64_t* sizes,
                           const mvs_jpegdec_params* jpeg_params, mvs_jpegdec_stats* jpeg_stats, mvs_lens_stats* lens_stats, const char* who_view, const char* who,
                           bool accept_png = false, mvs_pngdec_stats* png_stats = nullptr, const mvs_view_level* levels = nullptr, mvs_level_stats* level_stats = nullptr);
// k_level.hip (DESIGN.md section 4 "View input" item 14): ONE span launch halves the images of T `level` times (1 .. 4) from the staging
// into dst; d0 != 0: the source fetch is lens.h lens_pixel, and the pixels without a source are counted into lens_st as lens_kernel counts
// them (full-size pixels).  Returns with the stream drained.  keep_level_run: full-size keep words (`src`, the layout of the validity
// mask) -> the level's keep words, one launch.  check_levels: the refusals of an mvs_view_level list against the views at their level.
struct LevelItem { const uint8_t* src; uint8_t* dst; int32_t width, height; uint32_t level; float flen, d0, d1; };
struct KeepLevelItem { const uint32_t* src; uint32_t* keep; int32_t width, height; uint32_t level, pad_; };
void level_run(mvs_ctx* ctx, const std::vector<LevelItem>& T, const char* who, mvs_level_stats& st, mvs_lens_stats& lens_st);
void keep_level_run(mvs_ctx* ctx, const std::vector<KeepLevelItem>& T, float& ms);
void check_levels(const mvs_view* views, const mvs_view_level* levels, uint32_t n, const char* who);
void level_release(mvs_ctx* ctx);
// k_lens.hip: host images through staging in groups of at most `cap` bytes: image k (src[k], w[k] x h[k], lens[k], level[k]) -> dst[k]; `view`
// names image k in a refusal.  Level 0: lens_kernel (dist0 == 0 copies), above: level_run.  level_st may be null where every level is 0.
void stage_pixels(mvs_ctx* ctx, const std::vector<const uint8_t*>& src, const std::vector<uint8_t*>& dst, const std::vector<uint32_t>& w, const std::vector<uint32_t>& h,
                  const std::vector<mvs_lens>& lens, const std::vector<uint32_t>& level, const std::vector<uint32_t>& view, uint64_t cap, const char* who, mvs_lens_stats& st,
                  mvs_level_stats* level_st);
// k_tone.hip: the mode of a parameter struct checked (throws MVS_ERR_INVALID, `who` in front, for anything but none / gamma); the device
// table of the context for tone mapping `gamma` -- built from tone.h and uploaded on first use, or what tone_table_set put there
// (256 host floats; null: the gamma table again; the harness entry mvs_ctx_tone_table)
uint32_t tone_mode(uint32_t tone_mapping, const char* who);
const float* tone_table_dev(mvs_ctx* ctx);
void tone_table_set(mvs_ctx* ctx, const float* table256);
// rows f5 / f6 (k_texpatch.hip): the views' parameters on the device and the checks on the caller's labels and faces -- throws MVS_ERR_LABELING
// for a label above the number of views, MVS_ERR_INVALID for a vertex id >= n_verts; `who` starts the message
void patch_check_inputs(mvs_ctx* ctx, PatchTables& T, const uint32_t* d_labels, const char* who);
// the candidates of every label (get_subgraphs), their boxes, the merge loop, patch ids, every face's patch and position: fills T and
// T.C / n_patches / n_merged; throws MVS_ERR_LABELING when a labelled face leaves its view's image.  Needs patch_check_inputs first.
void build_patch_tables(mvs_ctx* ctx, PatchTables& T, const uint32_t* d_adj_ptr, const uint32_t* d_adj, const uint32_t* d_labels, const char* who);

// ---- every other function one source file defines and another calls: declared here and nowhere else, grouped by the defining file ----
// api.hip
mvs_status api_fail(mvs_status st, const std::string& msg);   // records the message of mvs_last_error, returns st
// the caller's adjacency lists (host or device) as ctx->r_adj_ptr / r_adj in the order of the active table; table_order: they already are
void set_adjacency(mvs_ctx* ctx, const uint32_t* adj_ptr, const uint32_t* adj, int on_device, bool table_order);
// host ranges src[k][0, bytes[k]) -> device dst[k] through the device's pinned upload ring; returns with the stream drained
void upload_pieces_through_ring(mvs_ctx* ctx, const uint8_t* const* src, uint8_t* const* dst, const size_t* bytes, size_t n);
void release_upload_rings();   // frees the pinned upload ring of every device (mvs_release_cached; the next host-image upload allocates again)
// solve.hip
void sweep_graph_release(mvs_ctx* ctx);   // destroys the sweep loop's executable graph and capture stream
// k_prep.hip
void prepare_views(mvs_ctx* ctx, bool need_gmi, const size_t* d_gmi_off, const size_t* d_mask_off);   // image preparation of all views (ctx->d_views uploaded)
void undistort_image(mvs_ctx* ctx, const uint8_t* d_src, uint8_t* d_dst, int w, int h, double flen, double d0, double d1);
// k_bvh.hip
void build_scene_order(mvs_ctx* ctx);    // the resident mesh along a Hilbert curve: ctx->iv / ifc / inr, f_perm / f_pos
bool scene_order_commit(mvs_ctx* ctx);   // true: the upper levels of the order overflowed and it was rebuilt without them -- derive again what came from it
void build_bvh(mvs_ctx* ctx);            // BVH + vertex -> face incidence of the mesh in the layout of build_scene_order
void trace_rays(mvs_ctx* ctx);
void build_vertex_faces(mvs_ctx* ctx, const uint32_t* d_faces, uint32_t F, uint32_t NV);   // vertex -> incident faces (CSR ctx->vf_ptr / vf)
// k_kdorder.hip
void kd_refine_order(mvs_ctx* ctx, const float* verts, const uint32_t* faces, uint32_t* order, uint32_t F, uint32_t window, uint32_t leaf_window);   // upper levels of the face order
// k_dc.hip
void dc_phase1(mvs_ctx* ctx, const mvs_settings* st);     // everything up to the per-face sorted infos + the local maximum quality
void dc_phase2(mvs_ctx* ctx);                             // histogram of the local qualities against the (possibly all-reduced) maximum
void dc_phase3(mvs_ctx* ctx, mvs_dc_stats* stats);        // percentile from the (possibly all-reduced) histogram, cost write
void dc_run(mvs_ctx* ctx, const mvs_settings* st, mvs_dc_stats* stats);   // the three phases, or the ranged walk (option "dc_range_pairs")
void dc_prune_labels(mvs_ctx* ctx, uint32_t kmax);        // prunes the context's own active table in place
// postprocess_face_infos on host lists (every face's list reversed): outlier detection, then phases 2 and 3
void dc_postprocess(mvs_ctx* ctx, uint32_t nf, uint32_t n_views, const uint32_t* h_ptr, const uint16_t* h_view_rev, const float* h_q_rev, const float* h_col_rev, const mvs_settings* st);
// k_order.hip
bool table_to_caller_order(mvs_ctx* ctx, bool with_quality);   // the active table -> ctx->u_*; false: it already is in the caller's order (read r_*)
void adjacency_to_table_order(mvs_ctx* ctx, const uint32_t* d_adj_ptr, const uint32_t* d_adj, size_t E);   // device lists -> ctx->m_adj_ptr / m_adj
// device lists in the caller's numbering -> out_ptr / out_adj in the order `perm` (position -> caller's id; `pos` its inverse), list order kept
void renumber_adjacency(mvs_ctx* ctx, uint32_t F, const uint32_t* perm, const uint32_t* pos, const uint32_t* d_adj_ptr, const uint32_t* d_adj, size_t E,
                        DBuf<uint32_t>& out_ptr, DBuf<uint32_t>& out_adj);
// k_patch.hip
// components of equal labels -> ctx->p_label_ptr [n_labels + 1], p_comp_ptr [C + 1], p_comp_faces [F]; returns C
uint32_t get_subgraphs(mvs_ctx* ctx, const uint32_t* d_adj_ptr, const uint32_t* d_adj, const uint32_t* d_labels, uint32_t F, uint32_t n_labels);
// k_region.hip
uint32_t mrf_region_round(mvs_ctx* ctx);   // one round of region moves on the best labeling (needs mrf_exact_costs); returns the regions moved
// the MRF solver -- node ranges [nb0, ne0) are positions of the active table
// k_mrf_setup.hip
void mrf_setup(mvs_ctx* ctx, const mvs_mrf_params* params);   // the solver's tables for the active table and adjacency
// k_mrf_sweep.hip
void mrf_sweep(mvs_ctx* ctx, uint32_t nb0, uint32_t ne0);     // one sweep = every colour phase in turn
void mrf_sweep_phase(mvs_ctx* ctx, uint32_t phase, uint32_t nb0, uint32_t ne0, int part = MRF_PART_ALL);   // one colour phase, both zones or one
// k_mrf_polish.hip
void mrf_sweep_energy_reduce(mvs_ctx* ctx, unsigned long long* out2 = nullptr);   // the last sweep's per-block energy partials -> ctx->m_energy (and out2)
void mrf_energy(mvs_ctx* ctx, bool best, uint32_t nb0, uint32_t ne0, bool reduce = true);   // energy of the current decode or the best labeling -> ctx->m_energy
void mrf_keep_best(mvs_ctx* ctx);                             // best labeling := the current decode
void mrf_exact_costs(mvs_ctx* ctx, uint32_t nb0, uint32_t ne0);   // position and exact unary of every label of the best labeling (idempotent)
// one bookkeeping step of the device-side stop rule; energy = the all-reduced pair, or null: per-block partials (or the peers' tables)
void mrf_step(mvs_ctx* ctx, const unsigned long long* energy, const unsigned long long* const* peer_tab = nullptr, uint32_t n_peer = 0, uint32_t peer_off = 0);
void mrf_poll(mvs_ctx* ctx, uint32_t step, mvs_mrf_progress* out);   // waits for the report of one of the last 16 steps
void mrf_icm_gain(mvs_ctx* ctx, uint32_t nb0, uint32_t ne0);  // ICM on the best labeling: gains and candidates
void mrf_icm_apply(mvs_ctx* ctx, uint32_t nb0, uint32_t ne0); // ... the winners move; the count lands in words->icm_n_moved
// labels of the best labeling into d_labels; out = {bad, unseen}; caller_order: the whole graph's labels at the caller's face ids
void mrf_labels(mvs_ctx* ctx, uint32_t nb0, uint32_t ne0, uint32_t* d_labels, uint32_t out[2], bool caller_order = false);
void resolve_best(mvs_ctx* ctx);                              // ctx->b_sel / b_lab / b_cost := the best labeling's buffers (one read-back)
// The best labeling may have changed on the device (a bookkeeping step, keep_best, a replayed graph of sweeps): which buffer holds it,
// the exact costs derived from it and the ICM's active list are stale until somebody asks again.
inline void best_labeling_may_have_changed(mvs_ctx* ctx) { ctx->icm_dirty_valid = false; ctx->best_resolved = false; ctx->exact_valid = false; }

// ---- around the body of an entry point: what it throws becomes the call's status and the message of mvs_last_error ----
#define MVS_CATCH_TO_STATUS                                                                \
    catch (const mvs::StatusError& e) { return mvs::api_fail(e.st, e.what()); }            \
    catch (const mvs::HipError& e) { return mvs::api_fail(MVS_ERR_HIP, e.what()); }        \
    catch (const std::exception& e) { return mvs::api_fail(MVS_ERR_HIP, e.what()); }
template <class Body>
mvs_status api_guard(Body&& body) {
    try { body(); } MVS_CATCH_TO_STATUS
    return MVS_OK;
}
// the same as a bracket around the statements of a function that returns mvs_status; MVS_CTX_API_BEGIN makes ctx->device current first
#define MVS_API_BEGIN try {
#define MVS_API_END } MVS_CATCH_TO_STATUS return MVS_OK;
#define MVS_CTX_API_BEGIN MVS_API_BEGIN MVS_HIP(hipSetDevice(ctx->device));
}  // namespace mvs
