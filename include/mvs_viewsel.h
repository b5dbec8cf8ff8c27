/* mvs_viewsel.h -- C ABI of the MI355X-native view-selection hot path.
 *
 * Drop-in boundary for nmoehrle/mvs-texturing's
 *     tex::calculate_data_costs   (libs/tex/texturing.h:66-69,
 *                                  libs/tex/calculate_data_costs.cpp:308-323)
 *     tex::postprocess_face_infos (libs/tex/texturing.h:71-74)   [folded into the above]
 *     tex::view_selection         (libs/tex/texturing.h:79-80,
 *                                  libs/tex/view_selection.cpp:18-133)
 * as called from apps/texrecon/texrecon.cpp:98-127.  Plain pointers and sizes
 * only: no MVE / STL / torch types cross this boundary.  The header-only C++
 * adapter include/tex_viewsel.hpp re-exposes the reference's own signatures
 * on top of these entry points; INTEGRATION.md shows the texrecon-side patch.
 *
 * All kernels are hand-written HIP for gfx950; there is NO CPU fallback: every
 * entry point fails with MVS_ERR_HIP when no usable device is present.
 */
#ifndef MVS_VIEWSEL_H
#define MVS_VIEWSEL_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    MVS_OK = 0,
    MVS_ERR_INVALID = 1,        /* bad argument */
    MVS_ERR_TOO_MANY_FACES = 2, /* "Exeeded maximal number of faces"  calculate_data_costs.cpp:315-316 */
    MVS_ERR_TOO_MANY_VIEWS = 3, /* "Exeeded maximal number of views"  calculate_data_costs.cpp:317-318 */
    MVS_ERR_LABELING = 4,       /* "Incorrect labeling"               view_selection.cpp:126-128 */
    MVS_ERR_HIP = 5,            /* HIP runtime / device failure (see mvs_last_error) */
    MVS_ERR_STATE = 6,          /* call order violated (e.g. view selection before data costs) */
    MVS_ERR_UNSUPPORTED = 7
} mvs_status;

/* mve::TriangleMesh fields read at calculate_data_costs.cpp:136-138 */
typedef struct {
    uint32_t n_verts;
    uint32_t n_faces;
    const float* verts;        /* 3 * n_verts, xyz                      mesh->get_vertices()     */
    const uint32_t* faces;     /* 3 * n_faces, vertex indices           mesh->get_faces()        */
    const float* face_normals; /* 3 * n_faces, unit normals             mesh->get_face_normals() */
} mvs_mesh;

/* tex::TextureView fields read by the path (texture_view.h:43-48) + the decoded
 * image that TextureView::load_image() (texture_view.cpp:96-100) would hold. */
typedef struct {
    float pos[3];      /* TextureView::pos                      */
    float viewdir[3];  /* TextureView::viewdir                  */
    float K[9];        /* TextureView::projection, row major    */
    float w2c[16];     /* TextureView::world_to_cam, row major  */
    int32_t width;
    int32_t height;
    const uint8_t* rgb; /* width*height*3 interleaved RGB8 (mve::ByteImage layout) */
} mvs_view;

/* Host images that exist only while they are needed.  tex::calculate_data_costs loads and releases ONE view's image per iteration
 * (calculate_data_costs.cpp:157 tv.load_image() ... :231 tv.release_image()): its host peak is one decoded image, whatever the number of
 * views.  An entry point that takes an image source asks for the pixels view by view -- acquire(user, j) returns the RGB8 pixels of view j
 * (width / height as in views[j]; mvs_view.rgb is ignored), release(user, j) hands them back -- both on the CALLING thread, with at most
 * max_in_flight (0 = 4) views acquired at any time: a batch is acquired, copied to the device and released.  acquire returns NULL when the
 * image cannot be produced: the call fails with MVS_ERR_INVALID after releasing every view acquired so far (as every failure does). */
typedef const uint8_t* (*mvs_image_acquire_fn)(void* user, uint32_t view);
typedef void (*mvs_image_release_fn)(void* user, uint32_t view);
typedef struct {
    mvs_image_acquire_fn acquire;
    mvs_image_release_fn release;
    void* user;
    uint32_t max_in_flight;
} mvs_image_source;

/* tex::Settings fields the path reads (settings.h:85,87,90; enums settings.h:59-74) */
enum { MVS_DATA_TERM_AREA = 0, MVS_DATA_TERM_GMI = 1 };
enum { MVS_OUTLIER_NONE = 0, MVS_OUTLIER_GAUSS_DAMPING = 1, MVS_OUTLIER_GAUSS_CLAMPING = 2 };
typedef struct {
    int32_t data_term;                 /* default MVS_DATA_TERM_GMI   (settings.h:85) */
    int32_t outlier_removal;           /* default MVS_OUTLIER_NONE    (settings.h:87) */
    int32_t geometric_visibility_test; /* default 1                   (settings.h:90) */
} mvs_settings;

/* tex::DataCosts = SparseTable<uint32_t, uint16_t, float> (texturing.h:36,
 * sparse_table.h:29-110) as CSR over faces: column i of the table is
 * view_id/cost[col_ptr[i] .. col_ptr[i+1]), view ids strictly ascending
 * (calculate_data_costs.cpp:272), costs in [0,1] (:295-296). */
typedef struct {
    uint32_t n_faces;   /* SparseTable::cols() */
    uint32_t n_views;   /* SparseTable::rows() */
    uint64_t nnz;
    uint32_t* col_ptr;  /* n_faces + 1 */
    uint16_t* view_id;  /* nnz */
    float* cost;        /* nnz */
} mvs_csr;

/* Solver controls.  The reference hard-codes its mapMAP configuration
 * (view_selection.cpp:84,103-115); mapMAP is replaced by a GPU-resident
 * tree-reweighted max-product solver -- colour-phased Gauss-Seidel sweeps + monotone ICM polish --
 * whose knobs are below.  mvs_mrf_default_params gives the shipped defaults
 * (200 / 20 / 5 / 0.005 / 0.2 / 0.8 / 50 / 0).  Round 6 scored damping schedule x stop rule in milliseconds
 * (profiles/r06_schedule_score_c3.json): alpha = 0.2 on every fourth sweep with window 5 / 0.5 % reaches +0.99 % over the LP bound
 * in 39 sweeps at BASELINE config 3, where rounds 1 - 5 (alpha on odd sweeps, 0.2 %) took 44 sweeps to +0.94 %. */
typedef struct {
    int32_t max_sweeps;
    int32_t min_sweeps;
    int32_t window;         /* stop when the best energy gained < min_improvement over `window` sweeps; cf. StopWhenReturnsDiminish(5, 0.01) view_selection.cpp:84 */
    float min_improvement;
    float damping;          /* alpha of m' = (1 - alpha) new + alpha old on every FOURTH sweep (1st, 5th, 9th, ...); the others are undamped */
    float rho;
    int32_t icm_iters;
    int32_t region_rounds;  /* > 0: after the ICM polish, up to this many rounds of REGION MOVES (a connected same-label patch takes a
                               neighbouring patch's label when that lowers the energy; csrc/k_region.hip), each followed by a fresh
                               polish.  0 = off (default).  Single-context solves only: the sharded path refuses it. */
} mvs_mrf_params;

typedef struct {
    uint64_t energy_fixed;  /* 32.32 fixed point: sum_i D_i(l_i) + #cut edges */
    double energy;
    uint64_t cut_edges;
    uint32_t sweeps;
    uint32_t icm_iters;
    uint32_t unseen;        /* "faces have not been seen"  view_selection.cpp:129,132 */
    uint32_t region_rounds; /* rounds of region moves that moved something */
    uint32_t region_moves;  /* regions relabelled in total */
} mvs_mrf_stats;

typedef struct {
    /* After a ranged pass (option "dc_range_pairs") pairs, the five cull counters, nnz_pre, nnz, footprints_lane_group and footprints_rewalked
     * are sums over the ranges and EQUAL the unranged pass's values (each is a count per (face, view) pair); max_quality and percentile are
     * the global ones; rays, ray_nodes, ray_tris, ray_packets, ray_packets_generic and ray_leaf_rounds are sums over the ranges and MAY
     * EXCEED the unranged values: a vertex shared by faces of two ranges is traced once per range. */
    uint64_t pairs;
    /* the five cull counters and `rays` are filled only with mvs_set_option("stats", 1) */
    uint64_t cull_backface;     /* calculate_data_costs.cpp:183-185 */
    uint64_t cull_angle;        /* :187-188 */
    uint64_t cull_outside;      /* :191 */
    uint64_t cull_occluded;     /* :194-215 */
    uint64_t cull_zero_quality; /* :222 */
    uint64_t nnz_pre;           /* FaceProjectionInfos emitted (:227-228) */
    uint64_t nnz;
    uint64_t rays;              /* (vertex, view) rays traced -- each distinct ray once (once per range of a ranged pass) */
    uint64_t ray_nodes;         /* BVH node visits of the 64-ray packets: one 128-byte node = 4 child boxes each  (only with mvs_set_option("count_rays", 1)) */
    uint64_t ray_tris;          /* triangles fetched: 16 per leaf a packet's rays enter   (idem) */
    uint64_t ray_packets;         /* 64-ray packets traced (with "stats") */
    uint64_t ray_packets_generic; /* ... of which with mixed / degenerate direction signs: the unspecialised slab test */
    float max_quality;          /* :278-281 */
    float percentile;           /* :288 */
    uint64_t footprints_lane_group; /* sampled footprints above "info_wave_area" pixels: summed by a 16-lane group (integer pixel sums) */
    uint64_t footprints_rewalked;   /* ... of which the exactness certificate could not decide: re-walked in the reference's serial fp64 order */
    uint64_t ray_leaf_rounds;       /* rounds of 4 candidate rays x 16 triangles at the leaves ("count_rays") */
} mvs_dc_stats;

const char* mvs_last_error(void);
const char* mvs_status_string(mvs_status s);
void mvs_mrf_default_params(mvs_mrf_params* p);
void mvs_default_settings(mvs_settings* s);

/* ------------------------------------------------------------------------
 * One-shot host entry points: what the tex:: adapter calls.  Inputs are host
 * pointers borrowed for the duration of the call.
 * ------------------------------------------------------------------------ */

/* The two drop-ins below are what texrecon calls back to back (texrecon.cpp:100,121).  mvs_data_costs parks its device context --
 * table resident -- in a one-slot stash with a fingerprint of the table it handed out; mvs_view_selection solves on that context when
 * the table it is given has the same fingerprint (no context set-up, no table upload), and uploads it as usual otherwise.
 * After its solve mvs_view_selection parks the context as a spare: the next one-shot call reuses its stream, device buffers and graph.
 * At most two contexts are parked; their device memory stays allocated until mvs_release_cached() or the end of the process.
 * The stash is per PROCESS (texrecon's pattern: one caller thread, one scene): concurrent callers are safe -- it is locked, and every
 * thread has its own call profile -- but only the last table handed out stays parked; the one-shot calls run on the device named by
 * the environment variable MVS_DEVICE (default 0).
 * Host images (mvs_scene_set_views with host pointers, hence every one-shot call) reach the device through a ring of library-owned
 * pinned buffers filled by host threads (MVS_UPLOAD_THREADS, default min(8, cores / 2); up to 256 MB of pinned memory per device, kept
 * until mvs_release_cached()); nothing of the caller's address space is registered with the driver.  Environment
 * MVS_HOST_UPLOAD=register pins the caller's pages in place instead (hipHostRegister; opt-in: see csrc/api.hip), =pageable copies
 * from pageable memory (~4x slower).  (MVS_PIN_HOST_IMAGES=1 / 0 are the older spellings of register / pageable.)
 * Environment MVS_KEEP_TABLE=0 switches all of that off; mvs_release_cached() frees what is parked; mvs_last_call_profile() = wall-clock
 * breakdown (JSON object) of the calling thread's last one-shot call. */
void mvs_release_cached(void);
const char* mvs_last_call_profile(void);

/* replaces tex::calculate_data_costs (texturing.h:66-69).  `out` is library
 * allocated (nnz is unknown up front); release with mvs_csr_free. */
mvs_status mvs_data_costs(const mvs_mesh* mesh, const mvs_view* views, uint32_t n_views,
                          const mvs_settings* settings, mvs_csr* out, mvs_dc_stats* stats);
void mvs_csr_free(mvs_csr* csr);

/* replaces tex::view_selection (texturing.h:79-80).  adj_ptr/adj: UniGraph
 * adjacency lists (uni_graph.h:22) flattened in list order; labels_out[F] is
 * caller allocated and receives UniGraph::labels (0 = unseen, else view+1). */
mvs_status mvs_view_selection(const mvs_csr* costs, const uint32_t* adj_ptr, const uint32_t* adj,
                              const mvs_mrf_params* params, uint32_t* labels_out,
                              mvs_mrf_stats* stats);

/* ---- the same two drop-ins without the bulk copies (what include/tex_viewsel.hpp calls) ----
 * mvs_data_costs_stream: tex::calculate_data_costs whose result is handed over in CHUNKS of consecutive faces while the next chunk is
 * still on its way from the device -- the caller's container fill (SparseTable::set_value, calculate_data_costs.cpp:291-298) hides the
 * download.  fn(user, first_face, n_faces, col_ptr, view_id, cost): col_ptr[0 .. n_faces] are ABSOLUTE entry offsets of the faces
 * first_face .. first_face + n_faces - 1, view_id / cost hold the chunk's entries from offset col_ptr[0] on (entry k of the table is
 * view_id[k - col_ptr[0]]); the arrays are valid during the call only.  shape_out (may be NULL) receives n_faces / n_views / nnz (its
 * pointers stay NULL).  The table stays parked on the device with its fingerprint, computed on the device.
 * mvs_view_selection_cached: tex::view_selection on the parked table whose fingerprint the caller computed from ITS container -- no
 * table crosses the bus; MVS_ERR_STATE when no parked table has that fingerprint and shape (the caller then flattens its container
 * and calls mvs_view_selection).  Fingerprint of a table of F faces, V views, n entries (order independent, so it can be summed in
 * pieces):  mvs_fp_mix(F, V) + mvs_fp_mix(n, 1) + sum_{i < F} mvs_fp_mix(i, col_ptr[i + 1])
 *           + sum_{k < n} mvs_fp_mix(2^40 + k, view_id[k] << 32 | bits(cost[k])),   all arithmetic modulo 2^64. */
static inline uint64_t mvs_fp_mix(uint64_t k, uint64_t v) {
    uint64_t x = (k * 0x9E3779B97F4A7C15ull) ^ (v + 0x7F4A7C15D6E8FEB8ull); x ^= x >> 29; x *= 0xBF58476D1CE4E5B9ull; x ^= x >> 32; return x;
}
typedef void (*mvs_csr_chunk_fn)(void* user, uint32_t first_face, uint32_t n_faces, const uint32_t* col_ptr, const uint16_t* view_id, const float* cost);
mvs_status mvs_data_costs_stream(const mvs_mesh* mesh, const mvs_view* views, uint32_t n_views, const mvs_settings* settings,
                                 mvs_csr_chunk_fn fn, void* user, mvs_csr* shape_out, mvs_dc_stats* stats);
/* the same with the host images supplied view by view through an mvs_image_source, see above: host memory is bounded by max_in_flight decoded
 * images instead of the whole scene's -- what the replacement of tex::calculate_data_costs calls (integration/view_selection_mi355x.cpp) */
mvs_status mvs_data_costs_stream_from(const mvs_mesh* mesh, const mvs_view* views, uint32_t n_views, const mvs_image_source* images,
                                      const mvs_settings* settings, mvs_csr_chunk_fn fn, void* user, mvs_csr* shape_out, mvs_dc_stats* stats);
mvs_status mvs_view_selection_cached(uint64_t fingerprint, uint32_t n_faces, uint32_t n_views, uint64_t nnz,
                                     const uint32_t* adj_ptr, const uint32_t* adj, const mvs_mrf_params* params,
                                     uint32_t* labels_out, mvs_mrf_stats* stats);

/* File-level boundary against an UNMODIFIED texrecon (-D / -L flags):
 * SparseTable::save_to_file (sparse_table.h:112-136) and
 * vector_to_file<std::size_t> (util.h:104-113, texrecon.cpp:130-136). */
mvs_status mvs_write_spt(const mvs_csr* csr, const char* path);
mvs_status mvs_read_spt(const char* path, mvs_csr* out);
mvs_status mvs_write_labeling_vec(const uint32_t* labels, uint32_t n_faces, const char* path);

/* ------------------------------------------------------------------------
 * SURVEY.md 8(f) row f1 -- the two stages immediately BEFORE the path (apps/texrecon/texrecon.cpp:78-92)
 * ------------------------------------------------------------------------ */
/* replaces tex::prepare_mesh (libs/tex/texturing.h:45-46, prepare_mesh.cpp:57-70): removes redundant faces
 * (prepare_mesh.cpp:14-55) and computes face normals; faces_out / normals_out hold 3 * n_faces entries.  MVS_ERR_INVALID ("vertex id out of
 * range") when an index in faces is >= n_verts. */
mvs_status mvs_prepare_mesh(uint32_t n_verts, const float* verts, uint32_t n_faces, const uint32_t* faces,
                            uint32_t* faces_out, float* normals_out, uint32_t* n_kept);
/* replaces tex::build_adjacency_graph (texturing.h:58-60, build_adjacency_graph.cpp:16-53): UniGraph adjacency lists
 * flattened in list order; adj_ptr_out[n_faces + 1] caller allocated, *adj_out malloc'ed by the library (free()).  MVS_ERR_INVALID ("vertex id
 * out of range") when an index in faces is >= n_verts.  MVS_ERR_UNSUPPORTED for a face with more than 48 neighbours of smaller id or
 * more than 48 of larger id; in a mesh that has a face with a repeated vertex, for a face with more than 48 neighbours in all or with
 * more than 128 other faces at its vertices. */
mvs_status mvs_build_adjacency_graph(uint32_t n_verts, uint32_t n_faces, const uint32_t* faces,
                                     uint32_t* adj_ptr_out, uint32_t** adj_out, uint64_t* n_entries);

/* ------------------------------------------------------------------------
 * SURVEY.md 8(f) row f3 -- the step immediately AFTER the path: UniGraph::get_subgraphs
 * (libs/tex/uni_graph.cpp:21-55), which generate_texture_patches calls once per label
 * (generate_texture_patches.cpp:469-475).  All labels at once:
 *   subgraphs of label L = components [label_ptr[L], label_ptr[L + 1]), in the reference's order (ascending
 *   smallest face); component c = comp_faces[comp_ptr[c] .. comp_ptr[c + 1]) in the reference's BFS queue order.
 * labels[i] < n_labels (view_selection writes view + 1, 0 = unseen: n_labels = n_views + 1).
 * ------------------------------------------------------------------------ */
typedef struct mvs_subgraphs {
    uint32_t n_faces, n_labels, n_components;
    uint32_t* label_ptr;    /* [n_labels + 1] */
    uint32_t* comp_ptr;     /* [n_components + 1] */
    uint32_t* comp_faces;   /* [n_faces] */
} mvs_subgraphs;
/* host arrays in, library-allocated host arrays out (mvs_subgraphs_free) */
mvs_status mvs_get_subgraphs(uint32_t n_faces, const uint32_t* adj_ptr, const uint32_t* adj, const uint32_t* labels,
                             uint32_t n_labels, mvs_subgraphs* out);
void mvs_subgraphs_free(mvs_subgraphs* sg);

/* ------------------------------------------------------------------------
 * Resident (context) API: inputs live in HBM across calls; used by bench.py,
 * the GPU tests and the multi-GPU driver.  Pointers flagged *_on_device are
 * device pointers owned by the caller (e.g. torch tensors) and must stay
 * alive while the context uses them.
 * ------------------------------------------------------------------------ */
typedef struct mvs_ctx mvs_ctx;

mvs_status mvs_ctx_create(int device, mvs_ctx** out);
void mvs_ctx_destroy(mvs_ctx* ctx);
/* hipStream_t to launch on from now on (NULL = the device's default stream); a fresh context owns a private stream */
mvs_status mvs_ctx_set_stream(mvs_ctx* ctx, void* hip_stream);
mvs_status mvs_ctx_synchronize(mvs_ctx* ctx);
/* integer options (any other name is MVS_ERR_INVALID).  Only "max_labels" changes results; every other option leaves tables, labels and
 * energies bit for bit as they are.
 *   diagnostics:
 *     "stats"                 0/1, default 0: fill the cull-reason counters of mvs_dc_stats; costs atomics
 *     "count_rays"            0/1, default 0: node visits, triangles fetched and leaf rounds of the occlusion rays into mvs_dc_stats
 *     "verbose"               0/1, default 0: progress on stderr
 *     "profile"               0/1, default 0: per-stage GPU times for mvs_ctx_get_profile
 *   the model:
 *     "max_labels"            default 0 = off = the reference's model; 1 .. 65535: label-space compression (CHANGES RESULTS)
 *   data costs:
 *     "dc_range_pairs"        default 0 (environment MVS_DC_RANGE_PAIRS): B > 0: mvs_ctx_data_costs walks the context's faces in consecutive
 *                             ranges of exactly max(1, floor(B / n_views)) faces (the last range holds the rest), keeps what each range
 *                             leaves and takes maximum, histogram and percentile once over all of them: ONE table, bit for bit the
 *                             unranged one, with phase 1's working set bounded by the range.  0 = one range, unless faces x views
 *                             reaches 0xFFFFFFF0: then the fewest equal ranges that stay below it.  Like every option but
 *                             "max_labels" it changes no table, label or energy.  The sharded path ignores it (one range per rank).
 *                             Two 32-bit limits remain whatever the ranges (MVS_ERR_UNSUPPORTED): the qualities ALL ranges keep until the
 *                             percentile is known must number fewer than 0xFFFFFFF0 (the histogram counts its values in one 32-bit word,
 *                             as the reference's int does), and so must the entries of the table that comes out (after "max_labels").
 *                             The kept arrays (6 bytes per kept quality, beside the table) are released when the call returns.
 *                             The environment variable is read when a context is created and again by every one-shot call
 *                             (mvs_data_costs, mvs_data_costs_stream), whose contexts outlive the call.
 *     "info_wave_area"        default 32 (environment MVS_INFO_WAVE_AREA): sampled footprints above this many pixels are summed by a
 *                             16-lane group under an exactness certificate; 0 = every footprint in the reference's serial order
 *     "info_words"            0/1, default 1: the smaller footprints of the gradient term are read four pixels per load and summed as
 *                             integers under the same certificate, by one lane each; 0 = their serial fp64 walk
 *     "info_wave_area_words"  default 384: the "info_wave_area" threshold where "info_words" applies
 *     "info_cert_shift"       default 0: test hook, widens the certificate by this many bits (forces the serial fallback)
 *     "prep_fused"            0/1, default 1: luminance + Sobel in one pass through LDS; 0 = two passes
 *     "face_order"            0/1, default 1: the library lays the faces out along a Hilbert curve; 0 = the caller's face numbering is kept
 *     "bvh_window"            default 262144: upper levels of the face order are cut exactly inside aligned windows of this many faces
 *                             (rounded up to a power of two); 0 = the whole mesh, 1 = no upper-level cuts
 *     "bvh_upper_min_faces"   default 1000000 (environment MVS_BVH_UPPER_MIN_FACES): smaller meshes keep the curve order above the window
 *     "ray_xcd"               0/1, default 1: XCD-aware block order of the occlusion-ray kernel
 *   solver:
 *     "mrf_lag"               default 1: sweeps the host queues ahead of the energy reports it reads
 *     "mrf_graph"             0/1, default 1: the sweep loop is replayed from a hipGraph; 0 = direct launches
 *     "mrf_xcd"               0/1, default 1: XCD-aware block order of the sweep kernels
 *     "mrf_blocks_per_cu"     default 0 = at most as many blocks per fast sweep launch as are resident; n > 0: at most 256 n
 *     "mrf_force_generic"     0/1, default 0: test hook, every node takes the generic sweep kernel
 *     "mrf_force_lists"       0/1, default 0: test hook, the solver's set-up works from the neighbours' view lists instead of view-set bitmaps
 *   (the sharded sweep loop's transport is no option: the communicator decides it, see mvs_shard_transport_info) */
mvs_status mvs_set_option(mvs_ctx* ctx, const char* name, int64_t value);

/* with option "profile": per-stage GPU time from hipEvents recorded on the context's stream,
 * as a JSON object {"stage": [total_ms, launches], ...}; clears the record */
mvs_status mvs_ctx_get_profile(mvs_ctx* ctx, char* buf, size_t buf_size);

mvs_status mvs_scene_set_mesh(mvs_ctx* ctx, const mvs_mesh* mesh, int on_device);
/* views: HOST array of n structs; their rgb pointers are device pointers iff rgb_on_device.
 * ONE rule for every view input (mvs_scene_set_views, _from, _jpeg, _lens): a refused call leaves the context WITHOUT views, whatever it
 * held before and however many views the call brought -- until a view input succeeds mvs_ctx_data_costs is MVS_ERR_STATE (not the empty
 * table of a successful call with zero views), and so are mvs_scene_set_view_masks and the read-back of a view's image. */
mvs_status mvs_scene_set_views(mvs_ctx* ctx, const mvs_view* views, uint32_t n_views, int rgb_on_device);
/* host images supplied view by view -- an mvs_image_source; mvs_view.rgb is ignored */
mvs_status mvs_scene_set_views_from(mvs_ctx* ctx, const mvs_view* views, uint32_t n_views, const mvs_image_source* images);
/* restrict the data-cost computation to the faces at POSITIONS [begin, end) of the library's face order (the caller's ids with
 * option "face_order" = 0); the whole mesh stays the occluder set.  Default: all faces.  (Building block of the sharded drivers.) */
mvs_status mvs_scene_set_face_range(mvs_ctx* ctx, uint32_t begin, uint32_t end);

/* tex::calculate_data_costs on the resident scene; result stays on the device.  The (face, view) pairs that pass the culls are ranked
 * in 32 bits per range of faces: a scene of 2^32 pairs and more is walked in ranges (option "dc_range_pairs").  What has to fit 32 bits
 * then is the number of qualities that survive the culls in all ranges together (the histogram's count word) and the table that comes out
 * (its column pointers; see "max_labels") -- a scene beyond either is MVS_ERR_UNSUPPORTED. */
mvs_status mvs_ctx_data_costs(mvs_ctx* ctx, const mvs_settings* settings, mvs_dc_stats* stats);
/* What the last data-cost pass of the context did: the number of face ranges it walked and the faces of its FIRST range (every range
 * but the last has that many).  An unranged pass, a phase-wise pass and mvs_postprocess_face_infos report (1, faces of the pass); so does
 * a pass with nothing to evaluate -- an empty mesh reports (1, 0), a scene without views (1, faces).  Either pointer may be NULL.
 * MVS_ERR_STATE before the first pass. */
mvs_status mvs_ctx_dc_ranges(mvs_ctx* ctx, uint32_t* n_ranges, uint32_t* range_faces);
/* The same, split at the global barrier of postprocess_face_infos
 * (calculate_data_costs.cpp:278-288): csrc/shard.hip all-reduces the maximum quality and the
 * 10000-bin histogram between the phases (a driver of its own reaches the two buffers through
 * include/mvs_viewsel_blocks.h):
 *   phase1: everything up to the per-face sorted infos + local max quality
 *   phase2: histogram of local qualities against the (global) max
 *   phase3: percentile from the (globally summed) histogram + cost write   */
mvs_status mvs_ctx_dc_phase1(mvs_ctx* ctx, const mvs_settings* settings);
mvs_status mvs_ctx_dc_phase2(mvs_ctx* ctx);
/* the histogram travels as MVS_HIST_WORDS u32 = 10000 bins + [10000] = number of values */
#define MVS_HIST_WORDS 10001
mvs_status mvs_ctx_dc_phase3(mvs_ctx* ctx, mvs_dc_stats* stats);

/* device-resident result of the last data-cost call AS THE LIBRARY KEEPS IT: column p is the face at position p of the library's
 * own face order (see "Face order" below; mvs_ctx_table_order gives the caller's id of every column), for a face range the faces
 * of the range with local indices.  mvs_ctx_costs_download returns the caller's numbering. */
mvs_status mvs_ctx_costs_device(mvs_ctx* ctx, mvs_csr* device_view);
/* *ordered = 1: the active table lives in the library's own order and perm_device[p] (caller-owned DEVICE array of n_faces words, may
 * be NULL) receives the caller's face id of column p -- for the table of a face range (mvs_scene_set_face_range: end - begin columns,
 * the positions [begin, end) of the order) that many words; *ordered = 0: the table is in the caller's order (uploaded tables,
 * option "face_order" = 0), nothing is written */
mvs_status mvs_ctx_table_order(mvs_ctx* ctx, uint32_t* perm_device, int* ordered);
/* copy it to freshly malloc'ed host arrays (release with mvs_csr_free); with
 * quality_out != NULL also returns the un-normalised qualities (malloc'ed, nnz floats).  The table of the whole mesh leaves in the
 * caller's numbering; the table of a face range leaves as it is: column k = the face at position begin + k of the library's order,
 * i.e. the caller's face perm[begin + k] (mvs_ctx_table_order / mvs_ctx_partition_faces). */
mvs_status mvs_ctx_costs_download(mvs_ctx* ctx, mvs_csr* host_out, float** quality_out);
/* replace the resident costs by caller-provided ones (host or device pointers) */
mvs_status mvs_ctx_costs_upload(mvs_ctx* ctx, const mvs_csr* csr, int on_device);

/* ------------------------------------------------------------------------
 * Face order and partition.  The reference hands the path its faces in mesh-file order (calculate_data_costs.cpp:136-138,
 * texrecon.cpp:73-92); the library assumes nothing about that order.  Every data-cost pass first lays the resident mesh out along
 * a Hilbert curve on the device (faces by centroid, vertices by position; csrc/k_bvh.hip build_scene_order) and works on that
 * copy: culls, rays, footprints, the cost table, the solver's node order and the parts of the sharded path all follow it.
 * Inputs and outputs keep the caller's numbering: adjacency lists are renumbered on entry (list order kept), the colouring of the
 * solver is keyed on the caller's ids, labels and downloaded tables come back at the caller's face ids -- results are
 * bit-identical whatever order the mesh arrives in.  mvs_set_option("face_order", 0) keeps the caller's face numbering as the
 * internal order (a caller that laid the faces out itself).
 *
 * mvs_ctx_partition_faces: the order of the resident mesh -- perm_device[p] (device, n_faces words, may be NULL) = the caller's
 * id of the face at position p -- and its cut part_begin[0 .. world] (host, may be NULL) into `world` contiguous parts of equal
 * size: the partition of the sharded path below (METIS is not available; a contiguous range of a Hilbert order is
 * a compact patch).  mvs_partition_faces: the same for host arrays (mesh->face_normals may be NULL); device = env MVS_DEVICE.
 * ------------------------------------------------------------------------ */
mvs_status mvs_ctx_partition_faces(mvs_ctx* ctx, int world, uint32_t* perm_device, uint32_t* part_begin);
mvs_status mvs_partition_faces(const mvs_mesh* mesh, int world, uint32_t* perm_out /* [n_faces] */, uint32_t* part_begin_out /* [world + 1] */);

/* tex::build_adjacency_graph on the resident mesh; the result stays on the device (pointers returned) */
mvs_status mvs_ctx_build_adjacency(mvs_ctx* ctx, uint32_t** adj_ptr_device, uint32_t** adj_device, uint64_t* n_entries);

/* tex::view_selection on the resident costs.  adjacency: host or device pointers.
 * labels_out (n_faces u32) may be a host or a device pointer (labels_on_device). */
mvs_status mvs_ctx_view_selection(mvs_ctx* ctx, const uint32_t* adj_ptr, const uint32_t* adj,
                                  int adj_on_device, const mvs_mrf_params* params,
                                  uint32_t* labels_out, int labels_on_device, mvs_mrf_stats* stats);

/* solver progress as tracked on the device (mvs_ctx_mrf_step) */
typedef struct mvs_mrf_progress {
    uint32_t sweep;        /* sweeps accounted so far (stops counting once `stopped`) */
    uint32_t stopped;      /* the stop rule has fired (or max_sweeps reached) */
    uint32_t improved;     /* the last accounted sweep lowered the best energy */
    uint32_t stop_sweep;   /* sweep at which the rule fired = mvs_mrf_stats.sweeps */
    uint64_t energy;       /* TRACKING energy of the last accounted sweep: the energy under the 16-bit unaries the sweeps see, an
                              integer in units of 1 / 65535 (sum of cost codes + 65535 per cut edge).  It drives the stop rule and the
                              choice of the best sweep; mvs_mrf_stats reports the exact 32.32 fixed-point energy of the result */
    uint64_t best;         /* best tracking energy so far */
    uint32_t w;            /* decode buffer (0 / 1) the NEXT sweep writes */
    uint32_t best_w;       /* decode buffer holding the best labeling so far: "keep the best" flips the two indices, nothing is copied */
} mvs_mrf_progress;

/* message element index of the first real run: elements [0, MVS_MRF_MSG_BASE) of the solver's message array are a reserved all-zero
 * run (k_mrf_setup.hip): halo index lists start from here */
#define MVS_MRF_MSG_BASE 256u
/* The sweep is colour-phased Gauss-Seidel: the adjacency graph is coloured at set-up (n_phases colours, each an independent set) and
 * one sweep = for phase in 0 .. n_phases - 1: the nodes of that colour recompute their outgoing messages in place. */
mvs_status mvs_ctx_mrf_num_phases(mvs_ctx* ctx, uint32_t* n_phases);
/* diagnostics of the last mvs_ctx_view_selection calls of this context: out[0] = hipGraph launches of the sweep loop (four sweeps each;
 * option "mrf_graph", default 1), out[1] = re-captures pushed into the executable graph with hipGraphExecUpdate, out[2] = graph
 * instantiations, out[3] = nodes the sweep routes to the generic kernel (degree > 3 or a column of > 255 labels at or next to the node) */
mvs_status mvs_ctx_mrf_diagnostics(mvs_ctx* ctx, uint32_t out[4]);
/* The sharded path -- the product's only multi-GPU driver -- is mvs_comm_* / mvs_shard_* below (csrc/shard.hip).  The per-phase
 * BUILDING BLOCKS a driver of its own would be made of (sweep one colour phase of a node range, gather / scatter halo elements,
 * step, poll, ICM gain / apply, ...) are declared in include/mvs_viewsel_blocks.h and live in a library of their own,
 * libmvs_blocks.so: the harness of the CPU multi-process tests (tests/tools/multigpu.py) is built on them. */


/* row f3 on a context: inputs host or device (flags); with out_on_device the three arrays of `out` are device
 * pointers owned by the context (valid until its next get_subgraphs call), otherwise malloc'ed host copies */
mvs_status mvs_ctx_get_subgraphs(mvs_ctx* ctx, uint32_t n_faces, const uint32_t* adj_ptr, const uint32_t* adj, int adj_on_device,
                                 const uint32_t* labels, int labels_on_device, uint32_t n_labels, mvs_subgraphs* out,
                                 int out_on_device);

/* Tone mapping (tex::Settings::tone_mapping, settings.h): the field `tone_mapping` of mvs_gsl_params, mvs_patch_params and mvs_atlas_params.
 * MVS_TONE_NONE (the default of every *_default_params) is `texrecon -t none`; MVS_TONE_GAMMA is `-t gamma`: a view's pixel value is
 * gamma_pow(byte / 255.0f, 2.2f) wherever rows f5, f6 and f10 read one -- the crop's fill (255, 0, 255) included
 * (generate_texture_patches.cpp:126-132: everything global and local seam leveling see is linearised) -- and row f8 applies
 * gamma_pow(v, 1.0f / 2.2f) to every channel value in front of float_to_byte (generate_texture_atlases.cpp:102-104).  Any other
 * value: MVS_ERR_INVALID, the context stays usable.  gamma_pow is csrc/tone.h -- one text for host and device, the same bits on both
 * (DESIGN.md section 4 "Tone mapping").
 * mvs_gamma_correct: values[i] = gamma_pow(values[i], power) on n host floats, in place; needs no GPU.  mvs_ctx_gamma_correct: the same
 * by a kernel on the context's stream, values on the host or on the device -- the same bits.  power must be finite and > 0
 * (MVS_ERR_INVALID otherwise).  mvs_tone_table: the 256 values of a view's bytes under `mode`. */
enum { MVS_TONE_NONE = 0, MVS_TONE_GAMMA = 1 };
mvs_status mvs_gamma_correct(float* values, uint64_t n, float power);
mvs_status mvs_ctx_gamma_correct(mvs_ctx* ctx, float* values, uint64_t n, float power, int on_device);
mvs_status mvs_tone_table(uint32_t mode, float out[256]);

/* Row f5: tex::global_seam_leveling (libs/tex/global_seam_leveling.cpp), tone mapping as params->tone_mapping says, from the caller's labels
 * (0 = unseen, L = view L - 1) on the context's mesh and views; no data-cost pass is needed.  adj_ptr / adj: the face adjacency
 * of mvs_ctx_get_subgraphs.  The definition -- the vertex rows, the patches generate_texture_patches would make, the seam samples,
 * the normal equations and their Jacobi-preconditioned CG -- is DESIGN.md section 4 "Global seam leveling"; every output is the
 * same bits on any device.  Everything is keyed on the caller's face and vertex ids:
 *   x_ptr[v] .. x_ptr[v + 1]: the unknowns (x rows) of vertex v, one per distinct non-zero label of its faces, labels ascending
 *   (x_label); x_adjust[3 row + c]: the adjustment of that (vertex, label) in channel c, mean removed;
 *   corner_adjust[9 f + 3 k + c]: the adjustment of corner k of face f (zeros for label 0) -- upstream's patch_adjust_values
 *   (global_seam_leveling.cpp:300-318), face by face.
 * MVS_ERR_LABELING when a label exceeds the number of views or a labelled face's box leaves its view's image (the asserts of
 * generate_candidate); MVS_ERR_STATE without mesh or views.  With out_on_device the four arrays are device pointers owned by
 * the context (valid until its next call), otherwise malloc'ed host copies (mvs_gsl_result_free). */
typedef struct mvs_gsl_params {
    float tolerance;          /* CG tolerance (1e-4) */
    uint32_t max_iterations;  /* per channel (1000) */
    float lambda;             /* weight of the smoothness rows Gamma (0.1) */
    uint32_t tone_mapping;    /* MVS_TONE_NONE (default) or MVS_TONE_GAMMA: the seam samples read linearised texels */
} mvs_gsl_params;
void mvs_gsl_default_params(mvs_gsl_params* p);
typedef struct mvs_gsl_result {
    uint32_t n_verts, n_faces, x_rows, reserved;
    uint32_t* x_ptr;          /* [n_verts + 1] */
    uint32_t* x_label;        /* [x_rows] */
    float* x_adjust;          /* [3 x_rows] */
    float* corner_adjust;     /* [9 n_faces] */
} mvs_gsl_result;
typedef struct mvs_gsl_stats {
    uint64_t patches, merged;          /* texture patches; candidates absorbed by another of their label */
    uint64_t x_rows, a_rows, gamma_rows, lhs_nnz_lower;
    uint64_t seam_edges, samples;      /* seam-edge entries of all A rows; bilinear samples taken */
    uint32_t iterations[3];            /* CG iterations per channel (the breaking iteration not counted) */
    float error[3];                    /* sqrt(|r|^2 / |Rhs|^2) per channel */
    float ms_rows, ms_patches, ms_system, ms_solve, ms_output, ms_total;   /* device time per phase */
} mvs_gsl_stats;
mvs_status mvs_ctx_global_seam_leveling(mvs_ctx* ctx, const uint32_t* adj_ptr, const uint32_t* adj, int adj_on_device,
                                        const uint32_t* labels, int labels_on_device, const mvs_gsl_params* params,
                                        mvs_gsl_result* out, int out_on_device, mvs_gsl_stats* stats);
void mvs_gsl_result_free(mvs_gsl_result* r);
/* host copies of the last call's system (tests): Lhs as its lower triangle (CSR, columns ascending), Rhs [3 x_rows], the A rows
 * (x rows a_col[2 r] with +1, a_col[2 r + 1] with -1) and b [3 a_rows], x before the mean [3 x_rows]; mvs_gsl_system_free */
typedef struct mvs_gsl_system {
    uint32_t x_rows, a_rows;
    uint64_t lhs_nnz;
    uint32_t* lhs_ptr; uint32_t* lhs_col; float* lhs_val;
    float* rhs; uint32_t* a_col; float* b; float* x_raw;
} mvs_gsl_system;
mvs_status mvs_ctx_gsl_system(mvs_ctx* ctx, mvs_gsl_system* out);
void mvs_gsl_system_free(mvs_gsl_system* s);

/* Row f6: generate_texture_patches for the labelled faces (generate_texture_patches.cpp:78-138, :484-508) followed by
 * TexturePatch::adjust_colors (texture_patch.cpp:41-122) on every patch, tone mapping as params->tone_mapping says: from the caller's labels and the
 * per-corner adjustments of row f5 (corner_adjust[9 f + 3 k + c]; NULL = zeros, upstream's branch without global seam leveling,
 * texrecon.cpp:173-184) to the packed patch images and masks.  The definition is DESIGN.md section 4 "Texture patches"; every
 * array is the same bits on any device and in every run.  The call stands alone: it needs the mesh and the views, no data-cost
 * pass and no previous mvs_ctx_global_seam_leveling.  Patch p (ids in label order, as row f5 numbers them):
 *   label[p]; box[4 p ..] = min_x, min_y, width, height of its frame in the view's pixels (one pixel of border, so min may be -1);
 *   faces[face_ptr[p] .. face_ptr[p + 1]): its face list in upstream's order (the surviving candidate's faces, then the absorbed
 *   lists); texcoords[6 e + 2 k ..]: corner k of list entry e in the patch's pixels;
 *   pixels [pix_ptr[p], pix_ptr[p + 1]): the patch row-major, patches back to back: image[3 i + c] (float, interleaved RGB),
 *   validity[i] in {0, 255}, blending[i] in {0, 64, 255}.
 * params.max_pixels (0 = no cap): when the pixel total exceeds it the call fails with MVS_ERR_UNSUPPORTED before the pixel arrays
 * are allocated; stats (patches, merged, listed_faces, pixels) is filled all the same.  MVS_ERR_LABELING / MVS_ERR_STATE as row f5.
 * With out_on_device the arrays are device pointers owned by the context (valid until its next texture_patches or debug_patches
 * call or its destruction), otherwise malloc'ed host copies (mvs_patch_set_free). */
typedef struct mvs_patch_params {
    uint64_t max_pixels;      /* refuse a result of more pixels than this (0: no cap) */
    uint32_t tone_mapping;    /* MVS_TONE_NONE (default) or MVS_TONE_GAMMA: the crop is linearised before adjust_colors */
    uint32_t reserved;
} mvs_patch_params;
void mvs_patch_default_params(mvs_patch_params* p);
typedef struct mvs_patch_set {
    uint32_t n_patches, n_listed;   /* n_listed = face_ptr[n_patches]: the labelled faces */
    uint64_t n_pixels;              /* pix_ptr[n_patches] */
    uint32_t* label;          /* [n_patches] */
    int32_t* box;             /* [4 n_patches] */
    uint32_t* face_ptr;       /* [n_patches + 1] */
    uint32_t* faces;          /* [n_listed] */
    float* texcoords;         /* [6 n_listed] */
    uint64_t* pix_ptr;        /* [n_patches + 1] */
    float* image;             /* [3 n_pixels] */
    uint8_t* validity;        /* [n_pixels] */
    uint8_t* blending;        /* [n_pixels] */
} mvs_patch_set;
typedef struct mvs_patch_stats {
    uint64_t patches, merged;             /* as mvs_gsl_stats */
    uint64_t listed_faces, degenerate_faces;   /* list entries; those adjust_colors skips (area < FLT_EPSILON) */
    uint64_t pixels, valid_pixels, near_pixels;   /* all; validity 255; blending 64 */
    float ms_tables, ms_lists, ms_mark, ms_resolve, ms_total;   /* device time: patch tables; geometry, lists and scans; mark; resolve */
    float reserved;
} mvs_patch_stats;
mvs_status mvs_ctx_texture_patches(mvs_ctx* ctx, const uint32_t* adj_ptr, const uint32_t* adj, int adj_on_device,
                                   const uint32_t* labels, int labels_on_device, const float* corner_adjust, int adjust_on_device,
                                   const mvs_patch_params* params, mvs_patch_set* out, int out_on_device, mvs_patch_stats* stats);
void mvs_patch_set_free(mvs_patch_set* s);

/* Row f7: tex::local_seam_leveling (local_seam_leveling.cpp:105-204) on a patch set as mvs_patch_set describes it (the tone mapping
 * is not read: the row works on the patch images it is given), labelled faces only: seam-edge and seam-vertex colours (the mean over the patches that meet there) are written into every
 * patch, prepare_blending_mask(strip_width) fixes everything but a strip along the patch border, and the strip is re-solved as a
 * Poisson problem that keeps the original image's Laplacian (poisson_blend with alpha 1); pixels of mask 64 lose their validity.
 * The definition is DESIGN.md section 4 "Local seam leveling"; upstream's direct solve is replaced by conjugate gradients per patch
 * (one fixed reduction tree per unknown count: every output is the same bits on any device, in every run, whatever else is in the
 * set).  Needs the mesh, not the views.  `patches` may be the device output of mvs_ctx_texture_patches (patches_on_device: ALL its
 * arrays are device pointers) or host arrays; it is not modified.  Output: image [3 n_pixels], validity [n_pixels] and the PREPARED
 * blending mask [n_pixels] (0 inner / outside, 64 and 128 fixed, 255 strip), packed as the input (pix_ptr); with out_on_device
 * device pointers owned by the context (valid until its next local_seam_leveling call), otherwise malloc'ed (mvs_lsl_result_free).
 * params.max_iterations = 0 returns the state before the solve.  MVS_ERR_LABELING when a listed face's label differs from its
 * patch's or a face id is out of range; MVS_ERR_STATE without a mesh; MVS_ERR_UNSUPPORTED for a patch of label 0, texture
 * coordinates that are not finite or beyond 2^20, or totals that would wrap 32 bits (pixels, samples, keys). */
typedef struct mvs_lsl_params {
    float tolerance;          /* CG stops at sqrt(|r|^2 / |b|^2) < tolerance, per patch and channel (1e-6) */
    uint32_t max_iterations;  /* per patch and channel (700); 0: no solve */
    uint32_t strip_width;     /* prepare_blending_mask's argument (20; at most 250) */
    uint32_t lds_bytes;       /* a patch whose solver image (12 B per pixel + 16 B per unknown) exceeds this takes the global-memory
                                 path (147456 = the default and the most; 0: every patch) -- same arithmetic, same bits */
} mvs_lsl_params;
void mvs_lsl_default_params(mvs_lsl_params* p);
typedef struct mvs_lsl_result {
    uint32_t n_patches, reserved;
    uint64_t n_pixels;
    float* image;             /* [3 n_pixels] */
    uint8_t* validity;        /* [n_pixels] */
    uint8_t* blending;        /* [n_pixels] */
} mvs_lsl_result;
typedef struct mvs_lsl_stats {
    uint64_t seam_edges, skipped_pairs;          /* seam edges listed; adjacent pairs of different labels that do not share exactly two vertices */
    uint64_t vertex_infos, edge_projections;     /* (vertex, patch) infos; (seam edge, patch) projections = lines */
    uint64_t colour_samples, invalid_samples;    /* bilinear samples taken (edges and vertices); those upstream's valid_pixel would refuse */
    uint64_t vertex_writes, line_writes;         /* pixel writes attempted by vertices / by lines */
    uint64_t written_pixels, outside_frame, invalid_writes;   /* distinct pixels written; writes dropped outside the frame; writes onto validity 0 */
    uint64_t strip_pixels, fixed_pixels, demoted;             /* unknowns; pixels of mask 64 / 128; 255s without four usable neighbours, held fixed */
    uint64_t patches_lds, patches_global, pixels_global;      /* patches solved in LDS / in global memory (patches without unknowns in neither); pixels of the latter */
    uint64_t iterations_total, hit_max_iterations;            /* over patches and channels; patches with a channel that ran into max_iterations */
    uint32_t iterations_max; float error_max;                 /* over patches and channels; error = sqrt(|r|^2 / |b|^2) */
    float ms_topology, ms_colours, ms_writes, ms_mask, ms_solve, ms_total;   /* device time per phase */
} mvs_lsl_stats;
mvs_status mvs_ctx_local_seam_leveling(mvs_ctx* ctx, const uint32_t* adj_ptr, const uint32_t* adj, int adj_on_device,
                                       const uint32_t* labels, int labels_on_device, const mvs_patch_set* patches, int patches_on_device,
                                       const mvs_lsl_params* params, mvs_lsl_result* out, int out_on_device, mvs_lsl_stats* stats);
void mvs_lsl_result_free(mvs_lsl_result* r);

/* Row f8: tex::generate_texture_atlases (generate_texture_atlases.cpp:35-166, texture_atlas.cpp, rectangular_bin.cpp) on a patch set
 * as mvs_patch_set describes it (row f7's image and validity merged over row f6's set; `label` and `blending` are not read), tone
 * mapping as params->tone_mapping says: the patches are ordered and packed into square atlases (256 .. 8192, padding = size >> 7), their pixels quantised
 * (float_to_byte_image) and copied with their validity, every atlas dilated by apply_edge_padding, the texture coordinates moved into
 * the atlas and merged.  The definition is DESIGN.md section 4 "Texture atlases"; every array is the same bits on any device and in
 * every run.  Needs neither mesh nor views; `patches` is all host arrays or all device pointers (patches_on_device) and is not
 * modified.  For A = n_atlases, in upstream's creation order:
 *   atlas_size[a]; atlas a's pixels are image[3 atlas_pix_ptr[a] ..) (uint8, interleaved RGB, row-major, after the edge padding);
 *   patch_atlas[p], patch_pos[2 p ..] = rect.min_x, rect.min_y (the patch's pixel (0, 0) lies `padding` further in both directions);
 *   patch_order: the patches in insertion order (grouped by atlas); faces[face_ptr[a] .. face_ptr[a + 1]): atlas a's faces (patches in
 *   insertion order, list order within a patch), texcoords[6 e + 2 k ..]: corner k of entry e before the merge;
 *   texcoords_merged[2 (tc_ptr[a] + i) ..]: coordinate i of atlas a, texcoord_ids[3 e + k]: its id within the atlas.
 * params.max_pixels (0 = no cap): when the atlases' pixel total exceeds it the call fails with MVS_ERR_UNSUPPORTED before the pixel
 * arrays are allocated; stats (atlases, pixels, free_rects_peak) is filled all the same.  MVS_ERR_UNSUPPORTED as well for a patch with
 * width + 128 >= 8192 or height + 128 >= 8192 (upstream asserts) and for a texture coordinate that is not finite once it is in the atlas.
 * The packing itself runs on the host inside the call.  With
 * out_on_device the arrays are device pointers owned by the context (valid until its next texture_atlases call or its destruction),
 * otherwise malloc'ed host copies (mvs_atlas_set_free). */
typedef struct mvs_atlas_params {
    uint64_t max_pixels;      /* refuse a result of more atlas pixels than this (0: no cap) */
    uint32_t tone_mapping;    /* MVS_TONE_NONE (default) or MVS_TONE_GAMMA: gamma_pow(v, 1.0f / 2.2f) in front of float_to_byte */
    uint32_t reserved;
} mvs_atlas_params;
void mvs_atlas_default_params(mvs_atlas_params* p);
typedef struct mvs_atlas_set {
    uint32_t n_atlases, n_patches, n_listed, n_merged;   /* n_merged = tc_ptr[n_atlases] */
    uint64_t n_pixels;              /* atlas_pix_ptr[n_atlases] */
    uint32_t* atlas_size;           /* [n_atlases] */
    uint64_t* atlas_pix_ptr;        /* [n_atlases + 1] */
    uint8_t* image;                 /* [3 n_pixels] */
    uint32_t* patch_atlas;          /* [n_patches] */
    int32_t* patch_pos;             /* [2 n_patches] */
    uint32_t* patch_order;          /* [n_patches] */
    uint32_t* face_ptr;             /* [n_atlases + 1] */
    uint32_t* faces;                /* [n_listed] */
    float* texcoords;               /* [6 n_listed] */
    uint32_t* tc_ptr;               /* [n_atlases + 1] */
    float* texcoords_merged;        /* [2 n_merged] */
    uint32_t* texcoord_ids;         /* [3 n_listed] */
} mvs_atlas_set;
typedef struct mvs_atlas_stats {
    uint64_t atlases, atlases_by_size[6];          /* all; of side 256, 512, 1024, 2048, 4096, 8192 */
    uint64_t pixels, valid_pixels, padded_pixels;  /* atlas pixels; validity 255 before the padding; filled by the padding */
    uint64_t free_rects_peak, merged_texcoords;    /* longest free list of a bin; texcoords after the merge */
    float ms_pack, ms_compose, ms_pad, ms_texcoords, ms_total;   /* ms_pack: HOST time (ordering, packing, per-patch tables and their uploads); device time: clear, quantise and scatter; sweeps; coordinates and merge; ms_total: the sum of the four */
    float reserved;
} mvs_atlas_stats;
mvs_status mvs_ctx_texture_atlases(mvs_ctx* ctx, const mvs_patch_set* patches, int patches_on_device, const mvs_atlas_params* params,
                                   mvs_atlas_set* out, int out_on_device, mvs_atlas_stats* stats);
void mvs_atlas_set_free(mvs_atlas_set* a);

/* Row f9: tex::build_model (build_obj_model.cpp:18-80), ObjModel::save (obj_model.cpp:23-71) and MaterialLib::save_to_files
 * (material_lib.cpp:20-46) on the context's mesh and an atlas set as mvs_atlas_set describes it: the text of `<name>.obj` and
 * `<name>.mtl`, byte for byte what upstream's writers produce, formatted on the device (csrc/k_model.hip; the definition is DESIGN.md
 * section 4 "Model output"; the same bytes on any device and in every run).  Of `atlases` only n_atlases, n_listed, n_merged, face_ptr,
 * faces, tc_ptr, texcoords_merged and texcoord_ids are read by mvs_ctx_build_model (image and atlas_size may be NULL there);
 * mvs_ctx_save_model reads atlas_size, atlas_pix_ptr and image as well.  `atlases` is all host arrays or all device pointers
 * (atlases_on_device) and is not modified.  vertex_normals: [3 n_verts] floats on the host or the device (normals_on_device), or NULL:
 * then the `vn` lines are left out and the faces are written V/T instead of V/T/V.  `name` (at most 255 bytes) is what the `mtllib` and
 * `map_Kd` lines carry; mvs_ctx_save_model takes the part of `prefix` after the last '/'.
 *   obj [obj_bytes], mtl [mtl_bytes]: the text, not NUL-terminated.  The .obj has n_atlases + 4 sections -- the mtllib line, the v, vt and
 *   vn lines, then one group per atlas (its usemtl line and its faces): section i is lines section_ptr[i] .. section_ptr[i + 1] and bytes
 *   section_bytes[i] .. section_bytes[i + 1] (both [n_atlases + 5], host arrays in either mode).
 * MVS_ERR_STATE without a mesh; MVS_ERR_INVALID for a face id >= n_faces, a texcoord id outside its atlas's range, a face_ptr / tc_ptr
 * that does not run from 0 to the totals, or a name that is too long; params.max_bytes (0 = no cap): when the .obj text exceeds it the
 * call fails with MVS_ERR_UNSUPPORTED after the measuring pass, with stats filled.  With out_on_device obj and mtl are device pointers
 * and the section arrays host arrays owned by the context (valid until its next build_model / save_model call or its destruction),
 * otherwise everything is malloc'ed (mvs_model_text_free).
 * mvs_ctx_save_model writes `<prefix>.obj`, `<prefix>.mtl` and per atlas `<prefix>_material<a>_map_Kd.png` (<a> zero-filled to four
 * characters): the text comes through a pinned buffer, the PNGs are written by up to 16 host threads.  PNG: 8-bit RGB, one IDAT.
 *   params.png_device 0 (default): the pixels are copied to the host and encoded there with filter 0 on every row; params.png_level 0
 *   (default) = stored deflate blocks, no dependency; 1 .. 9 = libz.so.1 resolved at run time, MVS_ERR_UNSUPPORTED where it is absent.
 *   mvs_write_png is that encoder on a host image (rgb [height][width][3]).
 *   params.png_device 1: the atlases are encoded on the device (mvs_ctx_encode_pngs below: per-row filters, run-length matches and a
 *   dynamic Huffman block per 32 KiB chunk) and only the finished files are downloaded; needs no libz; png_level must be 0.  Any other
 *   png_device, or png_device 1 with png_level != 0, is MVS_ERR_INVALID.  stats.ms_png covers whichever route ran.
 *   params.image_format 1: the atlases become baseline JPEGs, encoded on the device (mvs_ctx_encode_jpegs below) with jpeg_quality
 *   1 .. 100 and jpeg_subsampling 0 (4:4:4) / 1 (4:2:0): the files are `<prefix>_material<a>_map_Kd.jpg` and the `map_Kd` lines of the
 *   .mtl name them (the one change in the text); png_level and png_device must be 0.  MVS_ERR_INVALID for any other image_format, a
 *   quality or subsampling outside those values, or a non-zero png_level / png_device beside image_format 1; MVS_ERR_UNSUPPORTED for an
 *   atlas side above 65535.  With image_format 0 jpeg_quality and jpeg_subsampling are not read, and glb_quantize is read by row f11 alone: a zeroed struct is the PNG
 *   route with stored blocks, as before.  stats.ms_png stays the one field for whichever encoder ran.
 *   The struct grew from 16 to 32 bytes with image_format: callers compiled against the 16-byte struct must be recompiled. */
typedef struct mvs_model_params {
    uint64_t max_bytes;       /* refuse an .obj of more bytes than this (0: no cap) */
    int32_t png_level;        /* 0 .. 9 */
    int32_t png_device;       /* 0: the PNGs are encoded on the host (png_level); 1: on the device */
    int32_t image_format;     /* 0: PNG (default); 1: JPEG */
    int32_t jpeg_quality;     /* 1 .. 100 (default 90); read under image_format 1 only */
    int32_t jpeg_subsampling; /* 0: 4:4:4; 1: 4:2:0 (default); read under image_format 1 only */
    int32_t glb_quantize;     /* row f11 only: 0 (default): float32 attributes, 32-bit indices; 1: KHR_mesh_quantization (below) */
} mvs_model_params;
void mvs_model_default_params(mvs_model_params* p);
typedef struct mvs_model_text {
    uint32_t n_atlases, reserved;
    uint64_t obj_bytes, mtl_bytes;
    char* obj;                      /* [obj_bytes] */
    char* mtl;                      /* [mtl_bytes] */
    uint64_t* section_ptr;          /* [n_atlases + 5] lines */
    uint64_t* section_bytes;        /* [n_atlases + 5] bytes */
} mvs_model_text;
typedef struct mvs_model_stats {
    uint64_t lines[5], bytes[5];                 /* of the .obj: mtllib line, v, vt, vn, all groups */
    uint64_t mtl_bytes;
    uint64_t wide_values, nonfinite_values;      /* floats of magnitude >= 2^64 (the multi-word route); inf / nan */
    float ms_measure, ms_scan, ms_write;         /* device time per phase */
    float ms_download, ms_files, ms_png;         /* host time of save_model: text to the host, the two text files, the PNGs (copy, encode, write) */
} mvs_model_stats;
mvs_status mvs_ctx_build_model(mvs_ctx* ctx, const mvs_atlas_set* atlases, int atlases_on_device, const float* vertex_normals, int normals_on_device,
                               const char* name, const mvs_model_params* params, mvs_model_text* out, int out_on_device, mvs_model_stats* stats);
mvs_status mvs_ctx_save_model(mvs_ctx* ctx, const mvs_atlas_set* atlases, int atlases_on_device, const float* vertex_normals, int normals_on_device,
                              const char* prefix, const mvs_model_params* params, mvs_model_stats* stats);
void mvs_model_text_free(mvs_model_text* t);
mvs_status mvs_write_png(const char* path, const uint8_t* rgb, uint32_t width, uint32_t height, int32_t level);

/* Row f9's compressed PNG route (DESIGN.md section 4 "Model output" item 7 defines the format; pixel parity with any PNG reader): every
 * row takes the PNG filter 0 .. 4 whose residuals have the smallest sum of absolute values, the filtered stream is cut into independent
 * chunks of 32768 bytes, and every chunk is one dynamic-Huffman block of literals and distance-1 matches (or a stored block where that
 * is no shorter) behind an empty stored block.
 * mvs_ctx_encode_pngs: the complete PNG files of n_images 8-bit RGB images in one call.  Image i is width[i] x height[i] pixels at
 * image + 3 pix_ptr[i] (pix_ptr [n_images + 1] runs from 0, pix_ptr[i + 1] - pix_ptr[i] = width[i] height[i]); with on_device all four
 * arrays are device pointers, otherwise host arrays.  out: file i is data[offsets[i] .. offsets[i + 1]) (host memory, malloc'ed:
 * mvs_png_set_free).  MVS_ERR_INVALID for an empty frame, arrays that do not agree or a null image with pixels; MVS_ERR_UNSUPPORTED
 * for an image whose raw or compressed stream reaches 0x7FF00000 bytes.
 * mvs_ctx_deflate_rle: the chunk, gather and checksum passes alone on n bytes (host or device): one zlib stream, malloc'ed (mvs_png_free).
 * mvs_encode_png_rle / mvs_deflate_rle: the same on the host, sequentially -- no GPU, no libz, the same bytes as the device gives. */
typedef struct mvs_png_stats {
    uint64_t raw_bytes, png_bytes;               /* filtered streams (height (3 width + 1) per image); the files */
    uint64_t chunks, stored_chunks;              /* all chunks; those that went out as a stored block */
    uint64_t filter_rows[5];                     /* rows per filter type */
    float ms_filter, ms_chunk, ms_gather;        /* device time per pass */
    float ms_download, ms_frame;                 /* host time: chunk table and streams to the host; checksums, CRCs and framing */
    float reserved;
} mvs_png_stats;
typedef struct mvs_png_set {
    uint32_t n_images, reserved;
    uint64_t n_bytes;
    uint8_t* data;                               /* [n_bytes] */
    uint64_t* offsets;                           /* [n_images + 1] */
} mvs_png_set;
mvs_status mvs_ctx_encode_pngs(mvs_ctx* ctx, uint32_t n_images, const uint32_t* width, const uint32_t* height, const uint64_t* pix_ptr, const uint8_t* image,
                               int on_device, mvs_png_set* out, mvs_png_stats* stats);
void mvs_png_set_free(mvs_png_set* p);
mvs_status mvs_ctx_deflate_rle(mvs_ctx* ctx, const uint8_t* bytes, uint64_t n, int on_device, uint8_t** out, uint64_t* out_bytes);
mvs_status mvs_encode_png_rle(const uint8_t* rgb, uint32_t width, uint32_t height, uint8_t** out, uint64_t* out_bytes);
mvs_status mvs_deflate_rle(const uint8_t* bytes, uint64_t n, uint8_t** out, uint64_t* out_bytes);
void mvs_png_free(uint8_t* bytes);

/* The JPEG route of rows f9 and f11 (DESIGN.md section 4 "Model output" item 9 and csrc/jpeg_base.h define the format bit for bit; any
 * JPEG decoder reads it): baseline sequential, 8 bit, JFIF, YCbCr 4:4:4 (subsampling 0) or 4:2:0 (subsampling 1), Annex K's quantiser
 * tables scaled by `quality` 1 .. 100, Annex K's Huffman tables, a restart interval of 8 MCUs.  Integer arithmetic throughout: the host
 * and the device give the same bytes.
 * mvs_ctx_encode_jpegs: the complete JPEG files of n_images 8-bit RGB images in one call; the arrays, on_device and `out` are those of
 * mvs_ctx_encode_pngs (mvs_jpeg_set_free releases out).  Every restart segment is coded by one workgroup (csrc/k_jpeg.hip), a second
 * pass gathers the segments, the host adds the headers.  MVS_ERR_INVALID for an empty frame, arrays that do not agree, a null image with
 * pixels, a quality outside 1 .. 100 or a subsampling other than 0 / 1; MVS_ERR_UNSUPPORTED for a side above 65535.
 * mvs_encode_jpeg: the same file on the host, sequentially (rgb [height][width][3]) -- no GPU, no library; malloc'ed (mvs_jpeg_free). */
typedef struct mvs_jpeg_stats {
    uint64_t raw_bytes, jpeg_bytes;              /* 3 bytes per pixel; the files */
    uint64_t segments;                           /* restart segments of all images */
    uint64_t stuffed_bytes;                      /* 0x00 bytes behind a 0xFF of entropy data */
    uint64_t marker_bytes;                       /* everything that is not entropy data: SOI .. SOS, the RST markers, EOI */
    float ms_segment, ms_gather;                 /* device time per pass */
    float ms_download, ms_frame;                 /* host time: segment table and entropy data to the host; headers and assembly */
} mvs_jpeg_stats;
typedef mvs_png_set mvs_jpeg_set;
mvs_status mvs_ctx_encode_jpegs(mvs_ctx* ctx, uint32_t n_images, const uint32_t* width, const uint32_t* height, const uint64_t* pix_ptr, const uint8_t* image,
                                int on_device, int32_t quality, int32_t subsampling, mvs_jpeg_set* out, mvs_jpeg_stats* stats);
void mvs_jpeg_set_free(mvs_jpeg_set* p);
mvs_status mvs_encode_jpeg(const uint8_t* rgb, uint32_t width, uint32_t height, int32_t quality, int32_t subsampling, uint8_t** out, uint64_t* out_bytes);
void mvs_jpeg_free(uint8_t* bytes);

/* View input: baseline JPEG files decoded on the device (DESIGN.md section 4 "View input" and csrc/jpeg_dec.h define the format accepted
 * and the arithmetic; the pixels are libjpeg-turbo's, bit for bit).  Accepted: one SOF0 frame of 8-bit samples, 1 component (written as
 * R = G = B) or 3 (Y, Cb, Cr; luma sampled 1x1, 2x1 or 2x2, chroma 1x1), one interleaved sequential scan, DQT of 8 bits, DHT classes and
 * ids 0 / 1, any restart interval or none.  Everything else is MVS_ERR_INVALID with a message that names the file and the reason.
 * The host reads the markers up to SOS; the entropy data goes to the device as it lies in the file and is unstuffed, cut into
 * subsequences of option "jpegdec_subseq_bytes" bytes that synchronise themselves, decoded, transformed and converted there
 * (csrc/k_jpegdec.hip).
 * mvs_ctx_decode_jpegs: the n files files[i][0, sizes[i]) -> their RGB images, back to back: image i is data[offsets[i], offsets[i + 1])
 *   = [height[i]][width[i]][3].  out_on_device 0: data is a malloc'ed host copy; 1: data is the context's device buffer, valid until the
 *   context's next decode.  width, height and offsets are host arrays either way; mvs_rgb_set_free releases what the library allocated.
 * mvs_scene_set_views_jpeg: mvs_scene_set_views with the images taken from files: view j's file is decoded straight into the context's
 *   image buffer of view j.  The frame's size must be views[j].width x height; views[j].rgb is not read.  Afterwards the context is
 *   exactly as mvs_scene_set_views on the decoded pixels leaves it.  A refusal leaves the context without views (the rule at mvs_scene_set_views:
 *   a data-cost pass is then MVS_ERR_STATE, no longer an empty table).  A view whose file
 *   pointer is null (a PNG, a progressive file) brings its decoded host pixels in views[j].rgb, which are uploaded as
 *   mvs_scene_set_views uploads them.  An image that needs lens undistortion no longer has to come as undistorted host pixels: with
 *   mvs_scene_set_views_lens (below) it stays a file, or the pixels it was decoded to, and is undistorted on the device.
 * mvs_jpeg_probe: MVS_OK and the frame's size when the file's headers are in the accepted format (the entropy data is not read).
 * params (null: the defaults): max_scratch_bytes bounds the device scratch of one batch (the entropy bytes, the states, 128 bytes of
 *   coefficients per block and the planes); the files are decoded in batches that fit, and a file that does not fit alone is refused.
 * stats are filled on refusals too.
 * mvs_decode_jpeg: the same image on the host, sequentially -- no GPU, no library; *rgb is malloc'ed (mvs_jpeg_free).  coefs (may be
 *   null): the quantised coefficients int16 [*n_blocks][64] in coding order, index v * 8 + u, malloc'ed (free()). */
typedef struct mvs_jpegdec_params {
    uint64_t max_scratch_bytes;                  /* default 1 GiB */
    uint64_t reserved;
} mvs_jpegdec_params;
typedef struct mvs_jpegdec_stats {
    uint64_t files, file_bytes, entropy_bytes;   /* entropy_bytes: SOS's end .. EOI as it lies in the files */
    uint64_t stuffed_bytes;                      /* 0x00 bytes behind a 0xFF of entropy data */
    uint64_t restart_segments, subsequences, windows;
    uint64_t sync_rounds_max, sync_launches;     /* most rounds one workgroup ran in one launch; launches of the synchronising kernel */
    uint64_t subseq_exact_after_pass1;           /* subsequences whose first guess already left the exact state */
    uint64_t blocks, batches;
    float ms_upload, ms_unstuff, ms_sync, ms_decode, ms_idct, ms_colour;
} mvs_jpegdec_stats;
typedef struct mvs_rgb_set {
    uint32_t n_images, on_device;
    uint64_t n_bytes;
    uint8_t* data;                               /* [n_bytes] */
    uint64_t* offsets;                           /* [n_images + 1] */
    uint32_t* width;                             /* [n_images] */
    uint32_t* height;                            /* [n_images] */
} mvs_rgb_set;
void mvs_jpegdec_default_params(mvs_jpegdec_params* p);
mvs_status mvs_ctx_decode_jpegs(mvs_ctx* ctx, const uint8_t* const* files, const uint64_t* sizes, uint32_t n, const mvs_jpegdec_params* params,
                                int out_on_device, mvs_rgb_set* out_set, mvs_jpegdec_stats* stats);
void mvs_rgb_set_free(mvs_rgb_set* p);
mvs_status mvs_scene_set_views_jpeg(mvs_ctx* ctx, const mvs_view* views, uint32_t n_views, const uint8_t* const* files, const uint64_t* sizes,
                                    const mvs_jpegdec_params* params, mvs_jpegdec_stats* stats);
mvs_status mvs_jpeg_probe(const uint8_t* data, uint64_t size, uint32_t* width, uint32_t* height);
mvs_status mvs_decode_jpeg(const uint8_t* data, uint64_t size, uint8_t** rgb, uint32_t* width, uint32_t* height, int16_t** coefs, uint64_t* n_blocks);

/* View input: PNG files inflated and unfiltered on the device (DESIGN.md section 4 "View input" and csrc/png_dec.h define the format
 * accepted and the arithmetic; PNG is lossless: the pixels are those of any PNG reader's 8-bit RGB, Pillow's convert("RGB"), bit for bit).
 * Accepted: bit depth 8, colour type 0, 2, 3, 4 or 6 (grey is written as R = G = B, alpha of any kind is dropped, tRNS is not read, a
 * palette index becomes its PLTE entry), compression 0, filter method 0, no interlace; IHDR first, PLTE (a multiple of 3 bytes, at most
 * 768; required for colour type 3) in front of the IDATs, one or more consecutive IDAT chunks; IEND is not required.  The host walks every
 * chunk by its length and checks the CRC of IHDR and PLTE.  IDAT CRCs are NOT checked: the zlib stream's Adler-32 is, and it covers every
 * byte that becomes a pixel.  zlib: CM 8, CINFO <= 7, FCHECK, no FDICT; stored, fixed and dynamic blocks.  Inflated bytes beyond
 * height * (1 + width * bytes per pixel) are ignored (the stream is still read to its end; its Adler-32, which covers them, is then not
 * checked).  Everything else is MVS_ERR_INVALID with a message that names the file and the reason: the other bit depths, Adam7, a missing
 * PLTE, IDATs that are not consecutive, a chunk running past the file, no IDAT, an unknown critical chunk; block type 3, LEN != ~NLEN, HLIT
 * above 286 or HDIST above 30, a used length symbol 286 / 287 or distance code 30 / 31, a repeat code 16 with no previous length, a repeat
 * past HLIT + HDIST, an over-subscribed code, an incomplete code (other than no distance code at all and zlib's single distance code of one
 * bit), no end-of-block code, a distance further back than the bytes produced, a stream that ends inside a symbol or before the final
 * block's end, an Adler-32 mismatch, fewer inflated bytes than the image needs, a filter type above 4 (with its row), palette indices at or
 * past PLTE's entries (with the count of such pixels).
 * Only the IDAT payloads cross the bus, through the pinned upload ring; one wave64 per stream inflates, the Adler-32 is summed in pieces,
 * and one wave per file unfilters bands of 64 rows, a lane per row, each one pixel behind the row above (csrc/k_pngdec.hip).
 * mvs_ctx_decode_pngs: the route on its own; arguments and result as mvs_ctx_decode_jpegs (params gives max_scratch_bytes: the zlib
 *   bytes, the inflated stream and, under a lens, the staged pixels of a batch; a file that does not fit alone is refused).
 * mvs_scene_set_views_files: the rule of mvs_scene_set_views_lens with one addition: a file that starts with the PNG signature takes the PNG
 *   route, any other file the JPEG route; a null file brings pixels in views[j].rgb.  lens == null: no view is undistorted.  The frame's size
 *   must be the view's.  Afterwards the context is exactly as mvs_scene_set_views on the decoded, undistorted pixels leaves it; a refusal
 *   leaves the context without views.  mvs_scene_set_views_jpeg and mvs_scene_set_views_lens refuse a PNG as before.
 * mvs_png_probe: MVS_OK and the frame's size when the file's chunks are in the accepted format (the zlib stream is not read).
 * stats are filled on refusals too.
 * mvs_decode_png: the same image on the host, sequentially -- no GPU, no library; *rgb is malloc'ed (mvs_png_free).  raw (may be null): the
 *   inflated, still filtered stream, height * (1 + width * bytes per pixel) bytes, malloc'ed (mvs_png_free). */
typedef struct mvs_pngdec_stats {
    uint64_t files, file_bytes, idat_chunks;
    uint64_t zlib_bytes, raw_bytes;              /* the IDAT payloads; the inflated streams as the images need them */
    uint64_t stored_blocks, fixed_blocks, dynamic_blocks;
    uint64_t filter_rows[5];                     /* rows per filter type */
    uint64_t batches;
    float ms_upload, ms_inflate, ms_adler, ms_unfilter;
} mvs_pngdec_stats;
mvs_status mvs_ctx_decode_pngs(mvs_ctx* ctx, const uint8_t* const* files, const uint64_t* sizes, uint32_t n, const mvs_jpegdec_params* params,
                               int out_on_device, mvs_rgb_set* out_set, mvs_pngdec_stats* stats);
mvs_status mvs_png_probe(const uint8_t* data, uint64_t size, uint32_t* width, uint32_t* height);
mvs_status mvs_decode_png(const uint8_t* data, uint64_t size, uint8_t** rgb, uint32_t* width, uint32_t* height, uint8_t** raw);

/* View input: lens undistortion on the device (row f4's arithmetic -- csrc/lens.h states it once for undistort_kernel, the batched kernel
 * and the host twin; DESIGN.md section 4 "View input").  A view comes as pixels or as a baseline JPEG file together with its lens, is
 * uploaded and / or decoded once into a staging buffer of the context, and ONE launch per batch (csrc/k_lens.hip) writes the
 * undistorted pixels of all the batch's views into the context's image buffers: the bytes of mvs_undistort_image on every image.
 * mvs_lens: the .cam file's focal length and distortion coefficients.  dist0 == 0: the image is taken as it is
 *   (generate_texture_views.cpp:153); dist1 != 0: the k2k4 model; dist1 == 0: the VisualSFM model.
 * mvs_scene_set_views_lens: lens[j] belongs to view j.  files == null: every view brings host pixels in views[j].rgb (sizes is not read, jpeg_stats
 *   stays zero, jpeg_params gives max_scratch_bytes only); otherwise the files[j] / views[j].rgb rule of every view is that of mvs_scene_set_views_jpeg.
 *   A view with dist0 != 0 goes through staging: the 3 * width * height bytes count towards its scratch in the batch cut of the files
 *   (jpeg_params->max_scratch_bytes), and pixel views are staged in groups of at most max_scratch_bytes; a view that does not fit alone is
 *   refused with its number and both sizes.  Views with dist0 == 0 take the path of mvs_scene_set_views_jpeg: no staging, no extra pass.
 *   Afterwards the context is exactly as mvs_scene_set_views on the undistorted pixels leaves it.  A refusal leaves the context without views
 *   (the rule at mvs_scene_set_views).
 * mvs_ctx_undistort_images: the route on its own -- n host images [heights[i]][widths[i]][3] -> their undistorted images back to back in
 *   an mvs_rgb_set as mvs_ctx_decode_jpegs returns one (out_on_device 1: the context's buffer, valid until its next call of this entry).
 *   Image starts are deliberately not aligned.  dist0 == 0 copies.
 * Refusals are MVS_ERR_INVALID and name the view and the reason: dist0 != 0 with flen not positive, a non-finite field, reserved != 0.
 * lens_stats (may be null) are filled on refusals too.
 * mvs_undistort_image_host: the same image on the host, sequentially -- no GPU. */
typedef struct mvs_lens { float flen, dist0, dist1; uint32_t reserved; } mvs_lens;
typedef struct mvs_lens_stats {
    uint64_t views_undistorted, views_copied;    /* by the batched kernel: dist0 != 0 / dist0 == 0 (mvs_ctx_undistort_images only) */
    uint64_t pixels, pixels_no_source;           /* of the undistorted views; pixels left black because they have no source */
    uint64_t staging_bytes, batches;             /* the most bytes staged at one time; launches of the batched kernel */
    float ms_upload, ms_undistort;               /* host time of the pixel uploads into staging; device time of the launches */
} mvs_lens_stats;
mvs_status mvs_scene_set_views_lens(mvs_ctx* ctx, const mvs_view* views, uint32_t n_views, const mvs_lens* lens, const uint8_t* const* files, const uint64_t* sizes,
                                    const mvs_jpegdec_params* jpeg_params, mvs_jpegdec_stats* jpeg_stats, mvs_lens_stats* lens_stats);
/* (the PNG view input above: files may be PNGs or baseline JPEGs; lens may be null) */
mvs_status mvs_scene_set_views_files(mvs_ctx* ctx, const mvs_view* views, uint32_t n_views, const mvs_lens* lens, const uint8_t* const* files, const uint64_t* sizes,
                                     const mvs_jpegdec_params* params, mvs_jpegdec_stats* jpeg_stats, mvs_pngdec_stats* png_stats, mvs_lens_stats* lens_stats);
mvs_status mvs_ctx_undistort_images(mvs_ctx* ctx, const uint8_t* const* images, const uint32_t* widths, const uint32_t* heights, const mvs_lens* lens, uint32_t n,
                                    int out_on_device, mvs_rgb_set* out_set, mvs_lens_stats* stats);
mvs_status mvs_undistort_image_host(const uint8_t* rgb, int32_t width, int32_t height, float flen, float dist0, float dist1, uint8_t* out);

/* View input: view masks (DESIGN.md section 4 "View input" item 10).  ONE rule: a masked pixel is an invalid pixel, and nothing else changes.
 * A view may carry a mask, one byte per pixel, [height][width] of the view, 0 = leave out, anything else = keep.  The view's validity
 * before the erosion is (flood-fill validity AND keep); under the gradient term erode_validity_mask runs on that.  The image, the gradient
 * magnitude and the footprint sampling are untouched: a (face, view) pair is dropped exactly when valid_pixel fails at one of its three
 * projected vertices, so a masked blob strictly inside one large projected triangle does not exclude that pair -- dilate the mask for a margin.
 * Rows f5 to f11 do not see masks.  Upstream has none.
 * mvs_scene_set_view_masks: masks[j] belongs to view j (null: view j has no mask); host arrays, or with on_device device arrays that stay
 *   valid during the call only.  Called after any view input (mvs_scene_set_views, _from, _jpeg, _lens) and before mvs_ctx_data_costs.  All
 *   null, n_views == 0 with masks == null, or a later view input clears the masks.  A scene without masks runs exactly as before.
 *   lens (null: none): lens[j].dist0 != 0 says that masks[j] is in the frame the camera took, as the photographs a user paints on are; it is
 *   then undistorted on the device with row f4's arithmetic, read as a one-channel image of 0 / 255: destination pixel (x, y) is kept iff
 *   it has a source and linear_at there gives the byte 255.  Views with dist0 == 0 use the mask as it is.
 *   Host masks travel through the pinned upload ring into the context's staging buffer in batches of at most max_scratch_bytes -- that of
 *   the view input the views came by (mvs_jpegdec_params; 1 GiB for mvs_scene_set_views) -- and one launch per batch packs them into keep
 *   words in the layout of the validity mask (csrc/k_viewmask.hip; under a lens csrc/k_lens.hip), kept for masked views only
 *   (4 * ceil(width / 32) * height bytes each).  A host mask that does not fit alone is refused with the view's number.
 *   Refusals name the reason and, where there is one, the view: n_views is not the context's (MVS_ERR_INVALID), no views
 *   (MVS_ERR_STATE), a non-finite lens field, reserved != 0, dist0 != 0 with flen not positive (MVS_ERR_INVALID).  A refusal leaves the
 *   context without masks.  stats (may be null) are filled on refusals too. */
typedef struct mvs_mask_stats {
    uint64_t views_masked, views_undistorted;    /* views that carry a mask; those of them whose mask went through the lens */
    uint64_t pixels, pixels_masked_out;          /* of the masked views; pixels left out, after undistortion */
    uint64_t device_bytes, staging_bytes, batches;   /* keep words held by the context; the most mask bytes staged at one time; batches */
    float ms_upload, ms_pack, ms_undistort;      /* host time of the uploads into staging; device time of the pack / the lens launches */
} mvs_mask_stats;
mvs_status mvs_scene_set_view_masks(mvs_ctx* ctx, const uint8_t* const* masks, uint32_t n_views, int on_device, const mvs_lens* lens, mvs_mask_stats* stats);

/* View input: pyramid levels -- views halved on the device on their way in (DESIGN.md section 4 "View input" item 14; csrc/level.h states
 * the arithmetic once for csrc/k_level.hip and the host twin).  What `scene::undist-L<k>` is to texrecon: the photograph crosses the bus
 * once, as the file or as its pixels, is decoded, undistorted in the frame the camera took and halved `level` times on the device, and
 * only the level image stays resident.  half(I) of a w x h image is (w + 1) / 2 x (h + 1) / 2 with
 *   half(I)(x, y, c) = (I(2x, y0, c) + I(x1, y0, c) + I(2x, y1, c) + I(x1, y1, c) + 2) >> 2,  x1 = min(2x + 1, w - 1), y1 = min(2y + 1, h - 1), y0 = 2y,
 * a box filter (DEFINED HERE from recollection of MVE's rescale_half_size<uint8_t>); level k is half applied k times, the bytes rounded
 * at every level.  Pixels without a source under a lens are black before they are averaged.
 * mvs_view_level: view j's level, 0 .. 4, and the size of its source.  views[j] (width, height, K) describes the view AT ITS LEVEL, which
 *   is what the kernels read; files[j] or views[j].rgb bring src_width x src_height pixels.  Level 0: the view is taken as it is.
 * mvs_scene_set_views_levels: mvs_scene_set_views_files with levels -- the same begin / commit rule, the same batches, PNG accepted.  A view
 *   with level > 0 is a staged view exactly as one with dist0 != 0: its 3 * src_width * src_height bytes count towards its scratch in the
 *   batch cut of the files, pixel views are staged in groups of at most max_scratch_bytes, and a view that does not fit alone is refused.
 *   A view with a lens and a level needs no second buffer: the kernel's source fetch is the lens'.  lens_stats->pixels_no_source counts
 *   full-size pixels.  Refusals (MVS_ERR_INVALID, with the view and the reason; the context is left without views): level > 4,
 *   reserved != 0, a source whose level size is not views[j]'s, a file whose frame is not src_width x src_height, a level image below
 *   2 x 2, and everything the file and lens entries refuse.
 *   Masks: mvs_scene_set_view_masks keeps its signature.  The context remembers every view's level and source size from this entry (every
 *   other view input resets them to level 0); the mask of a view with level > 0 has the SOURCE's size, and the level's keep bit is the AND
 *   of the source keep bits (after the lens, where there is one) over the clamped 2^k x 2^k block: a level pixel is kept iff everything
 *   that went into it is kept.  The full-size keep words of such a view (1 / 8 of its mask bytes) live in a scratch buffer per batch.
 * mvs_ctx_halve_images: the route on its own, shaped as mvs_ctx_undistort_images (lens may be null; level 0 copies or undistorts only).
 * mvs_halve_image_host / mvs_level_size: the host twin (out: exactly the level image's bytes) and the size of a level.  No GPU. */
typedef struct mvs_view_level { uint32_t level; int32_t src_width, src_height; uint32_t reserved; } mvs_view_level;
typedef struct mvs_level_stats {
    uint64_t views_halved, pixels_in, pixels_out;   /* views with level > 0; their source pixels and their level pixels */
    uint64_t pixels_no_source;                      /* of the halved views under a lens: full-size pixels left black (mvs_ctx_halve_images: of all images) */
    uint64_t batches, staging_bytes;                /* launches of the level kernel; the most bytes staged at one time, by the lens and the level route together */
    float ms_upload, ms_halve;                      /* host time of the pixel uploads into staging (both routes); device time of the level launches */
} mvs_level_stats;
mvs_status mvs_scene_set_views_levels(mvs_ctx* ctx, const mvs_view* views, uint32_t n_views, const mvs_view_level* levels, const mvs_lens* lens, const uint8_t* const* files,
                                      const uint64_t* sizes, const mvs_jpegdec_params* jpeg_params, mvs_jpegdec_stats* jpeg_stats, mvs_lens_stats* lens_stats, mvs_pngdec_stats* png_stats,
                                      mvs_level_stats* level_stats);
mvs_status mvs_ctx_halve_images(mvs_ctx* ctx, const uint8_t* const* images, const uint32_t* widths, const uint32_t* heights, const uint32_t* levels, const mvs_lens* lens, uint32_t n,
                                int out_on_device, mvs_rgb_set* out_set, mvs_level_stats* stats);
mvs_status mvs_halve_image_host(const uint8_t* rgb, int32_t width, int32_t height, uint32_t level, uint8_t* out);
mvs_status mvs_level_size(int32_t width, int32_t height, uint32_t level, int32_t* level_width, int32_t* level_height);

/* Row f10: the view-selection debug model, `texrecon --view_selection_model` (texrecon.cpp:216-236, generate_debug_embeddings.cpp):
 * every view's image is replaced by a flat colour of its own -- colour (position % 144) of an HSV sweep, position = the view's place in
 * the view list -- stamped all over with its three-digit id in cells of 13 x 6 pixels, and rows f6 (without adjust_colors), f8 and f9
 * run on those images: a model whose faces show which view textures them.  The definition is DESIGN.md section 4 "Debug model"; every
 * array is the same bits on any device and in every run.  view_ids: host array with one id per view, or NULL: the position (what
 * from_images_and_camera_files assigns); an id above 999 is MVS_ERR_UNSUPPORTED (upstream asserts).  Upstream's debug pass would run
 * hole filling on the faces of label 0; this library has none: faces of label 0 appear in no patch, as in rows f6 to f9.
 *   mvs_debug_view_style: background and font colour of the view at `position` (host only, no device needed).
 *   mvs_ctx_debug_embeddings: generate_debug_embeddings for n images of the caller's sizes (each side 0 .. 65535) at positions
 *     first_position + i, packed back to back as RGB8 row-major into rgb_out (3 * sum of width * height bytes, host or device; no
 *     alignment asked of a device pointer).  Needs neither mesh nor views.
 *   mvs_ctx_debug_patches: the patch set of the debug path exactly as row f6 lays it out (rows f8 and f9 take it unchanged): label,
 *     box, face_ptr, faces, texcoords and pix_ptr are row f6's for the same labels; image = byte / 255.0f of the view's debug image
 *     inside the view, (1, 0, 1) outside; validity 255 and blending 0 for every pixel (no adjust_colors: what TexturePatch's
 *     constructor leaves).  The context's real images are neither read nor written.  stats: valid_pixels = pixels, near_pixels =
 *     degenerate_faces = 0, ms_mark = 0, ms_resolve = the pixel kernel.  params.max_pixels and the errors are row f6's.  With
 *     out_on_device the arrays are the context's row-f6 buffers (valid until its next texture_patches or debug_patches call).
 *   mvs_ctx_view_selection_model: debug patches, row f8, row f9's save_model with everything left on the device in between: writes
 *     `<prefix>_view_selection.obj`, `.mtl` and `<prefix>_view_selection_material<a>_map_Kd.png` (`.jpg` under model_params.image_format 1: the parameters reach
 *     mvs_ctx_save_model unchanged).  Any params / stats may be NULL. */
mvs_status mvs_debug_view_style(uint32_t position, uint8_t bg[3], uint8_t fg[3]);
mvs_status mvs_ctx_debug_embeddings(mvs_ctx* ctx, uint32_t n, const int32_t* width, const int32_t* height, const uint32_t* view_ids,
                                    uint32_t first_position, uint8_t* rgb_out, int out_on_device);
mvs_status mvs_ctx_debug_patches(mvs_ctx* ctx, const uint32_t* adj_ptr, const uint32_t* adj, int adj_on_device, const uint32_t* labels,
                                 int labels_on_device, const uint32_t* view_ids, const mvs_patch_params* params, mvs_patch_set* out,
                                 int out_on_device, mvs_patch_stats* stats);
mvs_status mvs_ctx_view_selection_model(mvs_ctx* ctx, const uint32_t* adj_ptr, const uint32_t* adj, int adj_on_device, const uint32_t* labels,
                                        int labels_on_device, const uint32_t* view_ids, const float* vertex_normals, int normals_on_device,
                                        const char* prefix, const mvs_patch_params* patch_params, const mvs_atlas_params* atlas_params,
                                        const mvs_model_params* model_params, mvs_patch_stats* patch_stats, mvs_atlas_stats* atlas_stats,
                                        mvs_model_stats* model_stats);

/* Row f11 (not in upstream; defined here): the textured model as ONE binary glTF 2.0 file (.glb) -- the same inputs as
 * mvs_ctx_save_model, the definition is DESIGN.md section 4 "Model output" item 8, the buffers are built on the device (csrc/k_glb.hip)
 * and every byte is the same on any device and in every run.  A glTF vertex carries one index for position and texture coordinate
 * together, so the distinct pairs (global coordinate g, mesh vertex v) among the 3 n_listed corners are the vertices: they are numbered
 * in ascending (g, v), which leaves every atlas one contiguous range, and atlas a with faces becomes one primitive (material a, its
 * image the PNG -- or, under params.image_format 1, the JPEG with "mimeType": "image/jpeg" -- that mvs_ctx_save_model writes for the
 * same params, embedded) whose indices count from the start of its range.
 * POSITION, TEXCOORD_0 (texcoords_merged as it is: its origin is glTF's) and NORMAL (when vertex_normals is given) are the inputs' bits,
 * not rounded text.  Unlike the .obj the file holds only referenced vertices; faces of label 0 are in no atlas and so in no primitive.
 * An atlas set without atlas_size or image gives a file without images, textures and samplers.
 *   mvs_ctx_build_glb: the whole file in malloc'ed host memory (mvs_glb_free).  mvs_ctx_save_glb: the file at `path`, written once;
 *   a refusal leaves `path` untouched (nothing is opened before the last check), a write error removes what was written.  Running out
 *   of host memory is MVS_ERR_INVALID ("out of host memory"), as in every other row.
 * Refusals: those of mvs_ctx_build_model (MVS_ERR_STATE without a mesh; MVS_ERR_INVALID for a bad face id, texcoord id, face_ptr or
 * tc_ptr) and, for the images, of mvs_ctx_save_model (png_level, png_device, libz, image_format and the JPEG parameters); MVS_ERR_INVALID as well for a mesh face that names a
 * vertex >= n_verts.  MVS_ERR_UNSUPPORTED for a position or normal of a referenced vertex that is not finite (JSON has no inf or nan;
 * counted in stats.nonfinite_values per component of every glTF vertex) and for a file of 2^32 - 1 bytes or more or above
 * params.max_bytes (0 = no cap): checked on headers + geometry after the numbering pass, before the attribute buffers are allocated,
 * and on the whole file once the PNG sizes are known.  stats is filled either way (file_bytes: what was known at the refusal).
 *   params.glb_quantize 1 (DESIGN.md section 4 "Model output" item 10): the same pairs, numbering, primitives and images, with the
 *   geometry quantised under the extension KHR_mesh_quantization, which the file then requires: POSITION as UNSIGNED_SHORT on ONE grid
 *   for the whole file (step S = the largest extent of the three axes / 65535; the node's translation is the lower corner, its
 *   scale [S, S, S]; 8 bytes per vertex), TEXCOORD_0 as normalised UNSIGNED_SHORT (4 bytes), NORMAL as the unit normal in normalised
 *   BYTEs (4 bytes), and 16-bit indices for every primitive of at most 65 535 vertices -- 16 instead of 32 bytes per vertex, 2 instead
 *   of 4 per index.  A position is off by at most half a step, a texture coordinate by 0.5 / 65535, a unit normal's component by
 *   0.5 / 127.  A texture coordinate of a glTF vertex that is NaN or outside [0, 1] cannot be stored: MVS_ERR_UNSUPPORTED, counted
 *   in texcoords_out_of_range per component; a normal of length 0 is stored as (0, 0, 0) and counted in zero_normals (both below).
 *   The size checks run on the quantised sizes.  Any glb_quantize other than 0 / 1 is MVS_ERR_INVALID; mvs_ctx_save_model and
 *   mvs_ctx_build_model do not read the field.  mvs_glb_stats keeps its 96 bytes: what this route adds to the stats is
 *   mvs_glb_quant_stats, which mvs_ctx_glb_quant_stats copies out for the context's LAST build_glb / save_glb call, refused or not
 *   (all zero after a call with glb_quantize 0 and before the first call; MVS_ERR_INVALID for a null argument). */
typedef struct mvs_glb {
    uint64_t n_bytes;
    uint8_t* data;                               /* [n_bytes] */
} mvs_glb;
typedef struct mvs_glb_stats {
    uint64_t vertices, indices, primitives;      /* distinct (coordinate, vertex) pairs; 3 n_listed; atlases with faces */
    uint64_t json_bytes, geometry_bytes, image_bytes, file_bytes;   /* the JSON chunk's data (padded); attributes + indices; the PNGs with their padding; all */
    uint64_t nonfinite_values;                   /* inf / nan among the POSITION and NORMAL components of the glTF vertices */
    float ms_keys, ms_sort, ms_number, ms_indices, ms_gather;      /* device time per phase */
    float ms_png, ms_download, ms_file;          /* host time: the PNGs (copy, encode); geometry to the host; JSON and the file (or its assembly in memory) */
} mvs_glb_stats;
mvs_status mvs_ctx_build_glb(mvs_ctx* ctx, const mvs_atlas_set* atlases, int atlases_on_device, const float* vertex_normals, int normals_on_device,
                             const mvs_model_params* params, mvs_glb* out, mvs_glb_stats* stats);
mvs_status mvs_ctx_save_glb(mvs_ctx* ctx, const mvs_atlas_set* atlases, int atlases_on_device, const float* vertex_normals, int normals_on_device,
                            const char* path, const mvs_model_params* params, mvs_glb_stats* stats);
void mvs_glb_free(mvs_glb* g);
typedef struct mvs_glb_quant_stats {
    uint64_t zero_normals;                       /* glTF vertices whose normal has length 0: stored as (0, 0, 0) */
    uint64_t texcoords_out_of_range;             /* TEXCOORD_0 components of glTF vertices that are NaN or outside [0, 1]: the call was refused */
    uint64_t index16_primitives;                 /* primitives with 16-bit indices */
    float ms_bounds, reserved;                   /* device time of the file-wide bounds pass (between ms_indices and ms_gather) */
} mvs_glb_quant_stats;
mvs_status mvs_ctx_glb_quant_stats(mvs_ctx* ctx, mvs_glb_quant_stats* out);

/* Row f4: the undistortion step of from_images_and_camera_files (generate_texture_views.cpp:153-165): dist0 == 0 copies the
 * image; dist0 != 0 and dist1 != 0 is mve::image::image_undistort_k2k4(image, flen, dist0, dist1); dist0 != 0 and dist1 == 0 is
 * image_undistort_vsfm(image, flen, dist0).  rgb / out: host arrays of width * height * 3 bytes.  MVE is absent: the two
 * models are DEFINED in csrc/lens.h (and restated in the oracle) from recollection of mve/image_tools.h. */
mvs_status mvs_undistort_image(const uint8_t* rgb, int32_t width, int32_t height, float flen, float dist0, float dist1, uint8_t* out);

/* Label-space compression for scenes with hundreds of candidate views per face (BASELINE config 5): keeps, per face, the
 * max_labels entries with the smallest (cost, view id) pairs, in ascending view order; shorter columns are untouched.
 * NOT the reference's model (view_selection.cpp:46-47 keeps every candidate): off unless asked for -- here, or with
 * mvs_set_option(ctx, "max_labels", K), which applies it at the end of every data-cost pass (also of the sharded path).
 * With max_labels <= 255 every column takes the solver's fast path.  Works on the context's own table. */
mvs_status mvs_ctx_prune_labels(mvs_ctx* ctx, uint32_t max_labels);

/* tex::postprocess_face_infos (libs/tex/texturing.h:71-74; calculate_data_costs.cpp:253-306) for callers that hold their own
 * FaceProjectionInfos: infos of face i are entries info_ptr[i] .. info_ptr[i + 1] of view_id / quality / mean_color
 * (3 floats, YCbCr, read only when outlier removal is on) IN THE ORDER the caller's vectors hold them -- the outlier
 * detection sums in that order.  Output as mvs_data_costs (library-allocated, mvs_csr_free). */
mvs_status mvs_postprocess_face_infos(uint32_t n_faces, uint32_t n_views, const uint32_t* info_ptr, const uint16_t* view_id,
                                      const float* quality, const float* mean_color, const mvs_settings* settings,
                                      mvs_csr* out, mvs_dc_stats* stats);

/* ---- sharded view selection: one rank per GPU, host side in C++, RCCL halo exchange (csrc/shard.hip; DESIGN.md "Multi-GPU") ----
 * Faces are cut into `world` contiguous parts of the LIBRARY's face order ("Face order and partition" above: every rank derives
 * the same Hilbert order from the replicated mesh, so the mesh may arrive in any order): part_begin[0 .. world] are cut points
 * of that order, NULL = `world` equal parts.  Every rank holds the replicated scene and the full adjacency; it evaluates the data
 * costs of its part, keeps a cost table of the GLOBAL shape with only its own and its halo columns filled, sweeps its own
 * nodes and exchanges -- after every colour phase -- the message runs written in that phase over cut edges (as bytes) and the
 * labels of that phase's boundary nodes with the ranks that own the neighbours: grouped ncclSend / ncclRecv, neighbours
 * only.  Results are bit-identical to the single-GPU path for any number of parts.
 *
 * Transport of the sweep loop, decided by the communicator: over RCCL through the communicator (one pack launch, one grouped exchange,
 * one unpack launch per colour phase); over the in-process communicator, whose ranks address each other's device memory (one
 * process, one host thread per GPU of a node, peer access between the GPUs), "peer push": one launch per phase
 * stores the runs at their final places in the neighbours' arrays, ordering is by one stream event per phase and rank (waited for on
 * the stream, never on the host), the sweep's energy pair is published the same way and summed by every rank on the device.
 *
 * Communicators: RCCL (one process per GPU: mvs_comm_unique_id on rank 0, the 128 bytes travel by any means, mvs_comm_create_rccl
 * on every rank) or the in-process one (mvs_comm_create_local_devices: `world` host threads of ONE process, rank r driving a context
 * on devices[r]; distinct GPUs get hipDeviceEnablePeerAccess in both directions and the collectives are peer copies -- the
 * single-node route; MVS_ERR_UNSUPPORTED if two of the GPUs cannot address each other, RCCL serves such a node; devices == NULL or
 * all equal: the ranks time-slice one device, which is how a 1-GPU box tests it).
 * A rank whose call fails makes the other ranks' host-side waits of that call end with an error (no rank is left blocked); the
 * communicator stays usable for the next call. */
#define MVS_COMM_ID_BYTES 128
typedef struct mvs_comm mvs_comm;
typedef struct mvs_shard mvs_shard;
mvs_status mvs_comm_unique_id(uint8_t id_out[MVS_COMM_ID_BYTES]);
mvs_status mvs_comm_create_rccl(int device, int rank, int world, const uint8_t id[MVS_COMM_ID_BYTES], mvs_comm** out);
mvs_status mvs_comm_create_local(int world, mvs_comm** out /* [world] */);                                /* all ranks on the current device */
mvs_status mvs_comm_create_local_devices(int world, const int* devices /* [world] or NULL */, mvs_comm** out /* [world] */);
/* gives an in-process communicator up: the host-side waits of all its ranks inside sharded calls end with an error from now on (for a
 * rank whose driver failed outside the library: its peers are released instead of waiting for it).  IN-PROCESS COMMUNICATORS ONLY: over
 * RCCL (mvs_comm_create_rccl) this is a no-op, and a rank that fails inside a sharded call leaves its peers inside the collective they
 * entered -- ending the job is the launcher's business there (torch.distributed.run takes the whole group down when one process dies). */
void mvs_comm_abort(mvs_comm* comm);
/* *peer_push = 1: the ranks can store into each other's device memory (in-process communicator: a solve of more than one rank takes
 * the peer-push transport), 0: RCCL; any out may be NULL */
mvs_status mvs_comm_info(mvs_comm* comm, int* rank, int* world, int* peer_push);
void mvs_comm_destroy(mvs_comm* comm);
/* ctx: the rank's context with the FULL mesh and all views set; adjacency: device pointers to the full graph in the CALLER's face
 * numbering (read once, at creation) */
mvs_status mvs_shard_create(mvs_ctx* ctx, mvs_comm* comm, const uint32_t* part_begin /* host, [world + 1], or NULL */,
                            const uint32_t* adj_ptr_device, const uint32_t* adj_device, mvs_shard** out);
/* the caller's ids of the faces this rank owns, in the order of the labels mvs_shard_view_selection returns (ids_device may be NULL) */
mvs_status mvs_shard_own_faces(mvs_shard* shard, uint32_t* ids_device, uint32_t* n_own);
void mvs_shard_destroy(mvs_shard* shard);
/* tex::calculate_data_costs over all ranks; stats = this rank's pairs / culls, max_quality and percentile global */
mvs_status mvs_shard_data_costs(mvs_shard* shard, const mvs_settings* settings, mvs_dc_stats* stats, uint64_t* nnz_global);
/* tex::view_selection over all ranks; labels of the OWN faces (in the order of mvs_shard_own_faces) into labels_own_device; stats global */
mvs_status mvs_shard_view_selection(mvs_shard* shard, const mvs_mrf_params* params, uint32_t* labels_own_device, mvs_mrf_stats* stats);
/* halo plan of the last view selection: message bytes this rank sends per sweep, its boundary nodes, device time of the planning */
mvs_status mvs_shard_plan_info(mvs_shard* shard, uint64_t* msg_bytes_per_sweep, uint64_t* boundary_nodes, double* plan_ms);
/* transport of the last view selection: peer_push = 1 if the runs were stored into the peers' arrays (in-process communicator, more
 * than one rank, at least one colour phase), 0 if they went through the communicator's exchange; colour phases pushed so far (all
 * solves); ranks this one shares a cut with; colour phases per sweep */
mvs_status mvs_shard_transport_info(mvs_shard* shard, int* peer_push, uint64_t* phases_pushed, int* neighbours, uint32_t* colour_phases);

#ifdef __cplusplus
}
#endif
#endif /* MVS_VIEWSEL_H */
