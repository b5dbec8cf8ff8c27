/* mvs_viewsel_blocks.h -- BUILDING BLOCKS of a sharded driver (library libmvs_blocks.so, source csrc/mgpu.hip).
 *
 * NOT part of the product library.  The product's multi-GPU path is mvs_comm_* / mvs_shard_* of mvs_viewsel.h (csrc/shard.hip in
 * libmvs_viewsel.so).  These entry points expose the same device code one step lower -- one colour phase of a node range, gather /
 * scatter of halo elements by index list, the device-side step, ICM gain / apply -- so that a driver written elsewhere can own the
 * exchange.  In this repository they carry the Python harness of the CPU multi-process tests (tests/tools/multigpu.py over
 * torch.distributed / gloo: the collectives' call pattern at world size 2 and 4 without a second GPU) and scripts/rank_share_mrf.py.
 * Link order: libmvs_blocks.so needs libmvs_viewsel.so. */
#ifndef MVS_VIEWSEL_BLOCKS_H
#define MVS_VIEWSEL_BLOCKS_H
#include "mvs_viewsel.h"
#ifdef __cplusplus
extern "C" {
#endif

/* between mvs_ctx_dc_phase1 / 2 / 3 (mvs_viewsel.h): the local max quality (1 float) and the local histogram (MVS_HIST_WORDS u32) to /
 * from caller-owned DEVICE buffers, stream-ordered -- what a driver all-reduces at the barrier of calculate_data_costs.cpp:278-288 */
mvs_status mvs_ctx_dc_get_max(mvs_ctx* ctx, float* dst_device);
mvs_status mvs_ctx_dc_set_max(mvs_ctx* ctx, const float* src_device);
mvs_status mvs_ctx_dc_get_histogram(mvs_ctx* ctx, uint32_t* dst_device);
mvs_status mvs_ctx_dc_set_histogram(mvs_ctx* ctx, const uint32_t* src_device);
/* copy the resident costs into caller-owned DEVICE arrays (stream-ordered): counts[n_faces] = column lengths, view_id[nnz], cost[nnz]
 * -- the pieces a driver all-gathers into the global table */
mvs_status mvs_ctx_costs_export(mvs_ctx* ctx, uint32_t* counts_device, uint16_t* view_id_device, float* cost_device);
/* HARNESS ONLY (tests/test_gpu_occlusion_rays.py): the bit matrices of the occlusion-ray stage (csrc/k_bvh.hip) as the context's last
 * data-cost pass left them: which = 0 the NEED bits (some face on the vertex passed the culls for the view: the ray is traced), 1 the OCCLUDED
 * bits (what ray_packet3_kernel wrote).  View-major, (n_verts + 63) / 64 64-bit words per view, bit (v & 63) of word (v >> 6) = vertex v in
 * the CALLER's vertex numbering (the device matrices follow the library's curve order; the entry maps them back).  which = 2: that order
 * itself, n_verts 32-bit words, entry s = the caller's id of the vertex at curve position s -- 64 consecutive positions share a device word,
 * i.e. a ray packet.  *n_bytes = size of the matrix / the order; out_host == null: the size only.  MVS_ERR_STATE before a data-cost pass
 * with the geometric visibility test, when the last pass covered a face range and not the whole mesh, or (which = 0, 1) when it walked
 * the mesh in more than one range (option "dc_range_pairs"): the matrices then hold the last range's rays only. */
mvs_status mvs_ctx_ray_bits(mvs_ctx* ctx, int which, void* out_host, uint64_t cap_bytes, uint64_t* n_bytes);
/* HARNESS ONLY (tests/test_gpu_image_prep.py): what the image preparation (csrc/k_prep.hip prepare_views) of the context's last data-cost
 * pass left on the device, copied to the host as it lies -- the entry launches nothing and no pass does any work for it.
 *   which = 0  the view's gradient-magnitude image, width * height bytes (MVS_ERR_STATE when the last pass ran the area term: there is none);
 *   which = 1  the view's validity mask, height * mask_stride 32-bit words, mask_stride = (width + 31) / 32, bit (x & 31) of word
 *              (y, x >> 5) = pixel (x, y) -- eroded when the last pass ran the gradient term, plain with the area term;
 *   which = 2  the view's tile summary, (height + 31) / 32 rows of msum_stride = 2 * ((mask_stride + 63) / 64) words, bit (tx & 31) of word
 *              (ty, tx >> 5) = 32 x 32 tile (tx, ty).  Meaningful, like the mask, only for a view whose flag (which = 3) is 1: the shortcut for
 *              a scene without a black corner pixel skips the flood fill, the mask and the summary;
 *   which = 3  one byte per view of the context (`view` ignored): 1 = the DEVICE copy of the view table still carries the view's mask
 *              pointer, 0 = a shortcut nulled it (no view has a black corner pixel, or this view's summary came out all ones).
 * *n_bytes = the size; out_host == null: the size only; a buffer smaller than that, or view >= n_views: MVS_ERR_INVALID.  MVS_ERR_STATE before
 * a data-cost pass that evaluated (face, view) pairs of the scene (mvs_postprocess_face_infos and a pass over no faces prepare nothing).
 * Ranged passes (option "dc_range_pairs") and the ranks of the sharded driver ARE served: a ranged pass prepares the views in its first
 * range and every later range reads the same resident products; a rank runs the whole preparation on its own context. */
mvs_status mvs_ctx_prep_products(mvs_ctx* ctx, int which, uint32_t view, void* out_host, uint64_t cap_bytes, uint64_t* n_bytes);
/* HARNESS ONLY (tests/test_gpu_mrf_regions.py): mvs_ctx_costs_upload of a HOST table whose columns stand in POSITION order, column p being
 * the caller's face order_host[p] -- and the context left as a data-cost pass over the whole mesh leaves it (name_table_order, k_dc.hip): the
 * active table lives in "the library's own order", mvs_ctx_table_order returns `order`, its inverse is known, both on the device and owned
 * by the context (they take the place of the resident mesh's face order, which the next data-cost pass derives again; the next plain
 * mvs_ctx_costs_upload ends the ordered state).  So crafted tables reach the branches of the solver that translate positions into the
 * caller's ids -- colouring keys, the ICM winner rule, region names, the label scatter, the adjacency renumbering -- in ANY order, not
 * only behind a scene's data costs.  To be followed by mvs_ctx_view_selection only (adjacency and labels in the CALLER's numbering, as
 * always): the other consumers of an ordered table belong to a resident mesh.  MVS_ERR_INVALID, with the context untouched, when
 * order_host is not a permutation of 0 .. n_faces - 1; MVS_ERR_STATE on a context whose face order a shard has pinned (mvs_shard_create). */
mvs_status mvs_ctx_costs_upload_ordered(mvs_ctx* ctx, const mvs_csr* csr_in_position_order, const uint32_t* order_host);
/* HARNESS ONLY (tests/test_gpu_tone_mapping.py): replaces the 256-entry texel table that tone_mapping = MVS_TONE_GAMMA reads in rows f5, f6
 * and f10 (table256_host[b] = the value of byte b; the fill of the crop is entries 255, 0, 255) -- with a permuted byte / 255 table the
 * gamma instantiations can be held to the CPU models of tone mapping `none` on permuted images: every texel read has to go through the
 * table.  Null restores the gamma table (mvs_tone_table).  Row f8's correction is not affected. */
mvs_status mvs_ctx_tone_table(mvs_ctx* ctx, const float* table256_host_or_null);
/* HARNESS ONLY (tests/test_gpu_lens.py): the context's image of one view, width * height * 3 bytes, copied to the host as it lies -- whatever
 * mvs_scene_set_views, _jpeg or _lens left there; nothing is launched.  *n_bytes = the size; out_host == null: the size only; a smaller
 * buffer or view >= n_views: MVS_ERR_INVALID; MVS_ERR_STATE on a context without views. */
mvs_status mvs_ctx_view_image(mvs_ctx* ctx, uint32_t view, void* out_host, uint64_t cap_bytes, uint64_t* n_bytes);
/* HARNESS ONLY (tests/test_gpu_view_masks.py): the keep words of one view as mvs_scene_set_view_masks left them, height * ceil(width / 32)
 * 32-bit words (bit b of word wx of a row = pixel 32 wx + b), copied to the host; nothing is launched.  *n_bytes = the size, 0 for a view
 * without a mask; the other rules are mvs_ctx_view_image's. */
mvs_status mvs_ctx_view_keep_words(mvs_ctx* ctx, uint32_t view, void* out_host, uint64_t cap_bytes, uint64_t* n_bytes);

/* ---- multi-GPU MRF building blocks (one context per rank; DESIGN.md "Multi-GPU") ----
 * Every rank holds the FULL cost table and adjacency (288 GB of HBM make the
 * metadata cheap to replicate) and owns a contiguous node range.  The sweep is
 * colour-phased: within a phase a node's update depends only on nodes of other colours, which are
 * exchanged before their next use: results are bit-identical for any partition.  One sweep on rank r:
 *   for every colour phase: mrf_sweep_phase(own range) -> mrf_gather(MSG | LAB, boundary index lists) ->
 *   RCCL all-to-all by the driver -> mrf_scatter;  then mrf_energy(own range) ->
 *   all-reduce of the two u64 -> mrf_step.  The index lists are planned on the host from
 * col_ptr + adjacency alone (tests/tools/multigpu.py). */
/* solver arrays addressable by the halo exchange: messages, decoded labels (view + 1) of the current
 * sweep, ICM gains, labels of the best labeling so far */
enum { MVS_MRF_MSG = 0, MVS_MRF_LAB = 1, MVS_MRF_GAIN = 2, MVS_MRF_BEST_LAB = 3,
       /* combined addressing for one exchange per sweep: index < 2^31 -> MSG[index], else LAB[index & 0x7FFFFFFF] */
       MVS_MRF_MSG_LAB = 4 };
mvs_status mvs_ctx_mrf_setup(mvs_ctx* ctx, const uint32_t* adj_ptr, const uint32_t* adj, int adj_on_device,
                             const mvs_mrf_params* params);
/* NOTE: once the device-side stop rule has fired (mvs_mrf_progress.stopped, set by mvs_ctx_mrf_step) every later sweep / sweep phase
 * ends at its first instruction -- it changes no message, no decode and no energy partial: the best labeling is frozen.  A driver that
 * wants more sweeps than the rule allows raises max_sweeps / min_sweeps in the params of mvs_ctx_mrf_setup instead. */
/* The phases of a sweep run in ascending order, every sweep from phase 0.  A phase may be cut into several node ranges: consecutive calls
 * of the same phase belong to one sweep (one damping factor); a call whose phase number is smaller than the previous call's starts the next. */
mvs_status mvs_ctx_mrf_sweep_phase(mvs_ctx* ctx, uint32_t phase, uint32_t node_begin, uint32_t node_end);
/* Boundary-first phases (what csrc/shard.hip does per rank): marks_device[i] != 0 puts node i into the BOUNDARY zone of its colour class
 * (own nodes with an edge into another rank's part); a phase then runs as part 1 (boundary zone) -> hand-over -> part 2 (interior zone).
 * part 0 = both zones.  A solve keeps to one of the two modes.  Same values either way: a colour class is an independent set. */
mvs_status mvs_ctx_mrf_setup_marked(mvs_ctx* ctx, const uint32_t* adj_ptr, const uint32_t* adj, int adj_on_device,
                                    const mvs_mrf_params* params, const uint8_t* marks_device);
mvs_status mvs_ctx_mrf_sweep_phase_part(mvs_ctx* ctx, uint32_t phase, uint32_t node_begin, uint32_t node_end, int part);
/* all phases in turn over nodes [node_begin, node_end) (no exchange in between: unsharded use) */
mvs_status mvs_ctx_mrf_sweep(mvs_ctx* ctx, uint32_t node_begin, uint32_t node_end);
/* what the last set-up built, for tests that compare two builds or two routes of it byte for byte: which = 0 one 64-bit word, 1 = the
 * set-up worked from view-set bitmaps, 0 = from the view lists; 1 the fast nodes' records (32-bit words, the zero words in front included);
 * 2 their descriptors (48 bytes each, schedule order); 3 the identical-lists flag of every directed edge (bytes, adjacency order).
 * *n_bytes = size of the table; out_host == null: the size only */
mvs_status mvs_ctx_mrf_setup_tables(mvs_ctx* ctx, int which, void* out_host, uint64_t cap_bytes, uint64_t* n_bytes);
/* message layout for the halo planner: in_off_host[e] = first message element of the run of directed edge e
 * (adjacency-list order, e < adj_ptr[n_faces]); runs are laid out in (colour, face id) node order */
mvs_status mvs_ctx_mrf_layout(mvs_ctx* ctx, uint32_t* in_off_host, uint64_t n_edges);
/* dst[k] = array[idx[k]] / array[idx[k]] = src[k] in 4-byte exchange words (message elements are 8-bit codes and travel
 * zero-extended); MSG = the buffer the last sweep wrote */
mvs_status mvs_ctx_mrf_gather(mvs_ctx* ctx, int which, const uint32_t* idx_device, uint64_t n, void* dst_device);
mvs_status mvs_ctx_mrf_scatter(mvs_ctx* ctx, int which, const uint32_t* idx_device, uint64_t n, const void* src_device);
/* partial energy (32.32 fixed point) + cut count of labeling LAB or BEST_LAB over own nodes -> dst_device[2] */
mvs_status mvs_ctx_mrf_energy(mvs_ctx* ctx, int which_sel, uint32_t node_begin, uint32_t node_end, uint64_t* dst_device);
/* best labeling := current decode (call on every rank when the all-reduced energy improved) */
mvs_status mvs_ctx_mrf_keep_best(mvs_ctx* ctx);
/* Device-side bookkeeping of one sweep, so that the host never has to wait for a sweep's energy before it
 * enqueues the next one: given the (all-reduced) energy pair in energy_device (NULL = the context's own energy of
 * the last mvs_ctx_mrf_energy), a one-thread kernel advances the sweep counter, tracks the best energy, applies
 * the stop rule (StopWhenReturnsDiminish-style, view_selection.cpp:84) and, if the energy improved, a second kernel
 * copies the current decode into the best labeling.  Once the rule has fired every later step is a no-op, so the
 * host may run `lag` sweeps ahead and poll old reports.  The report of step n (1-based count of mvs_ctx_mrf_step
 * calls since mvs_ctx_mrf_setup) travels through a pinned ring of 16 slots. */
mvs_status mvs_ctx_mrf_step(mvs_ctx* ctx, const uint64_t* energy_device);
/* wait for the report of step `step` (must be within the last 16 issued) */
mvs_status mvs_ctx_mrf_poll(mvs_ctx* ctx, uint32_t step, mvs_mrf_progress* out);
/* ICM on the best labeling: gains of own nodes; then (after the GAIN halo exchange) apply in place */
mvs_status mvs_ctx_mrf_icm_gain(mvs_ctx* ctx, uint32_t node_begin, uint32_t node_end);
mvs_status mvs_ctx_mrf_icm_apply(mvs_ctx* ctx, uint32_t node_begin, uint32_t node_end, uint32_t* moved_device);
/* labels (view_selection.cpp:120-132) of own nodes of the best labeling into labels_device[node_end - node_begin]: nodes are COLUMNS
 * of the active table, i.e. positions of the library's face order after a data-cost pass of the context (mvs_ctx_table_order names the caller's
 * ids), the caller's ids after mvs_ctx_costs_upload or with option "face_order" = 0; mvs_ctx_view_selection returns the caller's ids */
mvs_status mvs_ctx_mrf_labels(mvs_ctx* ctx, uint32_t node_begin, uint32_t node_end, uint32_t* labels_device,
                              uint32_t* unseen_out);

#ifdef __cplusplus
}
#endif
#endif
