"""ctypes binding of csrc/libmvs_viewsel.so (include/mvs_viewsel.h).

Mirrors the reference interface for the path:
    calculate_data_costs(mesh, texture_views, settings) -> DataCosts   (libs/tex/texturing.h:66-69)
    view_selection(data_costs, graph, settings)  -> labels              (libs/tex/texturing.h:79-80)
Arrays may be numpy arrays (host) or torch CUDA tensors (device-resident; torch
is only used for the device memory and the stream).
"""
import contextlib
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# MVS_VIEWSEL_LIB: another build of the same library (A/B experiments on one GPU box: scripts/variants.sh)
_LIB_PATH = os.environ.get("MVS_VIEWSEL_LIB") or os.path.join(_HERE, "csrc", "libmvs_viewsel.so")
_BLOCKS_PATH = os.path.join(_HERE, "csrc", "libmvs_blocks.so")


class MvsError(RuntimeError):
    def __init__(self, status, message):
        super().__init__("%s (status %d)" % (message, status))
        self.status = status


class CMesh(C.Structure):
    _fields_ = [("n_verts", C.c_uint32), ("n_faces", C.c_uint32), ("verts", C.c_void_p), ("faces", C.c_void_p),
                ("face_normals", C.c_void_p)]


class CView(C.Structure):
    _fields_ = [("pos", C.c_float * 3), ("viewdir", C.c_float * 3), ("K", C.c_float * 9), ("w2c", C.c_float * 16),
                ("width", C.c_int32), ("height", C.c_int32), ("rgb", C.c_void_p)]


class Settings(C.Structure):
    """tex::Settings fields read by the path (libs/tex/settings.h:85,87,90)."""
    _fields_ = [("data_term", C.c_int32), ("outlier_removal", C.c_int32), ("geometric_visibility_test", C.c_int32)]

    DATA_TERMS = {"area": 0, "gmi": 1}                                        # settings.h:113-116
    OUTLIER = {"none": 0, "gauss_damping": 1, "gauss_clamping": 2}           # settings.h:123-126

    def __init__(self, data_term="gmi", outlier_removal="none", geometric_visibility_test=True):
        super().__init__(self.DATA_TERMS[data_term] if isinstance(data_term, str) else int(data_term),
                         self.OUTLIER[outlier_removal] if isinstance(outlier_removal, str) else int(outlier_removal),
                         1 if geometric_visibility_test else 0)


class CCsr(C.Structure):
    _fields_ = [("n_faces", C.c_uint32), ("n_views", C.c_uint32), ("nnz", C.c_uint64), ("col_ptr", C.c_void_p),
                ("view_id", C.c_void_p), ("cost", C.c_void_p)]


class MrfParams(C.Structure):
    _fields_ = [("max_sweeps", C.c_int32), ("min_sweeps", C.c_int32), ("window", C.c_int32),
                ("min_improvement", C.c_float), ("damping", C.c_float), ("rho", C.c_float), ("icm_iters", C.c_int32),
                ("region_rounds", C.c_int32)]


class MrfStats(C.Structure):
    _fields_ = [("energy_fixed", C.c_uint64), ("energy", C.c_double), ("cut_edges", C.c_uint64), ("sweeps", C.c_uint32),
                ("icm_iters", C.c_uint32), ("unseen", C.c_uint32), ("region_rounds", C.c_uint32), ("region_moves", C.c_uint32)]


class MrfProgress(C.Structure):
    _fields_ = [("sweep", C.c_uint32), ("stopped", C.c_uint32), ("improved", C.c_uint32), ("stop_sweep", C.c_uint32),
                ("energy", C.c_uint64), ("best", C.c_uint64), ("w", C.c_uint32), ("best_w", C.c_uint32)]


class Subgraphs(C.Structure):
    _fields_ = [("n_faces", C.c_uint32), ("n_labels", C.c_uint32), ("n_components", C.c_uint32),
                ("label_ptr", C.c_void_p), ("comp_ptr", C.c_void_p), ("comp_faces", C.c_void_p)]


class GslParams(C.Structure):
    _fields_ = [("tolerance", C.c_float), ("max_iterations", C.c_uint32), ("lam", C.c_float), ("tone_mapping", C.c_uint32)]


class GslResult(C.Structure):
    _fields_ = [("n_verts", C.c_uint32), ("n_faces", C.c_uint32), ("x_rows", C.c_uint32), ("reserved", C.c_uint32),
                ("x_ptr", C.c_void_p), ("x_label", C.c_void_p), ("x_adjust", C.c_void_p), ("corner_adjust", C.c_void_p)]


GSL_COUNTS = ("patches", "merged", "x_rows", "a_rows", "gamma_rows", "lhs_nnz_lower", "seam_edges", "samples")
GSL_MS = ("ms_rows", "ms_patches", "ms_system", "ms_solve", "ms_output", "ms_total")


class GslStats(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in GSL_COUNTS] + [("iterations", C.c_uint32 * 3), ("error", C.c_float * 3)] + [(k, C.c_float) for k in GSL_MS]


class GslSystem(C.Structure):
    _fields_ = [("x_rows", C.c_uint32), ("a_rows", C.c_uint32), ("lhs_nnz", C.c_uint64), ("lhs_ptr", C.c_void_p), ("lhs_col", C.c_void_p),
                ("lhs_val", C.c_void_p), ("rhs", C.c_void_p), ("a_col", C.c_void_p), ("b", C.c_void_p), ("x_raw", C.c_void_p)]


class PatchParams(C.Structure):
    _fields_ = [("max_pixels", C.c_uint64), ("tone_mapping", C.c_uint32), ("reserved", C.c_uint32)]


class PatchSet(C.Structure):
    _fields_ = [("n_patches", C.c_uint32), ("n_listed", C.c_uint32), ("n_pixels", C.c_uint64)] + \
               [(k, C.c_void_p) for k in ("label", "box", "face_ptr", "faces", "texcoords", "pix_ptr", "image", "validity", "blending")]


PATCH_COUNTS = ("patches", "merged", "listed_faces", "degenerate_faces", "pixels", "valid_pixels", "near_pixels")
PATCH_MS = ("ms_tables", "ms_lists", "ms_mark", "ms_resolve", "ms_total")


class PatchStats(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in PATCH_COUNTS] + [(k, C.c_float) for k in PATCH_MS] + [("reserved", C.c_float)]


class LslParams(C.Structure):
    _fields_ = [("tolerance", C.c_float), ("max_iterations", C.c_uint32), ("strip_width", C.c_uint32), ("lds_bytes", C.c_uint32)]


class LslResult(C.Structure):
    _fields_ = [("n_patches", C.c_uint32), ("reserved", C.c_uint32), ("n_pixels", C.c_uint64), ("image", C.c_void_p), ("validity", C.c_void_p),
                ("blending", C.c_void_p)]


LSL_COUNTS = ("seam_edges", "skipped_pairs", "vertex_infos", "edge_projections", "colour_samples", "invalid_samples", "vertex_writes", "line_writes",
              "written_pixels", "outside_frame", "invalid_writes", "strip_pixels", "fixed_pixels", "demoted", "patches_lds", "patches_global",
              "pixels_global", "iterations_total", "hit_max_iterations")
LSL_MS = ("ms_topology", "ms_colours", "ms_writes", "ms_mask", "ms_solve", "ms_total")


class LslStats(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in LSL_COUNTS] + [("iterations_max", C.c_uint32), ("error_max", C.c_float)] + [(k, C.c_float) for k in LSL_MS]


class AtlasParams(C.Structure):
    _fields_ = [("max_pixels", C.c_uint64), ("tone_mapping", C.c_uint32), ("reserved", C.c_uint32)]


ATLAS_ARRAYS = ("atlas_size", "atlas_pix_ptr", "image", "patch_atlas", "patch_pos", "patch_order", "face_ptr", "faces", "texcoords", "tc_ptr",
                "texcoords_merged", "texcoord_ids")


class AtlasSet(C.Structure):
    _fields_ = [("n_atlases", C.c_uint32), ("n_patches", C.c_uint32), ("n_listed", C.c_uint32), ("n_merged", C.c_uint32), ("n_pixels", C.c_uint64)] + \
               [(k, C.c_void_p) for k in ATLAS_ARRAYS]


ATLAS_COUNTS = ("atlases", "atlases_256", "atlases_512", "atlases_1024", "atlases_2048", "atlases_4096", "atlases_8192", "pixels", "valid_pixels",
                "padded_pixels", "free_rects_peak", "merged_texcoords")
ATLAS_MS = ("ms_pack", "ms_compose", "ms_pad", "ms_texcoords", "ms_total")


class AtlasStats(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ATLAS_COUNTS] + [(k, C.c_float) for k in ATLAS_MS] + [("reserved", C.c_float)]


class ModelParams(C.Structure):
    _fields_ = [("max_bytes", C.c_uint64), ("png_level", C.c_int32), ("png_device", C.c_int32),
                ("image_format", C.c_int32), ("jpeg_quality", C.c_int32), ("jpeg_subsampling", C.c_int32), ("glb_quantize", C.c_int32)]


class ModelText(C.Structure):
    _fields_ = [("n_atlases", C.c_uint32), ("reserved", C.c_uint32), ("obj_bytes", C.c_uint64), ("mtl_bytes", C.c_uint64), ("obj", C.c_void_p), ("mtl", C.c_void_p),
                ("section_ptr", C.c_void_p), ("section_bytes", C.c_void_p)]


MODEL_SECTIONS = ("header", "v", "vt", "vn", "groups")
MODEL_COUNTS = ("mtl_bytes", "wide_values", "nonfinite_values")
MODEL_MS = ("ms_measure", "ms_scan", "ms_write", "ms_download", "ms_files", "ms_png")


class ModelStats(C.Structure):
    _fields_ = [("lines", C.c_uint64 * 5), ("bytes", C.c_uint64 * 5)] + [(k, C.c_uint64) for k in MODEL_COUNTS] + [(k, C.c_float) for k in MODEL_MS]


GLB_COUNTS = ("vertices", "indices", "primitives", "json_bytes", "geometry_bytes", "image_bytes", "file_bytes", "nonfinite_values")
GLB_MS = ("ms_keys", "ms_sort", "ms_number", "ms_indices", "ms_gather", "ms_png", "ms_download", "ms_file")


class GlbStats(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in GLB_COUNTS] + [(k, C.c_float) for k in GLB_MS]


GLB_QUANT_COUNTS = ("zero_normals", "texcoords_out_of_range", "index16_primitives")
GLB_QUANT_MS = ("ms_bounds",)


class GlbQuantStats(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in GLB_QUANT_COUNTS] + [(k, C.c_float) for k in GLB_QUANT_MS] + [("reserved", C.c_float)]


class Glb(C.Structure):
    _fields_ = [("n_bytes", C.c_uint64), ("data", C.c_void_p)]


class DcStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("pairs", "cull_backface", "cull_angle", "cull_outside", "cull_occluded",
                                           "cull_zero_quality", "nnz_pre", "nnz", "rays", "ray_nodes", "ray_tris", "ray_packets", "ray_packets_generic")] + \
               [("max_quality", C.c_float), ("percentile", C.c_float), ("footprints_lane_group", C.c_uint64), ("footprints_rewalked", C.c_uint64), ("ray_leaf_rounds", C.c_uint64)]


PNG_COUNTS = ("raw_bytes", "png_bytes", "chunks", "stored_chunks")
PNG_MS = ("ms_filter", "ms_chunk", "ms_gather", "ms_download", "ms_frame")


class PngStats(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in PNG_COUNTS] + [("filter_rows", C.c_uint64 * 5)] + [(k, C.c_float) for k in PNG_MS] + [("reserved", C.c_float)]


JPEG_COUNTS = ("raw_bytes", "jpeg_bytes", "segments", "stuffed_bytes", "marker_bytes")
JPEG_MS = ("ms_segment", "ms_gather", "ms_download", "ms_frame")
IMAGE_FORMATS = {"png": 0, "jpeg": 1}


class JpegStats(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in JPEG_COUNTS] + [(k, C.c_float) for k in JPEG_MS]


JPEGDEC_COUNTS = ("files", "file_bytes", "entropy_bytes", "stuffed_bytes", "restart_segments", "subsequences", "windows", "sync_rounds_max", "sync_launches",
                  "subseq_exact_after_pass1", "blocks", "batches")
JPEGDEC_MS = ("ms_upload", "ms_unstuff", "ms_sync", "ms_decode", "ms_idct", "ms_colour")


class JpegDecParams(C.Structure):
    _fields_ = [("max_scratch_bytes", C.c_uint64), ("reserved", C.c_uint64)]


class JpegDecStats(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in JPEGDEC_COUNTS] + [(k, C.c_float) for k in JPEGDEC_MS]


PNGDEC_COUNTS = ("files", "file_bytes", "idat_chunks", "zlib_bytes", "raw_bytes", "stored_blocks", "fixed_blocks", "dynamic_blocks")
PNGDEC_MS = ("ms_upload", "ms_inflate", "ms_adler", "ms_unfilter")
PNGDEC_UNFILTER_BAND = 64      # rows of one band of png_unfilter_kernel (csrc/png_dec.h UNFILTER_BAND)
PNGDEC_UNFILTER_SEGMENT = 64   # pixels of a row it stages in LDS at a time (UNFILTER_SEGMENT)


class PngDecStats(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in PNGDEC_COUNTS] + [("filter_rows", C.c_uint64 * 5), ("batches", C.c_uint64)] + [(k, C.c_float) for k in PNGDEC_MS]


def _png_stats_dict(s):
    d = _stats_dict(s)
    d["filter_rows"] = list(s.filter_rows)
    return d


LENS_COUNTS = ("views_undistorted", "views_copied", "pixels", "pixels_no_source", "staging_bytes", "batches")
LENS_MS = ("ms_upload", "ms_undistort")


class Lens(C.Structure):
    _fields_ = [("flen", C.c_float), ("dist0", C.c_float), ("dist1", C.c_float), ("reserved", C.c_uint32)]


class LensStats(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in LENS_COUNTS] + [(k, C.c_float) for k in LENS_MS]


LEVEL_COUNTS = ("views_halved", "pixels_in", "pixels_out", "pixels_no_source", "batches", "staging_bytes")
LEVEL_MS = ("ms_upload", "ms_halve")
LEVEL_MAX = 4


class ViewLevel(C.Structure):
    _fields_ = [("level", C.c_uint32), ("src_width", C.c_int32), ("src_height", C.c_int32), ("reserved", C.c_uint32)]


class LevelStats(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in LEVEL_COUNTS] + [(k, C.c_float) for k in LEVEL_MS]


def _levels_list(levels, n):
    """`levels` of the set_views* calls -- an int or one int per view, or (n, 2) rows with the reserved word, which must be 0 -- as two
    lists of n ints: the levels and the reserved words"""
    if np.ndim(levels) == 0:
        return [int(levels)] * n, [0] * n
    a = np.asarray(levels, dtype=np.int64).reshape(len(levels), -1)
    assert a.shape[0] == n and a.shape[1] in (1, 2), "levels: %s for %d views" % (a.shape, n)
    return a[:, 0].tolist(), (a[:, 1].tolist() if a.shape[1] == 2 else [0] * n)


MASK_COUNTS = ("views_masked", "views_undistorted", "pixels", "pixels_masked_out", "device_bytes", "staging_bytes", "batches")
MASK_MS = ("ms_upload", "ms_pack", "ms_undistort")


class MaskStats(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in MASK_COUNTS] + [(k, C.c_float) for k in MASK_MS]


def _lens_array(lens, n):
    """an (n, 3) array of (flen, dist0, dist1) -- or (n, 4) with the reserved word, which must be 0 -- as the ABI's mvs_lens [n]"""
    a = np.asarray(lens, dtype=np.float32).reshape(n, -1) if n else np.zeros((0, 3), np.float32)
    assert a.shape[1] in (3, 4)
    arr = (Lens * max(n, 1))()
    for j in range(n):
        arr[j].flen, arr[j].dist0, arr[j].dist1 = float(a[j, 0]), float(a[j, 1]), float(a[j, 2])
        arr[j].reserved = int(a[j, 3]) if a.shape[1] == 4 else 0
    return arr


class RgbSet(C.Structure):
    _fields_ = [("n_images", C.c_uint32), ("on_device", C.c_uint32), ("n_bytes", C.c_uint64), ("data", C.c_void_p), ("offsets", C.c_void_p), ("width", C.c_void_p), ("height", C.c_void_p)]


class PngSet(C.Structure):
    _fields_ = [("n_images", C.c_uint32), ("reserved", C.c_uint32), ("n_bytes", C.c_uint64), ("data", C.c_void_p), ("offsets", C.c_void_p)]


def _stats_dict(s):
    return {f[0]: getattr(s, f[0]) for f in s._fields_}


def lib_path():
    return _LIB_PATH


def blocks_lib_path():
    return _BLOCKS_PATH


# entry points of include/mvs_viewsel_blocks.h (libmvs_blocks.so), everything else is the product library's
BLOCK_SYMBOLS = frozenset((
    "mvs_ctx_dc_get_max", "mvs_ctx_dc_set_max", "mvs_ctx_dc_get_histogram", "mvs_ctx_dc_set_histogram", "mvs_ctx_costs_export",
    "mvs_ctx_mrf_setup", "mvs_ctx_mrf_setup_marked", "mvs_ctx_mrf_sweep", "mvs_ctx_mrf_sweep_phase", "mvs_ctx_mrf_sweep_phase_part", "mvs_ctx_mrf_layout", "mvs_ctx_mrf_gather", "mvs_ctx_mrf_scatter",
    "mvs_ctx_mrf_energy", "mvs_ctx_mrf_keep_best", "mvs_ctx_mrf_step", "mvs_ctx_mrf_poll", "mvs_ctx_mrf_icm_gain", "mvs_ctx_mrf_icm_apply",
    "mvs_ctx_mrf_labels", "mvs_ctx_mrf_setup_tables", "mvs_ctx_ray_bits", "mvs_ctx_prep_products", "mvs_ctx_costs_upload_ordered", "mvs_ctx_tone_table", "mvs_ctx_view_image", "mvs_ctx_view_keep_words"))

TONE_MAPPINGS = {"none": 0, "gamma": 1}                                       # tex::ToneMapping (settings.h); the *_params.tone_mapping field


_lib = None


def load_library():
    """Loads the HIP library.  Raises if it has not been built: there is no fallback."""
    global _lib
    if _lib is not None:
        return _lib
    try:
        # When torch is installed, load it first: it ships its own HIP runtime (same soname as the system
        # one) and the process must end up with a single runtime shared by torch and this library.
        import torch  # noqa: F401
    except ImportError:
        pass
    if not os.path.exists(_LIB_PATH):
        raise MvsError(-1, "HIP library %s is missing: run `python mvs-texturing_amd/build.py` "
                           "(or __graft_entry__.build()); there is no CPU fallback" % _LIB_PATH)
    L = C.CDLL(_LIB_PATH)
    L.mvs_last_error.restype = C.c_char_p
    L.mvs_status_string.restype = C.c_char_p
    L.mvs_last_call_profile.restype = C.c_char_p
    vp, u32, u64, i32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int
    sig = {
        "mvs_mrf_default_params": [C.POINTER(MrfParams)], "mvs_default_settings": [C.POINTER(Settings)],
        "mvs_data_costs": [C.POINTER(CMesh), C.POINTER(CView), u32, C.POINTER(Settings), C.POINTER(CCsr), C.POINTER(DcStats)],
        "mvs_csr_free": [C.POINTER(CCsr)], "mvs_subgraphs_free": [C.POINTER(Subgraphs)],
        "mvs_view_selection": [C.POINTER(CCsr), vp, vp, C.POINTER(MrfParams), vp, C.POINTER(MrfStats)],
        "mvs_write_spt": [C.POINTER(CCsr), C.c_char_p], "mvs_read_spt": [C.c_char_p, C.POINTER(CCsr)],
        "mvs_write_labeling_vec": [vp, u32, C.c_char_p],
        "mvs_prepare_mesh": [u32, vp, u32, vp, vp, vp, C.POINTER(u32)],
        "mvs_build_adjacency_graph": [u32, u32, vp, vp, C.POINTER(vp), C.POINTER(u64)],
        "mvs_ctx_build_adjacency": [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(u64)],
        "mvs_get_subgraphs": [u32, vp, vp, vp, u32, C.POINTER(Subgraphs)],
        "mvs_ctx_get_subgraphs": [vp, u32, vp, vp, i32, vp, i32, u32, C.POINTER(Subgraphs), i32],
        "mvs_ctx_create": [i32, C.POINTER(vp)], "mvs_ctx_destroy": [vp], "mvs_ctx_set_stream": [vp, vp],
        "mvs_ctx_synchronize": [vp], "mvs_set_option": [vp, C.c_char_p, C.c_int64],
        "mvs_ctx_get_profile": [vp, C.c_char_p, C.c_size_t],
        "mvs_scene_set_mesh": [vp, C.POINTER(CMesh), i32], "mvs_scene_set_views": [vp, C.POINTER(CView), u32, i32],
        "mvs_scene_set_face_range": [vp, u32, u32],
        "mvs_ctx_data_costs": [vp, C.POINTER(Settings), C.POINTER(DcStats)], "mvs_ctx_dc_ranges": [vp, C.POINTER(u32), C.POINTER(u32)],
        "mvs_ctx_dc_phase1": [vp, C.POINTER(Settings)], "mvs_ctx_dc_get_max": [vp, vp], "mvs_ctx_dc_set_max": [vp, vp],
        "mvs_ctx_dc_phase2": [vp], "mvs_ctx_dc_get_histogram": [vp, vp], "mvs_ctx_dc_set_histogram": [vp, vp],
        "mvs_ctx_dc_phase3": [vp, C.POINTER(DcStats)],
        "mvs_ctx_costs_device": [vp, C.POINTER(CCsr)], "mvs_ctx_costs_download": [vp, C.POINTER(CCsr), C.POINTER(vp)],
        "mvs_ctx_costs_upload": [vp, C.POINTER(CCsr), i32], "mvs_ctx_costs_export": [vp, vp, vp, vp],
        "mvs_ctx_view_selection": [vp, vp, vp, i32, C.POINTER(MrfParams), vp, i32, C.POINTER(MrfStats)],
        "mvs_ctx_mrf_setup": [vp, vp, vp, i32, C.POINTER(MrfParams)], "mvs_ctx_mrf_sweep": [vp, u32, u32],
        "mvs_ctx_mrf_setup_marked": [vp, vp, vp, i32, C.POINTER(MrfParams), vp], "mvs_ctx_mrf_sweep_phase_part": [vp, u32, u32, u32, i32],
        "mvs_ctx_mrf_num_phases": [vp, C.POINTER(u32)], "mvs_ctx_mrf_diagnostics": [vp, C.POINTER(u32)], "mvs_ctx_mrf_sweep_phase": [vp, u32, u32, u32], "mvs_ctx_mrf_layout": [vp, vp, u64],
        "mvs_ctx_mrf_gather": [vp, i32, vp, u64, vp], "mvs_ctx_mrf_scatter": [vp, i32, vp, u64, vp],
        "mvs_ctx_mrf_energy": [vp, i32, u32, u32, vp], "mvs_ctx_mrf_keep_best": [vp],
        "mvs_ctx_mrf_step": [vp, vp], "mvs_ctx_mrf_poll": [vp, u32, C.POINTER(MrfProgress)],
        "mvs_ctx_mrf_icm_gain": [vp, u32, u32], "mvs_ctx_mrf_icm_apply": [vp, u32, u32, vp],
        "mvs_ctx_mrf_labels": [vp, u32, u32, vp, C.POINTER(u32)],
        "mvs_ctx_mrf_setup_tables": [vp, i32, vp, u64, C.POINTER(u64)],
        "mvs_ctx_ray_bits": [vp, i32, vp, u64, C.POINTER(u64)],
        "mvs_ctx_prep_products": [vp, i32, u32, vp, u64, C.POINTER(u64)],
        "mvs_ctx_costs_upload_ordered": [vp, C.POINTER(CCsr), vp],
        "mvs_ctx_tone_table": [vp, vp],
        "mvs_ctx_view_image": [vp, u32, vp, u64, C.POINTER(u64)], "mvs_ctx_view_keep_words": [vp, u32, vp, u64, C.POINTER(u64)],
        "mvs_scene_set_view_masks": [vp, vp, u32, i32, C.POINTER(Lens), C.POINTER(MaskStats)],
        "mvs_gamma_correct": [vp, u64, C.c_float], "mvs_ctx_gamma_correct": [vp, vp, u64, C.c_float, i32], "mvs_tone_table": [u32, vp],
        "mvs_ctx_prune_labels": [vp, u32], "mvs_undistort_image": [vp, C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_float, vp],
        "mvs_postprocess_face_infos": [u32, u32, vp, vp, vp, vp, C.POINTER(Settings), C.POINTER(CCsr), C.POINTER(DcStats)],
        "mvs_comm_unique_id": [vp], "mvs_comm_create_rccl": [i32, i32, i32, vp, C.POINTER(vp)], "mvs_comm_create_local": [i32, C.POINTER(vp)], "mvs_comm_create_local_devices": [i32, vp, C.POINTER(vp)],
        "mvs_comm_info": [vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)],
        "mvs_comm_destroy": [vp], "mvs_comm_abort": [vp], "mvs_shard_create": [vp, vp, vp, vp, vp, C.POINTER(vp)], "mvs_shard_destroy": [vp],
        "mvs_shard_data_costs": [vp, C.POINTER(Settings), C.POINTER(DcStats), C.POINTER(u64)],
        "mvs_shard_view_selection": [vp, C.POINTER(MrfParams), vp, C.POINTER(MrfStats)],
        "mvs_shard_plan_info": [vp, C.POINTER(u64), C.POINTER(u64), C.POINTER(C.c_double)],
        "mvs_shard_transport_info": [vp, C.POINTER(i32), C.POINTER(u64), C.POINTER(i32), C.POINTER(u32)],
        "mvs_shard_own_faces": [vp, vp, C.POINTER(u32)],
        "mvs_ctx_partition_faces": [vp, i32, vp, vp], "mvs_partition_faces": [C.POINTER(CMesh), i32, vp, vp],
        "mvs_ctx_table_order": [vp, vp, C.POINTER(i32)],
        "mvs_gsl_default_params": [C.POINTER(GslParams)], "mvs_gsl_result_free": [C.POINTER(GslResult)], "mvs_gsl_system_free": [C.POINTER(GslSystem)],
        "mvs_ctx_global_seam_leveling": [vp, vp, vp, i32, vp, i32, C.POINTER(GslParams), C.POINTER(GslResult), i32, C.POINTER(GslStats)],
        "mvs_ctx_gsl_system": [vp, C.POINTER(GslSystem)],
        "mvs_patch_default_params": [C.POINTER(PatchParams)], "mvs_patch_set_free": [C.POINTER(PatchSet)],
        "mvs_ctx_texture_patches": [vp, vp, vp, i32, vp, i32, vp, i32, C.POINTER(PatchParams), C.POINTER(PatchSet), i32, C.POINTER(PatchStats)],
        "mvs_lsl_default_params": [C.POINTER(LslParams)], "mvs_lsl_result_free": [C.POINTER(LslResult)],
        "mvs_ctx_local_seam_leveling": [vp, vp, vp, i32, vp, i32, C.POINTER(PatchSet), i32, C.POINTER(LslParams), C.POINTER(LslResult), i32, C.POINTER(LslStats)],
        "mvs_atlas_default_params": [C.POINTER(AtlasParams)], "mvs_atlas_set_free": [C.POINTER(AtlasSet)],
        "mvs_ctx_texture_atlases": [vp, C.POINTER(PatchSet), i32, C.POINTER(AtlasParams), C.POINTER(AtlasSet), i32, C.POINTER(AtlasStats)],
        "mvs_model_default_params": [C.POINTER(ModelParams)], "mvs_model_text_free": [C.POINTER(ModelText)],
        "mvs_ctx_build_model": [vp, C.POINTER(AtlasSet), i32, vp, i32, C.c_char_p, C.POINTER(ModelParams), C.POINTER(ModelText), i32, C.POINTER(ModelStats)],
        "mvs_ctx_save_model": [vp, C.POINTER(AtlasSet), i32, vp, i32, C.c_char_p, C.POINTER(ModelParams), C.POINTER(ModelStats)],
        "mvs_write_png": [C.c_char_p, vp, u32, u32, C.c_int32],
        "mvs_ctx_build_glb": [vp, C.POINTER(AtlasSet), i32, vp, i32, C.POINTER(ModelParams), C.POINTER(Glb), C.POINTER(GlbStats)],
        "mvs_ctx_save_glb": [vp, C.POINTER(AtlasSet), i32, vp, i32, C.c_char_p, C.POINTER(ModelParams), C.POINTER(GlbStats)], "mvs_glb_free": [C.POINTER(Glb)],
        "mvs_ctx_glb_quant_stats": [vp, C.POINTER(GlbQuantStats)],
        "mvs_ctx_encode_pngs": [vp, u32, vp, vp, vp, vp, i32, C.POINTER(PngSet), C.POINTER(PngStats)], "mvs_png_set_free": [C.POINTER(PngSet)],
        "mvs_ctx_deflate_rle": [vp, vp, u64, i32, C.POINTER(vp), C.POINTER(u64)], "mvs_png_free": [vp],
        "mvs_ctx_encode_jpegs": [vp, u32, vp, vp, vp, vp, i32, C.c_int32, C.c_int32, C.POINTER(PngSet), C.POINTER(JpegStats)], "mvs_jpeg_set_free": [C.POINTER(PngSet)],
        "mvs_encode_jpeg": [vp, u32, u32, C.c_int32, C.c_int32, C.POINTER(vp), C.POINTER(u64)], "mvs_jpeg_free": [vp],
        "mvs_jpegdec_default_params": [C.POINTER(JpegDecParams)], "mvs_rgb_set_free": [C.POINTER(RgbSet)],
        "mvs_ctx_decode_jpegs": [vp, vp, vp, u32, C.POINTER(JpegDecParams), i32, C.POINTER(RgbSet), C.POINTER(JpegDecStats)],
        "mvs_scene_set_views_jpeg": [vp, C.POINTER(CView), u32, vp, vp, C.POINTER(JpegDecParams), C.POINTER(JpegDecStats)],
        "mvs_jpeg_probe": [vp, u64, C.POINTER(u32), C.POINTER(u32)],
        "mvs_decode_jpeg": [vp, u64, C.POINTER(vp), C.POINTER(u32), C.POINTER(u32), C.POINTER(vp), C.POINTER(u64)],
        "mvs_ctx_decode_pngs": [vp, vp, vp, u32, C.POINTER(JpegDecParams), i32, C.POINTER(RgbSet), C.POINTER(PngDecStats)],
        "mvs_png_probe": [vp, u64, C.POINTER(u32), C.POINTER(u32)],
        "mvs_decode_png": [vp, u64, C.POINTER(vp), C.POINTER(u32), C.POINTER(u32), C.POINTER(vp)],
        "mvs_scene_set_views_files": [vp, C.POINTER(CView), u32, C.POINTER(Lens), vp, vp, C.POINTER(JpegDecParams), C.POINTER(JpegDecStats), C.POINTER(PngDecStats), C.POINTER(LensStats)],
        "mvs_scene_set_views_lens": [vp, C.POINTER(CView), u32, C.POINTER(Lens), vp, vp, C.POINTER(JpegDecParams), C.POINTER(JpegDecStats), C.POINTER(LensStats)],
        "mvs_ctx_undistort_images": [vp, vp, vp, vp, C.POINTER(Lens), u32, i32, C.POINTER(RgbSet), C.POINTER(LensStats)],
        "mvs_undistort_image_host": [vp, C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_float, vp],
        "mvs_scene_set_views_levels": [vp, C.POINTER(CView), u32, C.POINTER(ViewLevel), C.POINTER(Lens), vp, vp, C.POINTER(JpegDecParams), C.POINTER(JpegDecStats), C.POINTER(LensStats),
                                       C.POINTER(PngDecStats), C.POINTER(LevelStats)],
        "mvs_ctx_halve_images": [vp, vp, vp, vp, vp, C.POINTER(Lens), u32, i32, C.POINTER(RgbSet), C.POINTER(LevelStats)],
        "mvs_halve_image_host": [vp, C.c_int32, C.c_int32, u32, vp], "mvs_level_size": [C.c_int32, C.c_int32, u32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)],
        "mvs_encode_png_rle": [vp, u32, u32, C.POINTER(vp), C.POINTER(u64)], "mvs_deflate_rle": [vp, u64, C.POINTER(vp), C.POINTER(u64)],
        "mvs_debug_view_style": [u32, vp, vp], "mvs_ctx_debug_embeddings": [vp, u32, vp, vp, vp, u32, vp, i32],
        "mvs_ctx_debug_patches": [vp, vp, vp, i32, vp, i32, vp, C.POINTER(PatchParams), C.POINTER(PatchSet), i32, C.POINTER(PatchStats)],
        "mvs_ctx_view_selection_model": [vp, vp, vp, i32, vp, i32, vp, vp, i32, C.c_char_p, C.POINTER(PatchParams), C.POINTER(AtlasParams), C.POINTER(ModelParams),
                                         C.POINTER(PatchStats), C.POINTER(AtlasStats), C.POINTER(ModelStats)],
        "mvs_data_costs_stream": [C.POINTER(CMesh), C.POINTER(CView), u32, C.POINTER(Settings), vp, vp, C.POINTER(CCsr), C.POINTER(DcStats)],
        "mvs_view_selection_cached": [u64, u32, u32, u64, vp, vp, C.POINTER(MrfParams), vp, C.POINTER(MrfStats)],
    }
    # The per-phase building blocks (include/mvs_viewsel_blocks.h) live in a library of their own, libmvs_blocks.so -- the harness of
    # the CPU multi-process tests (tests/tools/multigpu.py) and a few measuring scripts use them, the product does not.  Their entry points are
    # attached to the same handle; without that library (a variant build, a product-only install) they are simply absent.
    blocks = None
    if os.path.exists(_BLOCKS_PATH):
        try:
            blocks = C.CDLL(_BLOCKS_PATH, mode=C.RTLD_GLOBAL)
        except OSError:
            blocks = None
    L._blocks_declared = []
    for name, argtypes in sig.items():
        if name in BLOCK_SYMBOLS:
            if blocks is None:
                continue
            fn = getattr(blocks, name)
            setattr(L, name, fn)
            L._blocks_declared.append(name)
        else:
            fn = getattr(L, name)
        fn.argtypes = argtypes
        if name not in ("mvs_mrf_default_params", "mvs_default_settings", "mvs_csr_free", "mvs_subgraphs_free", "mvs_gsl_default_params",
                        "mvs_gsl_result_free", "mvs_gsl_system_free", "mvs_patch_default_params", "mvs_patch_set_free", "mvs_lsl_default_params", "mvs_lsl_result_free", "mvs_atlas_default_params", "mvs_atlas_set_free", "mvs_model_default_params", "mvs_model_text_free", "mvs_glb_free", "mvs_png_set_free", "mvs_png_free", "mvs_jpeg_set_free", "mvs_jpeg_free", "mvs_jpegdec_default_params", "mvs_rgb_set_free", "mvs_ctx_destroy", "mvs_comm_destroy", "mvs_comm_abort", "mvs_shard_destroy"):
            fn.restype = C.c_int
    L._declared = sorted([k for k in sig.keys() if k not in BLOCK_SYMBOLS] + ["mvs_last_error", "mvs_status_string"])
    L._blocks = blocks
    _lib = L
    return L


def _check(L, st):
    if st != 0:
        raise MvsError(st, L.mvs_last_error().decode() or L.mvs_status_string(st).decode())


def _is_torch(a):
    return type(a).__module__.startswith("torch")


class DevArray:
    """A raw device array owned by the library (pointer + length), accepted wherever a CUDA tensor is."""
    is_cuda = True

    def __init__(self, ptr, n):
        self.ptr, self.shape = int(ptr or 0), (int(n),)

    def data_ptr(self):
        return self.ptr

    def is_contiguous(self):
        return True


def _ptr(a):
    """(pointer, on_device) of a numpy array or torch tensor."""
    if a is None:
        return None, 0
    if _is_torch(a) or isinstance(a, DevArray):
        assert a.is_contiguous()
        return C.c_void_p(a.data_ptr()), 1 if a.is_cuda else 0
    assert a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(C.c_void_p), 0


def _default_params(cls, fn_name, kw):
    """the library's defaults of a parameter struct with overrides"""
    p = cls()
    getattr(load_library(), fn_name)(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def default_mrf_params(**kw):
    return _default_params(MrfParams, "mvs_mrf_default_params", kw)


def _check_with_stats(L, rc, stats):
    """_check for the calls that fill their stats before they refuse: the MvsError carries them as `.stats`"""
    try:
        _check(L, rc)
    except MvsError as e:
        e.stats = stats
        raise


def _download(res, shapes, free_fn):
    """the arrays {name: (count, dtype)} of a result struct: DevArrays owned by the context (free_fn None: the call left them on the
    device), else flat host copies, after which free_fn releases the library's own"""
    if free_fn is None:
        return {k: DevArray(getattr(res, k), n) for k, (n, _) in shapes.items()}
    out = {}
    for k, (n, dt) in shapes.items():
        out[k] = np.frombuffer(C.string_at(getattr(res, k), n * np.dtype(dt).itemsize), dt).copy() if n else np.zeros(0, dt)
    free_fn(C.byref(res))
    return out


def _patch_set_struct(patches, dts):
    """the arrays `dts` ({name: dtype}) of a patch-set dict as a PatchSet: (ps, held, on_device) -- all host arrays (made contiguous and
    flat; `held` keeps them alive) or all DevArrays / CUDA tensors; n_patches is counted on box, which every row reads"""
    dev = [_is_torch(patches[k]) or isinstance(patches[k], DevArray) for k in dts]
    assert all(dev) or not any(dev), "the patch set must be all host or all device arrays"
    on_device = dev[0]
    held = {k: patches[k] if on_device else np.ascontiguousarray(patches[k], dts[k]).reshape(-1) for k in dts}
    count = lambda x: int(x.numel()) if _is_torch(x) else int(x.shape[0])   # tensors of any shape, DevArrays and flat numpy arrays alike
    ps = PatchSet()
    ps.n_patches = count(held["box"]) // 4; ps.n_listed = count(held["faces"]); ps.n_pixels = count(held["validity"])
    for k in dts:
        setattr(ps, k, _ptr(held[k])[0] if (on_device or held[k].size) else None)
    return ps, held, 1 if on_device else 0


class DataCosts:
    """tex::DataCosts (SparseTable<u32,u16,float>, libs/tex/sparse_table.h) as CSR by face."""

    def __init__(self, n_faces, n_views, col_ptr, view_id, cost, quality=None):
        self.n_faces, self.n_views = int(n_faces), int(n_views)
        self.col_ptr, self.view_id, self.cost, self.quality = col_ptr, view_id, cost, quality

    cols = property(lambda self: self.n_faces)   # SparseTable::cols()
    rows = property(lambda self: self.n_views)   # SparseTable::rows()

    @property
    def nnz(self):
        return int(self.col_ptr[-1])

    def col(self, i):
        """SparseTable::col(i): list of (view_id, cost)"""
        a, b = int(self.col_ptr[i]), int(self.col_ptr[i + 1])
        return list(zip(self.view_id[a:b].tolist(), self.cost[a:b].tolist()))

    def _struct(self):
        s = CCsr(self.n_faces, self.n_views, self.nnz, 0, 0, 0)
        s.col_ptr, dev0 = _ptr(self.col_ptr)
        s.view_id, dev1 = _ptr(self.view_id)
        s.cost, dev2 = _ptr(self.cost)
        assert dev0 == dev1 == dev2
        return s, dev0

    def save_to_file(self, path):
        """SparseTable::save_to_file (libs/tex/sparse_table.h:112-136)"""
        L = load_library()
        s, dev = self._struct()
        assert not dev, "download first"
        _check(L, L.mvs_write_spt(C.byref(s), path.encode()))


class PrepProducts:
    """One view's image-preparation products as read back by Context.prep_products: gmi (uint8 (h, w) or None), mask_words and summary_words
    (uint32, rows as the device pads them)."""

    def __init__(self, width, height, gmi, mask_words, summary_words):
        self.width, self.height, self.gmi, self.mask_words, self.summary_words = width, height, gmi, mask_words, summary_words

    def mask_bits(self):
        """(valid bool (h, w), padding bool (h, 32 * mask_stride - w)): bit x & 31 of word (y, x >> 5) is pixel (x, y)"""
        bits = np.unpackbits(np.ascontiguousarray(self.mask_words).view(np.uint8).reshape(self.height, -1), axis=1, bitorder="little").astype(bool)
        return bits[:, :self.width], bits[:, self.width:]

    def summary_bits(self):
        """(tiles bool (ceil(h / 32), mask_stride), padding bool: the bits of tile columns >= mask_stride)"""
        bits = np.unpackbits(np.ascontiguousarray(self.summary_words).view(np.uint8).reshape(self.summary_words.shape[0], -1), axis=1, bitorder="little").astype(bool)
        ms = self.mask_words.shape[1]
        return bits[:, :ms], bits[:, ms:]


class Context:
    """Resident scene + results on one GPU (mvs_ctx)."""

    def __init__(self, device=0):
        self.L = load_library()
        h = C.c_void_p()
        _check(self.L, self.L.mvs_ctx_create(device, C.byref(h)))
        self.h = h
        self.device = int(device)
        self._keep = {}

    def close(self):
        if getattr(self, "h", None):
            self.L.mvs_ctx_destroy(self.h)
            self.h = None

    __del__ = close

    def set_stream(self, stream_handle):
        _check(self.L, self.L.mvs_ctx_set_stream(self.h, C.c_void_p(stream_handle)))

    def synchronize(self):
        _check(self.L, self.L.mvs_ctx_synchronize(self.h))

    def set_option(self, name, value):
        _check(self.L, self.L.mvs_set_option(self.h, name.encode(), int(value)))

    def get_profile(self):
        """{"stage": [total_ms, launches]} since the last call (needs set_option("profile", 1))"""
        import json
        buf = C.create_string_buffer(1 << 16)
        _check(self.L, self.L.mvs_ctx_get_profile(self.h, buf, len(buf)))
        return json.loads(buf.value.decode())

    def set_mesh(self, verts, faces, normals):
        pv, d0 = _ptr(verts); pf, d1 = _ptr(faces); pn, d2 = _ptr(normals)
        assert d0 == d1 == d2
        m = CMesh(int(verts.shape[0]), int(faces.shape[0]), pv, pf, pn)
        self._keep["mesh"] = (verts, faces, normals)
        self.n_faces = int(faces.shape[0])
        _check(self.L, self.L.mvs_scene_set_mesh(self.h, C.byref(m), d0))

    def set_views(self, cams, images, lens=None, masks=None, levels=None):
        """cams: dict of arrays pos, viewdir, K, w2c, width, height; images: list of (H,W,3) u8 numpy / torch cuda.
        levels: an int or one int per view, 0 .. 4 -- set_views_files(cams, [None] * V, images=images, ..., levels=levels): the images are host
        arrays at the SOURCE's size, cams describe the views at their level (mvs_scene_set_views_levels; returns its stats dict).
        lens: an (n, 3) float32 array of (flen, dist0, dist1) per view -- the images are then host arrays as the camera took them, and the
        views with dist0 != 0 are undistorted on the device (mvs_scene_set_views_lens; returns the lens stats).
        masks: set_view_masks(masks, lens=lens) behind the views (its stats: self.mask_stats).
        A refused call raises MvsError and leaves the context without views (n_views == 0): data_costs then raises status 6 until a
        set_views* succeeds."""
        V = len(images)
        if levels is not None:
            return self.set_views_files(cams, [None] * V, images=images, lens=lens, masks=masks, levels=levels)
        if lens is not None:
            st = self._set_views_files(cams, [None] * V, images, lens, None)["lens"]
            if masks is not None:
                self.set_view_masks(masks, lens=lens)
            return st
        self._set_views_plain(cams, images)
        if masks is not None:
            self.set_view_masks(masks)

    def _set_views_plain(self, cams, images):
        V = len(images)
        arr = self._view_array(cams, V)
        dev = None
        for j in range(V):
            arr[j].rgb, d = _ptr(images[j])
            assert dev is None or dev == d
            dev = d
        rc = self.L.mvs_scene_set_views(self.h, arr, V, dev or 0)
        self._views_set(V, cams, rc, images)
        _check(self.L, rc)

    def _view_array(self, cams, V):
        arr = (CView * V)()
        for j in range(V):
            v = arr[j]
            v.pos[:] = np.asarray(cams["pos"][j], dtype=np.float32).tolist()
            v.viewdir[:] = np.asarray(cams["viewdir"][j], dtype=np.float32).tolist()
            v.K[:] = np.asarray(cams["K"][j], dtype=np.float32).ravel().tolist()
            v.w2c[:] = np.asarray(cams["w2c"][j], dtype=np.float32).ravel().tolist()
            v.width, v.height = int(cams["width"][j]), int(cams["height"][j])
        return arr

    def _views_set(self, V, cams, rc, held=None):
        """the bookkeeping behind every set_views*: the V views of cams (`held` keeps their images alive), or none after a refusal (rc != 0)"""
        ok = rc == 0
        self._keep["views"] = held if ok else None
        self._view_sizes = [(int(cams["width"][j]), int(cams["height"][j])) for j in range(V)] if ok else []
        self._mask_sizes = list(self._view_sizes)   # (set_views_files(levels=) puts the sources' sizes here)
        self.n_views = V if ok else 0

    @staticmethod
    def _pixel_views(arr, files, images, levels=None):
        """the views without a file bring host pixels: arr[j].rgb points into the returned arrays, which the caller holds during the call"""
        pixels = [None if f is not None else np.ascontiguousarray(images[j], np.uint8) for j, f in enumerate(files)]
        for j, px in enumerate(pixels):
            if px is not None:
                assert px.ndim == 3 and px.shape[2] == 3 and (levels is not None or px.shape == (arr[j].height, arr[j].width, 3))
                arr[j].rgb = px.ctypes.data_as(C.c_void_p)
        return pixels

    def _rgb_set_images(self, res, n, shapes, on_device):
        """an RgbSet as a list of (H, W, 3) uint8 arrays, or with on_device of (DevArray, H, W); shapes: every image's (H, W), None: the set's own"""
        off = np.frombuffer(C.string_at(res.offsets, 8 * (n + 1)), np.uint64)
        if shapes is None:
            shapes = list(zip(np.frombuffer(C.string_at(res.height, 4 * n), np.uint32).tolist(), np.frombuffer(C.string_at(res.width, 4 * n), np.uint32).tolist())) if n else []
        if on_device:
            out = [(DevArray(res.data + int(off[i]), int(off[i + 1] - off[i])), int(h), int(w)) for i, (h, w) in enumerate(shapes)]
        else:
            data = np.frombuffer(C.string_at(res.data, res.n_bytes), np.uint8)
            out = [data[int(off[i]):int(off[i + 1])].reshape(int(h), int(w), 3).copy() for i, (h, w) in enumerate(shapes)]
        self.L.mvs_rgb_set_free(C.byref(res))
        return out

    @staticmethod
    def _file_arrays(files):
        """a list of JPEG files (bytes) as the arrays of pointers and sizes the ABI takes; `held` keeps the bytes alive"""
        held = [None if f is None else bytes(f) for f in files]
        n = len(held)
        ptrs = (C.c_char_p * max(n, 1))(*held)
        sizes = (C.c_uint64 * max(n, 1))(*[0 if f is None else len(f) for f in held])
        return held, ptrs, sizes

    def _set_views_files(self, cams, files, images, lens, params):
        """mvs_scene_set_views_jpeg, or with lens mvs_scene_set_views_lens: the jpeg stats, with a lens the lens stats under "lens"; a refusal
        raises MvsError with them as `.stats`"""
        V = len(files)
        arr = self._view_array(cams, V)
        held, ptrs, sizes = self._file_arrays(files)
        pixels = self._pixel_views(arr, files, images)   # (held during the call)
        st, ls, pp = JpegDecStats(), LensStats(), C.byref(params) if params is not None else None
        if lens is None:
            rc = self.L.mvs_scene_set_views_jpeg(self.h, arr, V, ptrs, sizes, pp, C.byref(st))
        else:
            any_file = any(f is not None for f in files)
            rc = self.L.mvs_scene_set_views_lens(self.h, arr, V, _lens_array(lens, V), ptrs if any_file else None, sizes if any_file else None, pp, C.byref(st), C.byref(ls))
        stats = _stats_dict(st)
        if lens is not None:
            stats["lens"] = _stats_dict(ls)
        self._views_set(V, cams, rc)
        _check_with_stats(self.L, rc, stats)
        return stats

    def set_view_masks(self, masks, lens=None):
        """mvs_scene_set_view_masks: masks[j] is view j's mask -- an (H, W) uint8 host array or torch cuda tensor of the view's size, 0 = leave
        the pixel out, anything else = keep -- or None for a view without one (all of them host arrays or all of them device tensors).  A
        masked pixel is an invalid pixel and nothing else changes (DESIGN.md section 4 "View input").  After any set_views*, before
        data_costs; None or all None clears the masks, and so does every later set_views*.  lens: the (n, 3) array of set_views(lens=) --
        the masks of views with dist0 != 0 are then in the frame the camera took and are undistorted on the device.  The mask of a view that
        came with a pyramid level > 0 (set_views*(levels=)) has the SOURCE's size; the level keeps a pixel iff everything that went into it
        is kept.  Returns the stats
        (also self.mask_stats); a refusal raises MvsError with them as `.stats` and leaves the context without masks."""
        V = getattr(self, "n_views", 0)
        masks = [None] * V if masks is None else list(masks)
        n = len(masks)
        held, dev = [], None
        for j, m in enumerate(masks):
            if m is None:
                held.append(None)
                continue
            if _is_torch(m):
                assert m.is_cuda and m.is_contiguous() and str(m.dtype) == "torch.uint8"
                d = 1
            else:
                m = np.ascontiguousarray(m, np.uint8)
                d = 0
            assert dev is None or dev == d, "host and device masks in one call"
            dev = d
            if j < len(getattr(self, "_mask_sizes", [])):
                w, h = self._mask_sizes[j]
                assert tuple(m.shape) == (h, w), "view %d: the mask is %s, the view (at its source's size) %d x %d" % (j, tuple(m.shape), w, h)
            held.append(m)
        ptrs = (C.c_void_p * max(n, 1))(*[None if m is None else (m.data_ptr() if dev else m.ctypes.data) for m in held])
        if dev:
            import torch
            torch.cuda.synchronize(self.device)   # the library reads on the context's stream, torch wrote on its own
        st = MaskStats()
        rc = self.L.mvs_scene_set_view_masks(self.h, ptrs, n, dev or 0, _lens_array(lens, n) if lens is not None else None, C.byref(st))
        self.mask_stats = _stats_dict(st)
        _check_with_stats(self.L, rc, self.mask_stats)
        return self.mask_stats

    def view_keep_bits(self, j):
        """view j's keep bits as set_view_masks left them on the device, bool (H, W), and the padding bits of its words -- or None for a
        view without a mask (mvs_ctx_view_keep_words, building-blocks library; test harness only)"""
        n = C.c_uint64()
        _check(self.L, self.L.mvs_ctx_view_keep_words(self.h, j, None, 0, C.byref(n)))
        if not n.value:
            return None
        buf = np.empty(n.value // 4, np.uint32)
        _check(self.L, self.L.mvs_ctx_view_keep_words(self.h, j, buf.ctypes.data_as(C.c_void_p), n.value, C.byref(n)))
        w, h = self._view_sizes[j]
        bits = np.unpackbits(buf.view(np.uint8).reshape(h, -1), axis=1, bitorder="little").astype(bool)
        return bits[:, :w], bits[:, w:]

    def undistort_images(self, images, lens, on_device=False):
        """mvs_ctx_undistort_images: the lens route on its own -- `images` (a list of (H, W, 3) uint8 host arrays) with lens[i] = (flen, dist0,
        dist1), undistorted in one call.  Returns (images, stats): a list of (H, W, 3) uint8 arrays, or with on_device a list of
        (DevArray, H, W) into the context's buffer, valid until the context's next call.  The same bytes as undistort_image gives."""
        n = len(images)
        imgs = [np.ascontiguousarray(i, np.uint8) for i in images]
        assert all(i.ndim == 3 and i.shape[2] == 3 for i in imgs)
        ptrs = (C.c_void_p * max(n, 1))(*[i.ctypes.data for i in imgs])
        w = (C.c_uint32 * max(n, 1))(*[i.shape[1] for i in imgs]); h = (C.c_uint32 * max(n, 1))(*[i.shape[0] for i in imgs])
        res, st = RgbSet(), LensStats()
        rc = self.L.mvs_ctx_undistort_images(self.h, ptrs, w, h, _lens_array(lens, n), n, 1 if on_device else 0, C.byref(res), C.byref(st))
        stats = _stats_dict(st)
        _check_with_stats(self.L, rc, stats)
        return self._rgb_set_images(res, n, [i.shape[:2] for i in imgs], on_device), stats

    def view_image(self, j):
        """the context's image of view j as it lies on the device, (H, W, 3) uint8 (mvs_ctx_view_image, building-blocks library; test
        harness only)"""
        n = C.c_uint64()
        _check(self.L, self.L.mvs_ctx_view_image(self.h, j, None, 0, C.byref(n)))
        buf = np.empty(n.value, np.uint8)
        _check(self.L, self.L.mvs_ctx_view_image(self.h, j, buf.ctypes.data_as(C.c_void_p), n.value, C.byref(n)))
        w, h = self._view_sizes[j]
        return buf.reshape(h, w, 3)

    def set_views_jpeg(self, cams, files, params=None, images=None, lens=None, masks=None, levels=None):
        """mvs_scene_set_views_jpeg: set_views with the images taken from baseline JPEG files (a list of bytes), decoded on the device
        straight into the context's image buffers (DESIGN.md section 4 "View input").  The frames' sizes must be cams' width / height.
        A view whose entry in `files` is None brings its pixels as images[j], an (H, W, 3) uint8 host array.
        Returns the stats; a refusal raises MvsError with them as `.stats` and leaves the context without views (n_views == 0): data_costs
        then raises status 6 until a set_views* succeeds.
        lens: an (n, 3) float32 array of (flen, dist0, dist1) per view -- the views with dist0 != 0, files and pixels alike, are undistorted
        on the device (mvs_scene_set_views_lens); the stats then carry the lens stats under "lens".
        masks: set_view_masks(masks, lens=lens) behind the views (its stats: self.mask_stats).
        levels: set_views_files(..., levels=levels), which see (its stats dict comes back)."""
        if levels is not None:
            return self.set_views_files(cams, files, params=params, images=images, lens=lens, masks=masks, levels=levels)
        st = self._set_views_files(cams, files, images, lens, params)
        if masks is not None:
            self.set_view_masks(masks, lens=lens)
        return st

    def decode_jpegs(self, files, params=None, on_device=False):
        """mvs_ctx_decode_jpegs: the view input route on its own -- `files` (a list of bytes, baseline JPEG) decoded in one call.  Returns
        (images, stats): a list of (H, W, 3) uint8 arrays, or with on_device a list of (DevArray, H, W) into the context's buffer, valid
        until the context's next decode.  The same bytes as the host twin decode_jpeg gives."""
        n = len(files)
        held, ptrs, sizes = self._file_arrays(files)
        res, st = RgbSet(), JpegDecStats()
        rc = self.L.mvs_ctx_decode_jpegs(self.h, ptrs, sizes, n, C.byref(params) if params is not None else None, 1 if on_device else 0, C.byref(res), C.byref(st))
        stats = _stats_dict(st)
        _check_with_stats(self.L, rc, stats)
        return self._rgb_set_images(res, n, None, on_device), stats

    def decode_pngs(self, files, params=None, on_device=False):
        """mvs_ctx_decode_pngs: the PNG view input route on its own -- `files` (a list of bytes: 8-bit PNGs, not interlaced) inflated and
        unfiltered on the device in one call.  Returns (images, stats) as decode_jpegs does (params: default_jpegdec_params, for its
        max_scratch_bytes).  The same bytes as the host twin decode_png gives; a refusal raises MvsError with the stats as `.stats`."""
        n = len(files)
        held, ptrs, sizes = self._file_arrays(files)
        res, st = RgbSet(), PngDecStats()
        rc = self.L.mvs_ctx_decode_pngs(self.h, ptrs, sizes, n, C.byref(params) if params is not None else None, 1 if on_device else 0, C.byref(res), C.byref(st))
        stats = _png_stats_dict(st)
        _check_with_stats(self.L, rc, stats)
        return self._rgb_set_images(res, n, None, on_device), stats

    def set_views_files(self, cams, files, params=None, images=None, lens=None, masks=None, levels=None, src_sizes=None):
        """mvs_scene_set_views_files: set_views_jpeg whose files may also be PNGs -- a file that starts with the PNG signature is inflated and
        unfiltered on the device, any other file takes the JPEG route, an entry None brings its pixels as images[j].  lens and masks as
        set_views_jpeg.  Returns {"png": ..., "jpeg": ..., "lens": ...}, the three routes' stats; a refusal raises MvsError with them as
        `.stats` and leaves the context without views.
        levels: an int or one int per view, 0 .. 4 -- pyramid levels (mvs_scene_set_views_levels; DESIGN.md section 4 "View input" item 14):
        files and images come at the SOURCE's size and are decoded, undistorted and halved `level` times on the device, cams describe the
        views AT THEIR LEVEL (level_size of the source), masks have the source's size.  The stats then carry "level".  src_sizes: every
        view's source (width, height) where the caller knows better than the files' headers and the images' shapes.  None: this call
        without levels, untouched."""
        V = len(files)
        arr = self._view_array(cams, V)
        held, ptrs, sizes = self._file_arrays(files)
        pixels = self._pixel_views(arr, files, images, levels)   # (held during the call)
        jst, pst, ls, vs = JpegDecStats(), PngDecStats(), LensStats(), LevelStats()
        any_file = any(f is not None for f in files)
        la = _lens_array(lens, V) if lens is not None else None
        pp = C.byref(params) if params is not None else None
        if levels is None:
            rc = self.L.mvs_scene_set_views_files(self.h, arr, V, la, ptrs if any_file else None, sizes if any_file else None, pp, C.byref(jst), C.byref(pst), C.byref(ls))
            stats = {"png": _png_stats_dict(pst), "jpeg": _stats_dict(jst), "lens": _stats_dict(ls)}
        else:
            lv, reserved = _levels_list(levels, V)
            src = [self._source_size(held[j], pixels[j], arr[j], lv[j]) for j in range(V)] if src_sizes is None else [tuple(int(v) for v in s) for s in src_sizes]
            va = (ViewLevel * max(V, 1))()
            for j in range(V):
                va[j].level, va[j].src_width, va[j].src_height, va[j].reserved = lv[j], src[j][0], src[j][1], reserved[j]
            rc = self.L.mvs_scene_set_views_levels(self.h, arr, V, va, la, ptrs if any_file else None, sizes if any_file else None, pp, C.byref(jst), C.byref(ls), C.byref(pst), C.byref(vs))
            stats = {"png": _png_stats_dict(pst), "jpeg": _stats_dict(jst), "lens": _stats_dict(ls), "level": _stats_dict(vs)}
        self._views_set(V, cams, rc)
        if levels is not None and rc == 0:
            self._mask_sizes = src
        _check_with_stats(self.L, rc, stats)
        if masks is not None:
            self.set_view_masks(masks, lens=lens)
        return stats

    @staticmethod
    def _source_size(file, pixels, view, level):
        """(width, height) of a view's source: its pixels' shape, its file's header -- or, for a file no probe reads, the size the level
        implies, so that the library refuses the file in its own words"""
        if pixels is not None:
            return int(pixels.shape[1]), int(pixels.shape[0])
        return png_probe(file) or jpeg_probe(file) or (int(view.width) << level, int(view.height) << level)

    def halve_images(self, images, levels, lens=None, on_device=False):
        """mvs_ctx_halve_images: the level route on its own -- `images` (a list of (H, W, 3) uint8 host arrays) halved levels[i] times (an int:
        all alike), under lens[i] = (flen, dist0, dist1) undistorted first, in one call.  Returns (images, stats) as undistort_images does.
        The same bytes as halve_host (of undistort_host) gives."""
        n = len(images)
        imgs = [np.ascontiguousarray(i, np.uint8) for i in images]
        assert all(i.ndim == 3 and i.shape[2] == 3 for i in imgs)
        lv, _ = _levels_list(levels, n)
        ptrs = (C.c_void_p * max(n, 1))(*[i.ctypes.data for i in imgs])
        w = (C.c_uint32 * max(n, 1))(*[i.shape[1] for i in imgs]); h = (C.c_uint32 * max(n, 1))(*[i.shape[0] for i in imgs])
        la = (C.c_uint32 * max(n, 1))(*lv)
        res, st = RgbSet(), LevelStats()
        rc = self.L.mvs_ctx_halve_images(self.h, ptrs, w, h, la, _lens_array(lens, n) if lens is not None else None, n, 1 if on_device else 0, C.byref(res), C.byref(st))
        stats = _stats_dict(st)
        _check_with_stats(self.L, rc, stats)
        return self._rgb_set_images(res, n, None, on_device), stats

    def set_face_range(self, begin, end):
        """positions [begin, end) of the library's face order (the caller's ids with option face_order = 0)"""
        _check(self.L, self.L.mvs_scene_set_face_range(self.h, begin, end))

    def partition_faces(self, world=1):
        """the library's own face order of the resident mesh and its cut into `world` equal contiguous parts:
        (perm uint32[F]: perm[p] = the caller's id of the face at position p, part_begin uint32[world + 1])"""
        import torch
        F = self.n_faces
        perm = torch.zeros(max(F, 1), dtype=torch.int32, device="cuda:%d" % self.device)
        torch.cuda.synchronize(self.device)   # the library writes on the context's stream, torch filled on its own
        part = np.zeros(world + 1, dtype=np.uint32)
        _check(self.L, self.L.mvs_ctx_partition_faces(self.h, int(world), C.c_void_p(perm.data_ptr()), part.ctypes.data_as(C.c_void_p)))
        return perm.cpu().numpy().view(np.uint32)[:F].copy(), part

    def table_order(self):
        """uint32[F]: the caller's face id of every column of the resident table as the library keeps it, or None (caller's order);
        after set_face_range(b, e) only the first e - b entries are meaningful (the columns of the range)"""
        import torch
        F = getattr(self, "n_faces", 0)       # (no mesh, no ordered upload: the table, if any, is in the caller's order and nothing is written)
        out = torch.zeros(max(F, 1), dtype=torch.int32, device="cuda:%d" % self.device)
        torch.cuda.synchronize(self.device)   # the library writes on the context's stream, torch filled on its own
        flag = C.c_int(0)
        _check(self.L, self.L.mvs_ctx_table_order(self.h, C.c_void_p(out.data_ptr()), C.byref(flag)))
        return out.cpu().numpy().view(np.uint32)[:F].copy() if flag.value else None

    def build_adjacency(self):
        """tex::build_adjacency_graph on the resident mesh; returns device-resident (adj_ptr, adj) usable by view_selection"""
        pp, pa, n = C.c_void_p(), C.c_void_p(), C.c_uint64(0)
        _check(self.L, self.L.mvs_ctx_build_adjacency(self.h, C.byref(pp), C.byref(pa), C.byref(n)))
        return DevArray(pp.value, self.n_faces + 1), DevArray(pa.value, n.value)

    def data_costs(self, settings=None):
        st = settings or Settings()
        ds = DcStats()
        _check(self.L, self.L.mvs_ctx_data_costs(self.h, C.byref(st), C.byref(ds)))
        return _stats_dict(ds)

    def dc_ranges(self):
        """(n_ranges, faces of the first range) of the last data-cost pass (mvs_ctx_dc_ranges; option "dc_range_pairs")"""
        n, per = C.c_uint32(0), C.c_uint32(0)
        _check(self.L, self.L.mvs_ctx_dc_ranges(self.h, C.byref(n), C.byref(per)))
        return n.value, per.value

    def costs_download(self):
        out = CCsr(); q = C.c_void_p()
        _check(self.L, self.L.mvs_ctx_costs_download(self.h, C.byref(out), C.byref(q)))
        F, nnz = out.n_faces, out.nnz
        def grab(ptr, ctype, n):
            return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(ctype)), (max(n, 1),))[:n].copy()
        res = DataCosts(F, out.n_views, grab(out.col_ptr, C.c_uint32, F + 1), grab(out.view_id, C.c_uint16, nnz),
                        grab(out.cost, C.c_float, nnz), grab(q.value, C.c_float, nnz))
        self.L.mvs_csr_free(C.byref(out))
        C.CDLL(None).free(q)
        return res

    def prune_labels(self, max_labels):
        """label-space compression of the resident table (mvs_ctx_prune_labels)"""
        _check(self.L, self.L.mvs_ctx_prune_labels(self.h, int(max_labels)))

    def costs_upload(self, dc):
        s, dev = dc._struct()
        self._keep["costs"] = dc
        _check(self.L, self.L.mvs_ctx_costs_upload(self.h, C.byref(s), dev))

    def costs_upload_ordered(self, dc, order):
        """mvs_ctx_costs_upload_ordered (building-blocks library; test harness only): the host table `dc`, given in the CALLER's numbering, is
        uploaded with its columns in the order `order` (order[p] = the caller's id of column p) and the context left as after a data-cost
        pass in the library's own face order: table_order() returns `order`.  Follow it with view_selection (adjacency and labels in the
        caller's numbering, as always) only."""
        order = np.ascontiguousarray(order, dtype=np.uint32)
        cp = np.asarray(dc.col_ptr, np.int64)
        assert len(order) == dc.n_faces == len(cp) - 1
        idx = order.astype(np.int64)
        ok = idx < dc.n_faces                                        # an id that is no face: an empty column; the library refuses the order
        K = np.where(ok, np.diff(cp)[np.minimum(idx, max(dc.n_faces - 1, 0))], 0) if dc.n_faces else np.zeros(0, np.int64)
        ptr = np.zeros(dc.n_faces + 1, np.uint32); ptr[1:] = np.cumsum(K)
        take = (np.repeat(cp[:-1][np.where(ok, idx, 0)] - ptr[:-1].astype(np.int64), K) + np.arange(int(ptr[-1]))) if dc.n_faces else np.zeros(0, np.int64)
        t = DataCosts(dc.n_faces, dc.n_views, ptr, np.ascontiguousarray(np.asarray(dc.view_id)[take]), np.ascontiguousarray(np.asarray(dc.cost)[take]))
        s, dev = t._struct()
        assert not dev, "a host table"
        _check(self.L, self.L.mvs_ctx_costs_upload_ordered(self.h, C.byref(s), order.ctypes.data_as(C.c_void_p)))
        self._keep["costs"] = t
        self.n_faces = dc.n_faces

    def view_selection(self, adj_ptr, adj, params=None, labels_out=None):
        """tex::view_selection on the resident costs; returns (labels u32[F], stats)."""
        p = params or default_mrf_params()
        pa, d0 = _ptr(adj_ptr); pb, d1 = _ptr(adj)
        assert d0 == d1
        F = int(adj_ptr.shape[0]) - 1
        if labels_out is None:
            labels_out = np.zeros(F, dtype=np.uint32)
        pl, dl = _ptr(labels_out)
        ms = MrfStats()
        self._keep["adj"] = (adj_ptr, adj)
        _check(self.L, self.L.mvs_ctx_view_selection(self.h, pa, pb, d0, C.byref(p), pl, dl, C.byref(ms)))
        return labels_out, _stats_dict(ms)


    def mrf_setup_tables(self):
        """what the last solve's set-up built (mvs_ctx_mrf_setup_tables, building-blocks library): {"bitmaps": the set-up worked from
        view-set bitmaps, "rec": uint32 record words, "desc": uint32 (n_fast, 12) descriptors, "ident": uint8 flag per directed edge}"""
        out = {}
        for which, key, dt in ((0, "bitmaps", np.uint64), (1, "rec", np.uint32), (2, "desc", np.uint32), (3, "ident", np.uint8)):
            n = C.c_uint64(0)
            _check(self.L, self.L.mvs_ctx_mrf_setup_tables(self.h, which, None, 0, C.byref(n)))
            buf = np.zeros(n.value // np.dtype(dt).itemsize, dtype=dt)
            if n.value:
                _check(self.L, self.L.mvs_ctx_mrf_setup_tables(self.h, which, buf.ctypes.data_as(C.c_void_p), n.value, C.byref(n)))
            out[key] = buf
        out["bitmaps"] = bool(out["bitmaps"][0]); out["desc"] = out["desc"].reshape(-1, 12)
        return out

    def ray_bits(self):
        """the bit matrices of the occlusion-ray stage after the last data-cost pass (mvs_ctx_ray_bits, building-blocks library; test harness
        only): (need, occl), bool arrays [n_views, n_verts] in the caller's vertex numbering -- need[j, v]: the ray from vertex v to camera j
        was traced, occl[j, v]: it was found occluded"""
        nv = int(self._keep["mesh"][0].shape[0])
        out = []
        for which in (0, 1):
            n = C.c_uint64(0)
            _check(self.L, self.L.mvs_ctx_ray_bits(self.h, which, None, 0, C.byref(n)))
            buf = np.zeros(n.value // 8, dtype=np.uint64)
            _check(self.L, self.L.mvs_ctx_ray_bits(self.h, which, buf.ctypes.data_as(C.c_void_p), n.value, C.byref(n)))
            bits = np.unpackbits(buf.view(np.uint8).reshape(self.n_views, -1), axis=1, bitorder="little")
            assert not bits[:, nv:].any()
            out.append(bits[:, :nv].astype(bool))
        return out[0], out[1]

    def ray_vertex_order(self):
        """uint32[n_verts]: the caller's id of the vertex at every position of the library's vertex order (mvs_ctx_ray_bits, which = 2): the
        rays of 64 consecutive positions and one view form a packet of the ray kernel"""
        n = C.c_uint64(0)
        _check(self.L, self.L.mvs_ctx_ray_bits(self.h, 2, None, 0, C.byref(n)))
        buf = np.zeros(n.value // 4, dtype=np.uint32)
        _check(self.L, self.L.mvs_ctx_ray_bits(self.h, 2, buf.ctypes.data_as(C.c_void_p), n.value, C.byref(n)))
        return buf

    def _prep_read(self, which, view, dtype):
        n = C.c_uint64(0)
        _check(self.L, self.L.mvs_ctx_prep_products(self.h, which, view, None, 0, C.byref(n)))
        buf = np.zeros(n.value // np.dtype(dtype).itemsize, dtype=dtype)
        _check(self.L, self.L.mvs_ctx_prep_products(self.h, which, view, buf.ctypes.data_as(C.c_void_p), n.value, C.byref(n)))
        return buf

    def prep_products(self, view):
        """what the image preparation of the last data-cost pass left on the device for one view (mvs_ctx_prep_products, building-blocks
        library; test harness only): a PrepProducts with gmi (uint8 (h, w), None after an area-term pass), mask_words (uint32 (h, mask_stride))
        and summary_words (uint32 (ceil(h / 32), msum_stride)) exactly as the device holds them"""
        mask = self._prep_read(1, view, np.uint32)                         # (raises what the entry refuses: no pass yet, no such view)
        w, h = self._view_sizes[view]
        mask = mask.reshape(h, -1)
        summary = self._prep_read(2, view, np.uint32).reshape((h + 31) // 32, -1)
        try:
            gmi = self._prep_read(0, view, np.uint8).reshape(h, w)
        except MvsError as e:
            if e.status != 6:                                              # MVS_ERR_STATE here: the last pass ran the area term
                raise
            gmi = None
        return PrepProducts(w, h, gmi, mask, summary)

    def prep_mask_flags(self):
        """uint8[n_views]: 1 = the DEVICE copy of the view table still carries the view's mask pointer after the last data-cost pass, 0 = a
        shortcut of the image preparation nulled it (mvs_ctx_prep_products, which = 3)"""
        return self._prep_read(3, 0, np.uint8)

    def mrf_diagnostics(self):
        """{graph_launches, graph_updates, graph_instantiations, generic_nodes} of this context's view selections"""
        out = (C.c_uint32 * 4)()
        _check(self.L, self.L.mvs_ctx_mrf_diagnostics(self.h, out))
        return dict(zip(("graph_launches", "graph_updates", "graph_instantiations", "generic_nodes"), [int(x) for x in out]))

    def get_subgraphs(self, adj_ptr, adj, labels, n_labels, on_device=False):
        """UniGraph::get_subgraphs for every label at once (row f3).  Host copies (label_ptr, comp_ptr, comp_faces), or
        with on_device=True DevArrays owned by the context (valid until the next call)."""
        pa, d0 = _ptr(adj_ptr); pb, d1 = _ptr(adj); pl, dl = _ptr(labels)
        assert d0 == d1
        F = int(adj_ptr.shape[0]) - 1
        sg = Subgraphs()
        self._keep["sg"] = (adj_ptr, adj, labels)
        _check(self.L, self.L.mvs_ctx_get_subgraphs(self.h, F, pa, pb, d0, pl, dl, int(n_labels), C.byref(sg), 1 if on_device else 0))
        if on_device:
            return DevArray(sg.label_ptr, n_labels + 1), DevArray(sg.comp_ptr, sg.n_components + 1), DevArray(sg.comp_faces, F)
        return _subgraphs_to_numpy(self.L, sg)

    def global_seam_leveling(self, adj_ptr, adj, labels, params=None, on_device=False):
        """Row f5: tex::global_seam_leveling on the context's mesh and views from the caller's labels (0 = unseen, L = view L - 1).
        Returns ({x_ptr, x_label, x_adjust (x_rows, 3), corner_adjust (F, 3, 3)}, stats); with on_device=True the four arrays are
        DevArrays owned by the context (valid until the next call).  params: default_gsl_params(...)."""
        pa, d0 = _ptr(adj_ptr); pb, d1 = _ptr(adj); pl, dl = _ptr(labels)
        assert d0 == d1
        p = params or default_gsl_params()
        res, st = GslResult(), GslStats()
        self._keep["gsl"] = (adj_ptr, adj, labels)
        _check(self.L, self.L.mvs_ctx_global_seam_leveling(self.h, pa, pb, d0, pl, dl, C.byref(p), C.byref(res), 1 if on_device else 0, C.byref(st)))
        stats = {k: int(getattr(st, k)) for k in GSL_COUNTS}
        stats.update({k: float(getattr(st, k)) for k in GSL_MS})
        stats["iterations"] = [int(x) for x in st.iterations]
        stats["error"] = np.array(list(st.error), np.float32)
        NV, F, XR = int(res.n_verts), int(res.n_faces), int(res.x_rows)
        if on_device:
            return dict(x_ptr=DevArray(res.x_ptr, NV + 1), x_label=DevArray(res.x_label, XR), x_adjust=DevArray(res.x_adjust, 3 * XR),
                        corner_adjust=DevArray(res.corner_adjust, 9 * F)), stats
        out = dict(x_ptr=_grab(res.x_ptr, NV + 1, C.c_uint32), x_label=_grab(res.x_label, XR, C.c_uint32),
                   x_adjust=_grab(res.x_adjust, 3 * XR, C.c_float).reshape(XR, 3), corner_adjust=_grab(res.corner_adjust, 9 * F, C.c_float).reshape(F, 3, 3))
        self.L.mvs_gsl_result_free(C.byref(res))
        return out, stats

    def texture_patches(self, adj_ptr, adj, labels, corner_adjust=None, params=None, on_device=False):
        """Row f6: the texture patches of the labelled faces with TexturePatch::adjust_colors applied (DESIGN.md section 4 "Texture
        patches"), from the caller's labels and the per-corner adjustments of global_seam_leveling (corner_adjust (F, 3, 3) or its
        device array; None = zeros: masks only).  Returns (arrays, stats): label (P,), box (P, 4) = min_x, min_y, width, height,
        face_ptr (P + 1,), faces, texcoords (n_listed, 3, 2), pix_ptr (P + 1,) uint64, image (n_pixels, 3), validity, blending
        (n_pixels,) -- patch_view(arrays, i) cuts patch i out; with on_device=True DevArrays owned by the context (valid until the next
        texture_patches call).  A pixel total above params.max_pixels raises MvsError (status 7) with `.stats` holding the counts."""
        pa, d0 = _ptr(adj_ptr); pb, d1 = _ptr(adj); pl, dl = _ptr(labels)
        assert d0 == d1
        if corner_adjust is not None and not (_is_torch(corner_adjust) or isinstance(corner_adjust, DevArray)):
            corner_adjust = np.ascontiguousarray(corner_adjust, np.float32)
        pc, dc = _ptr(corner_adjust)
        p = params or default_patch_params()
        res, st = PatchSet(), PatchStats()
        self._keep["patches"] = (adj_ptr, adj, labels, corner_adjust)
        rc = self.L.mvs_ctx_texture_patches(self.h, pa, pb, d0, pl, dl, pc, dc, C.byref(p), C.byref(res), 1 if on_device else 0, C.byref(st))
        return self._patch_result(rc, res, st, on_device)

    def _patch_result(self, rc, res, st, on_device):
        """(arrays, stats) of a call that fills a PatchSet and PatchStats (texture_patches, debug_patches)"""
        stats = {k: int(getattr(st, k)) for k in PATCH_COUNTS}
        stats.update({k: float(getattr(st, k)) for k in PATCH_MS})
        _check_with_stats(self.L, rc, stats)
        P, NL, NP = int(res.n_patches), int(res.n_listed), int(res.n_pixels)
        shapes = dict(label=(P, np.uint32), box=(4 * P, np.int32), face_ptr=(P + 1, np.uint32), faces=(NL, np.uint32), texcoords=(6 * NL, np.float32),
                      pix_ptr=(P + 1, np.uint64), image=(3 * NP, np.float32), validity=(NP, np.uint8), blending=(NP, np.uint8))
        out = _download(res, shapes, None if on_device else self.L.mvs_patch_set_free)
        if on_device:
            return out, stats
        out["box"] = out["box"].reshape(P, 4); out["texcoords"] = out["texcoords"].reshape(NL, 3, 2); out["image"] = out["image"].reshape(NP, 3)
        return out, stats

    def debug_embeddings(self, sizes, view_ids=None, first_position=0, out=None):
        """Row f10: generate_debug_embeddings (DESIGN.md section 4 "Debug model") for images of the given (width, height) sizes at
        positions first_position + i of the view list: each a flat colour of its own stamped with its three-digit id (view_ids[i], or
        the position).  Returns the images packed back to back as one flat uint8 array (RGB, row-major), or fills `out` -- a CUDA
        tensor or DevArray of 3 * sum(w * h) bytes, any alignment -- and returns it.  An id above 999 raises MvsError (status 7)."""
        sizes = np.ascontiguousarray(sizes, np.int32).reshape(-1, 2)
        n = len(sizes)
        w = np.ascontiguousarray(sizes[:, 0]); h = np.ascontiguousarray(sizes[:, 1])
        ids = None if view_ids is None else np.ascontiguousarray(view_ids, np.uint32)
        assert ids is None or ids.shape == (n,)
        total = 3 * int((w.astype(np.int64) * h.astype(np.int64)).sum())
        if out is None:
            out = np.zeros(total, np.uint8)
        po, dev = _ptr(out)
        assert (int(out.numel()) if _is_torch(out) else int(out.shape[0])) >= total
        _check(self.L, self.L.mvs_ctx_debug_embeddings(self.h, n, _ptr(w)[0], _ptr(h)[0], _ptr(ids)[0], int(first_position), po, dev))
        return out

    def debug_patches(self, adj_ptr, adj, labels, view_ids=None, params=None, on_device=False):
        """Row f10: the patch set of the view-selection debug model -- texture_patches' geometry (label, box, face_ptr, faces, texcoords,
        pix_ptr: the same bits) with the pixels of the views' debug images (debug_embeddings of the context's view sizes), validity 255
        and blending 0 everywhere; the context's images are not touched.  view_ids: one id per view (host), None = the positions.
        Returns (arrays, stats) as texture_patches does; with on_device=True DevArrays owned by the context (valid until the next
        texture_patches or debug_patches call)."""
        pa, d0 = _ptr(adj_ptr); pb, d1 = _ptr(adj); pl, dl = _ptr(labels)
        assert d0 == d1
        ids = None if view_ids is None else np.ascontiguousarray(view_ids, np.uint32)
        p = params or default_patch_params()
        res, st = PatchSet(), PatchStats()
        self._keep["patches"] = (adj_ptr, adj, labels, ids)
        rc = self.L.mvs_ctx_debug_patches(self.h, pa, pb, d0, pl, dl, _ptr(ids)[0], C.byref(p), C.byref(res), 1 if on_device else 0, C.byref(st))
        return self._patch_result(rc, res, st, on_device)

    def view_selection_model(self, adj_ptr, adj, labels, prefix, view_ids=None, vertex_normals=None, patch_params=None, atlas_params=None, model_params=None):
        """Row f10 to files (`texrecon --view_selection_model`): debug_patches, texture_atlases and save_model with everything left on
        the device in between: writes `<prefix>_view_selection.obj`, `.mtl` and the atlas PNGs.  Returns the stats of the three rows
        as dict(patches=..., atlases=..., model=...)."""
        pa, d0 = _ptr(adj_ptr); pb, d1 = _ptr(adj); pl, dl = _ptr(labels)
        assert d0 == d1
        ids = None if view_ids is None else np.ascontiguousarray(view_ids, np.uint32)
        if vertex_normals is not None and not (_is_torch(vertex_normals) or isinstance(vertex_normals, DevArray)):
            vertex_normals = np.ascontiguousarray(vertex_normals, np.float32).reshape(-1)
        pn, dn = _ptr(vertex_normals)
        pp, ap, mp = patch_params or default_patch_params(), atlas_params or default_atlas_params(), model_params or default_model_params()
        ps, as_, ms = PatchStats(), AtlasStats(), ModelStats()
        self._keep["debug_model"] = (adj_ptr, adj, labels, ids, vertex_normals)
        rc = self.L.mvs_ctx_view_selection_model(self.h, pa, pb, d0, pl, dl, _ptr(ids)[0], pn, dn, os.fspath(prefix).encode(), C.byref(pp), C.byref(ap), C.byref(mp),
                                                 C.byref(ps), C.byref(as_), C.byref(ms))
        stats = dict(patches={k: (int if k in PATCH_COUNTS else float)(getattr(ps, k)) for k in PATCH_COUNTS + PATCH_MS},
                     atlases={k: (int if k in ATLAS_COUNTS else float)(getattr(as_, k)) for k in ATLAS_COUNTS + ATLAS_MS}, model=_model_stats(ms))
        _check_with_stats(self.L, rc, stats)
        return stats

    def local_seam_leveling(self, adj_ptr, adj, labels, patches, params=None, on_device=False):
        """Row f7: tex::local_seam_leveling on a patch set (DESIGN.md section 4 "Local seam leveling"): `patches` is the dict of
        texture_patches -- all host arrays or all DevArrays / CUDA tensors (its on_device=True output can be passed straight in) --
        and is not modified.  Returns ({image (n_pixels, 3), validity, blending (n_pixels,)}, stats): the blended image, validity
        after the blend and the PREPARED blending mask, packed as the input, so patch_view works on the result merged over the
        input dict; with on_device=True DevArrays owned by the context (valid until the next local_seam_leveling call).
        params: default_lsl_params(...); max_iterations=0 returns the state before the solve."""
        pa, d0 = _ptr(adj_ptr); pb, d1 = _ptr(adj); pl, dl = _ptr(labels)
        assert d0 == d1
        dts = dict(label=np.uint32, box=np.int32, face_ptr=np.uint32, faces=np.uint32, texcoords=np.float32, pix_ptr=np.uint64, image=np.float32,
                   validity=np.uint8, blending=np.uint8)
        ps, held, dev = _patch_set_struct(patches, dts)
        p = params or default_lsl_params()
        res, st = LslResult(), LslStats()
        self._keep["lsl"] = (adj_ptr, adj, labels, held)
        rc = self.L.mvs_ctx_local_seam_leveling(self.h, pa, pb, d0, pl, dl, C.byref(ps), dev, C.byref(p), C.byref(res),
                                                1 if on_device else 0, C.byref(st))
        stats = {k: int(getattr(st, k)) for k in LSL_COUNTS + ("iterations_max",)}
        stats["error_max"] = float(st.error_max)
        stats.update({k: float(getattr(st, k)) for k in LSL_MS})
        _check_with_stats(self.L, rc, stats)
        NP = int(res.n_pixels)
        shapes = dict(image=(3 * NP, np.float32), validity=(NP, np.uint8), blending=(NP, np.uint8))
        out = _download(res, shapes, None if on_device else self.L.mvs_lsl_result_free)
        if on_device:
            return out, stats
        out["image"] = out["image"].reshape(NP, 3)
        return out, stats

    def texture_atlases(self, patches, params=None, on_device=False):
        """Row f8: tex::generate_texture_atlases on a patch set (DESIGN.md section 4 "Texture atlases"): `patches` is the dict of
        texture_patches with row f7's image and validity merged over it -- all host arrays or all DevArrays / CUDA tensors; label and
        blending are not read -- and is not modified.  Needs neither mesh nor views.  Returns (arrays, stats): atlas_size (A,),
        atlas_pix_ptr (A + 1,) uint64, image (n_pixels, 3) uint8 -- atlas_view(arrays, a) cuts atlas a out --, patch_atlas (P,), patch_pos
        (P, 2), patch_order (P,), face_ptr (A + 1,), faces, texcoords (n_listed, 3, 2), tc_ptr (A + 1,), texcoords_merged (n_merged, 2),
        texcoord_ids (n_listed, 3); with on_device=True DevArrays owned by the context (valid until the next texture_atlases call).
        An atlas pixel total above params.max_pixels raises MvsError (status 7) with `.stats` holding the counts."""
        dts = dict(box=np.int32, face_ptr=np.uint32, faces=np.uint32, texcoords=np.float32, pix_ptr=np.uint64, image=np.float32, validity=np.uint8)
        ps, held, dev = _patch_set_struct(patches, dts)
        P = int(ps.n_patches)
        p = params or default_atlas_params()
        res, st = AtlasSet(), AtlasStats()
        self._keep["atlas"] = held
        rc = self.L.mvs_ctx_texture_atlases(self.h, C.byref(ps), dev, C.byref(p), C.byref(res), 1 if on_device else 0, C.byref(st))
        stats = {k: int(getattr(st, k)) for k in ATLAS_COUNTS}
        stats.update({k: float(getattr(st, k)) for k in ATLAS_MS})
        _check_with_stats(self.L, rc, stats)
        A, NL, NM, NP = int(res.n_atlases), int(res.n_listed), int(res.n_merged), int(res.n_pixels)
        shapes = dict(atlas_size=(A, np.uint32), atlas_pix_ptr=(A + 1, np.uint64), image=(3 * NP, np.uint8), patch_atlas=(P, np.uint32), patch_pos=(2 * P, np.int32),
                      patch_order=(P, np.uint32), face_ptr=(A + 1, np.uint32), faces=(NL, np.uint32), texcoords=(6 * NL, np.float32), tc_ptr=(A + 1, np.uint32),
                      texcoords_merged=(2 * NM, np.float32), texcoord_ids=(3 * NL, np.uint32))
        out = _download(res, shapes, None if on_device else self.L.mvs_atlas_set_free)
        if on_device:
            return out, stats
        out["image"] = out["image"].reshape(NP, 3); out["patch_pos"] = out["patch_pos"].reshape(P, 2); out["texcoords"] = out["texcoords"].reshape(NL, 3, 2)
        out["texcoords_merged"] = out["texcoords_merged"].reshape(NM, 2); out["texcoord_ids"] = out["texcoord_ids"].reshape(NL, 3)
        return out, stats

    def _model_call(self, atlases, vertex_normals, params):
        """the arguments build_model and save_model share: (AtlasSet, on_device, normals pointer, normals on device, params, held arrays)"""
        ps, held, dev = _atlas_set_struct(atlases)
        if vertex_normals is not None and not (_is_torch(vertex_normals) or isinstance(vertex_normals, DevArray)):
            vertex_normals = np.ascontiguousarray(vertex_normals, np.float32).reshape(-1)
            assert "mesh" not in self._keep or vertex_normals.size == 3 * int(self._keep["mesh"][0].shape[0]), "vertex_normals: one normal per mesh vertex"
        pn, dn = _ptr(vertex_normals)
        return ps, dev, pn, dn, params or default_model_params(), (held, vertex_normals)

    def build_model(self, atlases, vertex_normals=None, name="model", params=None, on_device=False):
        """Row f9: the text of tex::build_model + ObjModel::save + MaterialLib::save_to_files (DESIGN.md section 4 "Model output") on the
        context's mesh and an atlas set -- the dict of texture_atlases (all host arrays or all DevArrays / CUDA tensors; only face_ptr,
        faces, tc_ptr, texcoords_merged and texcoord_ids are read).  vertex_normals: (n_verts, 3) host or device array, or None: no `vn`
        lines, faces written V/T.  Returns ({obj, mtl: bytes, section_ptr, section_bytes: uint64 (A + 5,)}, stats); with on_device=True obj
        and mtl are DevArrays of bytes owned by the context (valid until its next build_model / save_model call).  An .obj above
        params.max_bytes raises MvsError (status 7) with `.stats` holding the counts."""
        ps, dev, pn, dn, p, held = self._model_call(atlases, vertex_normals, params)
        res, st = ModelText(), ModelStats()
        self._keep["model"] = held
        rc = self.L.mvs_ctx_build_model(self.h, C.byref(ps), dev, pn, dn, name.encode(), C.byref(p), C.byref(res), 1 if on_device else 0, C.byref(st))
        stats = _model_stats(st)
        _check_with_stats(self.L, rc, stats)
        NS = int(res.n_atlases) + 5
        sec = {k: np.frombuffer(C.string_at(getattr(res, k), 8 * NS), np.uint64).copy() for k in ("section_ptr", "section_bytes")}
        if on_device:
            return dict(obj=DevArray(res.obj, res.obj_bytes), mtl=DevArray(res.mtl, res.mtl_bytes), **sec), stats
        out = dict(obj=C.string_at(res.obj, res.obj_bytes), mtl=C.string_at(res.mtl, res.mtl_bytes), **sec)
        self.L.mvs_model_text_free(C.byref(res))
        return out, stats

    def save_model(self, atlases, prefix, vertex_normals=None, params=None):
        """Row f9 to files: `<prefix>.obj`, `<prefix>.mtl` and one `<prefix>_material<a>_map_Kd.png` per atlas (mvs_ctx_save_model; the
        atlas set needs atlas_size, atlas_pix_ptr and image as well).  Returns the stats; params: default_model_params(png_level=...) for
        the host encoder's level, default_model_params(png_device=1) for the PNGs compressed on the device (encode_pngs),
        default_model_params(image_format="jpeg", jpeg_quality=..., jpeg_subsampling=...) for `.jpg` files from the device (encode_jpegs)."""
        ps, dev, pn, dn, p, held = self._model_call(atlases, vertex_normals, params)
        st = ModelStats()
        self._keep["model"] = held
        rc = self.L.mvs_ctx_save_model(self.h, C.byref(ps), dev, pn, dn, os.fspath(prefix).encode(), C.byref(p), C.byref(st))
        stats = _model_stats(st)
        _check_with_stats(self.L, rc, stats)
        return stats

    def _glb_stats(self, st):
        """mvs_glb_stats as a dict, with the last call's mvs_glb_quant_stats (ms_bounds, zero_normals, texcoords_out_of_range,
        index16_primitives: all zero under glb_quantize 0) beside it"""
        qs = GlbQuantStats()
        _check(self.L, self.L.mvs_ctx_glb_quant_stats(self.h, C.byref(qs)))
        stats = _stats_dict(st)
        stats.update((k, getattr(qs, k)) for k in GLB_QUANT_COUNTS + GLB_QUANT_MS)
        return stats

    def build_glb(self, atlases, vertex_normals=None, params=None):
        """Row f11: the textured model as one binary glTF 2.0 file (mvs_ctx_build_glb; DESIGN.md section 4 "Model output" item 8) on the
        context's mesh and an atlas set -- the dict of texture_atlases, all host arrays or all DevArrays / CUDA tensors; without
        atlas_size or image the file carries no images.  vertex_normals: (n_verts, 3) host or device array, or None: no NORMAL attribute.
        Returns (bytes, stats).  params: default_model_params(...) as save_model reads it -- the embedded PNGs are the files it would
        write; max_bytes caps the file; glb_quantize=1 stores the geometry under KHR_mesh_quantization (item 10: 16-bit positions on
        one grid for the file, 16-bit texture coordinates, 8-bit unit normals, 16-bit indices per primitive where they fit).  A refusal
        raises MvsError with `.stats` holding the counts."""
        ps, dev, pn, dn, p, held = self._model_call(atlases, vertex_normals, params)
        res, st = Glb(), GlbStats()
        self._keep["glb"] = held
        rc = self.L.mvs_ctx_build_glb(self.h, C.byref(ps), dev, pn, dn, C.byref(p), C.byref(res), C.byref(st))
        stats = self._glb_stats(st)
        _check_with_stats(self.L, rc, stats)
        data = C.string_at(res.data, res.n_bytes)
        self.L.mvs_glb_free(C.byref(res))
        return data, stats

    def save_glb(self, atlases, path, vertex_normals=None, params=None):
        """Row f11 to a file: build_glb's bytes at `path`, written once (mvs_ctx_save_glb).  Returns the stats."""
        ps, dev, pn, dn, p, held = self._model_call(atlases, vertex_normals, params)
        st = GlbStats()
        self._keep["glb"] = held
        rc = self.L.mvs_ctx_save_glb(self.h, C.byref(ps), dev, pn, dn, os.fspath(path).encode(), C.byref(p), C.byref(st))
        stats = self._glb_stats(st)
        _check_with_stats(self.L, rc, stats)
        return stats

    @staticmethod
    def _image_set(images):
        """the arrays encode_pngs and encode_jpegs share: (n, width, height, pix, img, on_device)"""
        if isinstance(images, dict):
            held = _atlas_set_struct({k: images[k] for k in ("atlas_size", "atlas_pix_ptr", "image")})[1]
            size, pix, img = held["atlas_size"], held["atlas_pix_ptr"], held["image"]
            dev = 1 if (_is_torch(img) or isinstance(img, DevArray)) else 0
            n = int(size.numel()) if _is_torch(size) else int(size.shape[0])
            width = height = size
        elif len(images) and _is_torch(images[0]):
            import torch
            assert all(_is_torch(a) and a.is_cuda and a.dtype == torch.uint8 and a.dim() == 3 and a.shape[2] == 3 for a in images)
            n, dev = len(images), 1
            d = images[0].device
            width = torch.tensor([a.shape[1] for a in images], dtype=torch.int32, device=d)      # (the bits of a uint32 below 2^31)
            height = torch.tensor([a.shape[0] for a in images], dtype=torch.int32, device=d)
            pix = torch.tensor(np.concatenate([[0], np.cumsum([a.shape[0] * a.shape[1] for a in images])]).astype(np.int64), device=d)
            img = torch.cat([a.contiguous().reshape(-1) for a in images])
        else:
            arrs = [np.ascontiguousarray(a, np.uint8) for a in images]
            assert all(a.ndim == 3 and a.shape[2] == 3 for a in arrs)
            n, dev = len(arrs), 0
            width = np.array([a.shape[1] for a in arrs], np.uint32); height = np.array([a.shape[0] for a in arrs], np.uint32)
            pix = np.concatenate([[0], np.cumsum([a.shape[0] * a.shape[1] for a in arrs])]).astype(np.uint64)
            img = np.concatenate([a.reshape(-1) for a in arrs]) if arrs else np.zeros(0, np.uint8)
        return n, width, height, pix, img, dev

    def _encode_images(self, images, key, fn, stats_cls, stats_dict, free, *extra):
        """encode_pngs / encode_jpegs: one call of `fn` on the image set (`extra`: the arguments between on_device and the result), the
        files cut out of the set, the set released by `free`"""
        n, width, height, pix, img, dev = self._image_set(images)
        res, st = PngSet(), stats_cls()
        self._keep[key] = (width, height, pix, img)
        n_pix = int(img.numel()) if _is_torch(img) else int(img.shape[0])
        rc = fn(self.h, n, _ptr(width)[0], _ptr(height)[0], _ptr(pix)[0], _ptr(img)[0] if n_pix else None, dev, *extra, C.byref(res), C.byref(st))
        stats = stats_dict(st)
        _check_with_stats(self.L, rc, stats)
        off = np.frombuffer(C.string_at(res.offsets, 8 * (n + 1)), np.uint64)
        data = C.string_at(res.data, res.n_bytes)
        free(C.byref(res))
        return [data[int(off[i]):int(off[i + 1])] for i in range(n)], stats

    def encode_pngs(self, images):
        """The compressed PNG route of row f9 on its own (mvs_ctx_encode_pngs; DESIGN.md section 4 "Model output" item 7): `images` is a
        list of (H, W, 3) uint8 arrays -- all numpy or all CUDA tensors -- or an atlas-set dict (atlas_size, atlas_pix_ptr, image: all
        host or all device).  One call encodes them all.  Returns (list of bytes, one PNG file per image; stats)."""
        return self._encode_images(images, "png", self.L.mvs_ctx_encode_pngs, PngStats, _png_stats, self.L.mvs_png_set_free)

    def encode_jpegs(self, images, quality=90, subsampling=1):
        """The JPEG route of rows f9 / f11 on its own (mvs_ctx_encode_jpegs; DESIGN.md section 4 "Model output" item 9): `images` as
        encode_pngs takes them, quality 1 .. 100, subsampling 0 (4:4:4) or 1 (4:2:0).  One call encodes them all.  Returns (list of
        bytes, one baseline JPEG file per image; stats).  The same bytes as the host twin encode_jpeg gives."""
        return self._encode_images(images, "jpeg", self.L.mvs_ctx_encode_jpegs, JpegStats, _stats_dict, self.L.mvs_jpeg_set_free, int(quality), int(subsampling))

    def deflate_rle(self, data):
        """mvs_ctx_deflate_rle: the zlib stream (bytes) the chunk, gather and checksum passes of the compressed PNG route give the byte
        stream `data` -- bytes, a uint8 numpy array or a CUDA uint8 tensor"""
        if not (_is_torch(data) or isinstance(data, DevArray)):
            data = np.frombuffer(bytes(data), np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else np.ascontiguousarray(data, np.uint8).reshape(-1)
        n = int(data.numel()) if _is_torch(data) else int(data.shape[0])
        p, dev = _ptr(data)
        out, nb = C.c_void_p(), C.c_uint64()
        _check(self.L, self.L.mvs_ctx_deflate_rle(self.h, p if n else None, n, dev, C.byref(out), C.byref(nb)))
        return _take_bytes(self.L, out, nb)

    def gamma_correct(self, values, power):
        """mvs_ctx_gamma_correct: the tone mapping route on its own (csrc/tone.h gamma_pow on every value, by a kernel) -- a float32
        numpy array (returns a new one of the same shape) or a CUDA float32 tensor / DevArray (corrected IN PLACE and returned).  The
        same bits as the host twin gamma_correct gives."""
        if _is_torch(values) or isinstance(values, DevArray):
            n = int(values.numel()) if _is_torch(values) else int(values.shape[0])
            _check(self.L, self.L.mvs_ctx_gamma_correct(self.h, _ptr(values)[0] if n else None, n, float(power), 1))
            return values
        out = np.array(values, dtype=np.float32, order="C")
        _check(self.L, self.L.mvs_ctx_gamma_correct(self.h, out.ctypes.data if out.size else None, out.size, float(power), 0))
        return out

    def set_tone_table(self, table=None):
        """mvs_ctx_tone_table (building-blocks library; test harness only): replaces the 256 texel values tone_mapping = 1 reads in rows
        f5, f6 and f10 on this context; None restores the gamma table (tone_table("gamma"))"""
        if table is not None:
            table = np.ascontiguousarray(table, np.float32)
            assert table.shape == (256,)
        _check(self.L, self.L.mvs_ctx_tone_table(self.h, None if table is None else table.ctypes.data))

    def gsl_system(self):
        """host copies of the last global_seam_leveling's system: lower-triangle Lhs CSR (lhs_ptr, lhs_col, lhs_val), rhs (x_rows, 3),
        a_col (a_rows, 2), b (a_rows, 3), x_raw (x_rows, 3) = x before the mean"""
        s = GslSystem()
        _check(self.L, self.L.mvs_ctx_gsl_system(self.h, C.byref(s)))
        XR, AR, NZ = int(s.x_rows), int(s.a_rows), int(s.lhs_nnz)
        out = dict(lhs_ptr=_grab(s.lhs_ptr, XR + 1, C.c_uint32), lhs_col=_grab(s.lhs_col, NZ, C.c_uint32), lhs_val=_grab(s.lhs_val, NZ, C.c_float),
                   rhs=_grab(s.rhs, 3 * XR, C.c_float).reshape(XR, 3), a_col=_grab(s.a_col, 2 * AR, C.c_uint32).reshape(AR, 2),
                   b=_grab(s.b, 3 * AR, C.c_float).reshape(AR, 3), x_raw=_grab(s.x_raw, 3 * XR, C.c_float).reshape(XR, 3))
        self.L.mvs_gsl_system_free(C.byref(s))
        return out


def _grab(ptr, n, ctype):
    if n == 0:
        return np.zeros(0, np.uint32 if ctype is C.c_uint32 else np.float32)
    return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(ctype)), (n,)).copy()


def _tone(tone_mapping):
    """the value of the *_params.tone_mapping field: "none" | "gamma" or the number itself"""
    return TONE_MAPPINGS[tone_mapping] if isinstance(tone_mapping, str) else int(tone_mapping)


def _toned(params, default_fn, tone_mapping):
    """the parameters of one row for a module-level call: the library's defaults, or a copy of the caller's, in the mode `tone_mapping`
    ("none" leaves the caller's own field as it is)"""
    t = _tone(tone_mapping)
    if params is None:
        return default_fn(tone_mapping=t)
    p = type(params).from_buffer_copy(params)
    if t:
        p.tone_mapping = t
    return p


def gamma_correct(values, power):
    """mvs_gamma_correct: csrc/tone.h gamma_pow(value, power) on every value of a float32 array, on the host (DEFINED HERE for
    mve::image::gamma_correct; DESIGN.md section 4 "Tone mapping"); needs no GPU.  Returns a new array of the same shape."""
    L = load_library()
    out = np.array(values, dtype=np.float32, order="C")
    _check(L, L.mvs_gamma_correct(out.ctypes.data if out.size else None, out.size, float(power)))
    return out


def tone_table(mode):
    """mvs_tone_table: float32[256], the value of every byte of a view's image under tone mapping "none" (byte / 255) or "gamma"
    (gamma_pow(byte / 255, 2.2f))"""
    L = load_library()
    out = np.zeros(256, np.float32)
    _check(L, L.mvs_tone_table(_tone(mode), out.ctypes.data))
    return out


def default_gsl_params(**kw):
    """mvs_gsl_default_params (tolerance 1e-4, max_iterations 1000, lam 0.1, tone_mapping 0 = none) with overrides"""
    return _default_params(GslParams, "mvs_gsl_default_params", kw)


def default_patch_params(**kw):
    """mvs_patch_default_params (max_pixels 0 = no cap, tone_mapping 0 = none) with overrides"""
    return _default_params(PatchParams, "mvs_patch_default_params", kw)


def default_lsl_params(**kw):
    """mvs_lsl_default_params (tolerance 1e-6, max_iterations 700, strip_width 20, lds_bytes 147456) with overrides"""
    return _default_params(LslParams, "mvs_lsl_default_params", kw)


def default_atlas_params(**kw):
    """mvs_atlas_default_params (max_pixels 0 = no cap, tone_mapping 0 = none) with overrides"""
    return _default_params(AtlasParams, "mvs_atlas_default_params", kw)


def default_model_params(**kw):
    """mvs_model_default_params (max_bytes 0 = no cap, png_level 0 = stored deflate blocks, png_device 0 = PNGs encoded on the host,
    image_format 0 = PNG, jpeg_quality 90, jpeg_subsampling 1 = 4:2:0, glb_quantize 0 = float32 geometry in the .glb) with overrides;
    image_format: "png" | "jpeg" | 0 | 1; glb_quantize=1: build_glb / save_glb / texture_model(format="glb" | "both") write the geometry
    under KHR_mesh_quantization (DESIGN.md section 4 "Model output" item 10); the OBJ route does not read it"""
    if isinstance(kw.get("image_format"), str):
        if kw["image_format"] not in IMAGE_FORMATS:
            raise ValueError("default_model_params: image_format must be \"png\" or \"jpeg\", not %r" % (kw["image_format"],))
        kw = dict(kw, image_format=IMAGE_FORMATS[kw["image_format"]])
    return _default_params(ModelParams, "mvs_model_default_params", kw)


ATLAS_DTYPES = dict(atlas_size=np.uint32, atlas_pix_ptr=np.uint64, image=np.uint8, patch_atlas=np.uint32, patch_pos=np.int32, patch_order=np.uint32, face_ptr=np.uint32,
                    faces=np.uint32, texcoords=np.float32, tc_ptr=np.uint32, texcoords_merged=np.float32, texcoord_ids=np.uint32)


def _atlas_set_struct(atlases):
    """an atlas-set dict as an AtlasSet: (struct, held, on_device) -- all host arrays (made contiguous and flat; `held` keeps them alive) or
    all DevArrays / CUDA tensors; arrays that are absent or None stay NULL.  The counts come from face_ptr, faces, texcoords_merged and
    (when present) atlas_pix_ptr: a device-resident atlas_pix_ptr costs one 8-byte read."""
    have = {k: atlases[k] for k in ATLAS_ARRAYS if atlases.get(k) is not None}
    dev = [_is_torch(v) or isinstance(v, DevArray) for v in have.values()]
    assert all(dev) or not any(dev), "the atlas set must be all host or all device arrays"
    on_device = bool(dev) and dev[0]
    held = {k: v if on_device else np.ascontiguousarray(v, ATLAS_DTYPES[k]).reshape(-1) for k, v in have.items()}
    count = lambda x: int(x.numel()) if _is_torch(x) else int(x.shape[0])
    s = AtlasSet()
    s.n_atlases = count(held["face_ptr"]) - 1 if "face_ptr" in held else 0
    s.n_listed = count(held["faces"]) if "faces" in held else 0
    s.n_merged = count(held["texcoords_merged"]) // 2 if "texcoords_merged" in held else 0
    s.n_patches = count(held["patch_atlas"]) if "patch_atlas" in held else 0
    s.n_pixels = count(held["image"]) // 3 if "image" in held else 0
    for k, v in held.items():
        setattr(s, k, _ptr(v)[0] if (on_device or v.size) else None)
    return s, held, 1 if on_device else 0


def _model_stats(st):
    stats = {"lines": dict(zip(MODEL_SECTIONS, [int(x) for x in st.lines])), "bytes": dict(zip(MODEL_SECTIONS, [int(x) for x in st.bytes]))}
    stats.update({k: int(getattr(st, k)) for k in MODEL_COUNTS})
    stats.update({k: float(getattr(st, k)) for k in MODEL_MS})
    return stats


def _png_stats(st):
    # (not _stats_dict: filter_rows is an array, which goes out as a list, and the struct's reserved word stays out)
    stats = {k: int(getattr(st, k)) for k in PNG_COUNTS}
    stats["filter_rows"] = [int(x) for x in st.filter_rows]
    stats.update({k: float(getattr(st, k)) for k in PNG_MS})
    return stats


def _take_bytes(L, out, nb):
    z = C.string_at(out, nb.value)
    L.mvs_png_free(out)
    return z


def encode_png_rle(img):
    """mvs_encode_png_rle: the PNG file (bytes) of an (H, W, 3) uint8 host image by the host twin of the compressed route -- no GPU, no
    libz; the same bytes as Context.encode_pngs gives"""
    L = load_library()
    img = np.ascontiguousarray(img, dtype=np.uint8)
    assert img.ndim == 3 and img.shape[2] == 3
    out, nb = C.c_void_p(), C.c_uint64()
    _check(L, L.mvs_encode_png_rle(img.ctypes.data, img.shape[1], img.shape[0], C.byref(out), C.byref(nb)))
    return _take_bytes(L, out, nb)


def encode_jpeg(img, quality=90, subsampling=1):
    """mvs_encode_jpeg: the baseline JPEG file (bytes) of an (H, W, 3) uint8 host image by the host twin of the JPEG route -- no GPU, no
    library; the same bytes as Context.encode_jpegs gives"""
    L = load_library()
    img = np.ascontiguousarray(img, dtype=np.uint8)
    assert img.ndim == 3 and img.shape[2] == 3
    out, nb = C.c_void_p(), C.c_uint64()
    _check(L, L.mvs_encode_jpeg(img.ctypes.data, img.shape[1], img.shape[0], int(quality), int(subsampling), C.byref(out), C.byref(nb)))
    z = C.string_at(out, nb.value)
    L.mvs_jpeg_free(out)
    return z


def default_jpegdec_params(**kw):
    return _default_params(JpegDecParams, "mvs_jpegdec_default_params", kw)


def jpeg_probe(data):
    """mvs_jpeg_probe: (width, height) when the headers of the file `data` (bytes) are a baseline JPEG in the format the device route
    accepts, else None"""
    L = load_library()
    data = bytes(data)
    w, h = C.c_uint32(), C.c_uint32()
    return (w.value, h.value) if L.mvs_jpeg_probe(data, len(data), C.byref(w), C.byref(h)) == 0 else None


def decode_jpeg(data, coefficients=False):
    """mvs_decode_jpeg: the (H, W, 3) uint8 image of a baseline JPEG file (bytes) by the host twin of the view input route -- no GPU, no
    library; the same bytes as Context.decode_jpegs gives and as libjpeg-turbo decodes.  coefficients=True: (image, int16 [blocks, 64]),
    the quantised coefficients in coding order, index v * 8 + u."""
    L = load_library()
    data = bytes(data)
    out, w, h, co, nb = C.c_void_p(), C.c_uint32(), C.c_uint32(), C.c_void_p(), C.c_uint64()
    _check(L, L.mvs_decode_jpeg(data, len(data), C.byref(out), C.byref(w), C.byref(h), C.byref(co) if coefficients else None, C.byref(nb) if coefficients else None))
    img = np.frombuffer(C.string_at(out, 3 * w.value * h.value), np.uint8).reshape(h.value, w.value, 3).copy()
    L.mvs_jpeg_free(out)
    if not coefficients:
        return img
    c = np.frombuffer(C.string_at(co, 128 * nb.value), np.int16).reshape(-1, 64).copy()
    C.CDLL(None).free(co)
    return img, c


def png_probe(data):
    """mvs_png_probe: (width, height) when the chunks of the file `data` (bytes) are a PNG in the format the device route accepts (8 bit,
    colour type 0, 2, 3, 4 or 6, not interlaced), else None"""
    L = load_library()
    data = bytes(data)
    w, h = C.c_uint32(), C.c_uint32()
    return (w.value, h.value) if L.mvs_png_probe(data, len(data), C.byref(w), C.byref(h)) == 0 else None


def decode_png(data, raw=False):
    """mvs_decode_png: the (H, W, 3) uint8 image of a PNG file (bytes) by the host twin of the PNG view input route -- no GPU, no library;
    the same bytes as Context.decode_pngs gives and as Pillow's convert("RGB").  raw=True: (image, bytes), the inflated, still filtered
    stream of H * (1 + W * bytes per pixel) bytes."""
    L = load_library()
    data = bytes(data)
    out, w, h, rw = C.c_void_p(), C.c_uint32(), C.c_uint32(), C.c_void_p()
    _check(L, L.mvs_decode_png(data, len(data), C.byref(out), C.byref(w), C.byref(h), C.byref(rw) if raw else None))
    img = np.frombuffer(C.string_at(out, 3 * w.value * h.value), np.uint8).reshape(h.value, w.value, 3).copy()
    L.mvs_png_free(out)
    if not raw:
        return img
    bpp = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}[data[25]]
    stream = C.string_at(rw, h.value * (1 + w.value * bpp))
    L.mvs_png_free(rw)
    return img, stream


def deflate_rle(data):
    """mvs_deflate_rle: the zlib stream (bytes) of a byte stream by the host twin; the same bytes as Context.deflate_rle gives"""
    L = load_library()
    data = np.frombuffer(bytes(data), np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else np.ascontiguousarray(data, np.uint8).reshape(-1)
    out, nb = C.c_void_p(), C.c_uint64()
    _check(L, L.mvs_deflate_rle(data.ctypes.data if data.size else None, data.size, C.byref(out), C.byref(nb)))
    return _take_bytes(L, out, nb)


def write_png(path, rgb, level=0):
    """mvs_write_png: an (H, W, 3) uint8 host image as an 8-bit RGB PNG (level 0: stored blocks, 1 .. 9: libz.so.1)"""
    L = load_library()
    rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
    assert rgb.ndim == 3 and rgb.shape[2] == 3
    _check(L, L.mvs_write_png(os.fspath(path).encode(), rgb.ctypes.data, rgb.shape[1], rgb.shape[0], int(level)))


def vertex_normals(verts, faces):
    """area-weighted vertex normals of a triangle mesh in numpy, (n_verts, 3) float32: the sum of the incident faces' cross products,
    normalised (zero where it vanishes).  Plumbing for callers that have none -- NOT MVE's ensure_normals, whose weights differ."""
    verts = np.asarray(verts, np.float32); faces = np.asarray(faces, np.int64)
    a, b, c = verts[faces[:, 0]], verts[faces[:, 1]], verts[faces[:, 2]]
    n = np.cross(b - a, c - a).astype(np.float64)
    out = np.zeros((len(verts), 3), np.float64)
    for k in range(3):
        np.add.at(out, faces[:, k], n)
    norm = np.linalg.norm(out, axis=1, keepdims=True)
    return np.where(norm > 0, out / np.where(norm > 0, norm, 1), 0).astype(np.float32)


def atlas_view(arrays, a):
    """atlas a of Context.texture_atlases' host arrays: its (size, size, 3) uint8 image as a view of the packed array"""
    s = int(arrays["atlas_size"][a]); o = int(arrays["atlas_pix_ptr"][a])
    return arrays["image"][o:o + s * s].reshape(s, s, 3)


def patch_view(arrays, i):
    """patch i of Context.texture_patches' host arrays: (image (h, w, 3), validity (h, w), blending (h, w)) as views of the packed arrays"""
    w, h = int(arrays["box"][i, 2]), int(arrays["box"][i, 3])
    a, b = int(arrays["pix_ptr"][i]), int(arrays["pix_ptr"][i + 1])
    return arrays["image"][a:b].reshape(h, w, 3), arrays["validity"][a:b].reshape(h, w), arrays["blending"][a:b].reshape(h, w)


@contextlib.contextmanager
def _scene_context(scene, ctx):
    """the caller's context, or one of its own that is closed on the way out, with the scene's mesh and views set"""
    own = ctx is None
    ctx = ctx or Context()
    try:
        ctx.set_mesh(scene.verts, scene.faces, scene.normals)
        ctx.set_views(scene.cams, scene.images, masks=getattr(scene, "masks", None), levels=getattr(scene, "levels", None))
        yield ctx
    finally:
        if own:
            ctx.close()


def texture_patches(scene, labels, corner_adjust=None, ctx=None, tone_mapping="none"):
    """the texture patches (generate_texture_patches for the labelled faces + adjust_colors, texrecon.cpp:160-184) of a synth.Scene-like
    object and its labels: returns (arrays, stats) of Context.texture_patches.  tone_mapping: "none" | "gamma"."""
    with _scene_context(scene, ctx) as c:
        return c.texture_patches(np.ascontiguousarray(scene.adj_ptr, dtype=np.uint32), np.ascontiguousarray(scene.adj, dtype=np.uint32),
                                 np.ascontiguousarray(labels, dtype=np.uint32), corner_adjust, _toned(None, default_patch_params, tone_mapping))


def local_seam_leveling(scene, labels, params=None, ctx=None, tone_mapping="none"):
    """texrecon.cpp:169-189 for a synth.Scene-like object and its labels: global seam leveling (row f5), the texture patches with
    its adjustments (row f6) and local seam leveling (row f7), the patches staying on the device in between.  Returns (arrays, stats):
    the patch set of Context.texture_patches with image, validity and blending replaced by row f7's, and row f7's stats.
    tone_mapping: "none" | "gamma", passed to rows f5 and f6 (row f7 works on the patch images it is given)."""
    with _scene_context(scene, ctx) as c:
        a = np.ascontiguousarray(scene.adj_ptr, dtype=np.uint32); b = np.ascontiguousarray(scene.adj, dtype=np.uint32)
        lab = np.ascontiguousarray(labels, dtype=np.uint32)
        gp, pp = _toned(None, default_gsl_params, tone_mapping), _toned(None, default_patch_params, tone_mapping)
        gsl, _ = c.global_seam_leveling(a, b, lab, gp, on_device=True)
        dev, _ = c.texture_patches(a, b, lab, gsl["corner_adjust"], pp, on_device=True)
        out, stats = c.local_seam_leveling(a, b, lab, dev, params)
        host, _ = c.texture_patches(a, b, lab, gsl["corner_adjust"], pp)
        host.update(out)
        return host, stats


def texture_atlases(scene, labels, params=None, ctx=None, tone_mapping="none"):
    """texrecon.cpp:169-195 for a synth.Scene-like object and its labels: global seam leveling (row f5), the texture patches with its
    adjustments (row f6), local seam leveling (row f7) and the texture atlases (row f8), the patches staying on the device in
    between.  Returns (arrays, stats) of Context.texture_atlases.  tone_mapping: "none" | "gamma", passed to rows f5, f6 and f8."""
    with _scene_context(scene, ctx) as c:
        a = np.ascontiguousarray(scene.adj_ptr, dtype=np.uint32); b = np.ascontiguousarray(scene.adj, dtype=np.uint32)
        lab = np.ascontiguousarray(labels, dtype=np.uint32)
        return c.texture_atlases(_leveled_patches(c, a, b, lab, tone_mapping), _toned(params, default_atlas_params, tone_mapping))


def _leveled_patches(c, a, b, lab, tone_mapping):
    """rows f5 to f7 in the mode `tone_mapping` on a context with its scene set: the device patch set row f8 reads"""
    gsl, _ = c.global_seam_leveling(a, b, lab, _toned(None, default_gsl_params, tone_mapping), on_device=True)
    dev, _ = c.texture_patches(a, b, lab, gsl["corner_adjust"], _toned(None, default_patch_params, tone_mapping), on_device=True)
    lsl, _ = c.local_seam_leveling(a, b, lab, dev, on_device=True)
    dev = dict(dev); dev.update(image=lsl["image"], validity=lsl["validity"])
    return dev


def debug_view_style(position):
    """background and font colour of the view at `position` of the view list in the debug model: ((r, g, b), (r, g, b)) bytes
    (mvs_debug_view_style; needs no device)"""
    L = load_library()
    bg, fg = (C.c_uint8 * 3)(), (C.c_uint8 * 3)()
    _check(L, L.mvs_debug_view_style(int(position), bg, fg))
    return tuple(bg), tuple(fg)


def view_selection_model(scene, labels, prefix, view_ids=None, vertex_normals=None, ctx=None, tone_mapping="none"):
    """texrecon.cpp:216-236 for a synth.Scene-like object and its labels: writes the debug model `<prefix>_view_selection.obj`, `.mtl` and
    PNGs, whose faces carry the colour and the id of the view that textures them.  Returns Context.view_selection_model's stats.
    tone_mapping: "none" | "gamma", passed to the patches and the atlases -- the files are the same bytes in either mode."""
    with _scene_context(scene, ctx) as c:
        return c.view_selection_model(np.ascontiguousarray(scene.adj_ptr, dtype=np.uint32), np.ascontiguousarray(scene.adj, dtype=np.uint32),
                                      np.ascontiguousarray(labels, dtype=np.uint32), prefix, view_ids, vertex_normals,
                                      _toned(None, default_patch_params, tone_mapping), _toned(None, default_atlas_params, tone_mapping))


def texture_model(scene, labels, prefix, vertex_normals=None, params=None, ctx=None, view_selection_model=False, tone_mapping="none", format="obj"):
    """texrecon.cpp:169-208 for a synth.Scene-like object and its labels: rows f5 to f8 as texture_atlases runs them, then the model
    output (row f9) with the atlases left on the device: writes `<prefix>.obj`, `<prefix>.mtl` and the atlas PNGs.  Returns row f9's
    stats.  vertex_normals: (n_verts, 3) or None (no `vn` lines; vertex_normals(verts, faces) computes area-weighted ones).
    view_selection_model=True writes the debug model `<prefix>_view_selection.*` as well (Context.view_selection_model).
    tone_mapping: "none" | "gamma", passed to every row that reads it (f5, f6, f8 and the debug model).
    format: "obj" (default) | "glb" | "both".  "glb" writes `<prefix>.glb` alone (row f11, Context.save_glb) and returns its stats;
    "both" writes the OBJ route's files as "obj" does, then `<prefix>.glb`, and returns (row f9's stats, row f11's stats).  The debug
    model is an OBJ in every format."""
    if format not in ("obj", "glb", "both"):
        raise ValueError("texture_model: format must be \"obj\", \"glb\" or \"both\", not %r" % (format,))
    with _scene_context(scene, ctx) as c:
        a = np.ascontiguousarray(scene.adj_ptr, dtype=np.uint32); b = np.ascontiguousarray(scene.adj, dtype=np.uint32)
        lab = np.ascontiguousarray(labels, dtype=np.uint32)
        ap = _toned(None, default_atlas_params, tone_mapping)
        atlases, _ = c.texture_atlases(_leveled_patches(c, a, b, lab, tone_mapping), ap, on_device=True)
        stats = c.save_model(atlases, prefix, vertex_normals, params) if format != "glb" else None
        if format != "obj":
            glb_stats = c.save_glb(atlases, os.fspath(prefix) + ".glb", vertex_normals, params)
            stats = glb_stats if format == "glb" else (stats, glb_stats)
        if view_selection_model:   # texrecon.cpp:216-236: after the textured model, on the same context
            c.view_selection_model(a, b, lab, prefix, None, vertex_normals, _toned(None, default_patch_params, tone_mapping), ap, model_params=params)
        return stats


def global_seam_leveling(scene, labels, params=None, ctx=None, tone_mapping="none"):
    """tex::global_seam_leveling for a synth.Scene-like object (verts, faces, normals, cams, images, adj_ptr, adj) and its labels
    (texrecon.cpp:169-172): returns (arrays, stats) of Context.global_seam_leveling.  tone_mapping: "none" | "gamma"."""
    with _scene_context(scene, ctx) as c:
        return c.global_seam_leveling(np.ascontiguousarray(scene.adj_ptr, dtype=np.uint32), np.ascontiguousarray(scene.adj, dtype=np.uint32),
                                      np.ascontiguousarray(labels, dtype=np.uint32), _toned(params, default_gsl_params, tone_mapping))


def _subgraphs_to_numpy(L, sg):
    def grab(ptr, n):
        return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint32)), (max(n, 1),))[:n].copy()
    out = grab(sg.label_ptr, sg.n_labels + 1), grab(sg.comp_ptr, sg.n_components + 1), grab(sg.comp_faces, sg.n_faces)
    L.mvs_subgraphs_free(C.byref(sg))
    return out


def get_subgraphs(adj_ptr, adj, labels, n_labels):
    """UniGraph::get_subgraphs(label, &subgraphs) (libs/tex/uni_graph.cpp:21-55) for label = 0 .. n_labels - 1:
    subgraphs of label L are components label_ptr[L] .. label_ptr[L + 1]; component c is
    comp_faces[comp_ptr[c]:comp_ptr[c + 1]] in the reference's queue order."""
    L = load_library()
    adj_ptr = np.ascontiguousarray(adj_ptr, dtype=np.uint32); adj = np.ascontiguousarray(adj, dtype=np.uint32)
    labels = np.ascontiguousarray(labels, dtype=np.uint32)
    sg = Subgraphs()
    _check(L, L.mvs_get_subgraphs(len(adj_ptr) - 1, adj_ptr.ctypes.data, adj.ctypes.data, labels.ctypes.data, int(n_labels), C.byref(sg)))
    return _subgraphs_to_numpy(L, sg)


def calculate_data_costs(scene, settings=None, ctx=None):
    """tex::calculate_data_costs(mesh, &texture_views, settings, &data_costs) on a synth.Scene-like
    object (verts, faces, normals, cams, images).  Returns (DataCosts on the host, stats)."""
    with _scene_context(scene, ctx) as c:
        stats = c.data_costs(settings)
        return c.costs_download(), stats


def view_selection(data_costs, adj_ptr, adj, params=None, ctx=None):
    """tex::view_selection(data_costs, &graph, settings): returns (UniGraph labels, stats)."""
    own = ctx is None
    ctx = ctx or Context()
    try:
        ctx.costs_upload(data_costs)
        return ctx.view_selection(np.ascontiguousarray(adj_ptr, dtype=np.uint32), np.ascontiguousarray(adj, dtype=np.uint32), params)
    finally:
        if own:
            ctx.close()


def postprocess_face_infos(n_views, info_ptr, view_id, quality, mean_color, settings=None):
    """tex::postprocess_face_infos(settings, &face_projection_infos, &data_costs) (libs/tex/texturing.h:71-74): infos in CSR by
    face, in the caller's order.  Returns (DataCosts, stats)."""
    L = load_library()
    info_ptr = np.ascontiguousarray(info_ptr, dtype=np.uint32); view_id = np.ascontiguousarray(view_id, dtype=np.uint16)
    quality = np.ascontiguousarray(quality, dtype=np.float32)
    mean_color = None if mean_color is None else np.ascontiguousarray(mean_color, dtype=np.float32)
    st = settings or Settings()
    out = CCsr(); ds = DcStats()
    _check(L, L.mvs_postprocess_face_infos(len(info_ptr) - 1, int(n_views), info_ptr.ctypes.data, view_id.ctypes.data, quality.ctypes.data,
                                           None if mean_color is None else mean_color.ctypes.data, C.byref(st), C.byref(out), C.byref(ds)))
    F, nnz = out.n_faces, out.nnz
    def grab(ptr, ctype, n):
        return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(ctype)), (max(n, 1),))[:n].copy()
    res = DataCosts(F, out.n_views, grab(out.col_ptr, C.c_uint32, F + 1), grab(out.view_id, C.c_uint16, nnz), grab(out.cost, C.c_float, nnz))
    L.mvs_csr_free(C.byref(out))
    return res, _stats_dict(ds)


def undistort_image(rgb, flen, dist0, dist1):
    """the undistortion step of from_images_and_camera_files (generate_texture_views.cpp:153-165) on an (H, W, 3) uint8 image"""
    L = load_library()
    rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
    assert rgb.ndim == 3 and rgb.shape[2] == 3
    out = np.empty_like(rgb)
    _check(L, L.mvs_undistort_image(rgb.ctypes.data, rgb.shape[1], rgb.shape[0], float(flen), float(dist0), float(dist1), out.ctypes.data))
    return out


def undistort_host(rgb, flen, dist0, dist1):
    """mvs_undistort_image_host: undistort_image by the sequential host twin of csrc/lens.h -- no GPU; the same bytes"""
    L = load_library()
    rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
    assert rgb.ndim == 3 and rgb.shape[2] == 3
    out = np.empty_like(rgb)
    _check(L, L.mvs_undistort_image_host(rgb.ctypes.data, rgb.shape[1], rgb.shape[0], float(flen), float(dist0), float(dist1), out.ctypes.data))
    return out


def level_size(width, height, level):
    """mvs_level_size: (width, height) of a width x height image at pyramid level `level` (0 .. 4): halved `level` times, rounding up"""
    L = load_library()
    wl, hl = C.c_int32(), C.c_int32()
    _check(L, L.mvs_level_size(int(width), int(height), int(level), C.byref(wl), C.byref(hl)))
    return wl.value, hl.value


def halve_host(rgb, level):
    """mvs_halve_image_host: an (H, W, 3) uint8 image at pyramid level `level` by the sequential host twin of csrc/level.h -- no GPU; the
    bytes the device route leaves (DESIGN.md section 4 "View input" item 14)"""
    L = load_library()
    rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
    assert rgb.ndim == 3 and rgb.shape[2] == 3
    wl, hl = level_size(rgb.shape[1], rgb.shape[0], level)
    out = np.empty((hl, wl, 3), np.uint8)
    _check(L, L.mvs_halve_image_host(rgb.ctypes.data, rgb.shape[1], rgb.shape[0], int(level), out.ctypes.data))
    return out


def halve_mask_host(mask, level):
    """the keep rule of a pyramid level on the host: an (H, W) mask (0 = leave out) -> the level's (0 / 255): a level pixel is kept iff
    every source pixel of its clamped 2^level x 2^level block is kept"""
    m = (np.ascontiguousarray(mask) != 0)
    for _ in range(int(level)):
        h, w = m.shape
        ys, xs = np.minimum(np.arange(0, h + (h & 1), 2) + 1, h - 1), np.minimum(np.arange(0, w + (w & 1), 2) + 1, w - 1)
        m = m[0::2][:, 0::2] & m[0::2][:, xs] & m[ys][:, 0::2] & m[ys][:, xs]
    return m.astype(np.uint8) * 255


def partition_faces(verts, faces, world=1):
    """mvs_partition_faces on host arrays: (perm, part_begin) -- see Context.partition_faces"""
    L = load_library()
    verts = np.ascontiguousarray(verts, dtype=np.float32); faces = np.ascontiguousarray(faces, dtype=np.uint32)
    m = CMesh(int(verts.shape[0]), int(faces.shape[0]), verts.ctypes.data, faces.ctypes.data, None)
    perm = np.zeros(max(faces.shape[0], 1), dtype=np.uint32); part = np.zeros(world + 1, dtype=np.uint32)
    _check(L, L.mvs_partition_faces(C.byref(m), int(world), perm.ctypes.data_as(C.c_void_p), part.ctypes.data_as(C.c_void_p)))
    return perm[:faces.shape[0]], part


def prepare_mesh(verts, faces):
    """tex::prepare_mesh(mesh_info, mesh) (libs/tex/prepare_mesh.cpp:57-70): (faces without redundant ones, face normals)"""
    L = load_library()
    verts = np.ascontiguousarray(verts, dtype=np.float32); faces = np.ascontiguousarray(faces, dtype=np.uint32)
    F = faces.shape[0]
    fo = np.zeros((max(F, 1), 3), np.uint32); no = np.zeros((max(F, 1), 3), np.float32); kept = C.c_uint32(0)
    _check(L, L.mvs_prepare_mesh(verts.shape[0], verts.ctypes.data, F, faces.ctypes.data, fo.ctypes.data, no.ctypes.data, C.byref(kept)))
    return fo[:kept.value].copy(), no[:kept.value].copy()


def build_adjacency_graph(n_verts, faces):
    """tex::build_adjacency_graph(mesh, mesh_info, &graph) (libs/tex/build_adjacency_graph.cpp:16-53): (adj_ptr, adj)"""
    L = load_library()
    faces = np.ascontiguousarray(faces, dtype=np.uint32)
    F = faces.shape[0]
    adj_ptr = np.zeros(F + 1, np.uint32); pa = C.c_void_p(); n = C.c_uint64(0)
    _check(L, L.mvs_build_adjacency_graph(int(n_verts), F, faces.ctypes.data, adj_ptr.ctypes.data, C.byref(pa), C.byref(n)))
    adj = np.ctypeslib.as_array(C.cast(pa, C.POINTER(C.c_uint32)), (max(n.value, 1),))[:n.value].copy()
    C.CDLL(None).free(pa)
    return adj_ptr, adj
