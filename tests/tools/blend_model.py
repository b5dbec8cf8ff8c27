"""ctypes driver of the CPU model of row f7 (blend_model.cpp; DESIGN.md section 4 "Local seam leveling"), plus numpy statements of the
order-free rules the device uses (distance form of prepare_blending_mask) and of the Poisson system of item 8.  Built on first use
with g++ -O2 -mfma -ffp-contract=off -fno-fast-math.  Test infrastructure only."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "blend_model.cpp")
LIB = os.path.join(HERE, "libblend_model.so")
PATCH_ARRAYS = {"label": np.uint32, "box": np.int32, "face_ptr": np.uint32, "faces": np.uint32, "texcoords": np.float32, "pix_ptr": np.uint64,
                "image": np.float32, "validity": np.uint8, "blending": np.uint8}
ARRAYS = {"image": np.float32, "validity": np.uint8, "blending": np.uint8, "after_writes": np.float32, "blend_writes": np.uint8, "iters": np.uint32,
          "err": np.float32}
# the first 20 names are mvs_lsl_stats' counters in order (viewsel.LSL_COUNTS + iterations_max)
STATS = ("seam_edges", "skipped_pairs", "vertex_infos", "edge_projections", "colour_samples", "invalid_samples", "vertex_writes", "line_writes",
         "written_pixels", "outside_frame", "invalid_writes", "strip_pixels", "fixed_pixels", "demoted", "patches_lds", "patches_global",
         "pixels_global", "iterations_total", "hit_max_iterations", "iterations_max")
COUNTERS = ("overwrites", "zero_lines", "label0_seams", "duplicate_edges", "vertices_3", "inner_pixels", "ring_pixels", "sanitized", "clamped_idx")
DEFAULTS = dict(tolerance=1e-6, max_iterations=700, strip_width=20, lds_bytes=147456)
_lib = None


def build(force=False):
    if force or not os.path.exists(LIB) or os.path.getmtime(LIB) < os.path.getmtime(SRC):
        subprocess.check_call(["g++", "-O2", "-mfma", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-std=c++17", "-shared", "-o", LIB, SRC])
    return LIB


def load():
    global _lib
    if _lib is None:
        L = C.CDLL(build())
        vp = C.c_void_p
        L.blend_model_run.restype = vp
        L.blend_model_run.argtypes = [C.c_uint32, C.c_uint32, vp, vp, vp, vp, C.c_uint32, C.c_uint32, C.c_uint64] + [vp] * 9 + \
                                     [C.c_float, C.c_uint32, C.c_uint32, C.c_uint32]
        L.blend_model_status.argtypes = [vp]; L.blend_model_status.restype = C.c_int
        L.blend_model_stats.argtypes = [vp, vp, vp, vp]
        L.blend_model_array.argtypes = [vp, C.c_char_p, C.POINTER(C.c_uint64)]; L.blend_model_array.restype = vp
        L.blend_model_free.argtypes = [vp]
        L.blend_model_prepare_mask.argtypes = [C.c_int32, C.c_int32, vp, vp, C.c_uint32]; L.blend_model_prepare_mask.restype = None
        L.blend_model_solve.argtypes = [C.c_int32, C.c_int32, vp, vp, vp, C.c_float, C.c_uint32, vp, vp, vp]; L.blend_model_solve.restype = None
        _lib = L
    return _lib


def flat(patches):
    """a patch set (the model's, the library's, or a crafted dict) as flat contiguous arrays of the right types"""
    return {k: np.ascontiguousarray(patches[k], dt).reshape(-1) for k, dt in PATCH_ARRAYS.items()}


def run(n_verts, faces, adj_ptr, adj, labels, patches, **params):
    """(status, arrays, stats, counters): status 4 = MVS_ERR_LABELING (the rest None).  arrays: image (n_pixels, 3), validity, blending
    (the prepared mask), after_writes / blend_writes (the state after item 6), iters / err (P, 3)."""
    L = load()
    P = dict(DEFAULTS); P.update(params)
    faces = np.ascontiguousarray(faces, np.uint32); adj_ptr = np.ascontiguousarray(adj_ptr, np.uint32)
    adj = np.ascontiguousarray(adj, np.uint32); labels = np.ascontiguousarray(labels, np.uint32)
    if adj.size == 0:
        adj = np.zeros(1, np.uint32)
    a = flat(patches)
    NP = a["label"].size
    if NP == 0:
        a["pix_ptr"] = np.zeros(1, np.uint64); a["face_ptr"] = np.zeros(1, np.uint32)
    ptr = lambda x: x.ctypes.data if x.size else None
    h = L.blend_model_run(int(n_verts), len(faces), ptr(faces), ptr(adj_ptr), ptr(adj), ptr(labels), NP, a["faces"].size, a["validity"].size,
                          *[ptr(a[k]) for k in PATCH_ARRAYS], float(P["tolerance"]), int(P["max_iterations"]), int(P["strip_width"]), int(P["lds_bytes"]))
    try:
        st = L.blend_model_status(h)
        if st:
            return st, None, None, None
        out = {}
        for name, dt in ARRAYS.items():
            n = C.c_uint64()
            p = L.blend_model_array(h, name.encode(), C.byref(n))
            out[name] = np.frombuffer(C.string_at(p, n.value * np.dtype(dt).itemsize), dt).copy() if n.value else np.zeros(0, dt)
        if NP and out["after_writes"].size == 0:
            out["after_writes"] = a["image"].copy(); out["blend_writes"] = a["blending"].copy()
        out["image"] = out["image"].reshape(-1, 3); out["after_writes"] = out["after_writes"].reshape(-1, 3)
        out["iters"] = out["iters"].reshape(-1, 3); out["err"] = out["err"].reshape(-1, 3)
        s = (C.c_uint64 * len(STATS))(); c = (C.c_uint64 * len(COUNTERS))(); e = C.c_float()
        L.blend_model_stats(h, s, c, C.byref(e))
        stats = dict(zip(STATS, [int(x) for x in s])); stats["error_max"] = float(e.value)
        return 0, out, stats, dict(zip(COUNTERS, [int(x) for x in c]))
    finally:
        L.blend_model_free(h)


def run_scene(scene, labels, patches, **params):
    return run(len(scene.verts), scene.faces, scene.adj_ptr, scene.adj, labels, patches, **params)


def prepare_mask(validity, blending, strip_width=20):
    """upstream's prepare_blending_mask loops on one patch: (h, w) uint8 arrays -> the prepared mask"""
    L = load()
    val = np.ascontiguousarray(validity, np.uint8); bl = np.ascontiguousarray(blending, np.uint8).copy()
    h, w = val.shape
    L.blend_model_prepare_mask(w, h, val.ctypes.data, bl.ctypes.data, int(strip_width))
    return bl


def solve(mask, orig, after, tolerance=DEFAULTS["tolerance"], max_iterations=DEFAULTS["max_iterations"]):
    """the model's items 8 - 9 on one patch alone: mask (h, w), orig / after (h, w, 3) -> (solution, iters[3], err[3], (unknowns, fixed, demoted))"""
    L = load()
    m = np.ascontiguousarray(mask, np.uint8); o = np.ascontiguousarray(orig, np.float32); x = np.ascontiguousarray(after, np.float32).copy()
    h, w = m.shape
    it = np.zeros(3, np.uint32); err = np.zeros(3, np.float32); cnt = np.zeros(3, np.uint64)
    L.blend_model_solve(w, h, m.ctypes.data, o.ctypes.data, x.ctypes.data, float(tolerance), int(max_iterations), it.ctypes.data, err.ctypes.data, cnt.ctypes.data)
    return x, it, err, tuple(int(v) for v in cnt)


def patch(patches, arrays, i):
    """patch i: (image (h, w, 3), validity (h, w), blending (h, w)) of `arrays` (a result: image / validity / blending packed as the set)"""
    box = np.asarray(patches["box"]).reshape(-1, 4)
    w, h = int(box[i, 2]), int(box[i, 3])
    a, b = int(patches["pix_ptr"][i]), int(patches["pix_ptr"][i + 1])
    return np.asarray(arrays["image"]).reshape(-1, 3)[a:b].reshape(h, w, 3), arrays["validity"][a:b].reshape(h, w), arrays["blending"][a:b].reshape(h, w)


# ---- the order-free rules in numpy ----

def chessboard_distance(valid, cap):
    """distance (chessboard metric) of every pixel to the nearest invalid pixel or to the outside of the frame, capped"""
    h, w = valid.shape
    big = np.zeros((h + 2 * cap, w + 2 * cap), bool)
    big[cap:cap + h, cap:cap + w] = valid
    d = np.full((h, w), cap, np.int64)
    ok = np.ones((h, w), bool)
    for r in range(0, cap):            # ok after round r: every pixel within chessboard distance r is valid
        ring = np.ones((h, w), bool)
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                if max(abs(dx), abs(dy)) == r:
                    ring &= big[cap + dy:cap + dy + h, cap + dx:cap + dx + w]
        newly = ok & ~ring
        d[newly] = r
        ok &= ring
    return d


def rule_prepare_mask(validity, blending, strip_width=20):
    """item 7 in its distance form: sanitize, then distance > strip -> 0, distance == strip + 1 -> 128"""
    val = np.asarray(validity) != 0
    bl = np.asarray(blending, np.uint8).copy()
    h, w = bl.shape
    d = chessboard_distance(val, strip_width + 2)
    is255 = bl == 255
    san = np.zeros_like(val)
    san[1:-1, 1:-1] = (bl[1:-1, 1:-1] == 128) & is255[1:-1, :-2] & is255[1:-1, 2:] & is255[:-2, 1:-1] & is255[2:, 1:-1]
    bl[san] = 255
    bl[d > strip_width] = 0
    bl[d == strip_width + 1] = 128
    return bl


def poisson_system(mask, orig, after):
    """item 8 assembled independently: returns (A (scipy CSR, fp64, SPD form), rhs (n, 3) fp64 from the fp32 right-hand sides, idx (n,) flat
    pixel indices of the unknowns in row-major order)"""
    import scipy.sparse as sp
    m = np.asarray(mask); h, w = m.shape
    unk = np.zeros((h, w), bool)
    unk[1:-1, 1:-1] = (m[1:-1, 1:-1] == 255) & (m[1:-1, :-2] != 0) & (m[1:-1, 2:] != 0) & (m[:-2, 1:-1] != 0) & (m[2:, 1:-1] != 0)
    idx = np.flatnonzero(unk.ravel())
    num = -np.ones(h * w, np.int64); num[idx] = np.arange(len(idx))
    o = np.asarray(orig, np.float32).reshape(h * w, 3); x0 = np.asarray(after, np.float32).reshape(h * w, 3)
    f32 = np.float32
    lap = lambda img, j: f32(f32(f32(f32(f32(-4.0) * img[j]) + img[j - w]) + img[j - 1]) + img[j + 1]) + img[j + w]
    rows, cols, vals = [], [], []
    rhs = np.zeros((len(idx), 3), np.float64)
    for k, j in enumerate(idx):
        b = lap(o, j)                      # alpha = 1: the Laplacian of the original
        s = -b.astype(np.float64)
        rows.append(k); cols.append(k); vals.append(4.0)
        for nb in (j - w, j - 1, j + 1, j + w):
            if num[nb] >= 0:
                rows.append(k); cols.append(num[nb]); vals.append(-1.0)
            else:
                s = s + x0[nb].astype(np.float64)
        rhs[k] = s
    A = sp.csr_matrix((vals, (rows, cols)), shape=(len(idx), len(idx)))
    return A, rhs, idx
