"""ctypes driver of the CPU model of global seam leveling (seam_model.cpp; DESIGN.md section 4 "Global seam leveling").
Built on first use with g++ -O2 -mfma -ffp-contract=off -fno-fast-math.  Test infrastructure only."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "seam_model.cpp")
LIB = os.path.join(HERE, "libseam_model.so")
ARRAYS = {"x_ptr": np.uint32, "x_label": np.uint32, "ring_ptr": np.uint32, "ring": np.uint32, "a_col": np.uint32, "b": np.float32,
          "lhs_ptr": np.uint32, "lhs_col": np.uint32, "lhs_val": np.float32, "rhs": np.float32, "x_raw": np.float32,
          "x_adjust": np.float32, "corner_adjust": np.float32, "patch_label": np.uint32, "face_patch": np.uint32}
STATS = ("patches", "merged", "x_rows", "a_rows", "gamma_rows", "lhs_nnz_lower", "seam_edges", "samples")
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
        L.seam_model_run.restype = vp
        L.seam_model_run.argtypes = [C.c_uint32, vp, C.c_uint32, vp, C.c_uint32, vp, vp, vp, vp, vp, vp, vp, C.c_float, C.c_uint32, C.c_float]
        L.seam_model_status.argtypes = [vp]; L.seam_model_status.restype = C.c_int
        L.seam_model_stats.argtypes = [vp, vp, vp, vp]
        L.seam_model_array.argtypes = [vp, C.c_char_p, C.POINTER(C.c_uint64)]; L.seam_model_array.restype = vp
        L.seam_model_free.argtypes = [vp]
        _lib = L
    return _lib


def run(verts, faces, cams, images, adj_ptr, adj, labels, tolerance=1e-4, max_iterations=1000, lam=0.1):
    """(status, arrays, stats): status 4 = MVS_ERR_LABELING (arrays and stats None).  Arrays with three channels are interleaved
    per row (x_adjust[3 row + c]), corner_adjust[9 f + 3 k + c]; the Lhs is the FULL symmetric CSR (lower_csr keeps the lower part)."""
    L = load()
    V = len(images)
    verts = np.ascontiguousarray(verts, np.float32); faces = np.ascontiguousarray(faces, np.uint32)
    K = np.ascontiguousarray(np.asarray(cams["K"], np.float32).reshape(V, 9))
    w2c = np.ascontiguousarray(np.asarray(cams["w2c"], np.float32).reshape(V, -1)[:, :12])
    wh = np.ascontiguousarray(np.stack([np.asarray(cams["width"]), np.asarray(cams["height"])], 1).astype(np.int32))
    imgs = [np.ascontiguousarray(im, np.uint8) for im in images]
    ptrs = (C.c_void_p * max(V, 1))(*[im.ctypes.data for im in imgs])
    adj_ptr = np.ascontiguousarray(adj_ptr, np.uint32); adj = np.ascontiguousarray(adj, np.uint32)
    if adj.size == 0:
        adj = np.zeros(1, np.uint32)
    labels = np.ascontiguousarray(labels, np.uint32)
    h = L.seam_model_run(len(verts), verts.ctypes.data, len(faces), faces.ctypes.data, V, K.ctypes.data, w2c.ctypes.data, wh.ctypes.data,
                         ptrs, adj_ptr.ctypes.data, adj.ctypes.data, labels.ctypes.data, tolerance, max_iterations, lam)
    try:
        st = L.seam_model_status(h)
        if st:
            return st, None, None
        out = {}
        for name, dt in ARRAYS.items():
            n = C.c_uint64()
            p = L.seam_model_array(h, name.encode(), C.byref(n))
            ct = C.c_uint32 if dt == np.uint32 else C.c_float
            out[name] = np.ctypeslib.as_array(C.cast(p, C.POINTER(ct)), (n.value,)).copy() if n.value else np.zeros(0, dt)
        s = (C.c_uint64 * 8)(); it = (C.c_uint32 * 3)(); er = (C.c_float * 3)()
        L.seam_model_stats(h, s, it, er)
        stats = dict(zip(STATS, [int(x) for x in s]))
        stats["iterations"] = [int(x) for x in it]
        stats["error"] = np.array(list(er), np.float32)
        return 0, out, stats
    finally:
        L.seam_model_free(h)


def run_scene(scene, labels, **kw):
    return run(scene.verts, scene.faces, scene.cams, scene.images, scene.adj_ptr, scene.adj, labels, **kw)


def lower_csr(ptr, col, val):
    """the lower triangle (col <= row) of a CSR matrix"""
    n = len(ptr) - 1
    rows = np.repeat(np.arange(n), np.diff(ptr.astype(np.int64)))
    keep = col.astype(np.int64) <= rows
    lp = np.zeros(n + 1, np.uint32)
    lp[1:] = np.cumsum(np.bincount(rows[keep], minlength=n))
    return lp, col[keep], val[keep]


# ---- inputs and checks shared by tests/test_seam_model.py (CPU) and tests/test_gpu_seam_leveling.py ----

def valid_views(scene, margin=2.0):
    """[F, V] bool: all three corners of the face project into view j with `margin` pixels to spare (float64, in front of the camera)"""
    V = len(scene.images)
    P = scene.verts[scene.faces].astype(np.float64)
    ok = np.zeros((len(scene.faces), V), bool)
    for j in range(V):
        w = np.asarray(scene.cams["w2c"][j], np.float64).ravel()[:12].reshape(3, 4)
        K = np.asarray(scene.cams["K"][j], np.float64).reshape(3, 3)
        q = (P @ w[:, :3].T + w[:, 3]) @ K.T
        with np.errstate(all="ignore"):
            px = q[..., 0] / q[..., 2] - 0.5; py = q[..., 1] / q[..., 2] - 0.5
        W, H = int(scene.cams["width"][j]), int(scene.cams["height"][j])
        ok[:, j] = np.all((q[..., 2] > 0) & (px >= margin) & (py >= margin) & (px <= W - 1 - margin) & (py <= H - 1 - margin), axis=1)
    return ok


def crafted_labelings(scene, seed=0):
    """labelings that keep every labelled face inside its view: name -> labels"""
    ok = valid_views(scene)
    rng = np.random.default_rng(seed)
    has = ok.any(1)
    first = np.where(has, 1 + ok.argmax(1), 0).astype(np.uint32)
    last = np.where(has, ok.shape[1] - ok[:, ::-1].argmax(1), 0).astype(np.uint32)
    rand = np.zeros(len(scene.faces), np.uint32)
    for f in np.nonzero(has)[0]:
        rand[f] = 1 + rng.choice(np.nonzero(ok[f])[0])
    blocks = np.where((np.arange(len(scene.faces)) // 40) % 2 == 0, first, last).astype(np.uint32)
    holes = rand.copy(); holes[rng.random(len(holes)) < 0.2] = 0
    return {"first": first, "last": last, "random": rand, "blocks": blocks, "random_with_unseen": holes}


def face_adjacency(faces):
    """faces sharing an edge (non-manifold edges included), ascending per face"""
    from collections import defaultdict
    e2f = defaultdict(list)
    for f, (a, b, c) in enumerate(np.asarray(faces).tolist()):
        for u, v in ((a, b), (b, c), (c, a)):
            if u != v:
                e2f[(min(u, v), max(u, v))].append(f)
    nb = [set() for _ in range(len(faces))]
    for fs in e2f.values():
        for f in fs:
            nb[f].update(g for g in fs if g != f)
    adj_ptr = np.zeros(len(faces) + 1, np.uint32)
    adj_ptr[1:] = np.cumsum([len(n) for n in nb])
    adj = np.array([g for n in nb for g in sorted(n)], np.uint32)
    return adj_ptr, adj


def grid_scene(n=6, W=64, H=48, fin=False, zero_edge=False, outside=False, seed=3, xs=None, ys=None):
    """an n x n vertex grid on the plane z = 1 seen by two identical pinhole cameras at the origin (different images): vertex (i, j)
    projects to pixel (xs[i], ys[j]); the first column and row land in [0, 1), so a candidate's frame starts at -1, and the last ones
    just below W - 1 / H - 1.  fin: a third face on an interior edge (non-manifold); zero_edge: a face with two vertices at the same
    point (an edge of length 0); outside: one vertex projects left of the image.  xs / ys: the n pixel columns / rows instead of
    the even spacing."""
    import mvs_texturing_amd as M
    f = 50.0; cx, cy = W / 2.0, H / 2.0
    xs = np.linspace(0.3, W - 1.6, n) if xs is None else np.asarray(xs, np.float64)
    ys = np.linspace(0.4, H - 1.7, n) if ys is None else np.asarray(ys, np.float64)
    assert len(xs) == n and len(ys) == n
    verts = [[(x + 0.5 - cx) / f, (y + 0.5 - cy) / f, 1.0] for y in ys for x in xs]
    faces = []
    for j in range(n - 1):
        for i in range(n - 1):
            a, b, c, d = j * n + i, j * n + i + 1, (j + 1) * n + i, (j + 1) * n + i + 1
            faces += [[a, b, c], [b, d, c]]
    if fin:
        a, b = (n // 2) * n + n // 2, (n // 2) * n + n // 2 + 1
        p = (np.array(verts[a]) + np.array(verts[b])) / 2 * 0.9      # nearer the cameras, same pixel column range
        verts.append(p.tolist()); faces.append([a, b, len(verts) - 1])
    if zero_edge:
        a, b = n + 1, n + 2
        verts.append(list(verts[a])); faces.append([a, len(verts) - 1, b])
    if outside:
        verts[0] = [(-3.0 + 0.5 - cx) / f, verts[0][1], 1.0]
    s = M.synth.Scene()
    s.verts = np.ascontiguousarray(np.array(verts, np.float32))
    s.faces = np.ascontiguousarray(np.array(faces, np.uint32))
    s.normals = np.ascontiguousarray(np.tile(np.float32([0, 0, -1]), (len(faces), 1)))
    s.adj_ptr, s.adj = face_adjacency(s.faces)
    K = np.float32([f, 0, cx, 0, f, cy, 0, 0, 1])
    rng = np.random.default_rng(seed)
    s.cams = {"pos": np.zeros((2, 3), np.float32), "viewdir": np.tile(np.float32([0, 0, 1]), (2, 1)), "K": np.stack([K, K]),
              "w2c": np.stack([np.eye(4, dtype=np.float32).ravel()] * 2), "width": np.int32([W, W]), "height": np.int32([H, H])}
    s.images = [np.ascontiguousarray(rng.integers(0, 256, (H, W, 3)).astype(np.uint8)) for _ in range(2)]
    return s


def grid_labels(scene):
    """left half of the grid view 1, right half view 2 (by the face's first corner); extra faces view 2"""
    x = scene.verts[scene.faces[:, 0], 0]
    return np.where(x < np.median(x), 1, 2).astype(np.uint32)


def normal_residual(arrays, x_rows):
    """||Lhs x_raw - Rhs|| / ||Rhs|| per channel in float64 (scipy), from the model's full CSR"""
    import scipy.sparse as sp
    A = sp.csr_matrix((arrays["lhs_val"].astype(np.float64), arrays["lhs_col"], arrays["lhs_ptr"].astype(np.int64)), shape=(x_rows, x_rows))
    x = arrays["x_raw"].reshape(x_rows, 3).astype(np.float64); b = arrays["rhs"].reshape(x_rows, 3).astype(np.float64)
    out = []
    for c in range(3):
        nb = np.linalg.norm(b[:, c])
        out.append(0.0 if nb == 0 else float(np.linalg.norm(A @ x[:, c] - b[:, c]) / nb))
    return out


def seam_difference(a_col, b, x_adjust):
    """mean |colour2 - colour1| over the A rows before and after the adjustment: (mean |b|, mean |b - (x(v, l1) - x(v, l2))|)"""
    a_col = a_col.reshape(-1, 2); b = b.reshape(-1, 3); x = x_adjust.reshape(-1, 3)
    after = b - (x[a_col[:, 0]] - x[a_col[:, 1]])
    return float(np.abs(b).mean()), float(np.abs(after).mean())


def planted_scene(scene, seed=5, amp=40):
    """the scene with a constant colour offset per view (clipped to u8)"""
    import copy
    rng = np.random.default_rng(seed)
    s = copy.copy(scene)
    off = rng.integers(-amp, amp + 1, (len(scene.images), 3))
    s.images = [np.ascontiguousarray(np.clip(im.astype(np.int32) + off[j], 0, 255).astype(np.uint8)) for j, im in enumerate(scene.images)]
    return s
