"""ctypes driver of the CPU model of row f6 (patch_model.cpp; DESIGN.md section 4 "Texture patches"), plus a numpy statement of the
order-free rule the device uses.  Built on first use with g++ -O2 -mfma -ffp-contract=off -fno-fast-math.  Test infrastructure only."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "patch_model.cpp")
LIB = os.path.join(HERE, "libpatch_model.so")
ARRAYS = {"label": np.uint32, "box": np.int32, "face_ptr": np.uint32, "faces": np.uint32, "texcoords": np.float32, "pix_ptr": np.uint64,
          "image": np.float32, "validity": np.uint8, "blending": np.uint8}
STATS = ("patches", "merged", "listed_faces", "degenerate_faces", "pixels", "valid_pixels", "near_pixels")
COUNTERS = ("absorbed", "inside_twice", "near_then_inside", "degenerate", "frame_negative", "magenta_near", "magenta_inside", "magenta", "clamped",
            "chain", "absorber_later", "equal_boxes")
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
        L.patch_model_run.restype = vp
        L.patch_model_run.argtypes = [C.c_uint32, vp, C.c_uint32, vp, C.c_uint32, vp, vp, vp, vp, vp, vp, vp, vp]
        L.patch_model_adjust_colors.argtypes = [C.c_int32, C.c_int32, vp, C.c_uint32, vp, vp, vp, vp, vp]
        L.patch_model_adjust_colors.restype = None
        L.patch_model_status.argtypes = [vp]; L.patch_model_status.restype = C.c_int
        L.patch_model_stats.argtypes = [vp, vp, vp]
        L.patch_model_array.argtypes = [vp, C.c_char_p, C.POINTER(C.c_uint64)]; L.patch_model_array.restype = vp
        L.patch_model_free.argtypes = [vp]
        _lib = L
    return _lib


def run(verts, faces, cams, images, adj_ptr, adj, labels, corner_adjust=None):
    """(status, arrays, stats, counters): status 4 = MVS_ERR_LABELING (the rest None).  Arrays are flat, as mvs_patch_set has them."""
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
    ca = None if corner_adjust is None else np.ascontiguousarray(corner_adjust, np.float32).reshape(-1)
    assert ca is None or ca.size == 9 * len(faces)
    h = L.patch_model_run(len(verts), verts.ctypes.data, len(faces), faces.ctypes.data, V, K.ctypes.data, w2c.ctypes.data, wh.ctypes.data,
                          ptrs, adj_ptr.ctypes.data, adj.ctypes.data, labels.ctypes.data, None if ca is None else ca.ctypes.data)
    try:
        st = L.patch_model_status(h)
        if st:
            return st, None, None, None
        out = {}
        for name, dt in ARRAYS.items():
            n = C.c_uint64()
            p = L.patch_model_array(h, name.encode(), C.byref(n))
            out[name] = np.frombuffer(C.string_at(p, n.value * np.dtype(dt).itemsize), dt).copy() if n.value else np.zeros(0, dt)
        s = (C.c_uint64 * len(STATS))(); c = (C.c_uint64 * len(COUNTERS))()
        L.patch_model_stats(h, s, c)
        return 0, out, dict(zip(STATS, [int(x) for x in s])), dict(zip(COUNTERS, [int(x) for x in c]))
    finally:
        L.patch_model_free(h)


def run_scene(scene, labels, corner_adjust=None):
    return run(scene.verts, scene.faces, scene.cams, scene.images, scene.adj_ptr, scene.adj, labels, corner_adjust)


def adjust_colors(w, h, image, texcoords, adjust):
    """the model's TexturePatch::adjust_colors on one patch: image (h, w, 3) float32, texcoords (n, 3, 2), adjust (n, 3, 3) ->
    (image, validity (h, w), blending (h, w), counters)"""
    L = load()
    img = np.ascontiguousarray(image, np.float32).reshape(h, w, 3).copy()
    tc = np.ascontiguousarray(texcoords, np.float32).reshape(-1, 6); av = np.ascontiguousarray(adjust, np.float32).reshape(-1, 9)
    assert len(tc) == len(av)
    val = np.zeros((h, w), np.uint8); bl = np.zeros((h, w), np.uint8)
    c = (C.c_uint64 * len(COUNTERS))()
    L.patch_model_adjust_colors(w, h, img.ctypes.data, len(tc), tc.ctypes.data if len(tc) else None, av.ctypes.data if len(av) else None,
                                val.ctypes.data, bl.ctypes.data, c)
    return img, val, bl, dict(zip(COUNTERS, [int(x) for x in c]))


def patch(arrays, i):
    """patch i of a flat patch set (the model's or the library's host arrays): (image (h, w, 3), validity (h, w), blending (h, w)) as views"""
    w, h = int(arrays["box"].reshape(-1, 4)[i, 2]), int(arrays["box"].reshape(-1, 4)[i, 3])
    a, b = int(arrays["pix_ptr"][i]), int(arrays["pix_ptr"][i + 1])
    assert b - a == w * h
    return arrays["image"].reshape(-1)[3 * a:3 * b].reshape(h, w, 3), arrays["validity"][a:b].reshape(h, w), arrays["blending"][a:b].reshape(h, w)


# ---- the order-free rule in numpy (fp32 arithmetic spelled out operation by operation) ----

def _f(x):
    return np.asarray(x, np.float32)


def rule_adjust_colors(w, h, image, texcoords, adjust, return_weights=False):
    """a pixel with an inside face takes the LAST such face of the list (blending 255); else with a near face the FIRST (64); else
    it is invalid (0, image 0).  Returns (image, validity, blending) [+ the winner's list index per pixel (-1: none) and its fp32
    barycentric weights (h, w, 3) with return_weights]."""
    img = _f(image).reshape(h, w, 3).copy()
    tc = _f(texcoords).reshape(-1, 3, 2); av = _f(adjust).reshape(-1, 3, 3)
    n = len(tc)
    win_in = np.zeros((h, w), np.int64); win_near = np.full((h, w), n, np.int64)
    eps = np.float32(np.finfo(np.float32).eps); sqrt_2 = np.float32(np.sqrt(2.0)); two = np.float32(2.0); one = np.float32(1.0)

    def bary(t, X, Y):
        (v1x, v1y), (v2x, v2y), (v3x, v3y) = t
        detT = _f(_f((v1x - v3x) * (v2y - v3y)) - _f((v1y - v3y) * (v2x - v3x)))
        with np.errstate(all="ignore"):
            alpha = _f(_f(_f((v2y - v3y) * _f(X - v3x)) + _f((v3x - v2x) * _f(Y - v3y))) / detT)
            beta = _f(_f(_f((v3y - v1y) * _f(X - v3x)) + _f((v1x - v3x) * _f(Y - v3y))) / detT)
        return alpha, beta, _f(_f(one - alpha) - beta)

    for i in range(n):
        t = tc[i]
        (v1x, v1y), (v2x, v2y), (v3x, v3y) = t
        area = _f(np.float32(0.5) * np.abs(_f(_f((v2x - v1x) * (v3y - v1y)) - _f((v2y - v1y) * (v3x - v1x)))))
        if area < eps:
            continue
        x0 = max(int(np.floor(t[:, 0].min())) - 1, 0); y0 = max(int(np.floor(t[:, 1].min())) - 1, 0)
        x1 = min(int(np.ceil(t[:, 0].max())) + 1, w); y1 = min(int(np.ceil(t[:, 1].max())) + 1, h)
        if x1 <= x0 or y1 <= y0:
            continue
        Y, X = np.meshgrid(np.arange(y0, y1, dtype=np.float32), np.arange(x0, x1, dtype=np.float32), indexing="ij")
        a, b, g = bary(t, X, Y)
        m = a.copy(); m = np.where(b < m, b, m); m = np.where(g < m, g, m)
        inside = m >= 0
        nrm = lambda dx, dy: _f(np.sqrt(_f(_f(dx * dx) + _f(dy * dy))))
        with np.errstate(all="ignore"):
            ha = _f(_f(_f(two * -a) * area) / nrm(v2x - v3x, v2y - v3y))
            hb = _f(_f(_f(two * -b) * area) / nrm(v1x - v3x, v1y - v3y))
            hc = _f(_f(_f(two * -g) * area) / nrm(v1x - v2x, v1y - v2y))
            near = ~inside & ~((ha > sqrt_2) | (hb > sqrt_2) | (hc > sqrt_2))
        wi = win_in[y0:y1, x0:x1]; wn = win_near[y0:y1, x0:x1]
        wi[inside] = i + 1                     # faces in ascending order: the last inside face stays
        wn[near & (wn == n)] = i               # the first near face stays
    valid = (win_in > 0) | (win_near < n)
    idx = np.where(win_in > 0, win_in - 1, np.where(win_near < n, win_near, 0))
    val = np.where(valid, 255, 0).astype(np.uint8)
    bl = np.where(win_in > 0, 255, np.where(win_near < n, 64, 0)).astype(np.uint8)
    wts = np.zeros((h, w, 3), np.float32)
    if n:
        T = tc[idx]                                  # (h, w, 3, 2): the winner's corners per pixel
        Y, X = np.meshgrid(np.arange(h, dtype=np.float32), np.arange(w, dtype=np.float32), indexing="ij")
        a, b, g = bary(((T[..., 0, 0], T[..., 0, 1]), (T[..., 1, 0], T[..., 1, 1]), (T[..., 2, 0], T[..., 2, 1])), X, Y)
        wts = np.stack([a, b, g], -1)
        A = av[idx]                                  # (h, w, 3 corners, 3 channels)
        with np.errstate(all="ignore"):
            for c in range(3):
                adj = _f(_f(_f(A[..., 0, c] * a) + _f(A[..., 1, c] * b)) + _f(A[..., 2, c] * g))
                img[..., c] = np.where(valid, _f(img[..., c] + adj), np.float32(0))
    else:
        img[:] = 0
    if return_weights:
        return img, val, bl, np.where(valid, idx, -1), wts
    return img, val, bl


def crop(scene, label, box):
    """the float crop of view label - 1 under frame box = (min_x, min_y, w, h); outside the view (255, 0, 255) / 255"""
    im = scene.images[label - 1]
    H, W = im.shape[:2]
    mx, my, w, h = [int(v) for v in box]
    out = np.empty((h, w, 3), np.uint8); out[:] = (255, 0, 255)
    xs = np.arange(mx, mx + w); ys = np.arange(my, my + h)
    okx = (xs >= 0) & (xs < W); oky = (ys >= 0) & (ys < H)
    out[np.ix_(oky, okx)] = im[np.ix_(ys[oky], xs[okx])]
    return out.astype(np.float32) / np.float32(255.0)


def island_scene():
    """seam_model.grid_scene(n=8, fin=True, zero_edge=True) labelled 1 everywhere except a ring of label 2 around one cell that keeps
    label 1: that cell is a second candidate of label 1 whose box lies inside the first one's, so the merge absorbs it, and its two
    faces are listed again on top of pixels the ring's neighbours already reach.  Returns (scene, labels)."""
    import seam_model as SM
    g = SM.grid_scene(n=8, fin=True, zero_edge=True)
    n = 8
    labels = np.ones(len(g.faces), np.uint32)
    cx = g.verts[g.faces[:, :3]].mean(1)                       # centroids on z = 1
    xs = np.unique(g.verts[:n * n, 0]); ys = np.unique(g.verts[:n * n, 1])
    ix = np.clip(np.searchsorted(xs, cx[:, 0]) - 1, 0, n - 2); iy = np.clip(np.searchsorted(ys, cx[:, 1]) - 1, 0, n - 2)
    ring = (ix >= 2) & (ix <= 4) & (iy >= 2) & (iy <= 4)
    core = (ix == 3) & (iy == 3)
    labels[ring & ~core] = 2
    return g, labels


def _grid_cells(g, n):
    """(ix, iy) of every face's cell in seam_model.grid_scene(n=n) (no fin, no extra faces)"""
    assert len(g.faces) == 2 * (n - 1) * (n - 1)
    cell = np.arange(len(g.faces)) // 2
    return cell % (n - 1), cell // (n - 1)


NESTED_REGIONS = ("outer", "annulus", "core")
NESTED_ORDERS = tuple((a, b, c) for a in NESTED_REGIONS for b in NESTED_REGIONS for c in NESTED_REGIONS if len({a, b, c}) == 3)


def nested_scene(order=None, seed=0):
    """seam_model.grid_scene(n=14, W=96, H=72), 338 faces; d = chessboard distance of a face's cell to cell (6, 6): label 2 where d is 4
    or 1, label 1 elsewhere.  Label 1 has three candidates whose boxes nest -- outer (d >= 5), annulus (d of 2 or 3), core (d == 0) --
    and label 2 two nested rings, so the merge ends with one patch per label whatever the candidate order, and in four of the six
    orders a candidate is absorbed that had absorbed another one: a chain.  Candidates are ordered by
    their smallest face, so `order` -- a permutation of NESTED_REGIONS, lowest first -- is produced by renumbering: the faces of the three
    regions in that order (shuffled within a region), then the two rings (inner first for every other order), vertices shuffled.
    order None: the grid as built (outer < annulus < core).  Returns (scene, labels, region): region[f] in 0 .. 2 indexes
    NESTED_REGIONS for the faces of label 1, 3 / 4 = the outer / inner ring of label 2."""
    import mvs_texturing_amd as M
    import seam_model as SM
    g = SM.grid_scene(n=14, W=96, H=72)
    ix, iy = _grid_cells(g, 14)
    d = np.maximum(np.abs(ix - 6), np.abs(iy - 6))
    region = np.select([d >= 5, d == 4, d >= 2, d == 1], [0, 3, 1, 4], 2)
    labels = np.where(region >= 3, 2, 1).astype(np.uint32)
    if order is None:
        return g, labels, region
    k = NESTED_ORDERS.index(tuple(order))
    rng = np.random.default_rng(seed + k)
    blocks = [NESTED_REGIONS.index(r) for r in order] + ([4, 3] if k % 2 else [3, 4])
    perm = np.concatenate([rng.permutation(np.flatnonzero(region == b)) for b in blocks])
    p = M.synth.permute_scene(g, seed=seed + k, face_perm=perm)
    return p, labels[p.face_perm], region[p.face_perm]


def equal_box_scene():
    """two candidates of one label with IDENTICAL boxes.  Two edge-connected regions of a planar mesh cannot both reach all four sides
    of a rectangle, so the boxes agree through their rounding: an 8 x 8 vertex grid whose first two and last two columns and rows fall
    into the same pixel (0.3 and 0.8; W - 1.9 and W - 1.4).  Label 1 = an L along the left and bottom borders (column 0 below the
    corner cell, the bottom row without its last cell) and an L along the top and right borders; label 2 = the two corner cells
    between them and the interior, a diagonal band from corner to corner.  Every box of label 1 is (-1, -1) .. (W - 1, H - 1); the
    corner cells of label 2 lie inside the interior's box and are absorbed too.  Returns (scene, labels)."""
    import seam_model as SM
    n, W, H = 8, 64, 48
    xs = np.concatenate([[0.3, 0.8], np.linspace(8.0, W - 9.0, n - 4), [W - 1.9, W - 1.4]])
    ys = np.concatenate([[0.4, 0.9], np.linspace(6.0, H - 7.0, n - 4), [H - 1.8, H - 1.3]])
    g = SM.grid_scene(n=n, W=W, H=H, xs=xs, ys=ys)
    ix, iy = _grid_cells(g, n)
    last = n - 2
    lower = ((ix == 0) & (iy >= 1)) | ((iy == last) & (ix < last))
    upper = ((iy == 0) & (ix >= 1)) | ((ix == last) & (iy < last))
    return g, np.where(lower | upper, 1, 2).astype(np.uint32)


def entry_pixels(arrays):
    """per list entry, the number of pixels adjust_colors visits for it: floor(min) - 1 .. ceil(max) + 1 exclusive, clamped to the
    patch's frame (0 for a face adjust_colors skips as degenerate).  The device walks an entry of up to 512 pixels with a group of
    lanes and a larger one with a block (k_texpatch.hip SMALL_MAX)."""
    tc = np.asarray(arrays["texcoords"], np.float32).reshape(-1, 3, 2)
    box = np.asarray(arrays["box"]).reshape(-1, 4)
    pid = np.repeat(np.arange(len(box)), np.diff(np.asarray(arrays["face_ptr"]).astype(np.int64)))
    w, h = box[pid, 2].astype(np.int64), box[pid, 3].astype(np.int64)
    x0 = np.maximum(np.floor(tc[..., 0].min(1)).astype(np.int64) - 1, 0); y0 = np.maximum(np.floor(tc[..., 1].min(1)).astype(np.int64) - 1, 0)
    x1 = np.minimum(np.ceil(tc[..., 0].max(1)).astype(np.int64) + 1, w); y1 = np.minimum(np.ceil(tc[..., 1].max(1)).astype(np.int64) + 1, h)
    u, v = tc[:, 1] - tc[:, 0], tc[:, 2] - tc[:, 0]
    area = np.float32(0.5) * np.abs(_f(_f(u[:, 0] * v[:, 1]) - _f(u[:, 1] * v[:, 0])))
    n = np.maximum(x1 - x0, 0) * np.maximum(y1 - y0, 0)
    return np.where(area < np.float32(np.finfo(np.float32).eps), 0, n)
