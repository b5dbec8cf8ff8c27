"""What the view-mask tests share (tests/test_view_masks_host.py, tests/test_gpu_view_masks.py): the mask patterns, the expected
image-preparation products of a masked view from the oracle's kernels and numpy, the small scene of the table tests, and which pairs of
an unmasked table survive a mask -- from float64 projections, so that the GPU's float32 projections are checked against something else."""
import numpy as np

import oracle_py as O
import util_cases as U

MASK_PATTERNS = ("all_keep", "all_zero", "corner_tl", "corner_tr", "corner_bl", "corner_br", "border_top", "border_left", "border_right", "border_bottom",
                 "interior", "col31", "col32", "col_last", "checker", "blob_at_black")


def mask_pattern(name, w, h):
    """(h, w) uint8, 0 = leave out; keep values are 1, 7, 128 and 255 by position: anything non-zero keeps.  A pattern the size cannot hold
    (a column beyond the width, an interior pixel in a 2-pixel image) degenerates to the nearest legal one."""
    yy, xx = np.mgrid[0:h, 0:w]
    m = np.choose((xx + 3 * yy) % 4, [1, 7, 128, 255]).astype(np.uint8)
    cx, cy = min(w - 1, max(0, w // 2)), min(h - 1, max(0, h // 2))
    if name == "all_keep": pass
    elif name == "all_zero": m[:] = 0
    elif name == "corner_tl": m[0, 0] = 0
    elif name == "corner_tr": m[0, w - 1] = 0
    elif name == "corner_bl": m[h - 1, 0] = 0
    elif name == "corner_br": m[h - 1, w - 1] = 0
    elif name == "border_top": m[0, cx] = 0
    elif name == "border_left": m[cy, 0] = 0
    elif name == "border_right": m[cy, w - 1] = 0
    elif name == "border_bottom": m[h - 1, cx] = 0
    elif name == "interior": m[cy, cx] = 0
    elif name == "col31": m[:, min(31, w - 1)] = 0
    elif name == "col32": m[:, min(32, w - 1)] = 0
    elif name == "col_last": m[:, w - 1] = 0
    elif name == "checker": m[(xx + yy) % 2 == 0] = 0
    elif name == "blob_at_black": m[:max(1, h // 2), :max(1, w // 2 + 1)] = 0       # overlaps whatever black region the image has at the corner (0, 0)
    else: raise KeyError(name)
    return np.ascontiguousarray(m)


def expected_products(img, keep, term):
    """the mask bits the device must hold for image `img` (h, w, 3) under the byte mask `keep` ((h, w) or None) and the data term:
    orc_validity_mask(rgb) AND keep, then orc_erode_validity_mask under the gradient term.  Returns (bits bool (h, w), tile summary bool)."""
    L = O.load()
    h, w = img.shape[:2]
    img = np.ascontiguousarray(img)
    plain = np.zeros((h, w), np.uint8); L.orc_validity_mask(O._ptr(img), w, h, O._ptr(plain))
    if keep is not None:
        plain = np.ascontiguousarray(plain * (np.asarray(keep) != 0).astype(np.uint8))
    if term == "gmi":
        L.orc_erode_validity_mask(O._ptr(plain), w, h)
    bits = plain.astype(bool)
    return bits, U.tile_summary_numpy(bits)


def keep_bits_under_lens(keep, lens):
    """the keep bits of a mask given in the camera's frame: oracle.undistort of the 0 / 255 replica, thresholded at 255"""
    k = np.where(np.asarray(keep) != 0, 255, 0).astype(np.uint8)
    if lens is None or lens[1] == 0.0:
        return k == 255
    rep = np.ascontiguousarray(np.repeat(k[:, :, None], 3, axis=2))
    out = O.undistort(rep, *lens)
    assert np.array_equal(out[:, :, 0], out[:, :, 1]) and np.array_equal(out[:, :, 0], out[:, :, 2])
    return out[:, :, 0] == 255


_SMALL = {}


def small_scene():
    """the table tests' scene: the n = 22 sphere with displacement, 6 views of 256 x 192 (every second one zoomed), images without zero pixels"""
    if "s" not in _SMALL:
        import mvs_texturing_amd as M
        s = M.synth.make_scene(n=22, n_views=6, width=256, height=192, displacement=0.15, layout=1, zoom_odd=1.3)
        s.images = [np.ascontiguousarray(np.maximum(i, 1)) for i in s.images]
        # Three vertices x two coordinates within 1e-3 of an integer: 1.2 % of the pairs of ANY scene in general position are undecided
        # in the sense of surviving_pairs, more than the 1 % the table test allows.  So the scene is taken out of that position: a
        # vertex that projects within 4e-3 pixel of an integer coordinate in some view is moved by a few 1e-4 of the sphere's radius
        # (some hundredths of a pixel) until few are left; normals and adjacency stay as they were.
        rng = np.random.default_rng(5)
        for _ in range(20):
            near = np.zeros(len(s.verts), bool)
            for j in range(s.n_views):
                px = project64(s, j)
                near |= (np.abs(px - np.rint(px)) < 4e-3).any(axis=1)
            if near.sum() <= len(s.verts) // 1000:
                break
            s.verts[near] += rng.uniform(-4e-4, 4e-4, (int(near.sum()), 3)).astype(np.float32)
        s.verts = np.ascontiguousarray(s.verts)
        _SMALL["s"] = s
    return _SMALL["s"]


def corner_regions(s):
    """a region R per view (bool (h, w), True = in R) that touches a corner and reaches well into the frame, through the projected mesh:
    a quadrant-sized rectangle from corner j % 4 with a diagonal edge, so that R's rim crosses pixel rows and columns at every slope"""
    out = []
    for j, img in enumerate(s.images):
        h, w = img.shape[:2]
        yy, xx = np.mgrid[0:h, 0:w]
        x = xx if j % 2 == 0 else w - 1 - xx
        y = yy if (j // 2) % 2 == 0 else h - 1 - yy
        out.append(np.ascontiguousarray((x * h + y * w) < (w * h * (0.9 + 0.015 * j))))   # (below 1: the two neighbouring corners stay outside)
    return out


def interior_blobs(s):
    """byte masks with arbitrary interior blobs (no blob touches the frame): discs and a bar, different per view"""
    out = []
    for j, img in enumerate(s.images):
        h, w = img.shape[:2]
        yy, xx = np.mgrid[0:h, 0:w]
        m = np.full((h, w), 255, np.uint8)
        for cx, cy, r in ((w * 0.35 + 7 * j, h * 0.4, 22 + 3 * j), (w * 0.65 - 5 * j, h * 0.6 + 2 * j, 17), (w * 0.5, h * 0.25 + 6 * j, 9)):
            m[(xx - cx) ** 2 + (yy - cy) ** 2 <= r * r] = 0
        m[h // 2 + 20:h // 2 + 24, 30:w - 40] = 0
        assert m[0].all() and m[-1].all() and m[:, 0].all() and m[:, -1].all() and not m.all()
        out.append(np.ascontiguousarray(m))
    return out


def project64(s, j):
    """pixel coordinates of every vertex in view j as TextureView::get_pixel_coords defines them, in float64: (n_verts, 2)"""
    w2c = s.cams["w2c"][j].astype(np.float64).reshape(4, 4); K = s.cams["K"][j].astype(np.float64).reshape(3, 3)
    p = s.verts.astype(np.float64) @ w2c[:3, :3].T + w2c[:3, 3]
    q = p @ K.T
    return q[:, :2] / q[:, 2:3] - 0.5


def surviving_pairs(s, table, bits, eps=1e-3):
    """for every pair of `table` (an unmasked table, CSR by face): (survives bool, decided bool) under the per-view mask bits `bits` --
    valid_pixel (texture_view.cpp:253-281) at the three projected vertices; a pair with a vertex within eps of an integer coordinate is
    undecided (the float32 projection may fall on the other side)"""
    F = table.n_faces
    face = np.repeat(np.arange(F), np.diff(table.col_ptr.astype(np.int64)))
    view = table.view_id.astype(np.int64)
    survives = np.ones(table.nnz, bool); decided = np.ones(table.nnz, bool)
    for j in range(s.n_views):
        sel = np.nonzero(view == j)[0]
        if not len(sel):
            continue
        h, w = bits[j].shape
        px = project64(s, j)[s.faces[face[sel]].astype(np.int64)]            # (n, 3, 2)
        near = np.abs(px - np.rint(px)) < eps
        decided[sel] = ~near.any(axis=(1, 2))
        x, y = px[..., 0], px[..., 1]
        inside = (x >= 0) & (x < w - 1) & (y >= 0) & (y < h - 1)
        fx = np.clip(np.floor(x).astype(np.int64), 0, w - 1); fy = np.clip(np.floor(y).astype(np.int64), 0, h - 1)
        fx1 = np.minimum(fx + 1, w - 1); fy1 = np.minimum(fy + 1, h - 1)
        b = bits[j]
        ok = inside & b[fy, fx] & b[fy1, fx] & b[fy, fx1] & b[fy1, fx1]
        survives[sel] = ok.all(axis=1)
    return survives, decided


def masked_table_from(table, survives):
    """the pattern and the costs of the masked table from the unmasked one's surviving pairs: qualities unchanged, costs 1 - min(1, q / p)
    in float32 with p = orc_percentile over the surviving qualities and their maximum (calculate_data_costs.cpp:291-296)"""
    import ctypes as C
    L = O.load()
    F = table.n_faces
    face = np.repeat(np.arange(F), np.diff(table.col_ptr.astype(np.int64)))
    q = np.ascontiguousarray(table.quality[survives], np.float32)
    col_ptr = np.zeros(F + 1, np.uint32); col_ptr[1:] = np.cumsum(np.bincount(face[survives], minlength=F))
    mx = np.float32(q.max()) if len(q) else np.float32(0)
    p = np.float32(L.orc_percentile(q.ctypes.data, len(q), C.c_float(float(mx)), C.c_float(0.995))) if len(q) else np.float32(1)
    cost = (np.float32(1.0) - np.minimum(np.float32(1.0), q / p)).astype(np.float32)
    return col_ptr, np.ascontiguousarray(table.view_id[survives]), q, cost
