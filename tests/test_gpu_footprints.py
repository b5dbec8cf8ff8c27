"""Face infos at camera resolutions (run with -m gpu on an MI355X): hand-built scenes whose footprints reach the sizes of real
captures -- multi-megapixel triangles on 45-60 MP images -- and scenes that straddle every threshold where the footprint sampler
changes strategy, each compared with the CPU oracle's serial fp64 walk bit for bit (col_ptr, view ids, quality and cost bits, cull
counters, labels).

Every scene is a plane z = 0 seen by cameras that look straight down (w2c = diag(1, -1, -1) plus a translation, f = camera
height = 8192): a world point (X, Y, 0) projects EXACTLY to the pixel coordinates (X - cx + W / 2 - 0.5, cy - Y + H / 2 - 0.5)
for coordinates on a 1/32 grid, so the triangles below are placed in pixel space to the exact bit."""
import numpy as np
import pytest

import mvs_texturing_amd as M
import oracle_py as O

pytestmark = pytest.mark.gpu

CULLS = ("cull_backface", "cull_angle", "cull_outside", "cull_occluded", "cull_zero_quality", "nnz_pre")
HEIGHT = 8192.0                      # camera height above the plane = focal length: pixel coordinates = world coordinates (shifted)
WRAP = 1 << 32                       # 32-bit integer sums wrap here


@pytest.fixture(autouse=True)
def _release_between_tests():
    """the scenes of this module hold up to a gigabyte of host images: hand them back before the next test starts"""
    yield
    import gc
    gc.collect()


def _cams(views):
    """views: list of (width, height, cx, cy, zoom): a camera at (cx, cy, HEIGHT) looking down -z, focal length zoom * HEIGHT"""
    V = len(views)
    cams = dict(pos=np.zeros((V, 3), np.float32), viewdir=np.zeros((V, 3), np.float32), K=np.zeros((V, 9), np.float32),
                w2c=np.zeros((V, 16), np.float32), width=np.zeros(V, np.int32), height=np.zeros(V, np.int32))
    for j, (w, h, cx, cy, zoom) in enumerate(views):
        cams["pos"][j] = (cx, cy, HEIGHT)
        cams["viewdir"][j] = (0.0, 0.0, -1.0)
        cams["K"][j] = (zoom * HEIGHT, 0.0, w / 2.0, 0.0, zoom * HEIGHT, h / 2.0, 0.0, 0.0, 1.0)
        cams["w2c"][j] = (1.0, 0.0, 0.0, -cx, 0.0, -1.0, 0.0, cy, 0.0, 0.0, -1.0, HEIGHT, 0.0, 0.0, 0.0, 1.0)
        cams["width"][j], cams["height"][j] = w, h
    return cams


def _view_at(w, h, sx=0.0, sy=0.0, zoom=1.0):
    """the camera under which world (X, Y) lands on pixel (zoom X - sx, zoom (-Y) - sy): world = pixel space of a view with sx = sy = 0"""
    return (w, h, (sx + w / 2.0 - 0.5) / zoom, -(sy + h / 2.0 - 0.5) / zoom, zoom)


def _plane_scene(tris_px, views, images):
    """triangles given in the pixel space of an unshifted view (list of three (x, y) each; shared vertices are merged), all normals +z"""
    pts, faces = {}, []
    for tri in tris_px:
        faces.append([pts.setdefault((float(x), float(y)), len(pts)) for x, y in tri])
    s = M.synth.Scene()
    s.verts = np.array([(x, -y, 0.0) for (x, y) in pts], np.float32)
    s.faces = np.array(faces, np.uint32)
    s.normals = np.tile(np.array([0.0, 0.0, 1.0], np.float32), (len(faces), 1))
    s.adj_ptr, s.adj = M.build_adjacency_graph(s.verts.shape[0], s.faces)
    s.cams = _cams(views)
    s.images = images
    return s


def _pixel_coords(s, j, f):
    """(3, 2) float32 pixel coordinates of face f in view j, in dmath.h pixel_coords' operation order"""
    K = s.cams["K"][j].reshape(3, 3); m = s.cams["w2c"][j].reshape(4, 4)
    out = np.zeros((3, 2), np.float32)
    for k, v in enumerate(s.verts[s.faces[f]]):
        c = [((m[r, 0] * v[0] + m[r, 1] * v[1]) + m[r, 2] * v[2]) + np.float32(1.0) * m[r, 3] for r in range(3)]
        q = [(K[r, 0] * c[0] + K[r, 1] * c[1]) + K[r, 2] * c[2] for r in range(3)]
        out[k] = (q[0] / q[2] - np.float32(0.5), q[1] / q[2] - np.float32(0.5))
    return out


def _inner_sum(plane, tri, margin=2.0):
    """(pixels, sum of `plane`) over the pixels whose centre lies inside `tri` (pixel coordinates) by at least `margin` pixels: a
    subset of the footprint the reference samples (texture_view.cpp:183-219 takes every pixel whose centre is inside), so both
    are lower bounds of the exact footprint's"""
    p = np.asarray(tri, np.float64)
    if (p[1, 0] - p[0, 0]) * (p[2, 1] - p[0, 1]) - (p[1, 1] - p[0, 1]) * (p[2, 0] - p[0, 0]) < 0:
        p = p[[0, 2, 1]]
    h, w = plane.shape
    n = total = 0
    y0, y1 = max(int(p[:, 1].min()), 0), min(int(np.ceil(p[:, 1].max())) + 1, h)
    for y in range(y0, y1):
        cy = y + 0.5
        lo, hi = -np.inf, np.inf
        for a, b in ((p[0], p[1]), (p[1], p[2]), (p[2], p[0])):
            # inside: cross(b - a, q - a) >= margin |b - a|  (q = (x + 0.5, cy)), linear in x
            ex, ey = b - a
            k = -ey                                      # coefficient of x
            r = margin * np.hypot(ex, ey) - (ex * (cy - a[1]) - ey * (0.5 - a[0]))
            if k > 0: lo = max(lo, r / k)
            elif k < 0: hi = min(hi, r / k)
            elif r > 0: lo = np.inf
        if not lo <= hi:
            continue
        xa, xb = max(int(np.ceil(lo)), 0), min(int(np.floor(hi)) + 1, w)
        if xb > xa:
            n += xb - xa
            total += int(plane[y, xa:xb].sum(dtype=np.int64))
    return n, total


def _gradient_magnitude(rgb):
    h, w = rgb.shape[:2]
    g = np.empty((h, w), np.uint8)
    O.load().orc_gradient_magnitude(O._ptr(rgb), w, h, O._ptr(g))
    return g


def _compare(ctx, s, kw, ref, rst, tag):
    st = ctx.data_costs(M.Settings(**kw))
    got = ctx.costs_download()
    assert np.array_equal(got.col_ptr, ref.col_ptr), (tag, "sparsity pattern differs")
    assert np.array_equal(got.view_id, ref.view_id), tag
    bad = np.flatnonzero(got.quality.view(np.uint32) != ref.quality.view(np.uint32))
    assert bad.size == 0, (tag, "%d of %d qualities differ, e.g. %s" % (bad.size, ref.nnz, [(float(got.quality[i]), float(ref.quality[i])) for i in bad[:4]]))
    assert np.array_equal(got.cost.view(np.uint32), ref.cost.view(np.uint32)), tag
    for k in CULLS:
        assert st[k] == rst[k], (tag, k, st[k], rst[k])
    return st


def _labels_equal(ctx, s, ref):
    lo, so = O.view_selection(ref, s.adj_ptr, s.adj)
    lg, sg = ctx.view_selection(s.adj_ptr, s.adj)
    assert np.array_equal(lo, lg) and so["energy_fixed"] == sg["energy_fixed"]


# ---- 1. footprints whose integer pixel sums pass 2^32 ----
# 45 MP (8256 x 5504) and 60 MP (9504 x 6336) views of a quad of two triangles, each ~ 22 M pixels in every view: the triangle with a
# horizontal edge takes the lane group's generic (non-`fast`) branch, the other one -- general edges -- its word branch (and, with
# info_wave_area_words at 2^30, the one-lane word walk of info_kernel).
BIG = [(8256, 5504, 0.0, 0.0, 1.0), (8256, 5504, 17.0, -11.0, 1.0), (8256, 5504, -23.0, 19.5, 1.0), (9504, 6336, -20.0, -12.0, 1.0),
       (9504, 6336, -250.0, -140.0, 1.06)]
QUAD = [(40.0, 60.0), (8200.0, 60.0), (8180.0, 5450.0), (70.0, 5440.0)]
BIG_TRIS = [(QUAD[0], QUAD[1], QUAD[2]), (QUAD[0], QUAD[2], QUAD[3])]


def _big_images(kind):
    """kind "gmi": vertical 2-pixel stripes of levels 1 / 255 (gradient magnitude 255), low contrast in every 13th band of 7
    rows (magnitudes below 255); kind "white": near-white RGB with a faint pattern, tinted per view, one view clearly apart"""
    images = []
    for j, (w, h, _, _, _) in enumerate(BIG):
        rows = np.arange(h)
        if kind == "gmi":
            col = np.where((np.arange(w) // 2) % 2 == 0, 1, 255).astype(np.uint8)
            img = np.empty((h, w, 3), np.uint8)
            img[...] = col[None, :, None]
            low = ((rows // 7) % 13) == 0
            contrast = (10 + (rows * 7 + j * 5) % 50).astype(np.uint8)
            img[low] = np.minimum(col[None, :], contrast[low, None])[:, :, None] + 1
        else:
            tint = [(252, 250, 248), (250, 252, 249), (251, 249, 252), (249, 251, 250), (255, 215, 236)][j]
            pat = ((np.arange(w)[None, :] // 3 + rows[:, None] // 5) % 4).astype(np.int16)
            img = np.empty((h, w, 3), np.uint8)
            for c in range(3):
                img[:, :, c] = np.minimum(255, tint[c] + pat) if tint[c] < 255 else 255 - pat
        images.append(img)
    return images


def _big_scene(kind):
    return _plane_scene(BIG_TRIS, [_view_at(w, h, sx, sy, z) for (w, h, sx, sy, z) in BIG], _big_images(kind))


def _assert_sums_wrap(s, plane_of_view):
    """the precondition, in exact integers: some (face, view) pair's pixel sum exceeds 2^32 - 1"""
    best = 0
    for j in range(s.n_views):
        plane = plane_of_view(j)
        for f in range(s.n_faces):
            n, total = _inner_sum(plane, _pixel_coords(s, j, f))
            assert n > 16_000_000, (j, f, n)         # every pair is a multi-megapixel footprint
            best = max(best, total)
    assert best > WRAP - 1, best
    return best


RUNS = {"default": {}, "serial": {"info_wave_area": 0}, "one-lane words": {"info_wave_area_words": 1 << 30}}


def _run_ways(s, plan):
    """plan: (mode, names of RUNS) pairs.  "serial" walks every footprint in the reference's order (info_kernel, one lane each: slow at
    22 M pixels) and localises a failure; "one-lane words" lets info_kernel's 32-bit word walk take every `fast` footprint it may"""
    c = M.Context(0)
    c.set_option("stats", 1)
    c.set_mesh(s.verts, s.faces, s.normals)
    c.set_views(s.cams, s.images)
    try:
        for kw, runs in plan:
            ref, rst = O.data_costs(s, **kw)
            assert ref.nnz == s.n_faces * s.n_views, "every view sees every face"
            for tag in runs:
                c.set_option("info_wave_area", 32); c.set_option("info_wave_area_words", 384)   # the defaults
                for k, v in RUNS[tag].items():
                    c.set_option(k, v)
                st = _compare(c, s, kw, ref, rst, (kw, tag))
                if tag == "serial":
                    assert st["footprints_lane_group"] == 0, st
                else:
                    assert st["footprints_lane_group"] > 0, (tag, st)
            _labels_equal(c, s, ref)
    finally:
        c.close()


def test_gradient_sums_past_2_32():
    """8-bit gradient magnitudes summed over 22 M pixel footprints: the 16 lanes' total and the one-lane word walk's sum pass
    2^32; every way of sampling equals the oracle's serial fp64 walk"""
    s = _big_scene("gmi")
    grads = {}
    _assert_sums_wrap(s, lambda j: grads.setdefault(j, _gradient_magnitude(s.images[j])))
    grads.clear()
    _run_ways(s, [(dict(), ("default", "serial", "one-lane words"))])


def test_colour_sums_past_2_32():
    """near-white colours summed over 22 M pixel footprints for photometric outlier detection: the channel sums pass 2^32
    (gauss_clamping with the gradient term, gauss_damping with the area term).  Five views per face, one in another tint: the
    covariance of the mean colours is above the detection's floor, and damping scales every quality by the Gaussian of its view's
    mean colour, so a wrong mean shows in the table.  (Clamping cannot reject anything among five views -- a sample's squared
    Mahalanobis distance stays below (n - 1)^2 / n -- its run checks the gradient qualities beside the colour sums.)"""
    s = _big_scene("white")
    _assert_sums_wrap(s, lambda j: s.images[j][:, :, 0])
    damped, plain = O.data_costs(s, data_term="area", outlier_removal="gauss_damping")[0], O.data_costs(s, data_term="area")[0]
    assert not np.array_equal(damped.quality, plain.quality)
    # (the one-lane word walk serves the gradient term without outlier removal only: nothing to run here)
    _run_ways(s, [(dict(data_term="gmi", outlier_removal="gauss_clamping"), ("default",)),
                  (dict(data_term="area", outlier_removal="gauss_damping"), ("default", "serial"))])


# ---- 2. footprints on either side of every threshold of the sampler ----
# Six views of widths 1025 .. 1031 (every residue mod 4: rows start at every byte offset of an aligned word, and the words around a
# span that reaches the end of a row straddle into the next one), each shifted so that the faces placed at the right / bottom border
# of the first view lie at ITS border.  Faces, in the first view's pixel space:
#   * AABB widths 95 / 96 / 96 + 1/32 / 97 pixels (k_dc.hip MVS_NARROW_PX: <= 96 is summed one scan line per lane), general edges
#     and with a vertical edge;
#   * 15 / 16 / 17 and 31 / 32 / 33 scan lines (the lane group's blocks of 16 lines), wide and narrow;
#   * areas of 31, 32, 33 and 383, 384, 385 pixels and halves between (info_wave_area = 32 with outlier removal, info_wave_area_words =
#     384 for the gradient term: `area > threshold` goes to the lane group);
#   * vertices within a pixel of each image border: at 1.25 / W - 2.25 (valid with the eroded mask of the gradient term too) and at
#     0.25 / W - 1.25 (valid for the area term only).
EDGE_VIEWS = [(1025, 771, 0.0, 0.0), (1026, 770, -1.0, 1.0), (1027, 769, -2.0, 2.0), (1028, 772, -3.0, -1.0), (1029, 773, -4.25, -2.25),
              (1031, 775, -6.0, -4.0)]


def _edge_tris():
    t = []
    for k, wd in enumerate((95.0, 96.0, 96.03125, 97.0)):
        x0 = 20.0 + 110.0 * k
        t.append(((x0, 10.25), (x0 + wd, 130.5), (x0 + 30.5, 310.75)))              # general edges
        x0 += 450.0
        t.append(((x0, 10.25), (x0, 310.25), (x0 + wd, 150.5)))                    # a vertical edge: not `fast`
    for k, lines in enumerate((15, 16, 17, 31, 32, 33)):
        y0 = 330.0 + 44.0 * (k % 3) + (132.0 if k >= 3 else 0.0)
        for x0, wd in ((20.0, 200.5), (240.0, 60.0)):                              # wide, narrow
            t.append(((x0, y0 + 0.25), (x0 + wd, y0 + lines / 2.0), (x0 + 57.25, y0 + lines - 0.75)))
        t.append(((330.0, y0 + 0.25), (330.0 + 180.0, y0 + 0.25 + lines / 3.0), (330.0 + 40.0, y0 + lines - 0.75)))
    for k, area in enumerate((31.0, 31.5, 32.0, 32.5, 33.0, 383.0, 383.5, 384.0, 384.5, 385.0)):
        x0, y0 = 560.0 + 45.0 * (k % 5), 330.0 + 40.0 * (k // 5)
        e = (2.0 * area + 3.0) / 32.0                                                # area of (0, 0), (32, 1), (3, e) = (32 e - 3) / 2
        t.append(((x0, y0), (x0 + 32.0, y0 + 1.0), (x0 + 3.0, y0 + e)))
    W, H = EDGE_VIEWS[0][:2]
    t += [((1.25, 1.25), (200.5, 1.75), (90.25, 150.5)),                               # top-left corner
          ((0.25, 620.5), (120.75, 600.25), (60.5, 700.75)),                           # left border, area term only
          ((W - 2.25, 600.25), (W - 125.5, 560.5), (W - 75.25, H - 2.25)),             # right / bottom border
          ((W - 1.25, 200.25), (W - 145.5, 260.5), (W - 25.25, 330.75)),               # right border, area term only
          ((2.5, H - 1.5), (150.25, H - 71.25), (80.75, H - 131.5)),                   # bottom-left, area term only
          ((600.25, H - 2.25), (900.5, H - 1.25), (760.0, H - 180.5))]                 # bottom border: spans ending at a row's end
    return t


def _edge_images():
    """noise (gradient magnitudes of every value; no black pixel) in a per-view tint, view 2 clearly apart"""
    rng = np.random.default_rng(31)
    images = []
    for j, (w, h, _, _) in enumerate(EDGE_VIEWS):
        tint = np.array([(0, 0, 0), (6, -4, 3), (-5, 5, 0), (40, -30, -35), (3, 2, -6), (-4, -2, 5)][j], np.int16)
        noise = rng.integers(30, 200, size=(h, w, 1), dtype=np.int16) + rng.integers(-20, 21, size=(h, w, 3), dtype=np.int16)
        images.append(np.clip(noise + tint, 1, 255).astype(np.uint8))
    return images


MODES = [dict(data_term=dt, outlier_removal=orm) for dt in ("gmi", "area") for orm in ("none", "gauss_clamping", "gauss_damping")]


def test_sampler_thresholds_against_the_oracle():
    s = _plane_scene(_edge_tris(), [_view_at(w, h, sx, sy) for (w, h, sx, sy) in EDGE_VIEWS], _edge_images())
    assert sorted({w % 4 for w, _, _, _ in EDGE_VIEWS}) == [0, 1, 2, 3]
    c = M.Context(0)
    c.set_option("stats", 1)
    c.set_mesh(s.verts, s.faces, s.normals)
    c.set_views(s.cams, s.images)
    try:
        for kw in MODES:
            ref, rst = O.data_costs(s, **kw)
            assert rst["cull_outside"] > 0 and ref.nnz > 4 * s.n_faces, rst
            for tag, opts in (("default", {}), ("group from 32", {"info_wave_area_words": 32})):
                c.set_option("info_wave_area_words", 384)
                for k, v in opts.items():
                    c.set_option(k, v)
                st = _compare(c, s, kw, ref, rst, (kw, tag))
                if kw["data_term"] == "gmi" or kw["outlier_removal"] != "none":
                    assert st["footprints_lane_group"] > 0, (kw, tag, st)
            _labels_equal(c, s, ref)
    finally:
        c.close()


# ---- 3. image preparation at camera resolutions ----
# Odd-sized 24 and 45 MP views with the black ring that undistortion leaves (every border pixel black: the validity flood fill
# starts along the whole border and runs through the ring), black spurs reaching in from it (flooded) and black islands inside (not
# flooded), plus one view with only a black corner; a grid of 3072 faces over the plane, many of them with a vertex in or next to the
# ring.  The fused luminance + Sobel kernel (1024-pixel strips) and the two-pass kernels, both data terms (the eroded mask and the
# plain one): every table and cull counter equals the oracle's.
PREP_VIEWS = [(6001, 4001, 3.0, -2.0, 6001 / 8257), (6001, 4001, -41.5, 17.0, 6001 / 8257 * 1.02), (8257, 5505, 0.0, 0.0, 1.0),
              (8257, 5505, 30.25, -22.75, 0.99), (8257, 5505, -12.0, 9.0, 1.0)]


def _ring_image(w, h, seed, ring=True):
    rng = np.random.default_rng(seed)
    img = (rng.integers(1, 256, size=(h, w, 3), dtype=np.uint8) | np.uint8(1))
    if ring:
        u = np.abs(np.linspace(-1.0, 1.0, w, dtype=np.float32))[None, :] ** 4
        v = np.abs(np.linspace(-1.0, 1.0, h, dtype=np.float32))[:, None] ** 4
        img[(u + v) > 0.72] = 0
        for k in range(6):                                       # spurs from the ring inwards, islands inside
            y = h // 7 * (k + 1)
            img[y:y + 3, : w // 5 + 97 * k] = 0
            img[y + h // 14: y + h // 14 + 5, w // 3 + 311 * k: w // 3 + 311 * k + 7] = 0
    else:
        img[: h // 9, : w // 11] = 0
    return img


def test_camera_resolution_image_preparation_against_the_oracle():
    n = 32
    xs, ys = np.linspace(-60.0, 8316.0, 3 * n // 2 + 1), np.linspace(-60.0, 5564.0, n + 1)
    tris = []
    for iy in range(n):
        for ix in range(3 * n // 2):
            a, b = (xs[ix], ys[iy]), (xs[ix + 1], ys[iy])
            c_, d = (xs[ix + 1], ys[iy + 1]), (xs[ix], ys[iy + 1])
            tris += [(a, b, c_), (a, c_, d)]
    images = [_ring_image(w, h, j, ring=j < 4) for j, (w, h, _, _, _) in enumerate(PREP_VIEWS)]
    s = _plane_scene(tris, [_view_at(w, h, sx, sy, z) for (w, h, sx, sy, z) in PREP_VIEWS], images)
    refs = {}
    for kw in (dict(), dict(data_term="area")):
        refs[kw.get("data_term", "gmi")] = O.data_costs(s, **kw)
    assert refs["gmi"][1]["cull_outside"] > refs["area"][1]["cull_outside"] > 0 and refs["gmi"][0].nnz > 1000
    for fused in (1, 0):
        c = M.Context(0)
        c.set_option("stats", 1); c.set_option("prep_fused", fused)
        c.set_mesh(s.verts, s.faces, s.normals)
        c.set_views(s.cams, s.images)
        try:
            for kw in (dict(), dict(data_term="area")):
                ref, rst = refs[kw.get("data_term", "gmi")]
                _compare(c, s, kw, ref, rst, (kw, fused))
        finally:
            c.close()
