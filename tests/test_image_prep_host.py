"""The CPU side of the image-preparation tests (tests/test_gpu_image_prep.py pins the kernels of csrc/k_prep.hip to the DEFINITION of their
products; this file pins the definitions): the tile summary of the validity mask as dmath.h valid_pixels3 consumes it -- compiled for the host,
with and without the summary -- against upstream's valid_pixel through the oracle (orc_valid_pixel_map, itself pinned in
tests/test_reference_pins.py) at every pixel position and on random triples; the numpy restatement of the summary on hand-written masks; what
sobel_pairs_image promises; and the numpy flood that counts Jacobi steps against the oracle's queue fill.  Everything is exact."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle_py as O
import util_cases as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = ((97, 67), (65, 66), (33, 33), (320, 240))


class _DV(C.Structure):      # dmh_view of csrc/dmath_host.cpp
    _fields_ = [("pos", C.c_float * 3), ("viewdir", C.c_float * 3), ("K", C.c_float * 9), ("w2c", C.c_float * 16),
                ("width", C.c_int32), ("height", C.c_int32), ("rgb", C.c_void_p), ("gmi", C.c_void_p), ("mask", C.c_void_p)]


class _DVS(C.Structure):     # dmh_view_sum: the view and the tile summary of its mask (null: every mask bit is read)
    _fields_ = [("view", _DV), ("msum", C.c_void_p), ("msum_stride", C.c_int32)]


def _shim():
    path = os.path.join(ROOT, "mvs-texturing_amd", "csrc", "libmvs_dmath_host.so")
    assert os.path.exists(path), "libmvs_dmath_host.so not built"
    D = C.CDLL(path)
    D.dmh_valid_pixels3.argtypes = [C.POINTER(_DVS), C.c_void_p, C.c_uint32, C.c_void_p]
    D.dmh_valid_pixels3.restype = None
    return D


def _positions(rng, w, h):
    """float32 (n, 3, 2): every position (x + d, y + d), d in {0, 0.5, 0.999}, x = -1 .. w, y = -1 .. h as a degenerate triple (p, p, p), then
    20 000 mixed triples -- nine in ten with all three vertices inside the image, where the mask decides"""
    gx, gy = np.meshgrid(np.arange(-1, w + 1), np.arange(-1, h + 1))
    g = np.stack([gx.ravel(), gy.ravel()], 1).astype(np.float64)
    grid = np.concatenate([g + d for d in (0.0, 0.5, 0.999)]).astype(np.float32)
    tri = (rng.random((20000, 3, 2)) * [w - 1, h - 1]).astype(np.float32)
    wide = (rng.random((2000, 3, 2)) * [w + 1, h + 1] - 1).astype(np.float32)
    tri[::10] = wide
    return np.ascontiguousarray(np.concatenate([np.repeat(grid[:, None, :], 3, axis=1), tri]), dtype=np.float32)


def _images(rng, w, h):
    out = dict(U.hostile_images(rng, w, h))
    out.update(U.small_hostile_images(rng, w, h))
    for bx, by in ((31, 31), (32, 32), (33, 33), (31, 33), (33, 31)):
        out["rim %d %d" % (bx, by)] = U.rim_blob(rng, w, h, bx, by)
    for corner in ("tr", "bl", "br"):
        for b in (32, 33):
            out["rim %s %d" % (corner, b)] = U.rim_blob(rng, w, h, b, b, corner)
    return out


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_valid_pixels3_with_the_summary_equals_upstream_valid_pixel(size):
    """valid_pixels3 with the tile summary == valid_pixels3 reading all twelve mask bits == the conjunction of upstream's valid_pixel over the
    three vertices, plain and eroded masks; on the rim patterns positions in tiles of BOTH summary answers are compared: both branches ran"""
    w, h = size
    D, L = _shim(), O.load()
    L.orc_valid_pixel_map.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_uint32, C.c_void_p]
    rng = np.random.default_rng(97 * w + h)
    xy = _positions(rng, w, h)
    n = len(xy)
    flat = np.ascontiguousarray(xy.reshape(-1, 2))
    inside = ((xy[..., 0] >= 0) & (xy[..., 0] < w - 1) & (xy[..., 1] >= 0) & (xy[..., 1] < h - 1)).all(axis=1)
    tx, ty = np.clip(xy[..., 0].astype(np.int64), 0, w - 1) >> 5, np.clip(xy[..., 1].astype(np.int64), 0, h - 1) >> 5
    imgs = _images(rng, w, h)
    assert "tile_rims" in imgs and "all_black" in imgs and "frame1" in imgs
    both = 0
    for name, img in imgs.items():
        for erode in (0, 1):
            mask = np.zeros((h, w), np.uint8); L.orc_validity_mask(O._ptr(img), w, h, O._ptr(mask))
            if erode: L.orc_erode_validity_mask(O._ptr(mask), w, h)
            mask = mask.astype(bool)
            words = U.pack_mask_words(mask)
            tiles = U.tile_summary_numpy(mask)
            sumw = U.pack_summary_words(tiles)
            one = np.zeros(3 * n, np.uint8)
            L.orc_valid_pixel_map(O._ptr(img), w, h, erode, O._ptr(flat), 3 * n, O._ptr(one))
            want = one.reshape(n, 3).all(axis=1)
            v = _DVS(); v.view.width, v.view.height, v.view.mask = w, h, words.ctypes.data
            got = {}
            for key, (ptr, stride) in (("summary", (sumw.ctypes.data, sumw.shape[1])), ("bits", (None, 0))):
                v.msum, v.msum_stride = ptr, stride
                out = np.full(n, 7, np.uint8)
                D.dmh_valid_pixels3(C.byref(v), xy.ctypes.data, n, out.ctypes.data)
                assert np.isin(out, (0, 1)).all()
                got[key] = out.astype(bool)
            for key in got:
                bad = np.nonzero(got[key] != want)[0]
                assert len(bad) == 0, (name, size, erode, key, len(bad), xy[bad[:4]].tolist())
            # both branches of valid_pixels3 ran: per rim pattern an in-range position in a tile whose bit is 1 and one in a tile whose bit is 0
            # -- wherever a tile with bit 1 HOLDS an in-range position (x < w - 1, y < h - 1: at 65 x 66 tile column 2 is pixel column 64 alone)
            whole = tiles[ty, tx].all(axis=1)                          # the summary answers without the mask
            assert want[inside & whole].all()                          # what the summary promises
            reach = tiles & (32 * np.arange(tiles.shape[1])[None, :] < w - 1) & (32 * np.arange(tiles.shape[0])[:, None] < h - 1)
            if name == "tile_rims" or (name.startswith("rim ") and name.split()[1].isdigit()):     # (blobs at the other corners can cover every tile)
                assert not tiles.all(), (name, size, erode)
                assert (inside & ~whole).any(), (name, size, erode)
                assert bool(reach.any()) == bool((inside & whole).any()), (name, size, erode)
                if w >= 97:
                    assert reach.any(), (name, size, erode)
                both += bool(reach.any())
    assert both >= (12 if w >= 97 else 1 if w > 33 else 0)      # (33 x 33: the one tile with in-range positions holds every blob)


def test_tile_summary_restatement_on_hand_written_masks():
    """tile (tx, ty) answers for the pixels [32 tx, 32 tx + 32] x [32 ty, 32 ty + 32]: 33 x 33 of them, so pixel column and row 32 belong to
    two tiles each and pixel (32, 32) to four"""
    m = np.ones((64, 64), bool)
    assert U.tile_summary_numpy(m).tolist() == [[True, True], [True, True]]
    a = m.copy(); a[32, 32] = False                                    # [y, x]: the one pixel all four tiles share
    assert U.tile_summary_numpy(a).tolist() == [[False, False], [False, False]]
    b = m.copy(); b[40, 31] = False                                    # x = 31: tile column 0 only; y = 40: tile row 1 only
    assert U.tile_summary_numpy(b).tolist() == [[True, True], [False, True]]
    c = m.copy(); c[0, 33] = False                                     # x = 33: tile column 1 only; y = 0: tile row 0 only
    assert U.tile_summary_numpy(c).tolist() == [[True, False], [True, True]]
    d = m.copy(); d[63, 32] = False                                    # x = 32: both tile columns; y = 63: tile row 1 only
    assert U.tile_summary_numpy(d).tolist() == [[True, True], [False, False]]
    assert U.pack_summary_words(U.tile_summary_numpy(b)).tolist() == [[3, 0], [2, 0]]
    assert U.pack_mask_words(b)[40].tolist() == [0x7FFFFFFF, 0xFFFFFFFF]
    e = np.ones((34, 2080), bool); e[5, 2050] = False                  # 65 tiles per row: two words of a second ballot
    t = U.tile_summary_numpy(e)
    assert t.shape == (2, 65) and not t[0, 64] and t[1, 64] and t[0, :64].all()
    assert U.pack_summary_words(t).tolist() == [[0xFFFFFFFF, 0xFFFFFFFF, 0, 0], [0xFFFFFFFF, 0xFFFFFFFF, 1, 0]]


@pytest.mark.parametrize("width", [1056, 1057])
def test_sobel_pairs_image_holds_what_it_promises(width):
    """every pair of Sobel sums 0 .. 256 of equal parity, signs, extremes -- asserted from the reference side here, where a broken generator
    fails without a GPU; and the numpy chain the assertion stands on (luminance, sums, truncated root) gives the oracle's gradient bytes"""
    img = U.sobel_pairs_image(width)
    h, w = img.shape[:2]
    assert w == width and 280 <= h <= 300
    U.assert_sobel_pairs_coverage(img)
    g = np.zeros((h, w), np.uint8)
    O.load().orc_gradient_magnitude(O._ptr(img), w, h, O._ptr(g))
    assert np.array_equal(g, U.gradient_magnitude_numpy(img))
    assert (np.bincount(g.ravel(), minlength=256) > 0).all()           # every result byte occurs
    rng = np.random.default_rng(3)
    noise = np.ascontiguousarray(rng.integers(0, 256, (37, 53, 3)).astype(np.uint8))
    g = np.zeros((37, 53), np.uint8)
    O.load().orc_gradient_magnitude(O._ptr(noise), 53, 37, O._ptr(g))
    assert np.array_equal(g, U.gradient_magnitude_numpy(noise))


def test_luminance_table():
    t = U.luminance_triples()
    assert t.shape == (U.LUM_MAX + 1, 3) and (t.astype(np.int32).sum(axis=1) > 0).all()
    assert np.array_equal(U.luminance_numpy(t), np.arange(U.LUM_MAX + 1))
    assert any(int(U.luminance_numpy(np.uint8([v, v, v]))) != v for v in range(256))      # grey is not always its own luminance


def test_numpy_jacobi_flood_equals_the_queue_fill():
    """the word-parallel flood that tests/test_gpu_image_prep.py counts steps with reaches what the oracle's queue fill reaches; the 320 x 240
    spiral needs more than 17 of its steps (the first step + one batch of 16 do not finish it), a line along row 1 one step per word"""
    L = O.load()
    rng = np.random.default_rng(11)
    for w, h in ((33, 4), (65, 66), (97, 67)):
        imgs = dict(U.small_hostile_images(rng, w, h))
        if w >= 65: imgs.update(U.hostile_images(rng, w, h))
        for name, img in imgs.items():
            reach, steps = U.jacobi_flood_steps(img)
            mask = np.zeros((h, w), np.uint8); L.orc_validity_mask(O._ptr(img), w, h, O._ptr(mask))
            assert np.array_equal(~reach, mask.astype(bool)), (name, w, h)
            if name == "hline": assert steps >= (w + 31) // 32
            if name in ("island", "checker", "corner_pixel"): assert steps == 0
    assert U.jacobi_flood_steps(U.hostile_images(rng, 320, 240)["spiral"], stop_after=17)[1] > 17


def test_small_patterns_fit_and_erode_as_described():
    rng = np.random.default_rng(5)
    L = O.load()
    for w, h in ((2, 2), (2, 5), (5, 2), (3, 3), (31, 3), (32, 2), (33, 4), (64, 3), (65, 66), (97, 67)):
        imgs = U.small_hostile_images(rng, w, h)
        assert set(imgs) <= set(U.SMALL_HOSTILE) and {"all_black", "corner_pixel", "first_row", "last_col"} <= set(imgs)
        assert (len(imgs) == len(U.SMALL_HOSTILE)) == (w >= 34 and h >= 7)
        for name, img in imgs.items():
            assert img.shape == (h, w, 3)
            mask = np.zeros((h, w), np.uint8); L.orc_validity_mask(O._ptr(img), w, h, O._ptr(mask))
            er = mask.copy(); L.orc_erode_validity_mask(O._ptr(er), w, h)
            assert (not np.array_equal(mask, er)) == U.erosion_bites(name, w, h), (name, w, h)
