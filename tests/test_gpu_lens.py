"""View input on the GPU: lens undistortion for pixel and JPEG views (DESIGN.md section 4 "View input"; csrc/k_lens.hip, csrc/lens.h).
oracle.undistort is the reference throughout (tests/test_lens_host.py holds the host twin to it on the same sizes and lenses).

The route on its own: Context.undistort_images on 56 images in one call, back to back, every start residue modulo 16 present -- the host copy
and the device buffer against the oracle and against undistort_image; images of a few 16-byte chunks at starts that make the head 0, 1
and 15 bytes long.  set_views(lens=) and set_views_jpeg(lens=): every view's image as it lies in the context (view_image) against the
oracle on the input pixels, and the table and labels against set_views on the oracle's images, bit for bit; a scratch cap that makes
every file view a batch of its own.  Refusals with their message and view number; the paths without a lens untouched."""
import io
import re

import numpy as np
import pytest

import mvs_texturing_amd as M
import oracle_py as O
import jpeg_full_decode as FD
from conftest import get_scene

pytestmark = pytest.mark.gpu

SIZES = ((2, 2), (3, 7), (5, 11), (16, 16), (17, 33), (64, 48), (97, 131))
LENSES = ((0.9, -0.2, 0.05), (1.3, 0.15, -0.03), (0.8, 0.1, 0.0), (1.1, -0.12, 0.0), (0.5, -0.5, 0.0), (0.5, 0.6, 0.0), (0.6, 0.9, 0.7), (1.0, 0.0, 0.3))
SCENE_LENS = {0: (0.9, -0.2, 0.05), 3: (1.1, -0.12, 0.0), 5: (1.0, 0.0, 0.3)}


@pytest.fixture(scope="module")
def ctx():
    c = M.Context(0)
    yield c
    c.close()


def image(h, w):
    """pixel values 1 .. 255: a black output pixel is one without a source"""
    return np.random.default_rng(1000 * h + w).integers(1, 256, (h, w, 3)).astype(np.uint8)


def black(img):
    return int((img.reshape(-1, 3) == 0).all(axis=1).sum())


def _same(images, refs):
    assert len(images) == len(refs)
    for k, (a, b) in enumerate(zip(images, refs)):
        assert a.shape == b.shape and a.dtype == np.uint8, k
        assert np.array_equal(a, b), "image %d (%s): %d bytes differ" % (k, a.shape, int((a != b).sum()))


def _starts(images):
    return np.concatenate([[0], np.cumsum([i.size for i in images])])[:-1]


# ---- the route on its own ----
@pytest.fixture(scope="module")
def all_cases():
    cases = [(size, lens) for size in SIZES for lens in LENSES]       # size-major: the starts then cover every residue
    images = [image(*size) for size, _ in cases]
    lens = np.array([l for _, l in cases], np.float32)
    refs = [O.undistort(i, *l) for i, (_, l) in zip(images, cases)]
    return cases, images, lens, refs


def test_route_on_its_own(ctx, all_cases):
    cases, images, lens, refs = all_cases
    assert len(images) == 56 and {int(s) % 16 for s in _starts(images)} == set(range(16))
    out, st = ctx.undistort_images(images, lens)
    _same(out, refs)
    n_copy = sum(1 for _, l in cases if l[1] == 0.0)
    assert st["views_copied"] == n_copy and st["views_undistorted"] == 56 - n_copy and st["batches"] == 1
    assert st["pixels"] == sum(h * w for (h, w), l in cases if l[1] != 0.0)
    assert st["pixels_no_source"] == sum(black(r) for r in refs) > 0
    assert st["staging_bytes"] >= sum(i.size for i in images)
    # the properties that keep the inputs from passing vacuously
    by = {c: r for c, r in zip(cases, refs)}
    for l in ((0.5, -0.5, 0.0), (0.6, 0.9, 0.7), (1.3, 0.15, -0.03), (1.1, -0.12, 0.0)):
        assert 0 < black(by[((97, 131), l)]) < 97 * 131
    for size in SIZES:
        assert np.array_equal(by[(size, (1.0, 0.0, 0.3))], image(*size))
    # the images left on the device: read through the deflate route, which takes device bytes and has a host twin
    dev, _ = ctx.undistort_images(images, lens, on_device=True)
    base = dev[0][0].ptr
    assert base % 16 == 0 and [a.ptr - base for a, _, _ in dev] == [int(s) for s in _starts(images)]
    for k, (arr, h, w) in enumerate(dev):
        assert (h, w, 3) == refs[k].shape and arr.shape == (refs[k].size,)
        assert ctx.deflate_rle(arr) == M.deflate_rle(refs[k].tobytes()), cases[k]


def test_route_equals_undistort_image(all_cases):
    cases, images, lens, refs = all_cases
    for k in range(len(cases)):
        assert np.array_equal(M.viewsel.undistort_image(images[k], *cases[k][1]), refs[k]), cases[k]


# an image of (h, w) for every product w h modulo 16: fillers that move the next image's start to any residue
FILLER = {(h * w) % 16: (h, w) for (h, w) in ((4, 4), (3, 11), (3, 6), (5, 7), (2, 2), (3, 7), (2, 3), (3, 13), (2, 4), (3, 3), (2, 5), (3, 9), (3, 4), (5, 9), (2, 7), (3, 5))}
# 3 w h = 12, 18, 18, 27, 30, 30, 36, 45, 48, 48, 54: the sizes nearest to 12, 15 .. 17, 31 .. 33 and 47 .. 49 bytes that w, h >= 2 realise
EDGE_SIZES = ((2, 2), (2, 3), (3, 2), (3, 3), (2, 5), (5, 2), (4, 3), (3, 5), (4, 4), (2, 8), (3, 6))


def test_store_edges(ctx):
    """images of one to four 16-byte chunks whose head (the bytes in front of the first 16-byte boundary) is 0, 1 and 15 bytes long"""
    assert len(FILLER) == 16
    images, lens, marks = [], [], []
    at = 0
    for k, (h, w) in enumerate(EDGE_SIZES):
        for head in (0, 1, 15):
            need = ((16 - head) % 16 - at) % 16              # the filler's bytes modulo 16; 3 w h = need  <=>  w h = 11 need (mod 16)
            fh, fw = FILLER[(11 * need) % 16]
            images.append(image(fh, fw)); lens.append(LENSES[len(images) % 3]); at += 3 * fh * fw
            assert (16 - at % 16) % 16 == head
            images.append(image(h, w) if head else image(h, w)[::-1].copy()); lens.append(LENSES[(k + head) % len(LENSES)]); marks.append((len(images) - 1, head))
            at += 3 * h * w
    refs = [O.undistort(i, *l) for i, l in zip(images, lens)]
    out, st = ctx.undistort_images(images, np.array(lens, np.float32))
    _same(out, refs)
    dev, _ = ctx.undistort_images(images, np.array(lens, np.float32), on_device=True)
    for k, head in marks:
        arr = dev[k][0]
        assert (16 - arr.ptr % 16) % 16 == head
        assert ctx.deflate_rle(arr) == M.deflate_rle(refs[k].tobytes()), (k, head)
    assert {i.size for i in (images[k] for k, _ in marks)} == {12, 18, 27, 30, 36, 45, 48, 54}


# ---- set_views(lens=) ----
def _table_and_labels(c, s, settings=None):
    c.data_costs(settings or M.Settings())
    t = c.costs_download()
    labels, _ = c.view_selection(s.adj_ptr, s.adj)
    return t, labels


def _same_result(a, b):
    (ta, la), (tb, lb) = a, b
    assert np.array_equal(ta.col_ptr, tb.col_ptr) and np.array_equal(ta.view_id, tb.view_id)
    assert np.array_equal(ta.cost.view(np.uint32), tb.cost.view(np.uint32))
    assert np.array_equal(la, lb)


def _area_clamping():
    st = M.Settings()
    st.data_term, st.outlier_removal = 0, 2
    return st


def _lens_rows(n, lenses):
    rows = np.zeros((n, 3), np.float32)
    rows[:, 0] = 1.0
    for j, l in lenses.items():
        rows[j] = l
    return rows


def _reference_route(s, pixels, lenses):
    """set_views on the oracle-undistorted images: (gmi result, area + gauss_clamping result), and those images"""
    undist = [O.undistort(p, *lenses[j]) if j in lenses else p for j, p in enumerate(pixels)]
    c = M.Context(0)
    try:
        c.set_mesh(s.verts, s.faces, s.normals); c.set_views(s.cams, undist)
        return (_table_and_labels(c, s), _table_and_labels(c, s, _area_clamping())), undist
    finally:
        c.close()


@pytest.fixture(scope="module")
def pixel_route():
    s = get_scene("tiny")
    return _reference_route(s, s.images, SCENE_LENS)


def test_set_views_lens(pixel_route):
    s = get_scene("tiny")
    ref, undist = pixel_route
    assert not np.array_equal(undist[0], s.images[0]) and not np.array_equal(undist[3], s.images[3]) and np.array_equal(undist[5], s.images[5])
    c = M.Context(0)
    try:
        c.set_mesh(s.verts, s.faces, s.normals)
        st = c.set_views(s.cams, s.images, lens=_lens_rows(s.n_views, SCENE_LENS))
        assert st["views_undistorted"] == 2 and st["views_copied"] == 0 and st["batches"] == 1 and st["pixels"] == 2 * 320 * 240
        assert st["pixels_no_source"] == sum(black(O.undistort(np.full((240, 320, 3), 1, np.uint8), *SCENE_LENS[j])) for j in (0, 3)) > 0
        assert st["staging_bytes"] == 2 * 320 * 240 * 3
        _same([c.view_image(j) for j in range(s.n_views)], undist)
        _same_result(_table_and_labels(c, s), ref[0])
        _same_result(_table_and_labels(c, s, _area_clamping()), ref[1])
        # one view per group of staging: the same pixels
        c.set_views_jpeg(s.cams, [None] * s.n_views, params=M.default_jpegdec_params(max_scratch_bytes=320 * 240 * 3), images=s.images, lens=_lens_rows(s.n_views, SCENE_LENS))
        _same([c.view_image(j) for j in range(s.n_views)], undist)
    finally:
        c.close()


# ---- set_views_jpeg(lens=) ----
JPEG_LENS = {3: (0.9, -0.2, 0.05), 4: (1.1, -0.12, 0.0), 5: (1.3, 0.15, -0.03), 6: (0.8, 0.1, 0.0)}


@pytest.fixture(scope="module")
def jpeg_scene():
    """views 0, 4: 4:2:0 files; 1, 3: 4:4:4; 2, 5: grayscale; 6: a PNG and 7: a progressive JPEG, both as host pixels.  (In this order no two
    neighbouring files fit the scratch the largest one needs with its staging: test_set_views_jpeg_lens checks that.)"""
    from PIL import Image
    s = get_scene("tiny")
    sampling = (2, 0, None, 0, 2, None)
    files = [FD.pillow_file(np.asarray(Image.fromarray(s.images[j]).convert("L")), quality=90) if v is None else FD.pillow_file(s.images[j], quality=90, subsampling=v)
             for j, v in enumerate(sampling)]
    png = io.BytesIO(); Image.fromarray(s.images[6]).save(png, "PNG")
    progressive = FD.pillow_file(s.images[7], quality=90, progressive=True)
    assert all(M.jpeg_probe(f) == (320, 240) for f in files) and M.jpeg_probe(progressive) is None
    pixels = [FD.pillow_decode(f) for f in files] + [np.asarray(Image.open(io.BytesIO(png.getvalue())).convert("RGB")), FD.pillow_decode(progressive)]
    assert np.array_equal(pixels[6], s.images[6])
    return s, files + [None, None], pixels


def _needs(c, s, files, pixels, lens):
    """the scratch every file view needs, read from the refusals: the cap is raised to the need of the view that was refused until none is"""
    needs, cap = {}, 1
    for _ in range(len(files) + 1):
        try:
            c.set_views_jpeg(s.cams, files, params=M.default_jpegdec_params(max_scratch_bytes=cap), images=pixels, lens=lens)
            return needs
        except M.MvsError as e:
            m = re.search(r"view (\d+) needs (\d+) bytes of (scratch|staging), max_scratch_bytes is (\d+)", str(e))
            assert e.status == 1 and m and int(m.group(4)) == cap, str(e)
            needs[int(m.group(1))] = int(m.group(2))
            cap = max(needs.values())
    raise AssertionError("still refused at the largest need")


def test_set_views_jpeg_lens(jpeg_scene):
    s, files, pixels = jpeg_scene
    ref, undist = _reference_route(s, pixels, JPEG_LENS)
    lens = _lens_rows(s.n_views, JPEG_LENS)
    n_files = sum(f is not None for f in files)
    c = M.Context(0)
    try:
        c.set_mesh(s.verts, s.faces, s.normals)
        st = c.set_views_jpeg(s.cams, files, images=pixels, lens=lens)
        assert st["files"] == n_files and st["batches"] == 1
        assert st["lens"]["views_undistorted"] == 4 and st["lens"]["batches"] == 2        # the PNG view's group, the files' batch
        _same([c.view_image(j) for j in range(s.n_views)], undist)
        for j in JPEG_LENS:
            assert not np.array_equal(undist[j], pixels[j])
        _same_result(_table_and_labels(c, s), ref[0])
        _same_result(_table_and_labels(c, s, _area_clamping()), ref[1])
        # a cap just above the largest single need: every distorted view is a batch of its own, staging is used again and again
        needs = _needs(c, s, files, pixels, lens)
        assert max(needs, key=needs.get) in JPEG_LENS and max(needs.values()) > 320 * 240 * 3
        every = []                                            # every file's need: its own scratch, and its staging where it has a lens
        for j in range(n_files):
            with pytest.raises(M.MvsError) as e:
                c.decode_jpegs([files[j]], params=M.default_jpegdec_params(max_scratch_bytes=1))
            every.append(int(re.search(r"needs (\d+) bytes of scratch", str(e.value)).group(1)) + (320 * 240 * 3 if j in JPEG_LENS else 0))
        assert max(every) == max(needs.values()) and all(every[j] + every[j + 1] > max(every) + 1 for j in range(n_files - 1)), every
        st = c.set_views_jpeg(s.cams, files, params=M.default_jpegdec_params(max_scratch_bytes=max(needs.values()) + 1), images=pixels, lens=lens)
        assert st["batches"] >= n_files and st["lens"]["batches"] == 4
        assert st["lens"]["staging_bytes"] == 320 * 240 * 3
        _same([c.view_image(j) for j in range(s.n_views)], undist)
        _same_result(_table_and_labels(c, s), ref[0])
    finally:
        c.close()


# ---- refusals ----
def test_refusals(pixel_route):
    s = get_scene("tiny")
    ref, undist = pixel_route
    good = _lens_rows(s.n_views, SCENE_LENS)

    def rows(j, row):
        r = np.zeros((s.n_views, 4), np.float32)
        r[:, :3] = good
        r[j] = row
        return r

    c = M.Context(0)
    try:
        c.set_mesh(s.verts, s.faces, s.normals)
        cases = [(dict(lens=rows(2, (0.0, 0.1, 0.0, 0))), "view 2", "positive focal length"),
                 (dict(lens=rows(4, (1.0, 0.1, np.nan, 0))), "view 4", "finite"),
                 (dict(lens=rows(6, (1.0, 0.1, 0.0, 1))), "view 6", "reserved must be 0"),
                 (dict(lens=good, params=M.default_jpegdec_params(max_scratch_bytes=1000)), "view 0", "needs 230400 bytes of staging, max_scratch_bytes is 1000")]
        for kw, view, why in cases:
            c.set_views(s.cams, s.images)                     # views are there ...
            with pytest.raises(M.MvsError) as e:
                c.set_views_jpeg(s.cams, [None] * s.n_views, images=s.images, **kw)
            assert e.value.status == 1 and view in str(e.value) and why in str(e.value), str(e.value)
            assert "lens" in e.value.stats
            with pytest.raises(M.MvsError) as e:             # ... and gone after the refusal
                c.data_costs(M.Settings())
            assert e.value.status == 6, str(e.value)
            with pytest.raises(M.MvsError) as e:
                c.view_image(0)
            assert e.value.status == 6
        for kw, view, why in cases[:3]:                       # the route on its own refuses the same lenses
            with pytest.raises(M.MvsError) as e:
                c.undistort_images(s.images, kw["lens"])
            assert e.value.status == 1 and view in str(e.value) and why in str(e.value)
        # a following good call works
        c.set_views(s.cams, s.images, lens=good)
        _same([c.view_image(j) for j in range(s.n_views)], undist)
        _same_result(_table_and_labels(c, s), ref[0])
    finally:
        c.close()


# ---- the paths without a lens ----
def test_default_paths_untouched(jpeg_scene):
    s, files, pixels = jpeg_scene
    zero = np.zeros((s.n_views, 3), np.float32)
    c = M.Context(0)
    try:
        c.set_mesh(s.verts, s.faces, s.normals)
        assert c.set_views(s.cams, s.images) is None
        _same([c.view_image(j) for j in range(s.n_views)], s.images)
        plain = _table_and_labels(c, s)
        st = c.set_views(s.cams, s.images, lens=zero)
        assert st["batches"] == 0 and st["staging_bytes"] == 0 and st["views_undistorted"] == 0
        _same([c.view_image(j) for j in range(s.n_views)], s.images)
        _same_result(_table_and_labels(c, s), plain)
        st = c.set_views_jpeg(s.cams, files, images=pixels)
        assert "lens" not in st
        _same([c.view_image(j) for j in range(s.n_views)], pixels)
        plain = _table_and_labels(c, s)
        st = c.set_views_jpeg(s.cams, files, images=pixels, lens=zero)
        assert st["lens"]["batches"] == 0 and st["lens"]["staging_bytes"] == 0 and st["batches"] == 1
        _same([c.view_image(j) for j in range(s.n_views)], pixels)
        _same_result(_table_and_labels(c, s), plain)
    finally:
        c.close()
