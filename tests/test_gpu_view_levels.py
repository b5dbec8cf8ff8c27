"""View input on the GPU: pyramid levels, views halved on the device on their way in (DESIGN.md section 4 "View input" item 14;
csrc/k_level.hip, csrc/level.h).  tests/tools/view_levels_model.py is the reference throughout (tests/test_view_levels_host.py holds the
host twin to it), under a lens the model of oracle.undistort.

The route on its own: Context.halve_images on every size x level in ONE call, back to back, every start residue modulo 16 present and
levels mixed in the launch, the host copy and the device buffer; then every image alone.  The same under the eight lenses.
set_views(levels=) and set_views_files(levels=) with JPEG, PNG and pixel views, a lens and per-view levels mixed in one call: every
view's image as it lies in the context, table and labels against set_views on the model's images bit for bit, a scratch cap that cuts
the views into batches, the cap one byte too small.  Masks at a level: the keep words against the AND rule.  Every refusal.  The calls
without levels untouched."""
import io
import re

import numpy as np
import pytest

import mvs_texturing_amd as M
import oracle_py as O
import jpeg_full_decode as FD
import util_cases as U
import view_levels_model as VL
from conftest import get_scene

pytestmark = pytest.mark.gpu

MVS_ERR_INVALID, MVS_ERR_STATE = 1, 6      # include/mvs_viewsel.h
WIDTHS = (2, 3, 4, 5, 6, 15, 16, 17, 21, 22, 31, 32, 33, 63, 64, 65, 127, 129, 257)
HEIGHTS = (2, 3, 5, 8, 9, 33)
# rows longer than one segment of a block (1024, 512, 128, 32 level pixels at levels 1 .. 4): two and three segments, the last one short
LONG = ((5, 1025), (3, 2051), (2, 4099), (17, 515))
LENSES = ((0.9, -0.2, 0.05), (1.3, 0.15, -0.03), (0.8, 0.1, 0.0), (1.1, -0.12, 0.0), (0.5, -0.5, 0.0), (0.5, 0.6, 0.0), (0.6, 0.9, 0.7), (1.0, 0.0, 0.3))


@pytest.fixture(scope="module")
def ctx():
    c = M.Context(0)
    yield c
    c.close()


def image(h, w):
    """pixel values 1 .. 255: a black pixel of an undistorted image is one without a source"""
    return np.random.default_rng(1000 * h + w).integers(1, 256, (h, w, 3)).astype(np.uint8)


def black(img):
    return int((img.reshape(-1, 3) == 0).all(axis=1).sum())


def _same(images, refs):
    assert len(images) == len(refs)
    for k, (a, b) in enumerate(zip(images, refs)):
        assert a.shape == b.shape and a.dtype == np.uint8, (k, a.shape, b.shape)
        assert np.array_equal(a, b), "image %d (%s): %d bytes differ, first at %s" % (k, a.shape, int((a != b).sum()), np.argwhere(a != b)[0].tolist())


# ---- 1. the route on its own ----
@pytest.fixture(scope="module")
def all_cases():
    sizes = [(h, w) for w in WIDTHS for h in HEIGHTS] + list(LONG)
    cases = [(size, level) for size in sizes for level in range(5)]         # levels alternate: mixed in the launch
    images = [image(*size) for size, _ in cases]
    refs = [VL.halve(i, level) for i, (_, level) in zip(images, cases)]
    return cases, images, refs


def test_route_on_its_own(ctx, all_cases):
    cases, images, refs = all_cases
    levels = [level for _, level in cases]
    starts = np.concatenate([[0], np.cumsum([r.size for r in refs])])[:-1]
    assert {int(s) % 16 for s in starts} == set(range(16))
    out, st = ctx.halve_images(images, levels)
    _same(out, refs)
    halved = [(i, r) for i, r, l in zip(images, refs, levels) if l]
    assert st["views_halved"] == len(halved) and st["batches"] == 1 and st["pixels_no_source"] == 0
    assert st["pixels_in"] == sum(i.size // 3 for i, _ in halved) and st["pixels_out"] == sum(r.size // 3 for _, r in halved)
    assert st["staging_bytes"] >= sum(i.size for i in images)
    # the images left on the device: read through the deflate route, which takes device bytes and has a host twin
    dev, _ = ctx.halve_images(images, levels, on_device=True)
    base = dev[0][0].ptr
    assert [a.ptr - base for a, _, _ in dev] == [int(s) for s in starts]
    for k, (arr, h, w) in enumerate(dev):
        assert (h, w, 3) == refs[k].shape
        assert ctx.deflate_rle(arr) == M.deflate_rle(refs[k].tobytes()), cases[k]


def test_every_image_alone(ctx, all_cases):
    cases, images, refs = all_cases
    for k, (size, level) in enumerate(cases):
        out, st = ctx.halve_images([images[k]], level)
        assert np.array_equal(out[0], refs[k]), (size, level)
        assert st["views_halved"] == (1 if level else 0)


# ---- 2. under a lens ----
def test_route_under_lenses(ctx):
    sizes = [(h, w) for w in WIDTHS for h in HEIGHTS] + [(5, 1025), (17, 515)]
    cases = [(size, level, LENSES[(k + level) % len(LENSES)]) for k, size in enumerate(sizes) for level in range(5)]
    images = [image(*size) for size, _, _ in cases]
    undist = [O.undistort(i, *l) for i, (_, _, l) in zip(images, cases)]
    refs = [VL.halve(u, level) for u, (_, level, _) in zip(undist, cases)]
    lens = np.array([l for _, _, l in cases], np.float32)
    out, st = ctx.halve_images(images, [level for _, level, _ in cases], lens=lens)
    _same(out, refs)
    none = sum(black(u) for u, (_, _, l) in zip(undist, cases) if l[1] != 0.0)
    assert st["pixels_no_source"] == none > 0                                 # full-size pixels, whatever the level
    assert any(black(u) and level for u, (_, level, _) in zip(undist, cases))
    assert any(not np.array_equal(u, i) for u, i in zip(undist, images))
    for k in range(0, len(cases), 37):                                        # ... and alone
        out, _ = ctx.halve_images([images[k]], [cases[k][1]], lens=lens[k:k + 1])
        assert np.array_equal(out[0], refs[k]), cases[k]


# ---- 3. the view inputs ----
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


def _source(img, level):
    """a photograph whose level `level` has img's size: img enlarged 2^level times with detail added, the last columns and rows cut off so
    that every size on the way down is odd"""
    n = 1 << level
    if not level:
        return img
    big = np.repeat(np.repeat(img, n, axis=0), n, axis=1).astype(np.int16)
    big += np.random.default_rng(level).integers(-9, 10, big.shape, dtype=np.int16)
    h, w = big.shape[:2]
    big = np.clip(big, 1, 255).astype(np.uint8)[:h - n + 1, :w - n + 1]
    assert VL.level_size(big.shape[1], big.shape[0], level) == (img.shape[1], img.shape[0])
    return np.ascontiguousarray(big)


SCENE_LEVELS = (1, 2, 1, 2, 1, 3, 1, 0)
SCENE_LENS = {6: (1.1, -0.12, 0.0)}


def _lens_rows(n, lenses):
    rows = np.zeros((n, 3), np.float32)
    rows[:, 0] = 1.0
    for j, l in lenses.items():
        rows[j] = l
    return rows


def _png(img, palette=False):
    from PIL import Image
    f = io.BytesIO()
    im = Image.fromarray(img)
    (im.quantize(256) if palette else im).save(f, "PNG")
    return f.getvalue()


def _scene_files(s, levels, lenses):
    """view 0: a 4:2:0 JPEG, 1: 4:4:4, 2: grayscale, 3: an RGB PNG, 4: a palette PNG, 5: pixels, 6: a 4:2:0 JPEG, 7: pixels -- photographs
    whose level levels[j] has the size of the scene's views.  pixels[j]: what Pillow reads from the file; model[j]: the image the context
    must hold"""
    from PIL import Image
    src = [_source(s.images[j], levels[j]) for j in range(s.n_views)]
    files = [FD.pillow_file(src[0], quality=90, subsampling=2), FD.pillow_file(src[1], quality=90, subsampling=0),
             FD.pillow_file(np.asarray(Image.fromarray(src[2]).convert("L")), quality=90), _png(src[3]), _png(src[4], palette=True), None,
             FD.pillow_file(src[6], quality=90, subsampling=2), None]
    pixels = [np.asarray(Image.open(io.BytesIO(f)).convert("RGB")) if f is not None else src[j] for j, f in enumerate(files)]
    model = [VL.halve(O.undistort(p, *lenses[j]) if j in lenses else p, levels[j]) for j, p in enumerate(pixels)]
    assert all(m.shape == (240, 320, 3) for m in model)
    return files, pixels, model


def _reference(s, model):
    c = M.Context(0)
    try:
        c.set_mesh(s.verts, s.faces, s.normals); c.set_views(s.cams, model)
        return _table_and_labels(c, s)
    finally:
        c.close()


@pytest.fixture(scope="module")
def level_scene():
    """the suite's small scene with levels 0 .. 3 mixed, view 6 under a lens; ref: set_views on the model"""
    s = get_scene("tiny")
    files, pixels, model = _scene_files(s, SCENE_LEVELS, SCENE_LENS)
    return s, files, pixels, model, _reference(s, model)


def test_set_views_levels_from_pixels(level_scene):
    s, files, pixels, model, ref = level_scene
    c = M.Context(0)
    try:
        c.set_mesh(s.verts, s.faces, s.normals)
        st = c.set_views(s.cams, pixels, lens=_lens_rows(s.n_views, SCENE_LENS), levels=SCENE_LEVELS)
        _same([c.view_image(j) for j in range(s.n_views)], model)
        assert st["level"]["views_halved"] == 7 and st["level"]["batches"] == 1 and st["lens"]["views_undistorted"] == 1
        assert st["level"]["pixels_out"] == 7 * 320 * 240 and st["level"]["pixels_in"] == sum(p.size // 3 for p, l in zip(pixels, SCENE_LEVELS) if l)
        assert st["level"]["staging_bytes"] == sum((p.size + 15) // 16 * 16 for p, l in zip(pixels, SCENE_LEVELS) if l)
        assert st["lens"]["pixels_no_source"] == black(O.undistort(np.full(pixels[6].shape, 1, np.uint8), *SCENE_LENS[6])) > 0
        _same_result(_table_and_labels(c, s), ref)
        # an int for all views: level 1 of the model is the model of level + 1
        c.set_views(s.cams, [_source(m, 1) for m in model], levels=1)
        _same([c.view_image(j) for j in range(s.n_views)], [VL.halve(_source(m, 1), 1) for m in model])
    finally:
        c.close()


def test_set_views_files_levels(level_scene):
    s, files, pixels, model, ref = level_scene
    lens = _lens_rows(s.n_views, SCENE_LENS)
    c = M.Context(0)
    try:
        c.set_mesh(s.verts, s.faces, s.normals)
        st = c.set_views_files(s.cams, files, images=pixels, lens=lens, levels=SCENE_LEVELS)
        _same([c.view_image(j) for j in range(s.n_views)], model)
        assert st["jpeg"]["files"] == 4 and st["png"]["files"] == 2 and st["level"]["views_halved"] == 7 and st["lens"]["views_undistorted"] == 1
        assert st["level"]["batches"] == 3                                    # the pixel view's group, the JPEGs' batch, the PNGs'
        _same_result(_table_and_labels(c, s), ref)
        # a cap one byte below the level-3 photograph's staging is refused, naming it; at its staging the views go up in groups
        with pytest.raises(M.MvsError) as e:
            c.set_views_files(s.cams, [None] * s.n_views, params=M.default_jpegdec_params(max_scratch_bytes=pixels[5].size - 1), images=pixels, levels=SCENE_LEVELS)
        assert "view 5 needs %d bytes of staging" % ((pixels[5].size + 15) // 16 * 16) in str(e.value), str(e.value)
        st = c.set_views_files(s.cams, [None] * s.n_views, params=M.default_jpegdec_params(max_scratch_bytes=(pixels[5].size + 15) // 16 * 16), images=pixels, lens=lens, levels=SCENE_LEVELS)
        assert st["level"]["batches"] >= 3
        _same([c.view_image(j) for j in range(s.n_views)], model)
    finally:
        c.close()


def _batches(need, cap):
    """the batch cut (csrc/view_batches.h): a batch takes its first item, then grows while the sum stays <= cap"""
    n, total = 0, None
    for v in need:
        if total is None or total + v > cap:
            n, total = n + 1, 0
        total += v
    return n


def test_every_view_a_batch_of_its_own():
    """all views at level 1: every photograph is 639 x 479, and at a cap of the largest single need no two files share a batch"""
    s = get_scene("tiny")
    levels, lenses = [1] * s.n_views, {0: (1.1, -0.12, 0.0), 3: (0.9, -0.2, 0.05), 5: (1.3, 0.15, -0.03)}
    files, pixels, model = _scene_files(s, levels, lenses)
    lens = _lens_rows(s.n_views, lenses)
    ref = _reference(s, model)
    staged = (639 * 479 * 3 + 15) // 16 * 16
    c = M.Context(0)
    try:
        c.set_mesh(s.verts, s.faces, s.normals)
        need = {}                                             # every file's need: its decoder's scratch, read from a refusal, and its staged pixels
        for j, f in enumerate(files):
            if f is not None:
                with pytest.raises(M.MvsError) as e:
                    (c.decode_pngs if f[:4] == b"\x89PNG" else c.decode_jpegs)([f], params=M.default_jpegdec_params(max_scratch_bytes=1))
                need[j] = int(re.search(r"needs (\d+) bytes of scratch", str(e.value)).group(1)) + staged
        cap = max(need.values())
        top = max(need, key=need.get)
        jpegs, pngs = [need[j] for j in (0, 1, 2, 6)], [need[j] for j in (3, 4)]
        print("needs", need, "cap", cap)
        st = c.set_views_files(s.cams, files, params=M.default_jpegdec_params(max_scratch_bytes=cap), images=pixels, lens=lens, levels=levels)
        assert st["jpeg"]["batches"] >= _batches(jpegs, cap) and st["png"]["batches"] >= _batches(pngs, cap)
        assert st["level"]["batches"] == _batches(jpegs, cap) + _batches(pngs, cap) + _batches([staged, staged], cap) >= 4
        assert st["level"]["views_halved"] == 8 and st["lens"]["views_undistorted"] == 3 and st["level"]["staging_bytes"] <= cap
        _same([c.view_image(j) for j in range(s.n_views)], model)
        _same_result(_table_and_labels(c, s), ref)
        # one byte below the largest need: refused, naming that view
        with pytest.raises(M.MvsError) as e:
            c.set_views_files(s.cams, files, params=M.default_jpegdec_params(max_scratch_bytes=cap - 1), images=pixels, lens=lens, levels=levels)
        assert e.value.status == MVS_ERR_INVALID and "view %d needs %d bytes of scratch, max_scratch_bytes is %d" % (top, cap, cap - 1) in str(e.value), str(e.value)
        assert c.n_views == 0
        # a cap of one photograph: every view is a group of its own as pixels
        st = c.set_views_files(s.cams, [None] * s.n_views, params=M.default_jpegdec_params(max_scratch_bytes=staged), images=pixels, lens=lens, levels=levels)
        assert st["level"]["batches"] == 8 and st["level"]["staging_bytes"] == staged
        _same([c.view_image(j) for j in range(s.n_views)], model)
    finally:
        c.close()


# ---- 4. masks at a level ----
MASK_SIZES = ((9, 31), (33, 32), (35, 33), (9, 63), (33, 64), (35, 65))       # (h, w) of the source


def _undistort_mask(mask, lens):
    rep = np.ascontiguousarray(np.repeat(np.where(mask != 0, 255, 0).astype(np.uint8)[:, :, None], 3, axis=2))
    return np.where(O.undistort(rep, *lens)[:, :, 0] == 255, 255, 0).astype(np.uint8)


def _mask_cases(level):
    """(source image, source mask or None) per view: random masks, a single masked source pixel in the clamped last column, the last row
    and the corner, a mask that keeps everything -- and views without a mask among them"""
    rng = np.random.default_rng(level)
    out = []
    for h, w in MASK_SIZES:
        dense = np.where(rng.random((h, w)) < 0.1, 0, rng.integers(1, 256, (h, w))).astype(np.uint8)
        singles = []
        for (y, x) in ((h // 2, w - 1), (h - 1, w // 3), (h - 1, w - 1)):
            m = np.full((h, w), 255, np.uint8); m[y, x] = 0
            singles.append(m)
        for m in [dense] + singles + [np.full((h, w), 7, np.uint8), None]:
            out.append((image(h, w), m))
    return out


@pytest.mark.parametrize("with_lens", (False, True), ids=("plain", "lens"))
@pytest.mark.parametrize("level", (1, 2))
def test_masks_at_a_level(level, with_lens):
    cases = _mask_cases(level)
    n = len(cases)
    lens = np.array([LENSES[k % len(LENSES)] if with_lens else (1.0, 0.0, 0.0) for k in range(n)], np.float32)
    flat = [(O.undistort(i, *l) if l[1] != 0.0 else i, None if m is None else (_undistort_mask(m, l) if l[1] != 0.0 else m)) for (i, m), l in zip(cases, lens.tolist())]
    model_images = [VL.halve(i, level) for i, _ in flat]
    model_keep = [None if m is None else VL.keep_level(m, level) for _, m in flat]
    model_masks = [None if k is None else np.where(k, 255, 0).astype(np.uint8) for k in model_keep]
    s = U.prep_scene(model_images)
    st = M.Settings(data_term="area")
    c, r = M.Context(0), M.Context(0)
    try:
        r.set_mesh(s.verts, s.faces, s.normals); r.set_views(s.cams, model_images, masks=model_masks)       # the level-0 route on the model
        r.data_costs(st)
        c.set_mesh(s.verts, s.faces, s.normals)
        c.set_views(s.cams, [i for i, _ in cases], lens=lens if with_lens else None, masks=[m for _, m in cases], levels=level)
        _same([c.view_image(j) for j in range(n)], model_images)
        ms = c.mask_stats
        assert ms["views_masked"] == sum(m is not None for _, m in cases) and ms["views_undistorted"] == sum(1 for (_, m), l in zip(cases, lens.tolist()) if m is not None and l[1] != 0.0)
        assert ms["pixels"] == sum(k.size for k in model_keep if k is not None) and ms["pixels_masked_out"] == sum(int((~k).sum()) for k in model_keep if k is not None)
        for j in range(n):
            got = c.view_keep_bits(j)
            if model_keep[j] is None:
                assert got is None, j
                continue
            bits, pad = got
            assert np.array_equal(bits, model_keep[j]) and not pad.any(), (j, cases[j][0].shape, int((bits != model_keep[j]).sum()))
            assert np.array_equal(bits, r.view_keep_bits(j)[0])
        if not with_lens:                                                     # one masked source pixel takes exactly its level pixel
            for j, (_, m) in enumerate(cases):
                if m is not None and (m == 0).sum() == 1:
                    (y, x), = np.argwhere(m == 0).tolist()
                    assert (~model_keep[j]).sum() == 1 and not model_keep[j][y >> level, x >> level]
        c.data_costs(st)
        ta, tb = c.costs_download(), r.costs_download()
        assert np.array_equal(ta.col_ptr, tb.col_ptr) and np.array_equal(ta.view_id, tb.view_id) and np.array_equal(ta.cost.view(np.uint32), tb.cost.view(np.uint32))
        flags = c.prep_mask_flags()
        assert np.array_equal(flags, r.prep_mask_flags()) and flags.any()
        for j in np.flatnonzero(flags).tolist():              # (a view without a validity mask has no products)
            pa, pb = c.prep_products(j), r.prep_products(j)
            assert np.array_equal(pa.mask_words, pb.mask_words) and np.array_equal(pa.summary_words, pb.summary_words), j
        # clearing restores the unmasked table
        c.set_view_masks(None); c.data_costs(st)
        r.set_view_masks(None); r.data_costs(st)
        tc, td = c.costs_download(), r.costs_download()
        assert np.array_equal(tc.col_ptr, td.col_ptr) and np.array_equal(tc.cost.view(np.uint32), td.cost.view(np.uint32))
        assert all(c.view_keep_bits(j) is None for j in range(n))
    finally:
        c.close(); r.close()


def test_masks_decide_the_table_at_a_level(level_scene):
    """the suite's small scene at its mixed levels: a disc masked on every photograph, at the source's size; table and labels (area term) are
    those of the level-0 route on the model's images with the model's level masks, and differ from the unmasked ones"""
    s, files, pixels, model, ref = level_scene
    lens = _lens_rows(s.n_views, SCENE_LENS)
    masks = []
    for p in pixels:
        h, w = p.shape[:2]
        yy, xx = np.mgrid[0:h, 0:w]
        masks.append(np.where((xx - w * 0.55) ** 2 + (yy - h * 0.5) ** 2 < (0.3 * h) ** 2, 0, 255).astype(np.uint8))
    model_masks = [np.where(VL.keep_level(_undistort_mask(m, SCENE_LENS[j]) if j in SCENE_LENS else m, SCENE_LEVELS[j]), 255, 0).astype(np.uint8) for j, m in enumerate(masks)]
    st = M.Settings(data_term="area")
    c = M.Context(0)
    try:
        c.set_mesh(s.verts, s.faces, s.normals)
        c.set_views(s.cams, model)
        plain = _table_and_labels(c, s, st)
        c.set_views(s.cams, model, masks=model_masks)
        want = _table_and_labels(c, s, st)
        assert want[0].nnz < 0.97 * plain[0].nnz, (want[0].nnz, plain[0].nnz)
        c.set_views_files(s.cams, files, images=pixels, lens=lens, masks=masks, levels=SCENE_LEVELS)
        for j in range(s.n_views):
            assert np.array_equal(c.view_keep_bits(j)[0], model_masks[j] != 0), j
        _same_result(_table_and_labels(c, s, st), want)
        c.set_view_masks(None)
        _same_result(_table_and_labels(c, s, st), plain)
    finally:
        c.close()


# ---- 5. refusals ----
def test_refusals(level_scene):
    s, files, pixels, model, ref = level_scene
    n = s.n_views
    lens = _lens_rows(n, SCENE_LENS)
    sizes = [(p.shape[1], p.shape[0]) for p in pixels]

    def levels(j, v):
        out = list(SCENE_LEVELS); out[j] = v
        return out

    def src(j, size):
        out = list(sizes); out[j] = size
        return out

    def cams(j, w, h):
        out = dict(s.cams)
        out["width"] = s.cams["width"].copy(); out["height"] = s.cams["height"].copy()
        out["width"][j], out["height"][j] = w, h
        return out

    bad_lens = np.zeros((n, 4), np.float32); bad_lens[:, :3] = lens; bad_lens[6] = (0.0, 0.1, 0.0, 0)
    tiny_px = list(pixels); tiny_px[5] = image(3, 2)
    cut = list(files); cut[1] = b"\xff\xd8" + bytes(100)                       # no JPEG, no PNG
    cases = [(dict(levels=levels(3, 5), src_sizes=sizes), "view 3", "is above 4"),
             (dict(levels=[(l, 1 if j == 4 else 0) for j, l in enumerate(SCENE_LEVELS)]), "view 4", "reserved must be 0"),
             (dict(levels=levels(1, 1), src_sizes=sizes), "view 1", "1277 x 957 at level 1 is 639 x 479, the view 320 x 240"),
             (dict(src_sizes=src(7, (321, 240))), "view 7", "321 x 240 at level 0 is 321 x 240, the view 320 x 240"),
             (dict(src_sizes=src(0, (640, 480))), "view 0", "the frame is 639 x 479, the view 640 x 480"),
             (dict(src_sizes=src(3, (1280, 960))), "view 3", "the frame is 1277 x 957, the view 1280 x 960"),
             (dict(images=tiny_px, cams=cams(5, 1, 2), levels=levels(5, 1)), "view 5", "below 2 x 2"),
             (dict(lens=bad_lens), "view 6", "positive focal length"),
             (dict(files=cut), "view 1", "view 1"),
             (dict(params=M.default_jpegdec_params(max_scratch_bytes=1000)), "view 5", "bytes of staging, max_scratch_bytes is 1000")]
    c = M.Context(0)
    try:
        c.set_mesh(s.verts, s.faces, s.normals)
        for kw, view, why in cases:
            c.set_views(s.cams, model)                        # views are there ...
            args = dict(files=files, images=pixels, lens=lens, levels=SCENE_LEVELS, cams=s.cams)
            args.update(kw)
            with pytest.raises(M.MvsError) as e:
                c.set_views_files(args.pop("cams"), args.pop("files"), **args)
            assert e.value.status == MVS_ERR_INVALID and view in str(e.value) and why in str(e.value), (why, str(e.value))
            assert "level" in e.value.stats and c.n_views == 0
            with pytest.raises(M.MvsError) as e:             # ... and gone after the refusal
                c.data_costs(M.Settings())
            assert e.value.status == MVS_ERR_STATE, str(e.value)
        # the route on its own refuses a level above 4 and the lens
        with pytest.raises(M.MvsError) as e:
            c.halve_images(pixels[5:7], [1, 5])
        assert e.value.status == MVS_ERR_INVALID and "view 1" in str(e.value) and "is above 4" in str(e.value)
        with pytest.raises(M.MvsError) as e:
            c.halve_images(pixels[5:7], 1, lens=bad_lens[5:7])
        assert e.value.status == MVS_ERR_INVALID and "view 1" in str(e.value) and "positive focal length" in str(e.value)
        # a following good call works
        c.set_views_files(s.cams, files, images=pixels, lens=lens, levels=SCENE_LEVELS)
        _same([c.view_image(j) for j in range(n)], model)
        _same_result(_table_and_labels(c, s), ref)
    finally:
        c.close()


# ---- 6. defaults ----
def _counts(d):
    return {k: ({a: b for a, b in v.items() if not a.startswith("ms_")} if isinstance(v, dict) else v) for k, v in d.items() if not k.startswith("ms_")}


def test_defaults_untouched(level_scene):
    s, _, _, _, _ = level_scene
    from PIL import Image
    files = [FD.pillow_file(s.images[0], quality=90, subsampling=2), _png(s.images[1]), None, None, FD.pillow_file(s.images[4], quality=90, subsampling=0), None, _png(s.images[6], palette=True), None]
    pixels = [np.asarray(Image.open(io.BytesIO(f)).convert("RGB")) if f is not None else s.images[j] for j, f in enumerate(files)]
    lens = _lens_rows(s.n_views, {2: (0.9, -0.2, 0.05), 4: (1.1, -0.12, 0.0)})
    c = M.Context(0)
    try:
        c.set_mesh(s.verts, s.faces, s.normals)
        for kw in (dict(), dict(lens=lens)):
            today = c.set_views_files(s.cams, files, images=pixels, **kw)
            assert "level" not in today
            images = [c.view_image(j) for j in range(s.n_views)]
            result = _table_and_labels(c, s)
            st = c.set_views_files(s.cams, files, images=pixels, levels=0, **kw)
            assert st["level"]["views_halved"] == 0 and st["level"]["batches"] == 0 and st["level"]["pixels_in"] == 0
            assert st["level"]["staging_bytes"] == today["lens"]["staging_bytes"] == (320 * 240 * 3 if kw else 0)   # what the lens route alone needs
            assert _counts({k: st[k] for k in today}) == _counts(today)
            _same([c.view_image(j) for j in range(s.n_views)], images)
            _same_result(_table_and_labels(c, s), result)
            st = c.set_views_files(s.cams, files, images=pixels, levels=[0] * s.n_views, **kw)
            assert _counts({k: st[k] for k in today}) == _counts(today)
            _same_result(_table_and_labels(c, s), result)
        # set_views and set_views_jpeg: levels=None is the call of before, levels=0 the same views
        assert c.set_views(s.cams, s.images) is None
        plain = _table_and_labels(c, s)
        st = c.set_views(s.cams, s.images, levels=0)
        assert st["level"]["views_halved"] == 0 and st["lens"]["batches"] == 0 and st["level"]["staging_bytes"] == 0
        _same([c.view_image(j) for j in range(s.n_views)], s.images)
        _same_result(_table_and_labels(c, s), plain)
        jf = [f if f is not None and f[:2] == b"\xff\xd8" else None for f in files]
        today = c.set_views_jpeg(s.cams, jf, images=pixels)
        assert "lens" not in today and "level" not in today
        result = _table_and_labels(c, s)
        st = c.set_views_jpeg(s.cams, jf, images=pixels, levels=0)
        assert _counts(st["jpeg"]) == _counts(today)
        _same_result(_table_and_labels(c, s), result)
    finally:
        c.close()
