"""View input on the GPU, PNG files (DESIGN.md section 4 "View input"; csrc/k_pngdec.hip): Context.decode_pngs gives, byte for byte, what
the host twin of csrc/png_dec.h gives (tests/test_png_decode_host.py holds the twin to Pillow and to a plain Python statement, bit for
bit) on the whole set of tests/tools/png_cases.py -- good files, hand-assembled deflate streams, the library's own files -- in one call
of many files and in calls of one file each.  The stats agree with the statement's counts: blocks per kind, rows per filter type, raw
bytes, IDAT chunks.  A scratch cap that forces three batches gives the same bytes.  Every refusal that only the device can see arrives
with its reason and the file's number, and the context stays usable.

set_views_files: the suite's small scene saved as PNG gives the table and the labels of set_views on Pillow's decode of the same files,
bit for bit; so does a mixed list of PNG, baseline JPEG and pixel views with a lens and masks behind some of them, against
set_views(lens=, masks=) on host-decoded pixels; a size mismatch is refused and leaves the context without views; set_views afterwards
works as before; a PNG handed to set_views_jpeg is still refused."""
import io
import re

import numpy as np
import pytest

import mvs_texturing_amd as M
import png_cases as PC
import jpeg_full_decode as FD
from conftest import get_scene

pytestmark = pytest.mark.gpu

CASES = dict(PC.good_cases())
CASES.update(PC.hand_cases())
NAMES = sorted(CASES)
REFUSALS = PC.refusals()
DEVICE_REFUSALS = sorted(k for k, (f, why, host) in REFUSALS.items() if not host)


@pytest.fixture(scope="module")
def ctx():
    c = M.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def twin():
    return {k: M.decode_png(CASES[k]) for k in NAMES}


def _same(images, refs):
    assert len(images) == len(refs)
    for k, (a, b) in enumerate(zip(images, refs)):
        assert a.shape == b.shape and a.dtype == np.uint8, k
        assert np.array_equal(a, b), "image %d: %d bytes differ" % (k, int((a != b).sum()))


def _counts(names):
    st = [PC.decode(CASES[k]) for k in names]
    return {"idat_chunks": sum(s["idat_chunks"] for s in st), "zlib_bytes": sum(s["zlib_bytes"] for s in st), "raw_bytes": sum(s["raw_bytes"] for s in st),
            "stored_blocks": sum(s["blocks"][0] for s in st), "fixed_blocks": sum(s["blocks"][1] for s in st), "dynamic_blocks": sum(s["blocks"][2] for s in st),
            "filter_rows": [sum(s["rows"][t] for s in st) for t in range(5)]}


def test_all_files_in_one_call(ctx, twin):
    images, st = ctx.decode_pngs([CASES[k] for k in NAMES])
    _same(images, [twin[k] for k in NAMES])
    assert st["files"] == len(NAMES) and st["batches"] == 1 and st["file_bytes"] == sum(len(CASES[k]) for k in NAMES)
    for k, v in _counts(NAMES).items():
        assert st[k] == v, (k, st[k], v)
    assert all(v > 0 for v in st["filter_rows"]) and st["stored_blocks"] and st["fixed_blocks"] and st["dynamic_blocks"]


@pytest.mark.parametrize("name", NAMES)
def test_one_file_per_call(ctx, twin, name):
    images, st = ctx.decode_pngs([CASES[name]])
    _same(images, [twin[name]])
    assert st["files"] == 1
    for k, v in _counts([name]).items():
        assert st[k] == v, (k, st[k], v)


def test_library_files(ctx, tmp_path):
    own = PC.library_cases(M, tmp_path)
    names = sorted(own)
    images, _ = ctx.decode_pngs([own[k] for k in names])
    _same(images, [M.decode_png(own[k]) for k in names])
    enc, _ = ctx.encode_pngs([images[0]])   # the device encoder's file of a decoded image comes back as that image
    again, _ = ctx.decode_pngs([bytes(enc[0])])
    _same(again, [images[0]])


def test_on_device_output(ctx, twin):
    """the images left on the device: read through the deflate route, which takes device bytes and has a host twin"""
    names = NAMES[3::40]
    out, _ = ctx.decode_pngs([CASES[k] for k in names], on_device=True)
    for k, (arr, h, w) in zip(names, out):
        assert (h, w, 3) == twin[k].shape and arr.shape == (h * w * 3,)
        assert ctx.deflate_rle(arr) == M.deflate_rle(twin[k].tobytes()), k


# ---- batches ----
def _scratch_needs(ctx, files):
    needs = []
    for f in files:
        with pytest.raises(M.MvsError) as e:
            ctx.decode_pngs([f], params=M.default_jpegdec_params(max_scratch_bytes=1))
        assert e.value.stats["files"] == 1 and e.value.stats["file_bytes"] == len(f)     # refused with the stats filled
        needs.append(int(re.search(r"needs (\d+) bytes of scratch", str(e.value)).group(1)))
    return needs


def _batches(needs, cap):
    n, total = 1, 0
    for v in needs:
        if total and total + v > cap:
            n += 1; total = 0
        total += v
    return n


def _cap_for(needs, batches):
    for cap in sorted({sum(needs[a:b]) for a in range(len(needs)) for b in range(a + 1, len(needs) + 1)}):
        if cap >= max(needs) and _batches(needs, cap) == batches:
            return cap
    raise AssertionError("no cap gives %d batches" % batches)


def test_three_batches(ctx, twin):
    names = NAMES[10:90:9]
    files = [CASES[k] for k in names]
    cap = _cap_for(_scratch_needs(ctx, files), 3)
    images, st = ctx.decode_pngs(files, params=M.default_jpegdec_params(max_scratch_bytes=cap))
    assert st["batches"] == 3
    _same(images, [twin[k] for k in names])


# ---- refusals the host cannot see: they come from the device, worded as the twin words them ----
@pytest.mark.parametrize("name", DEVICE_REFUSALS)
def test_device_refusals(ctx, twin, name):
    f, why, _ = REFUSALS[name]
    good = "64x48_c2_f5" if "64x48_c2_f5" in CASES else NAMES[0]
    with pytest.raises(M.MvsError) as e:
        ctx.decode_pngs([CASES[good], f])
    assert e.value.status == 1 and why in str(e.value) and "view 1" in str(e.value), str(e.value)
    assert e.value.stats["files"] == 2
    with pytest.raises(M.MvsError) as t:
        M.decode_png(f)
    assert str(e.value).split("view 1: ")[1] == str(t.value)   # the same message as the twin's, position included
    images, _ = ctx.decode_pngs([CASES[good]])
    _same(images, [twin[good]])


def test_host_refusals_name_the_view(ctx):
    f, why, _ = REFUSALS["adam7"]
    with pytest.raises(M.MvsError) as e:
        ctx.decode_pngs([CASES[NAMES[0]], CASES[NAMES[1]], f])
    assert why in str(e.value) and "view 2" in str(e.value)
    assert len(DEVICE_REFUSALS) >= 25


# ---- set_views_files ----
def _png(img, **kw):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(img).save(b, "PNG", **kw)
    return b.getvalue()


@pytest.fixture(scope="module")
def png_scene():
    s = get_scene("tiny")
    files = [_png(img) for img in s.images]
    pixels = [PC.pillow_rgb(f) for f in files]
    for a, b in zip(pixels, s.images):
        assert np.array_equal(a, b)
    return s, files, pixels


def _table_and_labels(c, s):
    c.data_costs(M.Settings())
    t = c.costs_download()
    labels, _ = c.view_selection(s.adj_ptr, s.adj)
    return t, labels


def _same_result(a, b):
    (ta, la), (tb, lb) = a, b
    assert np.array_equal(ta.col_ptr, tb.col_ptr) and np.array_equal(ta.view_id, tb.view_id)
    assert np.array_equal(ta.cost.view(np.uint32), tb.cost.view(np.uint32))
    assert np.array_equal(la, lb)


def test_set_views_files(png_scene):
    s, files, pixels = png_scene
    c = M.Context(0)
    try:
        c.set_mesh(s.verts, s.faces, s.normals); c.set_views(s.cams, pixels)
        ref = _table_and_labels(c, s)
        st = c.set_views_files(s.cams, files)
        assert st["png"]["files"] == s.n_views and st["png"]["batches"] == 1 and st["jpeg"]["files"] == 0
        assert c.n_views == s.n_views
        for j in (0, s.n_views - 1):
            assert np.array_equal(c.view_image(j), pixels[j])
        _same_result(_table_and_labels(c, s), ref)
        # a size mismatch between a file and its view is refused and leaves the context without views
        cams = {k: np.array(v).copy() for k, v in s.cams.items()}
        cams["width"][3] += 1
        with pytest.raises(M.MvsError) as e:
            c.set_views_files(cams, files)
        assert e.value.status == 1 and "view 3" in str(e.value) and "320 x 240" in str(e.value) and "321 x 240" in str(e.value)
        assert c.n_views == 0
        with pytest.raises(M.MvsError) as e:
            c.data_costs(M.Settings())
        assert e.value.status == 6
        # set_views afterwards works as before
        c.set_views(s.cams, pixels)
        _same_result(_table_and_labels(c, s), ref)
        # three batches: the same bytes, so the same table
        needs = []
        for f in files:
            with pytest.raises(M.MvsError) as e:
                c.decode_pngs([f], params=M.default_jpegdec_params(max_scratch_bytes=1))
            needs.append(int(re.search(r"needs (\d+) bytes of scratch", str(e.value)).group(1)))
        st = c.set_views_files(s.cams, files, params=M.default_jpegdec_params(max_scratch_bytes=_cap_for(needs, 3)))
        assert st["png"]["batches"] == 3
        _same_result(_table_and_labels(c, s), ref)
        # a corrupt file among the views
        bad = list(files); bad[5] = files[5][:len(files[5]) // 2] + files[5][len(files[5]) // 2 + 40:]
        with pytest.raises(M.MvsError) as e:
            c.set_views_files(s.cams, bad)
        assert "view 5" in str(e.value) and c.n_views == 0
        # a PNG handed to set_views_jpeg is still refused
        with pytest.raises(M.MvsError) as e:
            c.set_views_jpeg(s.cams, files)
        assert e.value.status == 1 and "view 0" in str(e.value) and c.n_views == 0
        c.set_views_files(s.cams, files)
        _same_result(_table_and_labels(c, s), ref)
    finally:
        c.close()


def test_set_views_files_mixed_with_lens_and_masks(png_scene):
    """PNG, baseline JPEG and pixel views in one list, a lens behind some of each kind and masks on some views"""
    s, files, pixels = png_scene
    V = s.n_views
    mixed, host = [], []
    for j in range(V):
        if j % 3 == 0:
            mixed.append(files[j]); host.append(pixels[j])
        elif j % 3 == 1:
            f = FD.pillow_file(s.images[j], quality=90, subsampling=2)
            mixed.append(f); host.append(FD.pillow_decode(f))
        else:
            mixed.append(None); host.append(np.ascontiguousarray(s.images[j]))
    lens = np.zeros((V, 3), np.float32)
    lens[:, 0] = 1.0
    for j in range(V):
        if j % 2 == 0:
            lens[j] = (0.9, -0.05 - 0.01 * j, 0.02 if j % 4 == 0 else 0.0)
    rs = np.random.RandomState(3)
    masks = [None] * V
    for j in (0, 1, 2, 4):
        m = np.full(pixels[j].shape[:2], 255, np.uint8)
        m[rs.randint(0, 120):, rs.randint(100, 300):] = 0
        masks[j] = m
    c = M.Context(0)
    try:
        c.set_mesh(s.verts, s.faces, s.normals)
        c.set_views(s.cams, host, lens=lens, masks=masks)
        ref = _table_and_labels(c, s)
        ref_images = [c.view_image(j).copy() for j in range(V)]
        st = c.set_views_files(s.cams, mixed, images=host, lens=lens, masks=masks)
        assert st["png"]["files"] == len(range(0, V, 3)) and st["jpeg"]["files"] == len(range(1, V, 3))
        assert st["lens"]["views_undistorted"] == len(range(0, V, 2))
        for j in range(V):
            assert np.array_equal(c.view_image(j), ref_images[j]), j
        _same_result(_table_and_labels(c, s), ref)
    finally:
        c.close()
