"""Row f9's compressed PNG route on the GPU (DESIGN.md section 4 "Model output" item 7; csrc/k_png.hip): Context.deflate_rle and
Context.encode_pngs give, byte for byte, what the host twin of csrc/png_rle.h gives (tests/test_png_rle_host.py holds the twin to zlib
and to a second statement of the filters) on the crafted streams and images of tests/tools/png_decode.py -- lengths around one and two
chunks, runs around the match lengths, runs that end at or straddle a chunk boundary: the smallest shapes at which the chunk indexing,
the carries across the threads' segments and the gather can go wrong -- in one call for all images, twice with the same bytes; models
saved with png_device 1 have the text and the pixels of the default route in fewer bytes; every refusal is followed by a good call; and
the route does not ask for libz."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import mvs_texturing_amd as M
import png_decode as PD
from conftest import ROOT, get_scene
from test_gpu_debug_model import _library_labels

pytestmark = pytest.mark.gpu

STREAMS, IMAGES = PD.streams(), PD.images()


@pytest.fixture(scope="module")
def ctx():
    c = M.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def twin_pngs():
    return {k: M.encode_png_rle(v) for k, v in IMAGES.items()}


@pytest.mark.parametrize("name", sorted(STREAMS))
def test_deflate_rle_equals_the_twin(ctx, name):
    data = STREAMS[name]
    z = ctx.deflate_rle(data)
    assert PD.inflate(z) == data
    assert len(z) <= PD.bound(len(data))
    assert z == M.deflate_rle(data)


def test_deflate_rle_of_a_device_array(ctx):
    import torch
    data = STREAMS["len_Cp1"]
    t = torch.frombuffer(bytearray(b"\x00" + data), dtype=torch.uint8).cuda()[1:]          # an odd device address
    assert ctx.deflate_rle(t) == M.deflate_rle(data)


def _check_pngs(pngs, stats, names, twin_pngs):
    rows = np.zeros(5, np.int64)
    for name, png in zip(names, pngs):
        assert png == twin_pngs[name], name
        pixels, filters, _ = PD.decode(png)
        assert np.array_equal(pixels, IMAGES[name]), name
        want, _ = PD.filtered(IMAGES[name])
        assert np.array_equal(filters, want), name
        rows += np.bincount(want, minlength=5)
    assert stats["filter_rows"] == rows.tolist()
    assert stats["png_bytes"] == sum(len(p) for p in pngs)
    assert stats["raw_bytes"] == sum(IMAGES[k].shape[0] * (3 * IMAGES[k].shape[1] + 1) for k in names)
    assert stats["chunks"] == sum(-(-IMAGES[k].shape[0] * (3 * IMAGES[k].shape[1] + 1) // PD.CHUNK) for k in names)


def test_encode_pngs_all_images_in_one_call(ctx, twin_pngs):
    import torch
    names = sorted(IMAGES)
    pngs, stats = ctx.encode_pngs([IMAGES[k] for k in names])
    _check_pngs(pngs, stats, names, twin_pngs)
    again, stats2 = ctx.encode_pngs([IMAGES[k] for k in names])
    assert again == pngs and stats2["filter_rows"] == stats["filter_rows"] and stats2["stored_chunks"] == stats["stored_chunks"]
    dev, stats3 = ctx.encode_pngs([torch.from_numpy(IMAGES[k]).cuda() for k in reversed(names)])
    _check_pngs(dev, stats3, list(reversed(names)), twin_pngs)
    assert ctx.encode_pngs([]) [0] == []


def test_encode_pngs_of_an_atlas_set(ctx, twin_pngs):
    """square images as the atlas-set dict save_model reads, on the host and on the device"""
    import torch
    names = ["zero_128x128", "pattern_256x256", "pattern_1x1"]
    size = np.array([IMAGES[k].shape[0] for k in names], np.uint32)
    pix = np.concatenate([[0], np.cumsum(size.astype(np.uint64) ** 2)]).astype(np.uint64)
    image = np.concatenate([IMAGES[k].reshape(-1, 3) for k in names])
    host, _ = ctx.encode_pngs(dict(atlas_size=size, atlas_pix_ptr=pix, image=image))
    assert host == [twin_pngs[k] for k in names]
    dev, _ = ctx.encode_pngs(dict(atlas_size=torch.from_numpy(size.astype(np.int32)).cuda(), atlas_pix_ptr=torch.from_numpy(pix.astype(np.int64)).cuda(),
                                  image=torch.from_numpy(image).cuda()))
    assert dev == host


def test_gather_at_every_alignment(ctx):
    """PD.alignment_images() in one call, from host arrays and from device tensors.  Every image is one chunk; chunk k lands 2 + 16 k
    bytes behind the chunks in front of it, each of which is its zlib stream without the 2 header bytes and the 4 of the Adler-32.  The
    sizes, not luck, spread those destinations over the residues modulo 16 and make a chunk shorter than its way to the next boundary."""
    import torch
    imgs = PD.alignment_images()
    want = [M.encode_png_rle(a) for a in imgs]
    chunk = np.array([len(p) - 57 - 6 for p in want])                  # 57: signature, IHDR, the IDAT chunk's frame, IEND
    start = 2 + 16 * np.arange(len(imgs)) + np.concatenate([[0], np.cumsum(chunk)[:-1]])
    assert len(set(int(x) % 16 for x in start)) >= 12
    assert any(n < (-s) % 16 for n, s in zip(chunk, start))
    host, stats = ctx.encode_pngs(imgs)
    for k, (got, exp) in enumerate(zip(host, want)):
        assert got == exp, PD.ALIGN_SIZES[k]
    assert stats["chunks"] == len(imgs)
    dev, _ = ctx.encode_pngs([torch.from_numpy(a).cuda() for a in imgs])
    assert dev == want


# (caller, start at 1, total not n_pixels, size against range): the messages as the library words them
_SET_REFUSALS = (
    ("encode_pngs", "encode_pngs: pix_ptr does not start at 0", "encode_pngs: image 0: width, height and pix_ptr do not agree", "encode_pngs: image 0: width, height and pix_ptr do not agree"),
    ("encode_jpegs", "encode_jpegs: pix_ptr does not start at 0", "encode_jpegs: image 0: width, height and pix_ptr do not agree", "encode_jpegs: image 0: width, height and pix_ptr do not agree"),
    ("save_model", "save_model: atlas_pix_ptr does not run from 0 to n_pixels", "save_model: atlas_pix_ptr does not run from 0 to n_pixels", "save_model: atlas 0: size and atlas_pix_ptr do not agree"),
    ("build_glb", "build_glb: atlas_pix_ptr does not run from 0 to n_pixels", "build_glb: atlas_pix_ptr does not run from 0 to n_pixels", "build_glb: atlas 0: size and atlas_pix_ptr do not agree"),
)


def test_image_set_refusals_per_caller(tmp_path):
    """an atlas_pix_ptr / pix_ptr that starts at 1, one whose total is not n_pixels and a size that disagrees with its range, through both
    encoders and through save_model and build_glb on both device routes: MVS_ERR_INVALID with the caller's own message, then a good call"""
    verts, faces, atlases = PD.tiny_model()
    c = M.Context(0)
    c.set_mesh(verts, faces, np.zeros((1, 3), np.float32))
    img = atlases["image"].reshape(16, 16, 3)
    png, jpg = M.encode_png_rle(img), M.encode_jpeg(img, 90, 1)
    cases = (dict(atlas_pix_ptr=np.array([1, 257], np.uint64)), dict(atlas_pix_ptr=np.array([0, 255], np.uint64)), dict(atlas_size=np.array([15], np.uint32)))
    routes = ((M.default_model_params(png_device=1), png, ".png"), (M.default_model_params(image_format=1), jpg, ".jpg"))
    calls = []                                                       # (message row, call on an atlas set -> the image's bytes)
    image_set = lambda a: {k: a[k] for k in ("atlas_size", "atlas_pix_ptr", "image")}
    calls.append((_SET_REFUSALS[0], lambda a: c.encode_pngs(image_set(a))[0][0], png))
    calls.append((_SET_REFUSALS[1], lambda a: c.encode_jpegs(image_set(a))[0][0], jpg))
    for p, want, ext in routes:
        def save(a, p=p, ext=ext):
            c.save_model(a, str(tmp_path / "m"), params=p)
            return open(str(tmp_path / ("m_material0000_map_Kd" + ext)), "rb").read()
        calls.append((_SET_REFUSALS[2], save, want))
        calls.append((_SET_REFUSALS[3], lambda a, p=p: c.build_glb(a, params=p)[0], want))
    for row, call, want in calls:
        for bad, message in zip(cases, row[1:]):
            with pytest.raises(M.MvsError) as e:
                call(dict(atlases, **bad))
            assert e.value.status == 1, (row[0], bad)                  # MVS_ERR_INVALID
            assert str(e.value) == message + " (status 1)", (row[0], bad)
            good = call(atlases)
            assert good == want or (row[0] == "build_glb" and good.count(want) == 1), (row[0], bad)
    c.close()


def _pngs_of(d):
    return {n: open(os.path.join(d, n), "rb").read() for n in sorted(os.listdir(d)) if n.endswith(".png")}


def test_models_with_device_pngs(tmp_path):
    """the textured model and the debug model of the tiny scene: the text byte for byte, the same files, the same pixels, fewer bytes"""
    import obj_model as OM
    s = get_scene("tiny")
    labels = _library_labels("tiny", s)
    normals = M.vertex_normals(s.verts, s.faces)
    os.makedirs(tmp_path / "a"); os.makedirs(tmp_path / "b")
    st_a = M.texture_model(s, labels, str(tmp_path / "a" / "t"), normals, view_selection_model=True)
    st_b = M.texture_model(s, labels, str(tmp_path / "b" / "t"), normals, params=M.default_model_params(png_device=1), view_selection_model=True)
    assert st_b["ms_png"] > 0 and st_a["bytes"] == st_b["bytes"]
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b")) and "t_view_selection.obj" in names
    for n in names:
        if not n.endswith(".png"):
            assert open(tmp_path / "a" / n, "rb").read() == open(tmp_path / "b" / n, "rb").read(), n
    stored, packed = _pngs_of(tmp_path / "a"), _pngs_of(tmp_path / "b")
    for kind in ("t_material", "t_view_selection_material"):
        mine = [n for n in stored if n.startswith(kind)]
        assert mine
        for n in mine:
            want, _ = OM.decode_png(stored[n])
            got, _, _ = PD.decode(packed[n])
            assert np.array_equal(got, want), n
            assert packed[n] == M.encode_png_rle(want), n
        assert sum(len(packed[n]) for n in mine) < sum(len(stored[n]) for n in mine), kind


def test_refusals_each_followed_by_a_good_call(tmp_path):
    verts, faces, atlases = PD.tiny_model()
    c = M.Context(0)
    c.set_mesh(verts, faces, np.zeros((1, 3), np.float32))
    good = lambda: c.save_model(atlases, str(tmp_path / "g"), params=M.default_model_params(png_device=1))
    want = M.encode_png_rle(atlases["image"].reshape(16, 16, 3))
    for bad in (dict(png_device=1, png_level=6), dict(png_device=2), dict(png_device=-1)):
        with pytest.raises(M.MvsError) as e:
            c.save_model(atlases, str(tmp_path / "bad"), params=M.default_model_params(**bad))
        assert e.value.status == 1, bad                       # MVS_ERR_INVALID
        assert not os.path.exists(str(tmp_path / "bad_material0000_map_Kd.png"))
        good()
        assert open(str(tmp_path / "g_material0000_map_Kd.png"), "rb").read() == want
    # a null image with pixels
    L = M.load_library()
    w = np.array([4], np.uint32); pix = np.array([0, 16], np.uint64)
    res, st = M.viewsel.PngSet(), M.viewsel.PngStats()
    rc = L.mvs_ctx_encode_pngs(c.h, 1, w.ctypes.data, w.ctypes.data, pix.ctypes.data, None, 0, C.byref(res), C.byref(st))
    assert rc == 1 and not res.data
    for w_, h_, pix_ in ((0, 4, 0), (4, 4, 15)):              # an empty frame; sizes that do not agree
        with pytest.raises(M.MvsError):
            L2 = np.array([w_], np.uint32), np.array([h_], np.uint32), np.array([0, pix_], np.uint64)
            rc = L.mvs_ctx_encode_pngs(c.h, 1, L2[0].ctypes.data, L2[1].ctypes.data, L2[2].ctypes.data, np.zeros(64, np.uint8).ctypes.data, 0, C.byref(res), C.byref(st))
            M.viewsel._check(L, rc)
    pngs, _ = c.encode_pngs([atlases["image"].reshape(16, 16, 3)])
    assert pngs == [want]
    c.close()


_CHILD = r"""
import os, sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {tools!r})
import numpy as np
import mvs_texturing_amd as M
import png_decode as PD
def opened():          # the loader logs every dlopen of an object, loaded before or not: "opening file=<path> [0]; direct_opencount=<n>"
    return sum(1 for ln in open("%s.%d" % (os.environ["LD_DEBUG_OUTPUT"], os.getpid()), errors="replace") if "opening file=" in ln and "libz.so" in ln)
verts, faces, atlases = PD.tiny_model()
c = M.Context(0)
c.set_mesh(verts, faces, np.zeros((1, 3), np.float32))
n0 = opened()
c.save_model(atlases, sys.argv[1] + "dev", params=M.default_model_params(png_device=1))
n1 = opened()
try:
    c.save_model(atlases, sys.argv[1] + "host", params=M.default_model_params(png_level=1))
    n2 = opened()
except M.MvsError:     # no libz.so.1 on this machine
    n2 = -1
c.close()
print("opened", n0, n1, n2)
"""


def test_device_pngs_do_not_ask_for_libz(tmp_path):
    """png_device 1 in a process whose product library never resolved libz: in a fresh process under the loader's own log, the call opens
    no libz (and png_level 1 right behind it does, where libz.so.1 exists: the log sees such requests)"""
    env = dict(os.environ, LD_DEBUG="files", LD_DEBUG_OUTPUT=str(tmp_path / "ld"))
    code = _CHILD.format(root=ROOT, tools=os.path.join(ROOT, "tests", "tools"))
    r = subprocess.run([sys.executable, "-c", code, str(tmp_path) + os.sep], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    n0, n1, n2 = [int(x) for x in r.stdout.strip().splitlines()[-1].split()[1:]]
    assert n1 == n0
    assert n2 == -1 or n2 == n1 + 1
    pixels, _, _ = PD.decode(open(str(tmp_path / "dev_material0000_map_Kd.png"), "rb").read())
    assert np.array_equal(pixels, PD.tiny_model()[2]["image"].reshape(16, 16, 3))
