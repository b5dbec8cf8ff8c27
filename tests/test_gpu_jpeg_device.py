"""The JPEG route of rows f9 and f11 on the GPU (DESIGN.md section 4 "Model output" item 9; csrc/k_jpeg.hip): Context.encode_jpegs gives,
byte for byte, what the host twin of csrc/jpeg_base.h gives (tests/test_jpeg_host.py holds the twin to a strict parser, a numpy statement
of the transform and Pillow) on the crafted images of tests/tools/jpeg_decode.py -- sides around the MCU sizes, MCU counts around the
restart interval, segments that straddle MCU rows, more than 16 segments, ZRL and EOB-only blocks, full-amplitude and heavily stuffed
data -- in one call for all images, from host arrays, from device tensors at an odd address in reversed order, twice, and as an atlas set;
the stats agree with the parser's counts; models saved with image_format 1 have the default route's .obj, its .mtl but for the extension
and the twin's JPEG of the default route's pixels; the .glb embeds those bytes as image/jpeg; the default route is unchanged around it;
every refusal is followed by a good call.

The .glb goes through the strict parser of tests/tools/glb_model.py, which knows PNG images only: the test hands it the JSON with every
image's "image/jpeg" -- asserted first -- rewritten to the type it expects, and the JPEG signature in place of the PNG one, so that all its
structural checks run on the file as it is."""
import ctypes as C
import json
import os
import types

import numpy as np
import pytest

import mvs_texturing_amd as M
import jpeg_decode as JD
import png_decode as PD
from conftest import get_scene
from test_gpu_debug_model import _library_labels

pytestmark = pytest.mark.gpu

IMAGES = JD.images()
NAMES = sorted(IMAGES)
MODES = ((90, 1), (90, 0), (100, 0), (1, 1), (50, 1))


@pytest.fixture(scope="module")
def ctx():
    c = M.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def twin():
    return {(n, q, s): M.encode_jpeg(IMAGES[n], q, s) for n in NAMES for q, s in MODES}


def _check(files, stats, names, q, s, twin):
    seg = stuffed = marker = 0
    for name, f in zip(names, files):
        assert f == twin[(name, q, s)], (name, q, s)
        P = JD.parse(f)
        seg += P["segments"]; stuffed += P["stuffed_bytes"]; marker += P["marker_bytes"]
    assert stats["segments"] == seg and stats["stuffed_bytes"] == stuffed and stats["marker_bytes"] == marker
    assert stats["jpeg_bytes"] == sum(len(f) for f in files)
    assert stats["raw_bytes"] == sum(3 * IMAGES[k].shape[0] * IMAGES[k].shape[1] for k in names)


@pytest.mark.parametrize("quality,sub", MODES)
def test_encode_jpegs_all_images_in_one_call(ctx, twin, quality, sub):
    import torch
    files, stats = ctx.encode_jpegs([IMAGES[k] for k in NAMES], quality, sub)
    _check(files, stats, NAMES, quality, sub, twin)
    again, stats2 = ctx.encode_jpegs([IMAGES[k] for k in NAMES], quality, sub)
    assert again == files and all(stats2[k] == stats[k] for k in M.viewsel.JPEG_COUNTS)
    rev = list(reversed(NAMES))
    flat = torch.frombuffer(bytearray(b"\x00" + b"".join(IMAGES[k].tobytes() for k in rev)), dtype=torch.uint8).cuda()[1:]      # an odd device address
    tensors, at = [], 0
    for k in rev:
        n = IMAGES[k].size
        tensors.append(flat[at:at + n].reshape(IMAGES[k].shape)); at += n
    assert tensors[0].data_ptr() % 2 == 1
    dev, stats3 = ctx.encode_jpegs(tensors, quality, sub)
    _check(dev, stats3, rev, quality, sub, twin)
    one, _ = ctx.encode_jpegs([tensors[3]], quality, sub)          # a lone image that starts in the middle of the allocation
    assert one == [twin[(rev[3], quality, sub)]]
    assert ctx.encode_jpegs([], quality, sub)[0] == []


def test_encode_jpegs_of_an_atlas_set(ctx, twin):
    """square images as the atlas-set dict save_model reads, on the host and on the device"""
    import torch
    names = ["photo_256", "side_17", "side_1", "checker_grey"]
    size = np.array([IMAGES[k].shape[0] for k in names], np.uint32)
    pix = np.concatenate([[0], np.cumsum(size.astype(np.uint64) ** 2)]).astype(np.uint64)
    image = np.concatenate([IMAGES[k].reshape(-1, 3) for k in names])
    host, _ = ctx.encode_jpegs(dict(atlas_size=size, atlas_pix_ptr=pix, image=image))
    assert host == [twin[(k, 90, 1)] for k in names]
    dev, _ = ctx.encode_jpegs(dict(atlas_size=torch.from_numpy(size.astype(np.int32)).cuda(), atlas_pix_ptr=torch.from_numpy(pix.astype(np.int64)).cuda(),
                                   image=torch.from_numpy(image).cuda()), quality=90, subsampling=1)
    assert dev == host


def test_gather_at_every_alignment(ctx):
    """PD.alignment_images() in one call, from host arrays and from device tensors.  At 4:2:0 every image is one segment (at most 3 x 2
    MCUs), which lands behind the entropy data of the images in front of it: a file without its header and EOI.  The sizes, not luck,
    spread those destinations over the residues modulo 16 and make segments shorter than their way to the next boundary; at 4:4:4 the
    larger images have two segments."""
    import torch
    imgs = PD.alignment_images()
    want = [M.encode_jpeg(a, 90, 1) for a in imgs]
    seg = np.array([len(f) - JD.HEADER_BYTES - 2 for f in want])
    start = np.concatenate([[0], np.cumsum(seg)[:-1]])
    assert len(set(int(x) % 16 for x in start)) >= 12
    assert any(n < (-s) % 16 for n, s in zip(seg, start))
    host, stats = ctx.encode_jpegs(imgs, 90, 1)
    for k, (got, exp) in enumerate(zip(host, want)):
        assert got == exp, PD.ALIGN_SIZES[k]
    assert stats["segments"] == len(imgs)
    dev, _ = ctx.encode_jpegs([torch.from_numpy(a).cuda() for a in imgs], 90, 1)
    assert dev == want
    assert ctx.encode_jpegs(imgs, 90, 0)[0] == [M.encode_jpeg(a, 90, 0) for a in imgs]


def _files(d):
    return {n: open(os.path.join(d, n), "rb").read() for n in sorted(os.listdir(d))}


def _parse_jpeg_glb(monkeypatch, data):
    import glb_model as GM
    seen = []

    def loads(text):
        j = json.loads(text)
        for im in j.get("images", []):
            seen.append(im["mimeType"])
            assert im["mimeType"] == "image/jpeg"
            im["mimeType"] = "image/png"
        return j
    with monkeypatch.context() as m:
        m.setattr(GM, "json", types.SimpleNamespace(loads=loads))
        m.setattr(GM, "PNG_SIG", b"\xff\xd8\xff\xe0\x00\x10JFIF\x00")
        got = GM.parse_glb(data)
    assert seen and len(seen) == len(got["images"])
    return got


def test_models_with_jpeg_images(tmp_path, monkeypatch):
    """the textured model and the debug model of the tiny scene, as OBJ and as .glb, with the default route before and after"""
    import glb_model as GM
    import obj_model as OM
    s = get_scene("tiny")
    labels = _library_labels("tiny", s)
    normals = M.vertex_normals(s.verts, s.faces)
    for d in "abcd":
        os.makedirs(tmp_path / d)
    jp = M.default_model_params(image_format="jpeg")
    assert (jp.image_format, jp.jpeg_quality, jp.jpeg_subsampling) == (1, 90, 1) and M.default_model_params().image_format == 0
    M.texture_model(s, labels, str(tmp_path / "a" / "t"), normals, view_selection_model=True, format="both")
    st_b, glb_b = M.texture_model(s, labels, str(tmp_path / "b" / "t"), normals, params=jp, view_selection_model=True, format="both")
    M.texture_model(s, labels, str(tmp_path / "c" / "t"), normals, view_selection_model=True, format="both")
    M.texture_model(s, labels, str(tmp_path / "d" / "t"), normals, params=M.default_model_params(image_format=1, jpeg_quality=60, jpeg_subsampling=0), format="glb")
    a, b, c = _files(tmp_path / "a"), _files(tmp_path / "b"), _files(tmp_path / "c")
    assert a == c                                                       # the default route before and after: byte for byte
    assert st_b["ms_png"] > 0 and glb_b["ms_png"] > 0
    assert sorted(b) == sorted(n[:-4] + ".jpg" if n.endswith(".png") else n for n in a) and not any(n.endswith(".png") for n in b)
    for n in ("t.obj", "t_view_selection.obj"):
        assert a[n] == b[n], n
    for n in ("t.mtl", "t_view_selection.mtl"):
        assert b"_map_Kd.png\n" in a[n] and a[n].replace(b"_map_Kd.png\n", b"_map_Kd.jpg\n") == b[n], n
    jpgs = []
    for kind in ("t_material", "t_view_selection_material"):
        mine = [n for n in a if n.startswith(kind)]
        assert mine
        for n in mine:
            pixels, _ = OM.decode_png(a[n])
            j = b[n[:-4] + ".jpg"]
            assert j == M.encode_jpeg(pixels, 90, 1), n
            assert JD.parse(j)["width"] == pixels.shape[1]
            if kind == "t_material":
                jpgs.append((pixels, j))
    got = _parse_jpeg_glb(monkeypatch, b["t.glb"])
    assert got["images"] == [j for _, j in jpgs]
    want = GM.parse_glb(a["t.glb"])                                      # the same geometry as the default file
    assert len(got["primitives"]) == len(want["primitives"])
    for p, q in zip(got["primitives"], want["primitives"]):
        assert all(np.array_equal(p[k], q[k]) for k in q)
    d = _files(tmp_path / "d")
    assert sorted(d) == ["t.glb"]
    assert _parse_jpeg_glb(monkeypatch, d["t.glb"])["images"] == [M.encode_jpeg(pixels, 60, 0) for pixels, _ in jpgs]


def test_refusals_each_followed_by_a_good_call(tmp_path):
    verts, faces, atlases = PD.tiny_model()
    c = M.Context(0)
    c.set_mesh(verts, faces, np.zeros((1, 3), np.float32))
    img = atlases["image"].reshape(16, 16, 3)
    want, want_png = M.encode_jpeg(img, 90, 1), None

    def good():
        c.save_model(atlases, str(tmp_path / "g"), params=M.default_model_params(image_format="jpeg"))
        assert open(str(tmp_path / "g_material0000_map_Kd.jpg"), "rb").read() == want
        assert c.build_glb(atlases, params=M.default_model_params(image_format=1))[0].count(want) == 1
        c.save_model(atlases, str(tmp_path / "p"))
        return open(str(tmp_path / "p_material0000_map_Kd.png"), "rb").read()
    want_png = good()
    for bad in (dict(image_format=1, png_level=6), dict(image_format=1, png_device=1), dict(image_format=1, jpeg_quality=0), dict(image_format=1, jpeg_quality=101),
                dict(image_format=1, jpeg_subsampling=2), dict(image_format=1, jpeg_subsampling=-1), dict(image_format=2), dict(image_format=-1)):
        for call in (lambda p: c.save_model(atlases, str(tmp_path / "bad"), params=p), lambda p: c.build_glb(atlases, params=p),
                     lambda p: c.save_glb(atlases, str(tmp_path / "bad.glb"), params=p)):
            with pytest.raises(M.MvsError) as e:
                call(M.default_model_params(**bad))
            assert e.value.status == 1, bad                       # MVS_ERR_INVALID
        assert not any(n.startswith("bad_material") or n == "bad.glb" for n in os.listdir(tmp_path)), bad
        assert good() == want_png
    with pytest.raises(ValueError):
        M.default_model_params(image_format="tiff")
    # with image_format 0 the JPEG words are not read
    c.save_model(atlases, str(tmp_path / "z"), params=M.default_model_params(jpeg_quality=-5, jpeg_subsampling=9))
    assert open(str(tmp_path / "z_material0000_map_Kd.png"), "rb").read() == want_png
    for q, s_ in ((0, 1), (101, 0), (90, 2)):
        with pytest.raises(M.MvsError) as e:
            c.encode_jpegs([img], q, s_)
        assert e.value.status == 1
        assert c.encode_jpegs([img])[0] == [want]
    # a side above 65535: the format's limit
    with pytest.raises(M.MvsError) as e:
        c.encode_jpegs([np.zeros((1, 65536, 3), np.uint8)])
    assert e.value.status == 7                                    # MVS_ERR_UNSUPPORTED
    wide, _ = c.encode_jpegs([np.zeros((1, 65535, 3), np.uint8)], 90, 0)
    assert wide == [M.encode_jpeg(np.zeros((1, 65535, 3), np.uint8), 90, 0)]
    # a null image with pixels; an empty frame; sizes that do not agree
    L = M.load_library()
    res, st = M.viewsel.PngSet(), M.viewsel.JpegStats()
    w = np.array([4], np.uint32); pix = np.array([0, 16], np.uint64)
    assert L.mvs_ctx_encode_jpegs(c.h, 1, w.ctypes.data, w.ctypes.data, pix.ctypes.data, None, 0, 90, 1, C.byref(res), C.byref(st)) == 1 and not res.data
    for w_, h_, pix_ in ((0, 4, 0), (4, 4, 15)):
        a3 = np.array([w_], np.uint32), np.array([h_], np.uint32), np.array([0, pix_], np.uint64)
        assert L.mvs_ctx_encode_jpegs(c.h, 1, a3[0].ctypes.data, a3[1].ctypes.data, a3[2].ctypes.data, np.zeros(64, np.uint8).ctypes.data, 0, 90, 1, C.byref(res), C.byref(st)) == 1
    assert c.encode_jpegs([img])[0] == [want]
    c.close()
