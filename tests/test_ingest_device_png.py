"""Ingest with the PNG views inflated and unfiltered on the device (ingest.run(..., device_png=True); DESIGN.md section 4 "View input"): a
scene folder of PNG views -- RGB, grey, palette, RGBA -- beside one interlaced PNG and one 16-bit PNG, which Pillow decodes as before,
and two JPEG views, writes the same .spt and .vec bytes as the default route, where Pillow decodes every view; with device_jpeg beside
it one call takes the files of both kinds.  load_scene(keep_png=True) keeps exactly the files png_probe accepts (no GPU)."""
import os

import numpy as np
import pytest
from PIL import Image

import mvs_texturing_amd as M
from mvs_texturing_amd import ingest
from conftest import get_scene


def _folder(tmp_path, with_mesh):
    """the tiny scene's folder with its views re-saved in several formats; returns (folder, mesh, the views png_probe must accept)"""
    s = get_scene("tiny")
    folder, mesh = str(tmp_path / "scene"), str(tmp_path / "mesh.ply")
    ingest.save_scene_folder(s, folder, mesh if with_mesh else None)
    accepted = set(range(s.n_views))
    for j in range(s.n_views):
        png = os.path.join(folder, "view_%04d.png" % j)
        im = Image.fromarray(s.images[j])
        if j == 1:
            im.convert("L").save(png)
        elif j == 2:
            im.quantize(256).save(png, bits=8)
        elif j == 3:
            im.convert("RGBA").save(png)
        elif j == 4:
            Image.fromarray(s.images[j].astype(np.uint16)[:, :, 0] * 257).save(png)   # 16 bit: Pillow decodes it
            accepted.discard(j)
        elif j in (5, 6):
            im.save(os.path.join(folder, "view_%04d.jpg" % j), "JPEG", quality=90, subsampling=2)
            os.remove(png)
            accepted.discard(j)
        elif j == 7:
            im.save(png, optimize=True)
    return s, folder, mesh, accepted


def test_keep_png_keeps_exactly_the_probed_files(tmp_path):
    s, folder, mesh, accepted = _folder(tmp_path, False)
    loaded = ingest.load_scene(folder, keep_png=True)
    assert {j for j, f in enumerate(loaded.png_files) if f is not None} == accepted
    assert all(f is None for f in loaded.jpeg_files)
    assert all((f is None) != (img is None) for f, img in zip(loaded.view_files, loaded.images))
    for j, f in enumerate(loaded.png_files):
        if f is not None:
            assert M.png_probe(f) == (int(loaded.cams["width"][j]), int(loaded.cams["height"][j]))
    plain = ingest.load_scene(folder)
    assert all(img is not None for img in plain.images) and all(f is None for f in plain.png_files)
    assert all(np.array_equal(plain.cams[k], loaded.cams[k]) for k in plain.cams)
    for j in accepted:
        assert np.array_equal(M.decode_png(loaded.png_files[j]), plain.images[j])
    both = ingest.load_scene(folder, keep_png=True, keep_jpeg=True)
    assert {j for j, f in enumerate(both.jpeg_files) if f is not None} == {5, 6} and {j for j, f in enumerate(both.png_files) if f is not None} == accepted
    assert [f is not None for f in both.view_files] == [j != 4 for j in range(s.n_views)]


@pytest.mark.gpu
def test_device_png_writes_the_same_files(tmp_path):
    s, folder, mesh, accepted = _folder(tmp_path, True)
    a, b, c = str(tmp_path / "host"), str(tmp_path / "device"), str(tmp_path / "both")
    ingest.run(folder, mesh, a)
    ingest.run(folder, mesh, b, device_png=True)
    ingest.run(folder, mesh, c, device_png=True, device_jpeg=True)
    for ext in ("_data_costs.spt", "_labeling.vec"):
        x, y, z = open(a + ext, "rb").read(), open(b + ext, "rb").read(), open(c + ext, "rb").read()
        assert len(x) > 16 and x == y and x == z, ext
