"""Ingest with the views decoded on the device (ingest.run(..., device_jpeg=True); DESIGN.md section 4 "View input"): a scene folder of
baseline JPEG views -- 4:2:0, 4:4:4 and grayscale -- beside one PNG view and one progressive JPEG view, which Pillow decodes as before,
writes the same .spt and .vec bytes as the default route, where Pillow decodes every view."""
import os

import numpy as np
import pytest
from PIL import Image

import mvs_texturing_amd as M
from mvs_texturing_amd import ingest
from conftest import get_scene

pytestmark = pytest.mark.gpu


def test_device_jpeg_writes_the_same_files(tmp_path):
    s = get_scene("tiny")
    folder, mesh = str(tmp_path / "scene"), str(tmp_path / "mesh.ply")
    ingest.save_scene_folder(s, folder, mesh)
    kept = 0
    for j in range(s.n_views):
        png = os.path.join(folder, "view_%04d.png" % j)
        if j == 2:
            continue                                                       # one PNG view
        im = Image.fromarray(s.images[j])
        kw = dict(quality=90, subsampling=2)
        if j == 4:
            kw = dict(quality=90, progressive=True)                        # not accepted by the device route: Pillow decodes it
        elif j == 5:
            kw = dict(quality=95, subsampling=0, optimize=True)
        elif j == 6:
            im = im.convert("L")
        im.save(os.path.join(folder, "view_%04d.jpg" % j), "JPEG", **kw)
        os.remove(png)
        kept += j != 4
    loaded = ingest.load_scene(folder, mesh, keep_jpeg=True)
    assert sum(f is not None for f in loaded.jpeg_files) == kept and loaded.jpeg_files[2] is None and loaded.jpeg_files[4] is None
    assert all((f is None) != (img is None) for f, img in zip(loaded.jpeg_files, loaded.images))
    plain = ingest.load_scene(folder, mesh)
    assert all(img is not None for img in plain.images) and all(np.array_equal(plain.cams[k], loaded.cams[k]) for k in plain.cams)
    a, b = str(tmp_path / "host"), str(tmp_path / "device")
    ingest.run(folder, mesh, a)
    ingest.run(folder, mesh, b, device_jpeg=True)
    for ext in ("_data_costs.spt", "_labeling.vec"):
        x, y = open(a + ext, "rb").read(), open(b + ext, "rb").read()
        assert len(x) > 16 and x == y, ext
