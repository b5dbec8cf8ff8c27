"""Ingest at a pyramid level (ingest.run(..., level=1); DESIGN.md section 4 "View input" item 14): a folder with one distorted JPEG view, one
plain JPEG view, PNG views and two NAME.mask.png files -- one of them on the distorted view -- writes the same .spt and .vec bytes
whatever is left to the device: nothing (Pillow decodes, the host twin undistorts, halves and ANDs the masks), the files (--device-jpeg
--device-png), the lens (--device-undistort), or all three.  The four agree with each other and differ from level 0."""
import os

import numpy as np
import pytest
from PIL import Image

from mvs_texturing_amd import ingest
from conftest import get_scene

pytestmark = pytest.mark.gpu


def test_every_route_writes_the_same_files_at_level_1(tmp_path):
    s = get_scene("tiny")
    folder, mesh = str(tmp_path / "scene"), str(tmp_path / "mesh.ply")
    ingest.save_scene_folder(s, folder, mesh)
    for j in (1, 4):                                       # two baseline JPEG views, view 1 distorted
        os.remove(os.path.join(folder, "view_%04d.png" % j))
        Image.fromarray(s.images[j]).save(os.path.join(folder, "view_%04d.jpg" % j), "JPEG", quality=90, subsampling=2)
    cam = os.path.join(folder, "view_0001.cam")
    lines = open(cam).read().splitlines()
    vals = lines[1].split()
    vals[1], vals[2] = "-0.11", "0.02"
    open(cam, "w").write(lines[0] + "\n" + " ".join(vals) + "\n")
    yy, xx = np.mgrid[0:240, 0:320]
    for j, (cx, cy) in ((1, (150, 121)), (2, (171, 99))):  # a disc left out of the distorted JPEG view and of a PNG view, painted on the photograph
        Image.fromarray(np.where((xx - cx) ** 2 + (yy - cy) ** 2 < 61 ** 2, 0, 255).astype(np.uint8)).save(os.path.join(folder, "view_%04d.mask.png" % j))

    routes = {"host": {}, "files": dict(device_jpeg=True, device_png=True), "lens": dict(device_undistort=True), "all": dict(device_jpeg=True, device_png=True, device_undistort=True)}
    # what is left to the device in each of them
    left = {k: ingest.load_scene(folder, masks=True, level=1, keep_jpeg=kw.get("device_jpeg", False), keep_png=kw.get("device_png", False), device_undistort=kw.get("device_undistort", False)).levels
            for k, kw in routes.items()}
    assert left["host"] == [0] * 8 and left["files"] == [1, 0, 1, 1, 1, 1, 1, 1] and left["lens"] == [0, 1, 0, 0, 0, 0, 0, 0] and left["all"] == [1] * 8
    out = {}
    for k, kw in routes.items():
        prefix = str(tmp_path / k)
        ingest.run(folder, mesh, prefix, masks=True, level=1, **kw)
        out[k] = [open(prefix + ext, "rb").read() for ext in ("_data_costs.spt", "_labeling.vec")]
    for k in routes:
        assert len(out[k][0]) > 16 and out[k] == out["host"], k
    zero, nomask = str(tmp_path / "zero"), str(tmp_path / "nomask")
    ingest.run(folder, mesh, zero, masks=True)
    ingest.run(folder, mesh, nomask, level=1, device_jpeg=True, device_png=True, device_undistort=True)
    assert open(zero + "_data_costs.spt", "rb").read() != out["host"][0]                  # the level decides something, and so do the masks at it
    assert open(nomask + "_data_costs.spt", "rb").read() != out["host"][0]
