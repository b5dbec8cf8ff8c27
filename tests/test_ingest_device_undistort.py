"""Ingest with the distorted views undistorted on the device, on their way in (ingest.run(..., device_jpeg=True, device_undistort=True);
DESIGN.md section 4 "View input"): a scene folder in which a baseline JPEG view and a PNG view carry distortion coefficients writes the
same .spt and .vec bytes as the default route, where Pillow decodes every view and mvs_undistort_image undistorts those two one by one.
load_scene keeps the distorted JPEG as a file and carries its lens; without the flags it returns what it returned before."""
import os

import numpy as np
import pytest
from PIL import Image

import oracle_py as O
from conftest import get_scene
from mvs_texturing_amd import ingest

pytestmark = pytest.mark.gpu

DIST = {1: ("-0.11", "0.02"), 2: ("-0.09", "0")}   # view 1: a baseline JPEG, k2k4; view 2: a PNG, VisualSFM


def test_device_undistort_writes_the_same_files(tmp_path):
    s = get_scene("tiny")
    folder, mesh = str(tmp_path / "scene"), str(tmp_path / "mesh.ply")
    ingest.save_scene_folder(s, folder, mesh)
    for j in (1, 4):                                       # two baseline JPEG views, one of them distorted
        os.remove(os.path.join(folder, "view_%04d.png" % j))
        Image.fromarray(s.images[j]).save(os.path.join(folder, "view_%04d.jpg" % j), "JPEG", quality=90, subsampling=2)
    for j, (d0, d1) in DIST.items():
        cam = os.path.join(folder, "view_%04d.cam" % j)
        lines = open(cam).read().splitlines()
        vals = lines[1].split()
        vals[1], vals[2] = d0, d1
        open(cam, "w").write(lines[0] + "\n" + " ".join(vals) + "\n")
    decoded = [np.asarray(Image.open(os.path.join(folder, "view_%04d.jpg" % j)).convert("RGB")) if j in (1, 4) else s.images[j] for j in range(s.n_views)]
    flen = [ingest.read_cam_file(os.path.join(folder, "view_%04d.cam" % j)).flen for j in range(s.n_views)]

    # without the flags: what load_scene returns today -- every view decoded, the two undistorted, no lens
    plain = ingest.load_scene(folder, mesh)
    assert plain.lens is None and all(f is None for f in plain.jpeg_files)
    for j in range(s.n_views):
        want = O.undistort(decoded[j], flen[j], float(DIST[j][0]), float(DIST[j][1])) if j in DIST else decoded[j]
        assert np.array_equal(plain.images[j], want), j
    assert not np.array_equal(plain.images[1], decoded[1]) and not np.array_equal(plain.images[2], decoded[2])
    # keep_jpeg alone still decodes and undistorts the distorted JPEG here
    kept = ingest.load_scene(folder, mesh, keep_jpeg=True)
    assert kept.lens is None and kept.jpeg_files[1] is None and kept.jpeg_files[4] is not None and np.array_equal(kept.images[1], plain.images[1])
    # device_undistort alone: pixels as the camera took them, with their lens
    raw = ingest.load_scene(folder, mesh, device_undistort=True)
    assert all(f is None for f in raw.jpeg_files) and all(np.array_equal(raw.images[j], decoded[j]) for j in range(s.n_views))
    # both: the distorted JPEG stays a file and carries its lens
    both = ingest.load_scene(folder, mesh, keep_jpeg=True, device_undistort=True)
    assert both.jpeg_files[1] is not None and both.images[1] is None and both.jpeg_files[4] is not None and both.jpeg_files[2] is None
    assert np.array_equal(both.images[2], decoded[2])
    for sc in (raw, both):
        assert sc.lens.shape == (s.n_views, 3) and sc.lens.dtype == np.float32
        for j in range(s.n_views):
            want = (flen[j], np.float32(DIST[j][0]), np.float32(DIST[j][1])) if j in DIST else (flen[j], 0.0, 0.0)
            assert tuple(sc.lens[j]) == tuple(np.float32(v) for v in want), j
        assert all(np.array_equal(sc.cams[k], plain.cams[k]) for k in plain.cams)

    a, b, c = str(tmp_path / "host"), str(tmp_path / "device"), str(tmp_path / "pixels")
    ingest.run(folder, mesh, a)
    ingest.run(folder, mesh, b, device_jpeg=True, device_undistort=True)
    ingest.run(folder, mesh, c, device_undistort=True)
    for ext in ("_data_costs.spt", "_labeling.vec"):
        x, y, z = open(a + ext, "rb").read(), open(b + ext, "rb").read(), open(c + ext, "rb").read()
        assert len(x) > 16 and x == y and x == z, ext
