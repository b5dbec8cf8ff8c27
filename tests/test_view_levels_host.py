"""Pyramid levels of the view input on the host (DESIGN.md section 4 "View input" item 14; csrc/level.h): the sequential twin M.halve_host
against the numpy restatement tests/tools/view_levels_model.py on the sizes where a clamp, an odd size or a level boundary can go wrong;
the properties that keep the test itself honest (the iterated mean is not the one-shot mean, MVE's float expression is the integer
one); the size law; the keep rule; ingest.load_scene(level=1); and tests/cpp/test_level.cpp -- a stand-alone program with its own main
-- under the address and undefined-behaviour sanitizers.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

import mvs_texturing_amd as M
from mvs_texturing_amd import ingest
import view_levels_model as VL
from conftest import get_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mvs-texturing_amd", "csrc")

EDGES = (15, 16, 17, 31, 32, 33, 63, 64, 65)
SIZES = [(h, w) for h in range(1, 10) for w in range(1, 10)] + [(a, a) for a in EDGES] + [(a, b) for a, b in zip(EDGES, EDGES[::-1]) if a != b] + [(15, 65), (64, 17), (33, 16)]


def image(h, w, seed=0):
    return np.random.default_rng(7919 * h + w + seed).integers(0, 256, (h, w, 3)).astype(np.uint8)


def test_twin_equals_model():
    for h, w in SIZES:
        img = image(h, w)
        for level in range(5):
            out = M.halve_host(img, level)
            ref = VL.halve(img, level)
            assert out.shape == ref.shape == VL.level_size(w, h, level)[::-1] + (3,), (h, w, level)
            assert np.array_equal(out, ref), (h, w, level)
    assert np.array_equal(M.halve_host(image(5, 7), 0), image(5, 7))


BLOCK = np.array([[1, 1, 1, 1], [0, 0, 0, 0], [1, 1, 0, 0], [0, 0, 0, 0]], np.uint8)


def test_rounded_at_every_level():
    img = np.ascontiguousarray(np.repeat(BLOCK[:, :, None], 3, axis=2))
    assert M.halve_host(img, 2).tolist() == [[[1, 1, 1]]] and VL.halve(img, 2).tolist() == [[[1, 1, 1]]]
    assert VL.one_shot(img, 2).tolist() == [[[0, 0, 0]]]


def test_not_the_one_shot_mean():
    img = image(64, 64, seed=5)
    assert np.array_equal(VL.one_shot(img, 1), VL.halve(img, 1))            # one level: the same function
    differ = (VL.one_shot(img, 2) != VL.halve(img, 2)).any(axis=2).mean()
    assert 0.1 < differ < 0.6, differ                                      # about 22 % of the bytes, more of the pixels
    assert 0.15 < (VL.one_shot(img, 2) != VL.halve(img, 2)).mean() < 0.3


def test_float_expression_is_the_integer_one():
    s = np.arange(1021, dtype=np.float32)
    mve = (np.float32(0.25) * s + np.float32(0.5)).astype(np.float32).astype(np.uint8)
    assert np.array_equal(mve, ((np.arange(1021) + 2) >> 2).astype(np.uint8))


def test_level_size_law():
    for w in list(range(1, 40)) + [63, 64, 65, 4000, 4001]:
        for h in (1, 2, 3, 17, 240, 3001):
            assert M.level_size(w, h, 0) == (w, h)
            for k in range(1, 5):
                assert M.level_size(w, h, k) == M.level_size(*M.level_size(w, h, 1), k - 1) == VL.level_size(w, h, k), (w, h, k)
                assert M.level_size(w, h, k) == (-(-w // (1 << k)), -(-h // (1 << k)))
    with pytest.raises(M.MvsError):
        M.level_size(4, 4, 5)
    with pytest.raises(M.MvsError):
        M.halve_host(image(4, 4), 5)


def test_keep_rule():
    """a level pixel is kept iff all that went into it is kept: the level of the 0 / 255 image is 255 exactly there"""
    rng = np.random.default_rng(3)
    for h, w in ((1, 1), (2, 3), (5, 5), (9, 31), (33, 65), (17, 64)):
        for density in (0.02, 0.3):
            mask = np.where(rng.random((h, w)) < density, 0, 255).astype(np.uint8)
            mask[-1, -1] = 0 if density < 0.1 else 255
            for level in range(5):
                keep = VL.keep_level(mask, level)
                via_image = VL.halve(np.repeat(mask[:, :, None], 3, axis=2), level)[:, :, 0] == 255
                assert np.array_equal(keep, via_image), (h, w, level)
                assert np.array_equal(M.halve_mask_host(mask, level), np.where(keep, 255, 0)), (h, w, level)
    # one masked source pixel in the clamped last column / row / corner of an odd size takes exactly its level pixel
    for (y, x) in ((0, 32), (32, 0), (32, 32), (7, 32)):
        mask = np.full((33, 33), 255, np.uint8)
        mask[y, x] = 0
        for level in (1, 2):
            keep = VL.keep_level(mask, level)
            assert (~keep).sum() == 1 and not keep[y >> level, x >> level]


def test_load_scene_level(tmp_path):
    s = get_scene("tiny")
    folder = str(tmp_path / "scene")
    ingest.save_scene_folder(s, folder)
    plain = ingest.load_scene(folder)
    assert plain.levels is None
    for level in (1, 2):
        lv = ingest.load_scene(folder, level=level)
        assert lv.levels == [0] * s.n_views                                   # halved here: nothing is left to the device
        for j, (cam_path, _) in enumerate(ingest.list_scene_folder(folder)):
            h, w = plain.images[j].shape[:2]
            wl, hl = VL.level_size(w, h, level)
            assert (int(lv.cams["width"][j]), int(lv.cams["height"][j])) == (wl, hl) and lv.src_sizes[j] == (wl, hl)
            arr = ingest.camera_arrays(ingest.read_cam_file(cam_path), wl, hl)
            for k in ("pos", "viewdir", "K", "w2c"):
                assert np.array_equal(lv.cams[k][j], arr[k].ravel()), (j, k)
            assert np.array_equal(lv.images[j], VL.halve(plain.images[j], level))
        assert not np.array_equal(lv.cams["K"], plain.cams["K"])
    kept = ingest.load_scene(folder, keep_png=True, level=1)                  # a view that stays a file is left to the device
    assert kept.levels == [1] * s.n_views and all(i is None for i in kept.images)
    assert kept.src_sizes == [(int(plain.cams["width"][j]), int(plain.cams["height"][j])) for j in range(s.n_views)]
    assert all(np.array_equal(kept.cams[k], ingest.load_scene(folder, level=1).cams[k]) for k in kept.cams)


def test_sanitized_program(tmp_path):
    exe = str(tmp_path / "test_level")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + CSRC, os.path.join(ROOT, "tests", "cpp", "test_level.cpp"), "-o", exe])
    cases = [(h, w, level) for (h, w) in ((1, 1), (2, 3), (3, 2), (5, 9), (9, 5), (15, 17), (17, 15), (33, 31), (31, 65)) for level in range(5)]
    with open(str(tmp_path / "manifest"), "w") as m:
        for k, (h, w, level) in enumerate(cases):
            (tmp_path / ("%d.rgb" % k)).write_bytes(image(h, w).tobytes())
            m.write("%d %d %d %d\n" % (k, w, h, level))
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "failures 0" in r.stdout and "images %d" % len(cases) in r.stdout
    for k, (h, w, level) in enumerate(cases):
        assert (tmp_path / ("%d.out" % k)).read_bytes() == VL.halve(image(h, w), level).tobytes(), (h, w, level)
