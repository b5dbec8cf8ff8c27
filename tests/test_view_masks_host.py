"""View masks, the host side (no GPU): the ingest convention NAME.mask.png, the host undistortion of a mask against the oracle, and the
conditions the GPU tests of tests/test_gpu_view_masks.py rely on, checked with the oracle and numpy alone."""
import os

import numpy as np
import pytest

import mvs_texturing_amd as M
import oracle_py as O
import util_view_masks as VM
from conftest import get_scene
from mvs_texturing_amd import ingest

LENSES = ((0.9, -0.2, 0.05), (1.3, 0.15, -0.03), (0.8, 0.1, 0.0), (1.1, -0.12, 0.0), (0.5, -0.5, 0.0), (0.5, 0.6, 0.0), (0.6, 0.9, 0.7), (1.0, 0.0, 0.3))


@pytest.fixture()
def folder(tmp_path):
    from PIL import Image
    s = get_scene("tiny")
    d = str(tmp_path / "scene")
    ingest.save_scene_folder(s, d)
    h, w = s.images[0].shape[:2]
    masks = {1: VM.mask_pattern("checker", w, h), 4: VM.mask_pattern("blob_at_black", w, h)}
    Image.fromarray(masks[1]).save(os.path.join(d, "view_0001.mask.png"))                                   # mode L, values 0 / 1 / 7 / 128 / 255
    Image.fromarray(np.repeat(masks[4][:, :, None], 3, axis=2)).save(os.path.join(d, "view_0004.mask.png"))  # mode RGB
    return s, d, masks


def test_mask_files_are_never_views(folder):
    s, d, masks = folder
    pairs = ingest.list_scene_folder(d)
    assert len(pairs) == s.n_views
    assert [os.path.basename(c) for c, _ in pairs] == ["view_%04d.cam" % j for j in range(s.n_views)]
    assert [os.path.basename(i) for _, i in pairs] == ["view_%04d.png" % j for j in range(s.n_views)]       # view_0001.mask.png sorts in front of view_0001.png
    assert sorted(os.listdir(d)).index("view_0001.mask.png") < sorted(os.listdir(d)).index("view_0001.png")


def test_flag_finds_masks_and_default_ignores_them(folder):
    s, d, masks = folder
    r = ingest.load_scene(d)
    assert r.masks is None and all(np.array_equal(a, b) for a, b in zip(r.images, s.images))
    r = ingest.load_scene(d, masks=True)
    assert len(r.masks) == s.n_views and all(np.array_equal(a, b) for a, b in zip(r.images, s.images))
    for j in range(s.n_views):
        if j in masks:
            assert r.masks[j].dtype == np.uint8 and np.array_equal(r.masks[j], np.where(masks[j] != 0, 255, 0))   # non-zero means keep
        else:
            assert r.masks[j] is None
    r = ingest.load_scene(d, masks=True, device_undistort=True)                                              # no distortion here: the same masks
    assert np.array_equal(r.masks[1], np.where(masks[1] != 0, 255, 0)) and r.masks[0] is None


def test_size_mismatch_is_refused_with_the_files_name(folder):
    from PIL import Image
    s, d, masks = folder
    Image.fromarray(np.full((10, 12), 255, np.uint8)).save(os.path.join(d, "view_0002.mask.png"))
    with pytest.raises(ValueError) as e:
        ingest.load_scene(d, masks=True)
    assert "view_0002.mask.png" in str(e.value) and "12 x 10" in str(e.value)
    assert ingest.load_scene(d).masks is None                                                                # without the flag the file is not even opened


@pytest.mark.parametrize("size", [(33, 5), (64, 48), (95, 7)], ids=lambda s: "%dx%d" % s)
def test_host_undistortion_of_a_mask_equals_the_oracle(size):
    """ingest.undistort_mask_host (M.undistort_host on the 0 / 255 replica, kept iff 255) against oracle.undistort on the 3-channel replica,
    thresholded at 255 -- the eight lenses of the lens tests, masks with keep values other than 255"""
    w, h = size
    rng = np.random.default_rng(w * 100 + h)
    for k, lens in enumerate(LENSES):
        keep = VM.mask_pattern(("checker", "interior", "col31", "blob_at_black")[k % 4], w, h)
        keep[rng.random((h, w)) < 0.1] = 0
        got = ingest.undistort_mask_host(keep, *lens)
        want = VM.keep_bits_under_lens(keep, lens)
        assert set(np.unique(got)) <= {0, 255} and np.array_equal(got == 255, want), (size, lens)
        if lens[1] != 0.0:
            assert not np.array_equal(want, keep != 0)                                                       # the lens moved something
        else:
            assert np.array_equal(want, keep != 0)                                                           # dist0 == 0: the mask as it is


def test_small_scene_conditions():
    """what T2 and T3 of tests/test_gpu_view_masks.py need of their scene, from the oracle alone: no zero pixel, painting R black removes
    at least 5 % of the pairs under the area term, and at most 1 % of the gradient-term pairs have a vertex within 1e-3 pixel of an
    integer coordinate"""
    s = VM.small_scene()
    assert all(int(i.sum(axis=2).min()) > 0 for i in s.images)
    full, _ = O.data_costs(s, data_term="area")
    R = VM.corner_regions(s)
    painted = M.synth.Scene(); painted.__dict__.update(s.__dict__)
    painted.images = [np.ascontiguousarray(np.where(r[:, :, None], 0, i).astype(np.uint8)) for i, r in zip(s.images, R)]
    for r in R:
        h, w = r.shape
        assert sum(bool(r[y, x]) for y in (0, h - 1) for x in (0, w - 1)) == 1 and 0.2 < r.mean() < 0.8       # touches exactly one corner, cuts the frame
    cut, _ = O.data_costs(painted, data_term="area")
    assert 0 < cut.nnz <= 0.95 * full.nnz, (cut.nnz, full.nnz)
    # the painted table is what valid_pixel on (not R) leaves of the full one (float64 projections, decided pairs only)
    bits = [VM.expected_products(i, (~r).astype(np.uint8), "area")[0] for i, r in zip(s.images, R)]
    survives, decided = VM.surviving_pairs(s, full, bits)
    face = np.repeat(np.arange(full.n_faces), np.diff(full.col_ptr.astype(np.int64)))
    in_cut = np.zeros(full.nnz, bool)
    keys = set(zip(np.repeat(np.arange(cut.n_faces), np.diff(cut.col_ptr.astype(np.int64))).tolist(), cut.view_id.tolist()))
    in_cut[:] = [(f, v) in keys for f, v in zip(face.tolist(), full.view_id.tolist())]
    assert np.array_equal(in_cut[decided], survives[decided]) and len(keys) == int(in_cut.sum())
    gmi, _ = O.data_costs(s, data_term="gmi")
    blobs = VM.interior_blobs(s)
    gbits = [VM.expected_products(i, b, "gmi")[0] for i, b in zip(s.images, blobs)]
    survives, decided = VM.surviving_pairs(s, gmi, gbits)
    assert (~decided).sum() <= 0.01 * gmi.nnz, ((~decided).sum(), gmi.nnz)
    assert 0.5 * gmi.nnz < survives.sum() < 0.98 * gmi.nnz                                                   # the blobs decide something, and not everything
