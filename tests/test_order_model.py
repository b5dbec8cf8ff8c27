"""tests/tools/order_model.py against itself: the checker of the library's face order accepts an order built by the same rules in numpy
and rejects that order with one fault in it -- the proof that the property check of tests/test_gpu_face_order.py is not vacuous."""
import numpy as np
import pytest

import order_model as OM
import util_cases as U
from conftest import get_scene


@pytest.fixture(scope="module")
def mesh():
    s = get_scene("spiky32")
    return s.verts, s.faces


@pytest.fixture(scope="module")
def ref0(mesh):
    """the reference order of the whole mesh cut top-down (bvh_window = 0), never modified"""
    r = OM.reference_order(mesh[0], mesh[1], 0)
    r.setflags(write=False)
    return r


def _node(mesh, order, cap, start):
    """(keys, half) of the node of capacity cap at `start` of `order`"""
    n = min(cap, len(order) - start)
    keys, _ = OM.node_keys(OM.centroids(mesh[0], mesh[1])[order[start:start + n].astype(np.int64)], cap)
    return keys, cap // 2


def _swapped_across(mesh, order, cap, start):
    """`order` with the lower half's smallest and the upper half's largest key of one node exchanged"""
    keys, half = _node(mesh, order, cap, start)
    a, b = int(np.argmin(keys[:half])), half + int(np.argmax(keys[half:]))
    assert keys[a] < keys[b]
    out = order.copy()
    out[[start + a, start + b]] = out[[start + b, start + a]]
    return out


def test_counts_and_capacities():
    """kd_refine_order's top capacity, and what the checker counts, for the sizes the GPU tests use"""
    assert OM.top_capacity(20480, 0) == 32768 and OM.top_capacity(20480, 8192) == 8192 and OM.top_capacity(20480, 262144) == 32768
    assert OM.top_capacity(20480, 1) == 2048 and OM.top_capacity(2048, 0) == 2048 and OM.top_capacity(8192, 0) == 8192
    e = OM.expected_counts(20480, 0)
    # capacities 32 768 (the whole mesh: cut), 16 384 (4096 faces in the second node: not cut), 8192 (the third: not cut), 4096 (five full nodes)
    assert (e["upper_levels"], e["upper_cut"], e["upper_uncut"]) == (4, 1 + 1 + 2 + 5, 0 + 1 + 1 + 0) and e["levels"] == 4 + 7
    e = OM.expected_counts(20480, 8192)
    assert (e["upper_levels"], e["upper_cut"], e["upper_uncut"]) == (2, 2 + 5, 1 + 0)      # three top windows, the last one half full
    e = OM.expected_counts(20480 - 1500, 0)
    assert e["uncut"] > e["upper_uncut"] > 0                                              # a partial last LDS window: uncut nodes inside it


@pytest.mark.parametrize("window", [0, 8192, 1])
def test_checker_accepts_the_reference_order(mesh, window):
    verts, faces = mesh
    order = OM.reference_order(verts, faces, window)
    rep = OM.check_order(verts, faces, order, window)
    assert rep["violations"] == []
    e = OM.expected_counts(len(faces), window)
    assert all(rep[k] == e[k] for k in e), (rep, e)
    assert OM.check_windows(order, OM.reference_order(verts, faces, 1), len(faces), window) == []
    # an odd face count: partial nodes at every level
    cut = faces[:-1500]
    order = OM.reference_order(verts, cut, window)
    rep = OM.check_order(verts, cut, order, window)
    assert rep["violations"] == [] and all(rep[k] == v for k, v in OM.expected_counts(len(cut), window).items())
    assert OM.check_order(verts, cut, order[:-1], window)["violations"] == ["not a permutation of the faces"]


@pytest.mark.parametrize("cap,start", [(32768, 0), (4096, 8192), (512, 16384 + 512)], ids=["top-cut", "cap-4096", "lds-window"])
def test_checker_rejects_a_swap_across_a_cut(mesh, ref0, cap, start):
    bad = _swapped_across(mesh, ref0, cap, start)
    rep = OM.check_order(mesh[0], mesh[1], bad, 0)
    assert any("capacity %d" % cap in v and "[%d," % start in v for v in rep["violations"]), rep["violations"]


@pytest.mark.parametrize("cap,start", [(32768, 0), (4096, 4096), (256, 2048)], ids=["top", "cap-4096", "lds-window"])
def test_checker_rejects_the_second_longest_axis(mesh, cap, start):
    bad = OM.reference_order(mesh[0], mesh[1], 0, axis_override=(cap, start))
    rep = OM.check_order(mesh[0], mesh[1], bad, 0)
    assert any("capacity %d" % cap in v and "[%d," % start in v for v in rep["violations"]), rep["violations"]


@pytest.mark.parametrize("cap,start", [(32768, 0), (16384, 0), (4096, 12288)], ids=["top", "cap-16384", "cap-4096"])
def test_checker_rejects_a_pivot_off_by_one_rank(mesh, ref0, cap, start):
    """only where the two ranks at the cut have different keys is there anything to reject"""
    keys, half = _node(mesh, ref0, cap, start)
    assert np.sort(keys)[half - 1] < np.sort(keys)[half]
    bad = OM.reference_order(mesh[0], mesh[1], 0, rank_shift=(cap, start))
    rep = OM.check_order(mesh[0], mesh[1], bad, 0)
    assert len(rep["violations"]) >= 1 and "capacity %d" % cap in rep["violations"][0] and "1 keys" in rep["violations"][0], rep["violations"]


def test_checker_rejects_exchanged_windows(mesh):
    """two windows exchanged whole: every cut inside them still holds, only the window sets say that the upper levels moved faces
    out of their window"""
    verts, faces = mesh
    F = len(faces)
    plain = OM.reference_order(verts, faces, 1)
    order = OM.reference_order(verts, faces, 8192)
    assert OM.check_windows(order, plain, F, 8192) == []
    bad = order.copy(); bad[:8192] = order[8192:16384]; bad[8192:16384] = order[:8192]
    assert OM.check_order(verts, faces, bad, 8192)["violations"] == []
    v = OM.check_windows(bad, plain, F, 8192)
    assert len(v) == 2 and "[0, 8192)" in v[0] and "[8192, 16384)" in v[1]
    bad = order.copy(); bad[[100, 9000]] = bad[[9000, 100]]                                  # one face in the wrong window
    assert len(OM.check_windows(bad, plain, F, 8192)) == 2


def test_ties_are_counted_and_negative_zero_sorts_below_zero():
    """the plain icosphere is full of equal centroid coordinates: some node above the LDS window has a tie at its pivot; -0.0 < +0.0
    in the upper levels' keys (kd_f2ord)"""
    s = get_scene("c1")
    order = OM.reference_order(s.verts, s.faces, 0)
    rep = OM.check_order(s.verts, s.faces, order, 0)
    assert rep["violations"] == [] and rep["upper_ties"] >= 1 and max(rep["tie_caps"]) > OM.LDS_WINDOW
    k = OM.f2ord(np.float32([-1.0, -0.0, 0.0, 1e-45, 1.0]))
    assert (np.diff(k.astype(np.int64)) > 0).all()


@pytest.mark.parametrize("m", [2048, 2049])
def test_tie_mesh_has_its_top_cut_inside_the_copies(m):
    """util_cases.tie_mesh: x is the longest extent, the ranks on either side of the top cut both hold the copies' key, exactly m keys
    equal it (KD_TIE_CAP of csrc/k_kdorder.hip is 2048), and the reference order has a tie at the top node"""
    verts, faces = U.tie_mesh(m)
    assert len(faces) == 8192 and OM.top_capacity(8192, 0) == 8192
    c = OM.centroids(verts, faces)
    ax, _, _ = OM.node_axis(c)
    keys = np.sort(OM.f2ord(c[:, 0]))
    zero = OM.f2ord(np.float32([0.0]))[0]
    assert ax == 0 and keys[4095] == keys[4096] == zero and int((keys == zero).sum()) == m and int((keys < zero).sum()) == 3072
    rep = OM.check_order(verts, faces, OM.reference_order(verts, faces, 0), 0)
    assert rep["violations"] == [] and 8192 in rep["tie_caps"]
