"""The face order behind the implicit BVH (csrc/k_kdorder.hip upper levels, csrc/k_bvh.hip refine_order_kernel) is what its kernels say
it is: every aligned node is cut in the middle of its capacity along the longest axis of its centroid box, by rank.  A wrong cut changes
no table and no label -- only the checker of tests/tools/order_model.py (proved non-vacuous on the CPU by tests/test_order_model.py)
sees it.  Only the mesh is loaded; the upper levels are forced on for test-sized meshes (bvh_upper_min_faces = 0).

With option face_order = 0 the order lives in the BVH's triangle slots alone (tri_order) and nothing exports it: that leg is not tested."""
import numpy as np
import pytest

import mvs_texturing_amd as M
import order_model as OM
import util_cases as U
from conftest import get_scene

pytestmark = pytest.mark.gpu

_orders = {}


def _order(key, verts, faces, window):
    """the library's order of the mesh for option bvh_window = window (computed once per (mesh, window), never modified)"""
    if (key, window) not in _orders:
        c = M.Context(0)
        c.set_option("bvh_upper_min_faces", 0); c.set_option("bvh_window", window)
        c.set_mesh(np.ascontiguousarray(verts, dtype=np.float32), np.ascontiguousarray(faces, dtype=np.uint32), np.zeros((len(faces), 3), np.float32))
        perm, _ = c.partition_faces(1)
        c.close()
        perm.setflags(write=False)
        _orders[(key, window)] = perm
    return _orders[(key, window)]


def _checked(key, verts, faces, window):
    """the order, checked: no violation, the node counts the window and the face count imply, the top windows' sets those of the order
    without upper levels"""
    perm = _order(key, verts, faces, window)
    rep = OM.check_order(verts, faces, perm, window)
    assert rep["violations"] == [], rep["violations"][:5]
    want = OM.expected_counts(len(faces), window)
    assert all(rep[k] == v for k, v in want.items()), (rep, want)
    assert OM.check_windows(perm, _order(key, verts, faces, 1), len(faces), window) == []
    return perm, rep


def _mesh(name):
    if name == "spiky32-permuted":
        s = M.synth.permute_scene(get_scene("spiky32"), seed=3)
    else:
        s = get_scene(name)
    return s.verts, s.faces


@pytest.mark.parametrize("name", ["spiky32", "spiky32-permuted"])
def test_whole_mesh_and_windows_of_8192(name):
    """20 480 faces.  bvh_window = 0: top capacity 32 768, four levels above the LDS window (32 768, 16 384, 8192, 4096), the tail node of
    4096 faces not cut at 16 384 nor at 8192.  bvh_window = 8192: three top windows, the last one half full (not cut at 8192), every
    window the same set of faces as in the order without upper levels.  The same mesh with faces and vertices in random order."""
    verts, faces = _mesh(name)
    assert len(faces) == 20480
    plain, rep1 = _checked(name, verts, faces, 1)
    assert rep1["upper_levels"] == 0
    perm, rep = _checked(name, verts, faces, 0)
    assert OM.top_capacity(len(faces), 0) == 32768 and rep["upper_levels"] == 4 and rep["upper_uncut"] == 2 and rep["upper_cut"] == 9
    assert not np.array_equal(perm, plain), "the upper levels did not run"
    perm, rep = _checked(name, verts, faces, 8192)
    assert OM.top_capacity(len(faces), 8192) == 8192 and -(-len(faces) // 8192) == 3 and len(faces) % 8192 == 4096
    assert rep["upper_levels"] == 2 and rep["upper_uncut"] == 1 and rep["upper_cut"] == 7
    assert not np.array_equal(perm, plain), "the upper levels did not run"


def test_plain_icosphere_ties_at_a_pivot():
    """"c1" is full of equal centroid coordinates: some node above the LDS window has keys equal to its pivot on both sides"""
    verts, faces = _mesh("c1")
    _checked("c1", verts, faces, 8192)
    perm, rep = _checked("c1", verts, faces, 0)
    assert rep["upper_ties"] >= 1 and max(rep["tie_caps"]) > OM.LDS_WINDOW


def test_face_count_off_every_tile():
    """18 980 faces: no multiple of the 4096 positions of a block of k_kdorder.hip nor of the 2048 of an LDS window"""
    verts, faces = _mesh("spiky32")
    faces = np.ascontiguousarray(faces[:-1500])
    assert len(faces) % 4096 and len(faces) % 2048
    for window in (0, 8192):
        _checked("spiky32-1500", verts, faces, window)


def test_tie_list_boundary():
    """KD_TIE_CAP = 2048 keys equal to the pivot of the top cut are ranked and placed; with 2049 the upper levels give up and the order is
    REBUILT without them -- exactly the order of bvh_window = 1.  (tests/test_order_model.py: the top cut falls inside the copies.)"""
    verts, faces = U.tie_mesh(2048)
    perm, rep = _checked("tie2048", verts, faces, 0)
    assert 8192 in rep["tie_caps"]
    assert not np.array_equal(perm, _order("tie2048", verts, faces, 1)), "the upper levels did not run"
    verts, faces = U.tie_mesh(2049)
    perm = _order("tie2049", verts, faces, 0)
    plain, _ = _checked("tie2049", verts, faces, 1)
    assert np.array_equal(perm, plain)
