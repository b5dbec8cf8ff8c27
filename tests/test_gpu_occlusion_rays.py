"""The occlusion rays (csrc/k_bvh.hip) bit by bit (run with -m gpu on an MI355X): on crafted scenes (tests/util_cases.py ray_*) the need bits
and the occluded bits that ray_packet3_kernel leaves behind are read back (mvs_ctx_ray_bits, building-blocks library) and EVERY (view, vertex)
bit is compared with the oracle's brute-force loop over all triangles for that one ray.  A wrong bit that the cost table would hide -- the
face was occluded through another vertex anyway -- fails here.  The oracle side of every scene (BVH == brute force, something occluded,
something not, the designed rays needed) runs in tests/test_oracle.py.  Every comparison is boolean or bit-exact."""
import numpy as np
import pytest

import mvs_texturing_amd as M
import oracle_py as O
import util_cases as U

pytestmark = pytest.mark.gpu
MVS_ERR_STATE = 6      # include/mvs_viewsel.h
CULLS = ("cull_backface", "cull_angle", "cull_outside", "cull_occluded", "cull_zero_quality", "nnz_pre")
SCENES = U.ray_scenes()
_REF = {}


def _reference(name):
    """(scene, table, stats, need, occl) of a crafted scene, computed once: need[j, v] = some face on v passed the culls in front of the
    rays (the oracle's pattern WITHOUT the visibility test is exactly the pass set: no zero-quality pairs in these scenes), occl[j, v] =
    the brute-force answer for the ray from vertex v to camera j wherever need is set"""
    if name not in _REF:
        s = SCENES[name]()
        ref, rst = O.data_costs(s)
        nv, sn = O.data_costs(s, geometric_visibility_test=False)
        assert rst["cull_zero_quality"] == 0 and sn["cull_zero_quality"] == 0 and rst["cull_occluded"] > 0 and ref.nnz > 0
        need = U.need_from_pass_pattern(s, nv.col_ptr, nv.view_id)
        _REF[name] = (s, ref, rst, need, U.ray_truth(s, need))
    return _REF[name]


def _run(s, **options):
    """one data-cost pass with default settings in a fresh context: (stats, table, need, occl, vertex order)"""
    c = M.Context(0)
    try:
        c.set_option("stats", 1)
        for k, v in options.items():
            c.set_option(k, v)
        c.set_mesh(s.verts, s.faces, s.normals); c.set_views(s.cams, s.images)
        st = c.data_costs(M.Settings())
        got = c.costs_download()
        need, occl = c.ray_bits()
        return st, got, need, occl, c.ray_vertex_order()
    finally:
        c.close()


def _assert_bits(need, occl, need_ref, occl_ref):
    bad = np.argwhere(need != need_ref)
    assert len(bad) == 0, "%d wrong need bits; (view, vertex) %s" % (len(bad), bad[:8].tolist())
    assert not (occl & ~need).any(), "occluded bits where no ray was needed: %s" % np.argwhere(occl & ~need)[:8].tolist()
    bad = np.argwhere(occl != occl_ref)
    assert len(bad) == 0, "%d wrong ray bits of %d rays; (view, vertex, got) %s" % (len(bad), need.sum(), [(j, v, bool(occl[j, v])) for j, v in bad[:8].tolist()])


def _packets(need, order):
    """non-empty 64-vertex words of the need matrix in the library's vertex order = packets the ray kernel traverses"""
    n = need[:, order]
    n = np.concatenate([n, np.zeros((n.shape[0], -n.shape[1] % 64), bool)], axis=1)
    return int(n.reshape(n.shape[0], -1, 64).any(axis=2).sum())


@pytest.mark.parametrize("name", list(SCENES))
def test_every_ray_bit_equals_the_brute_force_answer(name):
    """bits, table, counters and the paths taken, default settings"""
    s, ref, rst, need_ref, occl_ref = _reference(name)
    st, got, need, occl, order = _run(s)
    assert sorted(order.tolist()) == list(range(len(s.verts)))
    _assert_bits(need, occl, need_ref, occl_ref)
    assert st["rays"] == need.sum() and st["ray_packets"] == _packets(need, order)
    assert np.array_equal(got.col_ptr, ref.col_ptr), "sparsity pattern differs"
    assert np.array_equal(got.view_id, ref.view_id)
    assert np.array_equal(got.quality.view(np.uint32), ref.quality.view(np.uint32)) and np.array_equal(got.cost.view(np.uint32), ref.cost.view(np.uint32))
    for k in CULLS:
        assert st[k] == rst[k], k
    if name.startswith("terrace"):
        assert st["ray_packets_generic"] > 0          # directions with a zero component: the slab test that has to survive inf and NaN
    if name == "octants":
        # no packet took the generic slab test, and every view has packets: the eight views ran the eight sign-specialised instances
        assert st["ray_packets_generic"] == 0 and all(_packets(need[j:j + 1], order) > 0 for j in range(8))


@pytest.mark.parametrize("name", ["terrace", "confetti", "strip257"])
def test_options_that_must_not_change_a_bit(name):
    """block order over the XCDs, the counting instantiation, the caller's face numbering as the internal order: identical bit matrices;
    the counters of the counting build are consistent, and in the confetti scene candidate lists longer than one round occurred"""
    s, ref, rst, need_ref, occl_ref = _reference(name)
    for options in (dict(ray_xcd=0), dict(count_rays=1), dict(face_order=0)):
        st, got, need, occl, order = _run(s, **options)
        _assert_bits(need, occl, need_ref, occl_ref)
        assert np.array_equal(got.col_ptr, ref.col_ptr) and np.array_equal(got.cost.view(np.uint32), ref.cost.view(np.uint32))
        assert st["rays"] == need.sum() and st["cull_occluded"] == rst["cull_occluded"]
        if "count_rays" in options:
            assert st["ray_nodes"] >= st["ray_packets"] and st["ray_tris"] % 16 == 0 and st["ray_leaf_rounds"] * 16 >= st["ray_tris"] > 0, st
            if name == "confetti":
                assert st["ray_leaf_rounds"] > st["ray_tris"] // 16, st       # a leaf visit with more than four candidate rays
        else:
            assert st["ray_nodes"] == 0 and st["ray_tris"] == 0


@pytest.mark.parametrize("name", ["confetti", "terrace"])
def test_bits_do_not_depend_on_the_numbering(name):
    """faces and vertices in random order: the bits, mapped back to the original vertex ids, are those of the scene as built"""
    s, ref, rst, need_ref, occl_ref = _reference(name)
    _, _, need0, occl0, _ = _run(s)
    p = M.synth.permute_scene(s, seed=5)
    st, got, need, occl, _ = _run(p)
    back = np.empty(len(s.verts), np.int64); back[p.vert_perm] = np.arange(len(s.verts))    # old vertex -> new id
    assert np.array_equal(need[:, back], need0) and np.array_equal(occl[:, back], occl0)
    _assert_bits(need[:, back], occl[:, back], need_ref, occl_ref)
    assert st["cull_occluded"] == rst["cull_occluded"] and got.nnz == ref.nnz


def test_read_back_refuses_without_a_whole_pass_with_rays():
    """MVS_ERR_STATE before any pass, after a pass without the visibility test and after a pass over a face range; fine again afterwards"""
    s = _reference("strip17")[0]
    c = M.Context(0)
    try:
        def refused():
            for call in (c.ray_bits, c.ray_vertex_order):
                with pytest.raises(M.MvsError) as e:
                    call()
                assert e.value.status == MVS_ERR_STATE
        c.set_mesh(s.verts, s.faces, s.normals); c.set_views(s.cams, s.images)
        refused()
        c.data_costs(M.Settings(geometric_visibility_test=False))
        refused()
        c.data_costs(M.Settings())
        need, occl = c.ray_bits()
        assert need.shape == occl.shape == (s.n_views, len(s.verts)) and occl.any()
        c.set_face_range(0, s.n_faces // 2)
        refused()
        c.data_costs(M.Settings())
        refused()
        c.set_face_range(0, s.n_faces)
        c.data_costs(M.Settings())
        assert np.array_equal(c.ray_bits()[0], need)
    finally:
        c.close()
