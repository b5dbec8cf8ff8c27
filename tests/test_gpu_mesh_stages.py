"""Rows f1 and f3 of SURVEY.md 8(f) on the GPU past one tile and at their limits (csrc/k_mesh.hip, csrc/k_patch.hip): meshes of 20 480
faces (ten tiles of the 2048-element scan), thousands of components, BFS frontiers above one 256-node chunk, the capacity limits of the
adjacency kernels on either side, normals over the exponent range, vertex ids at and past n_verts -- against the oracle, integers exact
and normals bit for bit.  The case builders live in tests/util_cases.py; tests/test_oracle.py runs the oracle side of every case on the
CPU and checks that the cases are what they claim to be."""
import numpy as np
import pytest

import mvs_texturing_amd as M
import oracle_py as O
import util_cases as U
from conftest import get_scene

pytestmark = pytest.mark.gpu

MVS_ERR_INVALID, MVS_ERR_UNSUPPORTED = 1, 7      # include/mvs_viewsel.h


def _device_host(dev, dtype=np.uint32):
    """a DevArray of the context copied to the host through torch"""
    import torch
    dt = np.dtype(dtype)
    n = dev.shape[0]
    if n == 0:
        return np.zeros(0, dt)

    class _Dev:
        __cuda_array_interface__ = {"shape": (n * dt.itemsize,), "typestr": "|u1", "data": (dev.data_ptr(), False), "version": 2}
    return torch.as_tensor(_Dev(), device="cuda").cpu().numpy().view(dt)


def _ctx_adjacency(c, verts, faces):
    c.set_mesh(np.ascontiguousarray(verts, dtype=np.float32), np.ascontiguousarray(faces, dtype=np.uint32), np.zeros((len(faces), 3), np.float32))
    dev_ptr, dev_adj = c.build_adjacency()
    c.synchronize()
    return _device_host(dev_ptr), _device_host(dev_adj)


def _assert_f1_equals_oracle(name, verts, faces, c=None, n_verts=None):
    ap_o, ad_o = O.build_adjacency(faces)
    ap_g, ad_g = M.build_adjacency_graph(len(verts) if n_verts is None else n_verts, faces)
    assert np.array_equal(ap_o, ap_g) and np.array_equal(ad_o, ad_g), name
    f_o, n_o = O.prepare_mesh(verts, faces)
    f_g, n_g = M.prepare_mesh(verts, faces)
    assert np.array_equal(f_o, f_g), name
    assert np.array_equal(n_o.view(np.uint32), n_g.view(np.uint32)), name
    if c is not None:
        ap_c, ad_c = _ctx_adjacency(c, verts, faces)
        assert np.array_equal(ap_o, ap_c) and np.array_equal(ad_o, ad_c), name + " (context)"


@pytest.fixture(scope="module")
def ctx():
    c = M.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def small():
    """the mesh every refusal is followed by, with the oracle's answer (computed once, never modified)"""
    s = get_scene("tiny")
    return s.verts, s.faces, O.build_adjacency(s.faces)


def _assert_small_still_works(small, c=None):
    verts, faces, (ap_o, ad_o) = small
    ap, ad = M.build_adjacency_graph(len(verts), faces)
    assert np.array_equal(ap, ap_o) and np.array_equal(ad, ad_o)
    if c is not None:
        ap, ad = _ctx_adjacency(c, verts, faces)
        assert np.array_equal(ap, ap_o) and np.array_equal(ad, ad_o)


@pytest.mark.parametrize("name", ["built", "repeated", "duplicates", "open", "built-permuted", "repeated-permuted", "duplicates-permuted", "open-permuted"])
def test_row_f1_on_twenty_thousand_faces(ctx, name):
    """B.1: 20 480 faces / 10 242 vertices -- both adjacency paths over 160 blocks, the scans of build_adjacency and of prepare_mesh's
    compaction over ten tiles; one-shot entry points and the resident mesh of a context"""
    verts, faces = U.f1_large_meshes(get_scene("spiky32"))[name]
    _assert_f1_equals_oracle(name, verts, faces, ctx)


@pytest.mark.parametrize("name", sorted(U.f1_limit_meshes()))
def test_row_f1_capacity_limits(ctx, small, name):
    """B.2 / B.3: 48 neighbours are served and 49 refused on both adjacency paths; adjacency_kernel counts neighbours of smaller and of
    larger id separately (a face with 48 + 48 is served there and refused by adjacency_general_kernel, which keeps 48 in all); 128
    candidates are served and 129 refused.  Every refusal is MVS_ERR_UNSUPPORTED from the kernels' own overflow counter, and the next
    call -- one-shot and in the same context -- is served and correct."""
    verts, faces, refused = U.f1_limit_meshes()[name]
    if not refused:
        _assert_f1_equals_oracle(name, verts, faces, ctx)
        return
    with pytest.raises(M.MvsError) as e:
        M.build_adjacency_graph(len(verts), faces)
    assert e.value.status == MVS_ERR_UNSUPPORTED, str(e.value)
    with pytest.raises(M.MvsError) as e:
        _ctx_adjacency(ctx, verts, faces)
    assert e.value.status == MVS_ERR_UNSUPPORTED, str(e.value)
    _assert_small_still_works(small, ctx)
    f_o, n_o = O.prepare_mesh(verts, faces)                      # prepare_mesh has no such limit
    f_g, n_g = M.prepare_mesh(verts, faces)
    assert np.array_equal(f_o, f_g) and np.array_equal(n_o.view(np.uint32), n_g.view(np.uint32))


@pytest.mark.parametrize("name", ["scale2^-40", "scale2^-20", "scale2^20", "scale2^40", "translate2^20", "scale2^-70"])
def test_row_f1_normals_over_the_exponent_range(name):
    """B.4: the normals of compact_faces_kernel are the oracle's bit for bit from 2^-70 to 2^40 -- where the squared length leaves float32
    (2^-40, 2^40) and where the cross product itself is denormal (2^-70) included; what the oracle's own distance from a float64
    normal is at each scale is asserted on the CPU (tests/test_oracle.py test_row_f1_normals_over_the_exponent_range)"""
    verts, faces = U.f1_scaled_meshes(get_scene("tiny"))[name]
    f_o, n_o = O.prepare_mesh(verts, faces)
    f_g, n_g = M.prepare_mesh(verts, faces)
    assert np.array_equal(f_o, f_g)
    differ = np.nonzero((n_o.view(np.uint32) != n_g.view(np.uint32)).any(axis=1))[0]
    assert len(differ) == 0, (name, len(differ), n_o[differ[:3]], n_g[differ[:3]])


def test_row_f1_vertex_ids(small):
    """B.5: an index >= n_verts is MVS_ERR_INVALID ("vertex id out of range") at both one-shot entry points, before anything reaches the
    device; the largest valid id n_verts - 1 on either side of a power of two (the key bits of the edge sort) gives the oracle's lists"""
    verts, faces, _ = small
    nv = len(verts)
    for bad_id, n_verts in ((nv, nv), (0xFFFFFFFF, nv), (int(faces.max()), int(faces.max()))):
        f = faces.copy(); f[len(f) // 2, 1] = bad_id
        for call in (lambda: M.build_adjacency_graph(n_verts, f), lambda: M.prepare_mesh(verts[:n_verts], f)):
            with pytest.raises(M.MvsError) as e:
                call()
            assert e.value.status == MVS_ERR_INVALID and "vertex id out of range" in str(e.value)
        _assert_small_still_works(small)
    for name, (n_verts, v, f) in U.f1_id_meshes(get_scene("tiny")).items():
        assert int(f.max()) == n_verts - 1 and len(v) == n_verts
        _assert_f1_equals_oracle(name, v, f, n_verts=n_verts)


@pytest.fixture(scope="module")
def f3_cases():
    return U.f3_large_cases(get_scene("spiky32"))


@pytest.mark.parametrize("name", ["noisy40", "bands", "one_label", "sparse_labels", "multigraph", "multigraph2", "star", "path"])
def test_row_f3_past_one_tile_and_one_chunk(ctx, f3_cases, name):
    """C: get_subgraphs == the oracle element for element -- more than 2048 components (root compaction, (label, root) sort and comp_ptr
    over several tiles), components and frontiers far above one 256-node chunk with degrees around 20 and duplicate list entries, a
    hub whose list names every leaf twice, a path (one node per chunk), one label, 70 000 labels with empty ones at both ends; one-shot
    and twice in one context"""
    adj_ptr, adj, labels, n_labels = f3_cases[name]
    want = O.get_subgraphs(adj_ptr, adj, labels, n_labels)
    if name in ("noisy40", "sparse_labels"):
        assert len(want[1]) - 1 > 2048
    got = M.get_subgraphs(adj_ptr, adj, labels, n_labels)
    for w, g in zip(want, got):
        assert np.array_equal(w, g), name
    for rep in range(2):
        got = ctx.get_subgraphs(adj_ptr, adj, labels, n_labels)
        for w, g in zip(want, got):
            assert np.array_equal(w, g), (name, rep)
