"""Row f5 on the GPU: Context.global_seam_leveling equals the CPU model (tests/tools/seam_model.cpp) bit for bit -- structure, Lhs,
Rhs, b, x before and after the mean, per-corner adjustments, CG iterations and errors -- on the suite's scenes (labels from the
library's own view selection), shuffled meshes, crafted cases and the nested set of tests/test_patch_model.py (merge chains in every
candidate order, equal boxes); plus the checks of tests/test_seam_model.py on the GPU's output."""
import numpy as np
import pytest

import mvs_texturing_amd as M
import seam_model as SM
from conftest import get_scene
from test_patch_model import nested_set
from test_seam_model import CAPS, PLANTED_RATIO, TOLERANCES

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _model_built():
    SM.build()


def _ctx(s):
    c = M.Context(0)
    c.set_mesh(s.verts, s.faces, s.normals)
    c.set_views(s.cams, s.images)
    return c


_labels_cache = {}


def _library_labels(name, s):
    if name not in _labels_cache:
        c = _ctx(s)
        c.data_costs(M.Settings())
        _labels_cache[name], _ = c.view_selection(s.adj_ptr, s.adj)
        c.close()
    return _labels_cache[name]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32).ravel()


def _compare(s, labels, ctx=None, **kw):
    """one GPU run against the model; returns (gpu arrays, gpu stats, gpu system)"""
    st, want, wst = SM.run_scene(s, labels, **kw)
    assert st == 0
    c = ctx or _ctx(s)
    try:
        got, gst = c.global_seam_leveling(s.adj_ptr, s.adj, np.ascontiguousarray(labels, np.uint32),
                                          M.default_gsl_params(**{k: kw[k] for k in ("tolerance", "max_iterations") if k in kw}))
        sysg = c.gsl_system()
    finally:
        if ctx is None:
            c.close()
    assert np.array_equal(got["x_ptr"], want["x_ptr"]) and np.array_equal(got["x_label"], want["x_label"])
    lp, lc, lv = SM.lower_csr(want["lhs_ptr"], want["lhs_col"], want["lhs_val"])
    assert np.array_equal(sysg["lhs_ptr"], lp) and np.array_equal(sysg["lhs_col"], lc) and np.array_equal(_bits(sysg["lhs_val"]), _bits(lv))
    assert np.array_equal(sysg["a_col"].ravel(), want["a_col"])
    assert np.array_equal(_bits(sysg["b"]), _bits(want["b"])), "b differs"
    assert np.array_equal(_bits(sysg["rhs"]), _bits(want["rhs"])), "Rhs differs"
    assert gst["iterations"] == wst["iterations"], (gst["iterations"], wst["iterations"])
    assert np.array_equal(_bits(gst["error"]), _bits(wst["error"]))
    assert np.array_equal(_bits(sysg["x_raw"]), _bits(want["x_raw"])), "x before the mean differs"
    assert np.array_equal(_bits(got["x_adjust"]), _bits(want["x_adjust"]))
    assert np.array_equal(_bits(got["corner_adjust"]), _bits(want["corner_adjust"]))
    for k in SM.STATS:
        assert gst[k] == wst[k], (k, gst[k], wst[k])
    return got, gst, sysg


@pytest.mark.parametrize("name", ["tiny", "bumpy", "oddw", "mixed", "spiky", "close", "manyviews"])
def test_scenes_equal_the_model(name):
    s = get_scene(name)
    _, gst, _ = _compare(s, _library_labels(name, s))
    assert gst["a_rows"] > 0 and gst["x_rows"] > 0


@pytest.mark.parametrize("name", ["tiny", "bumpy"])
def test_shuffled_scenes_equal_the_model(name):
    s = get_scene(name)
    p = M.synth.permute_scene(s, seed=7)
    labels = _library_labels(name, s)[p.face_perm]
    got, _, _ = _compare(p, labels)
    # the same adjustments per face corner as the unshuffled run (the keys are the caller's ids; the arithmetic depends on the
    # numbering only through orders the definition fixes -- equal here up to those orders)
    want, _ = M.global_seam_leveling(s, _library_labels(name, s))
    assert np.allclose(got["corner_adjust"], want["corner_adjust"][p.face_perm], atol=2e-3)


def test_crafted_labelings_and_meshes():
    s = get_scene("tiny")
    lab = SM.crafted_labelings(s)
    _, gst, _ = _compare(s, lab["random"])
    assert gst["merged"] > 0                                              # candidates absorbed by a containing box
    _compare(s, lab["random_with_unseen"])
    _, gst, _ = _compare(s, lab["first"])                                 # a single label: Rhs = 0, no iteration
    assert gst["a_rows"] == 0 and gst["iterations"] == [0, 0, 0]
    for kw in (dict(), dict(fin=True), dict(zero_edge=True), dict(fin=True, zero_edge=True)):   # frame -1, a fin edge, a zero-length edge
        g = SM.grid_scene(**kw)
        _, gst, _ = _compare(g, SM.grid_labels(g))
        assert gst["a_rows"] > 0, kw
    g = SM.grid_scene()
    c = _ctx(g)                                                           # a fresh context without a data-cost pass
    got, gst = c.global_seam_leveling(g.adj_ptr, g.adj, np.zeros(len(g.faces), np.uint32))    # all labels 0: empty outputs
    assert gst["x_rows"] == 0 and len(got["x_adjust"]) == 0 and got["corner_adjust"].shape == (len(g.faces), 3, 3) and not np.any(got["corner_adjust"])
    c.close()


def test_nested_set_equals_the_model():
    """candidates absorbed through chains, in all six candidate orders, and two candidates with one box: the vertex projections go up
    several frames and the patch ids follow the merge"""
    for name, (g, labels) in nested_set().items():
        _, gst, _ = _compare(g, labels)
        assert gst["patches"] == 2 and gst["merged"] == 3 and gst["a_rows"] > 0, (name, gst)


def _caps_and_tolerances(s, labels, **kw):
    """every cap of test_seam_model.CAPS and both tolerances on ONE context, then an uncapped run on it: nothing of a cut-short replay
    of the captured graph (the device's done word, the ping-pong state, p) leaks into the next call.  kw: the tolerance of the capped
    and uncapped runs where it is not the default.  Returns the uncapped iterations."""
    c = _ctx(s)
    try:
        _, base, _ = _compare(s, labels, ctx=c, **kw)
        default = base["iterations"]
        for cap in CAPS:
            _, gst, _ = _compare(s, labels, ctx=c, max_iterations=cap, **kw)
            assert gst["iterations"] == [min(cap, d) for d in default], (cap, gst["iterations"], default)
        for tol in TOLERANCES:
            _, gst, _ = _compare(s, labels, ctx=c, tolerance=tol)
            assert max(gst["iterations"]) < 1000
        _, again, _ = _compare(s, labels, ctx=c, **kw)
        assert again["iterations"] == default and np.array_equal(_bits(again["error"]), _bits(base["error"]))
    finally:
        c.close()
    return default


@pytest.mark.parametrize("name", ["random", "blocks"])
def test_iteration_caps_around_the_graph_replay_and_tolerances(name):
    """caps inside (1, 15, 17, 31, 33), at the end of (16, 32) and before (0) the replays of 16 captured iterations"""
    s = get_scene("tiny")
    default = _caps_and_tolerances(s, SM.crafted_labelings(s)[name])
    assert min(default) > max(CAPS), default                              # every cap binds on every channel


def test_iteration_caps_with_a_single_reduction_block():
    g = SM.grid_scene()
    _, gst, _ = _compare(g, SM.grid_labels(g))
    assert 0 < gst["x_rows"] <= 256                                       # one tile: level two of the tree sums one partial
    default = _caps_and_tolerances(g, SM.grid_labels(g), tolerance=1e-7)  # 18 to 22 iterations at the default tolerance: below the later caps
    assert min(default) > max(CAPS), default


def test_host_and_device_inputs_and_repeat():
    import torch
    s = get_scene("bumpy")
    labels = _library_labels("bumpy", s)
    c = _ctx(s)
    a, _ = c.global_seam_leveling(s.adj_ptr, s.adj, labels)
    b, _ = c.global_seam_leveling(s.adj_ptr, s.adj, labels)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x, np.uint32).view(np.int32)).cuda()
    d, _ = c.global_seam_leveling(dev(s.adj_ptr), dev(s.adj), dev(labels))
    e, _ = c.global_seam_leveling(s.adj_ptr, s.adj, labels, on_device=True)          # device outputs held by the context
    c.synchronize()

    class _Dev:                                                                         # the context's buffer seen by torch, no copy
        __cuda_array_interface__ = {"shape": (9 * s.n_faces,), "typestr": "<f4", "data": (e["corner_adjust"].data_ptr(), False), "version": 2}
    ca = torch.as_tensor(_Dev(), device="cuda").cpu().numpy()
    c.close()
    assert np.array_equal(_bits(ca), _bits(a["corner_adjust"]))
    for k in ("x_ptr", "x_label"):
        assert np.array_equal(a[k], b[k]) and np.array_equal(a[k], d[k])
    for k in ("x_adjust", "corner_adjust"):
        assert np.array_equal(_bits(a[k]), _bits(b[k])) and np.array_equal(_bits(a[k]), _bits(d[k]))


def test_labeling_errors_leave_the_context_usable():
    g = SM.grid_scene()
    c = _ctx(g)
    with pytest.raises(M.MvsError) as e:
        c.global_seam_leveling(g.adj_ptr, g.adj, np.full(len(g.faces), 3, np.uint32))
    assert e.value.status == 4
    o = SM.grid_scene(outside=True)
    c2 = _ctx(o)
    with pytest.raises(M.MvsError) as e:
        c2.global_seam_leveling(o.adj_ptr, o.adj, SM.grid_labels(o))
    assert e.value.status == 4
    c2.close()
    _compare(g, SM.grid_labels(g), ctx=c)
    c.close()
    with pytest.raises(M.MvsError) as e:                                  # no mesh, no views
        M.Context(0).global_seam_leveling(g.adj_ptr, g.adj, SM.grid_labels(g))
    assert e.value.status == 6


def test_residual_and_planted_offsets_on_the_gpu():
    s = get_scene("tiny")
    for name in ("random", "blocks", "random_with_unseen"):
        labels = SM.crafted_labelings(s)[name]
        c = _ctx(s)
        got, gst = c.global_seam_leveling(s.adj_ptr, s.adj, labels)
        sysg = c.gsl_system()
        c.close()
        _, full, _ = SM.run_scene(s, labels)                              # the full symmetric Lhs of the same structure
        arrays = dict(lhs_ptr=full["lhs_ptr"], lhs_col=full["lhs_col"], lhs_val=full["lhs_val"], rhs=sysg["rhs"].ravel(), x_raw=sysg["x_raw"].ravel())
        res = SM.normal_residual(arrays, gst["x_rows"])
        for ch in range(3):
            assert res[ch] <= 2.0 * float(gst["error"][ch]) + 1e-6 and (gst["iterations"][ch] == 1000 or res[ch] <= 2e-3)
        p = SM.planted_scene(s)
        c = _ctx(p)
        got, gst = c.global_seam_leveling(p.adj_ptr, p.adj, labels)
        sysg = c.gsl_system()
        c.close()
        before, after = SM.seam_difference(sysg["a_col"], sysg["b"], got["x_adjust"])
        assert before > 0.05 and after <= PLANTED_RATIO * before, (name, before, after)


def test_config2_equals_the_model():
    s = M.synth.make_scene(**M.synth.CONFIGS[2])
    labels = _library_labels("config2", s)
    _, gst, _ = _compare(s, labels)
    assert gst["x_rows"] > 100000
