"""Ranged data costs inside one context (option "dc_range_pairs", csrc/k_dc.hip dc_ranged): the context's faces are walked in consecutive
ranges, maximum / histogram / percentile are taken once over all of them, ONE table comes out.  Every comparison here is bit for bit
against the unranged pass of the same context on the same scene: col_ptr, view_id, the uint32 views of quality and cost, table_order(),
the per-pair statistics, and labels + energy_fixed of view_selection on the ranged table.  The ray counters are sums over the ranges and
may exceed the unranged ones (a vertex shared by faces of two ranges is traced once per range)."""
import copy
import ctypes as C
import json
import os

import numpy as np
import pytest

import mvs_texturing_amd as M
import oracle_py as O
import util_cases as U
from conftest import get_scene
from test_gpu_parity import MODES

pytestmark = pytest.mark.gpu

# counts per (face, view) pair: equal to the unranged pass's
EQUAL_STATS = ("pairs", "cull_backface", "cull_angle", "cull_outside", "cull_occluded", "cull_zero_quality", "nnz_pre", "nnz",
               "footprints_lane_group", "footprints_rewalked")
# per ray of a range: sums over the ranges, never below the unranged pass's
RAY_STATS = ("rays", "ray_nodes", "ray_tris", "ray_packets", "ray_packets_generic", "ray_leaf_rounds")


@pytest.fixture(scope="module")
def ctx():
    c = M.Context(0)
    c.set_option("stats", 1); c.set_option("count_rays", 1)
    yield c
    c.set_option("dc_range_pairs", 0)
    c.close()


def _load(c, s):
    c.set_mesh(s.verts, s.faces, s.normals); c.set_views(s.cams, s.images)


def _pass(c, s, B, kw=None, solve=True):
    """one data-cost pass with option dc_range_pairs = B (+ the solve on its table): everything that is compared"""
    c.set_option("dc_range_pairs", B)
    st = c.data_costs(M.Settings(**(kw or {})))
    r = dict(stats=st, table=c.costs_download(), order=c.table_order(), ranges=c.dc_ranges())
    if solve:
        r["labels"], r["mrf"] = c.view_selection(s.adj_ptr, s.adj)
    return r


def _same_table(a, b):
    assert a.n_faces == b.n_faces and a.n_views == b.n_views and a.nnz == b.nnz
    assert np.array_equal(a.col_ptr, b.col_ptr), "sparsity pattern differs"
    assert np.array_equal(a.view_id, b.view_id)
    assert np.array_equal(a.quality.view(np.uint32), b.quality.view(np.uint32))
    assert np.array_equal(a.cost.view(np.uint32), b.cost.view(np.uint32))


def _same(got, ref):
    _same_table(got["table"], ref["table"])
    assert (got["order"] is None) == (ref["order"] is None)
    if ref["order"] is not None:
        assert np.array_equal(got["order"], ref["order"])
    g, r = got["stats"], ref["stats"]
    for k in EQUAL_STATS:
        assert g[k] == r[k], k
    for k in ("max_quality", "percentile"):
        assert np.float32(g[k]).view(np.uint32) == np.float32(r[k]).view(np.uint32), k
    for k in RAY_STATS:
        assert g[k] >= r[k], k
    if "labels" in ref:
        assert np.array_equal(got["labels"], ref["labels"])
        for k in ("energy_fixed", "cut_edges", "sweeps", "icm_iters", "unseen"):
            assert got["mrf"][k] == ref["mrf"][k], k


_REF = {}


def _unranged(c, name, mode):
    """the unranged pass of a (scene, mode), computed once and left unchanged"""
    if (name, mode) not in _REF:
        s = get_scene(name)
        _load(c, s)
        _REF[name, mode] = _pass(c, s, 0, MODES[mode])
    return _REF[name, mode]


@pytest.mark.parametrize("mode", list(MODES))
def test_ten_ranges_off_the_64_face_words_in_every_mode(ctx, mode):
    """bumpy, 9 680 faces x 12 views in ranges of 1000 faces: no boundary on a word of the bit matrices, a last range of 680; the outlier
    modes put the staged infos and the zero-quality erase on both sides of every boundary"""
    s = get_scene("bumpy")
    assert (s.n_faces, s.n_views) == (9680, 12)
    ref = _unranged(ctx, "bumpy", mode)
    assert ref["ranges"] == (1, 9680)
    _load(ctx, s)
    got = _pass(ctx, s, 12 * 1000, MODES[mode])
    assert got["ranges"] == (10, 1000)
    _same(got, ref)


def test_two_ranges_and_one_range_through_the_ranged_walk(ctx):
    s = get_scene("bumpy")
    ref = _unranged(ctx, "bumpy", "gmi_none_vis")
    _load(ctx, s)
    got = _pass(ctx, s, 12 * 4840, MODES["gmi_none_vis"])
    assert got["ranges"] == (2, 4840)
    _same(got, ref)
    got = _pass(ctx, s, 12 * 9680, MODES["gmi_none_vis"])          # one range, but kept and appended: the ranged code
    assert got["ranges"] == (1, 9680)
    _same(got, ref)
    for k in RAY_STATS:                                            # one range traces what the unranged pass traces
        assert got["stats"][k] == ref["stats"][k], k


def test_heavy_occlusion_in_seven_ranges_traces_less_than_twice_the_rays(ctx):
    """spiky32: 40 % of the front-facing pairs are occluded.  Seven ranges of the library's order; a range traces the rays of ITS faces'
    vertices only -- `rays` stays below twice the unranged count.  That a correct implementation stays under that cap on this scene is
    checked first, on the CPU: the oracle's pass pattern (no visibility test) gives the need bits of every range of the order."""
    s = get_scene("spiky32")
    F, V = s.n_faces, s.n_views
    per = -(-F // 7)
    ref = _unranged(ctx, "spiky32", "gmi_none_vis")
    _load(ctx, s)
    perm, _ = ctx.partition_faces(1)
    nv, sn = O.data_costs(s, geometric_visibility_test=False)
    need_all = int(U.need_from_pass_pattern(s, nv.col_ptr, nv.view_id).sum())
    cp = nv.col_ptr.astype(np.int64)
    need_ranges = 0
    for b in range(0, F, per):
        faces = np.sort(perm[b:b + per].astype(np.int64))
        sub = copy.copy(s); sub.faces = s.faces[faces]
        idx = np.concatenate([np.arange(cp[f], cp[f + 1]) for f in faces]) if len(faces) else np.zeros(0, np.int64)
        sub_ptr = np.concatenate([[0], np.cumsum(cp[faces + 1] - cp[faces])])
        need_ranges += int(U.need_from_pass_pattern(sub, sub_ptr, nv.view_id[idx]).sum())
    assert need_all <= need_ranges < 2 * need_all, (need_all, need_ranges)      # the scene's own boundary-vertex share
    got = _pass(ctx, s, V * per, MODES["gmi_none_vis"])
    assert got["ranges"] == (7, per)
    _same(got, ref)
    assert ref["stats"]["rays"] <= got["stats"]["rays"] < 2 * ref["stats"]["rays"]
    if sn["cull_zero_quality"] == 0:      # (the pattern is exactly the pass set then: the counts are the predicted ones)
        assert (ref["stats"]["rays"], got["stats"]["rays"]) == (need_all, need_ranges)


@pytest.mark.parametrize("max_labels,kw", [(7, dict()), (64, dict()), (0, dict(outlier_removal="gauss_damping")), (64, dict(outlier_removal="gauss_damping"))],
                         ids=["keep7", "keep64", "damping", "damping-keep64"])
def test_many_views_pruned_in_three_ranges(max_labels, kw):
    """manyviews (5 120 faces x 700 views, columns of 130 - 250 infos: above 78 of them outlier removal leaves the LDS-staged kernel):
    pruning is per column, so pruning range by range while appending equals pruning the whole table, nnz included"""
    s = get_scene("manyviews")
    per = -(-s.n_faces // 3)
    c = M.Context(0)
    try:
        c.set_option("stats", 1); c.set_option("max_labels", max_labels)
        _load(c, s)
        ref = _pass(c, s, 0, kw)
        got = _pass(c, s, s.n_views * per, kw)
        assert ref["ranges"] == (1, s.n_faces) and got["ranges"] == (3, per)
        _same(got, ref)
        if max_labels:
            K = np.diff(got["table"].col_ptr.astype(np.int64))
            assert K.max() == max_labels and got["stats"]["nnz"] == got["table"].nnz < got["stats"]["nnz_pre"]
    finally:
        c.close()


def test_one_face_per_range_inside_a_user_range(ctx):
    """tiny, the context's faces are positions [100, 164): B = n_views walks them one face at a time"""
    s = get_scene("tiny")
    _load(ctx, s)
    try:
        ctx.set_face_range(100, 164)
        ref = _pass(ctx, s, 0, solve=False)
        got = _pass(ctx, s, s.n_views, solve=False)
        assert ref["ranges"] == (1, 64) and got["ranges"] == (64, 1)
        assert got["table"].n_faces == 64 and got["table"].nnz > 0
        _same(got, ref)
        assert np.array_equal(got["order"][:64], ctx.partition_faces(1)[0][100:164])
        with pytest.raises(M.MvsError):                      # a range's table is no input for the solver, ranged or not
            ctx.view_selection(s.adj_ptr, s.adj)
    finally:
        ctx.set_face_range(0, s.n_faces)
    _same(_pass(ctx, s, s.n_views * 100), _pass(ctx, s, 0))


def _with_copies_of_one_triangle(s0, n_dup=6000):
    s = copy.copy(s0)
    s.faces = np.ascontiguousarray(np.concatenate([s0.faces, np.repeat(s0.faces[:1], n_dup, axis=0)]))
    s.normals = np.ascontiguousarray(np.concatenate([s0.normals, np.repeat(s0.normals[:1], n_dup, axis=0)]))
    return s


def test_order_rebuilt_in_the_first_range_restarts_the_walk():
    """thousands of equal centroid coordinates at a cut: the upper levels of the face order give up, the order is rebuilt while the first
    range is evaluated and the walk starts again.  The mesh of tiny + 6 000 copies of one triangle, and util_cases.tie_mesh(2049) in
    front of tiny's cameras.  That the order WAS rebuilt shows in the profile: a pass that starts again records dc_order twice (and one
    dc_cull more than it has ranges); the run without upper levels records it once."""
    s0 = get_scene("tiny")
    tv, tf = U.tie_mesh(2049)
    t = copy.copy(s0); t.verts, t.faces = tv, tf
    t.normals = np.ascontiguousarray(U.normals_float64(tv, tf).astype(np.float32))
    for s in (_with_copies_of_one_triangle(s0), t):
        F = len(s.faces)
        tabs = []
        for min_faces, B in ((0xFFFFFFFF, 0), (0, 0), (0, s.n_views * -(-F // 4))):
            c = M.Context(0)
            try:
                c.set_option("bvh_upper_min_faces", min_faces); c.set_option("bvh_window", 0); c.set_option("dc_range_pairs", B)
                c.set_option("profile", 1)
                c.set_mesh(s.verts, s.faces, s.normals); c.set_views(s.cams, s.images)
                st = c.data_costs(M.Settings())
                tabs.append((c.costs_download(), c.table_order(), st))
                assert c.dc_ranges() == ((4, -(-F // 4)) if B else (1, F))
                prof = c.get_profile()
                restarts = 1 if min_faces == 0 else 0
                assert prof["dc_order"][1] == 1 + restarts and prof["dc_prep"][1] == 1 + restarts, (min_faces, B, prof)
                assert prof["dc_cull"][1] == c.dc_ranges()[0] + restarts
            finally:
                c.close()
        for tab, order, st in tabs[1:]:
            _same_table(tab, tabs[0][0])
            assert np.array_equal(order, tabs[0][1])          # the rebuilt order IS the order without upper levels
            assert st["nnz"] == tabs[0][2]["nnz"] and st["pairs"] == F * s.n_views


def test_callers_numbering_and_a_permuted_mesh(ctx):
    s0 = get_scene("bumpy")
    s = M.synth.permute_scene(s0, seed=21)
    B = s.n_views * 1000
    _load(ctx, s)
    ref = _pass(ctx, s, 0)
    got = _pass(ctx, s, B)
    assert got["ranges"] == (10, 1000)
    _same(got, ref)
    ctx.set_option("face_order", 0)
    try:
        ref0 = _pass(ctx, s, 0)
        got0 = _pass(ctx, s, B)
        assert ref0["order"] is None and got0["order"] is None
        _same(got0, ref0)
        _same_table(got0["table"], ref["table"])              # (tables cross the ABI in the caller's numbering either way)
    finally:
        ctx.set_option("face_order", 1)


def test_environment_variable_reaches_the_one_shot_calls(monkeypatch):
    """MVS_DC_RANGE_PAIRS is how mvs_data_costs and the link-time drop-in get the option: same table, same labels, and the table still
    waits on the device for the mvs_view_selection that follows"""
    s = get_scene("bumpy")
    L = M.load_library()

    def one_shot():
        mesh = M.viewsel.CMesh(s.verts.shape[0], s.n_faces, s.verts.ctypes.data, s.faces.ctypes.data, s.normals.ctypes.data)
        views = (M.viewsel.CView * s.n_views)()
        for j in range(s.n_views):
            v = views[j]
            v.pos[:] = s.cams["pos"][j].tolist(); v.viewdir[:] = s.cams["viewdir"][j].tolist()
            v.K[:] = s.cams["K"][j].tolist(); v.w2c[:] = s.cams["w2c"][j].tolist()
            v.width, v.height, v.rgb = int(s.cams["width"][j]), int(s.cams["height"][j]), s.images[j].ctypes.data
        out = M.viewsel.CCsr(); st = M.Settings(); ds = M.viewsel.DcStats()
        assert L.mvs_data_costs(C.byref(mesh), views, s.n_views, C.byref(st), C.byref(out), C.byref(ds)) == 0, L.mvs_last_error()
        p_dc = json.loads(L.mvs_last_call_profile().decode())
        grab = lambda p, t, n: np.ctypeslib.as_array(C.cast(p, C.POINTER(t)), (max(n, 1),))[:n].copy()
        tab = (grab(out.col_ptr, C.c_uint32, s.n_faces + 1), grab(out.view_id, C.c_uint16, out.nnz), grab(out.cost, C.c_float, out.nnz).view(np.uint32))
        labels = np.zeros(s.n_faces, np.uint32); ms = M.viewsel.MrfStats()
        assert L.mvs_view_selection(C.byref(out), s.adj_ptr.ctypes.data, s.adj.ctypes.data, None, labels.ctypes.data, C.byref(ms)) == 0, L.mvs_last_error()
        p_vs = json.loads(L.mvs_last_call_profile().decode())
        L.mvs_csr_free(C.byref(out))
        return tab, labels, ms.energy_fixed, ds.nnz, p_dc, p_vs

    try:
        L.mvs_release_cached()                                    # no context parked by an earlier test: each call below makes or
        monkeypatch.delenv("MVS_DC_RANGE_PAIRS", raising=False)   # re-reads what the variable says NOW
        tab0, l0, e0, n0, p_dc0, _ = one_shot()
        assert p_dc0["dc_ranges"] == 1
        L.mvs_release_cached()
        monkeypatch.setenv("MVS_DC_RANGE_PAIRS", str(12 * 1000))
        tab1, l1, e1, n1, p_dc, p_vs = one_shot()
        assert p_dc["dc_ranges"] == 10                            # the one-shot pass WAS ranged
        # a context the library parked under one value of the variable does not keep it: the next call is made on the parked context
        monkeypatch.setenv("MVS_DC_RANGE_PAIRS", str(12 * 4840))
        tab2, l2, e2, n2, p_dc2, p_vs2 = one_shot()
        assert p_dc2["dc_ranges"] == 2 and p_dc2["table_kept_on_device"] is True and p_vs2["table_reused_on_device"] is True
        for a, b in zip(tab0, tab2):
            assert np.array_equal(a, b)
        assert np.array_equal(l0, l2) and e0 == e2 and n0 == n2
        monkeypatch.delenv("MVS_DC_RANGE_PAIRS")
        assert one_shot()[4]["dc_ranges"] == 1
        monkeypatch.setenv("MVS_DC_RANGE_PAIRS", str(12 * 1000))
        c = M.Context(0)                                          # (the variable is read where a context is made)
        try:
            _load(c, s); c.data_costs(M.Settings())
            assert c.dc_ranges() == (10, 1000)
        finally:
            c.close()
    finally:
        L.mvs_release_cached()
    for a, b in zip(tab0, tab1):
        assert np.array_equal(a, b)
    assert np.array_equal(l0, l1) and e0 == e1 and n0 == n1
    assert p_dc["table_kept_on_device"] is True and p_vs["table_reused_on_device"] is True


def test_no_state_leaks_from_one_call_to_the_next():
    """two ranged calls with different ranges, then an unranged one, on one context"""
    s = get_scene("tiny")
    c = M.Context(0)
    try:
        c.set_option("stats", 1)
        _load(c, s)
        fresh = _pass(c, s, 0)
        a = _pass(c, s, s.n_views * 77)
        b = _pass(c, s, s.n_views * 333)
        u = _pass(c, s, 0)
        assert a["ranges"] == (-(-s.n_faces // 77), 77) and b["ranges"] == (-(-s.n_faces // 333), 333) and u["ranges"] == (1, s.n_faces)
        for r in (a, b, u):
            _same(r, fresh)
        for k in RAY_STATS:
            assert u["stats"][k] == fresh["stats"][k], k
    finally:
        c.close()


def test_profile_accumulates_every_stage_over_the_ranges():
    """mvs_ctx_get_profile: the per-range stages are recorded once per range, order / BVH / prep once per pass, the append once"""
    s = get_scene("bumpy")
    c = M.Context(0)
    try:
        _load(c, s)
        c.set_option("profile", 1)
        per_range = ("dc_cull", "dc_need", "dc_rays", "dc_rank_scan", "dc_face_info", "dc_csr")
        c.set_option("dc_range_pairs", 0); c.data_costs(M.Settings())
        p0 = c.get_profile()
        assert "dc_append" not in p0 and all(p0[k][1] == 1 for k in per_range + ("dc_order", "dc_bvh_build", "dc_prep"))
        c.set_option("dc_range_pairs", 12 * 1000); c.data_costs(M.Settings())
        assert c.dc_ranges() == (10, 1000)
        p = c.get_profile()
        for k in per_range:
            assert p[k][1] == 10 and p[k][0] > 0.0, (k, p[k])
        for k in ("dc_order", "dc_bvh_build", "dc_prep", "dc_append"):
            assert p[k][1] == 1, (k, p[k])
        assert set(p) == set(p0) | {"dc_append"} and p["dc_post"][1] >= 1
    finally:
        c.close()


def test_ray_bits_say_no_after_a_ranged_pass():
    """the need / occluded matrices hold the LAST range's rays only: the building block refuses instead of handing out wrong bits"""
    s = get_scene("bumpy")
    c = M.Context(0)
    try:
        _load(c, s)
        c.set_option("dc_range_pairs", 0); c.data_costs(M.Settings())
        need0, occl0 = c.ray_bits()
        c.set_option("dc_range_pairs", 12 * 1000); c.data_costs(M.Settings())
        assert c.dc_ranges() == (10, 1000)
        with pytest.raises(M.MvsError) as ei:
            c.ray_bits()
        assert ei.value.status == 6 and "ranges" in str(ei.value)
        c.set_option("dc_range_pairs", 0); c.data_costs(M.Settings())
        need1, occl1 = c.ray_bits()
        assert np.array_equal(need0, need1) and np.array_equal(occl0, occl1) and need1.any()
    finally:
        c.close()


def test_nothing_to_evaluate_with_the_option_set():
    """an empty mesh reports (1, 0), a scene without views (1, faces): one range, an empty table (include/mvs_viewsel.h)"""
    s = get_scene("tiny")
    c = M.Context(0)
    try:
        c.set_option("dc_range_pairs", 8 * 50)
        with pytest.raises(M.MvsError):
            c.dc_ranges()                                         # no pass yet
        c.set_mesh(s.verts, s.faces, s.normals); c.set_views({k: v[:0] for k, v in s.cams.items()}, [])
        st = c.data_costs(M.Settings()); dc = c.costs_download()
        assert c.dc_ranges() == (1, s.n_faces)
        assert dc.nnz == 0 and dc.n_faces == s.n_faces and (dc.col_ptr == 0).all() and st["nnz"] == 0 and st["pairs"] == 0
        labels, ms = c.view_selection(s.adj_ptr, s.adj)
        assert (labels == 0).all() and ms["unseen"] == s.n_faces
        c.set_mesh(s.verts, np.zeros((0, 3), np.uint32), np.zeros((0, 3), np.float32)); c.set_views(s.cams, s.images)
        st = c.data_costs(M.Settings()); dc = c.costs_download()
        assert c.dc_ranges() == (1, 0)
        assert dc.nnz == 0 and dc.n_faces == 0 and st["nnz"] == 0 and st["pairs"] == 0
        c.set_mesh(s.verts, s.faces, s.normals)                   # ... and the context is as good as new
        _same(_pass(c, s, 8 * 50), _pass(c, s, 0))
    finally:
        c.close()


# How often one data_costs call records each dc_* stage (mvs_ctx_get_profile), per case: (context options, settings).  The dictionaries
# were read off the build of the commit BEFORE the host code of csrc/k_dc.hip was split into a function per stage, with _stage_counts
# below; a stage that moves between functions keeps its number of brackets.  "gmi_none" spells out what Settings() defaults to, so it
# equals "defaults"; "area_damping" is one case more than were asked for (the area term's kernels, the lane group on colours alone).
# The route of mvs_postprocess_face_infos has a test of its own below: the call itself runs on a temporary context whose profile no
# call can read.
STAGE_CASES = {
    "defaults": (dict(), dict()),
    "clamping": (dict(), dict(outlier_removal="gauss_clamping")),
    "novis": (dict(), dict(geometric_visibility_test=False)),
    "gmi_none": (dict(), dict(data_term="gmi", outlier_removal="none")),        # the WORDS kernels
    "area_damping": (dict(), dict(data_term="area", outlier_removal="gauss_damping")),
    "keep4": (dict(max_labels=4), dict()),
    "three_ranges": (dict(dc_range_pairs=12 * 3227), dict()),
}
_ONE_RANGE = dict(dc_order=1, dc_bvh_build=1, dc_prep=1, dc_cull=1, dc_need=1, dc_rays=1, dc_rank_scan=1, dc_face_info=1, dc_csr=1, dc_post=3)   # dc_post: local maximum, histogram, percentile + costs
STAGE_COUNTS = {
    "defaults": _ONE_RANGE,
    "clamping": _ONE_RANGE,
    "novis": dict(dc_order=1, dc_prep=1, dc_cull=1, dc_rank_scan=1, dc_face_info=1, dc_csr=1, dc_post=3),
    "gmi_none": _ONE_RANGE,
    "area_damping": _ONE_RANGE,
    "keep4": dict(_ONE_RANGE, dc_prune=1),
    "three_ranges": dict(dc_order=1, dc_bvh_build=1, dc_prep=1, dc_cull=3, dc_need=3, dc_rays=3, dc_rank_scan=3, dc_face_info=3, dc_csr=3, dc_post=4, dc_append=1),
}


def _stage_counts(case):
    """({stage: times recorded} of one data_costs call after a warm-up pass, its table, the table of the same call with stats = 1)"""
    opts, kw = STAGE_CASES[case]
    s = get_scene("bumpy")
    c = M.Context(0)
    try:
        _load(c, s)
        c.set_option("profile", 1)
        for k, v in opts.items():
            c.set_option(k, v)
        c.data_costs(M.Settings(**kw)); c.get_profile()               # warm-up: allocations, the first order / BVH
        if case == "three_ranges":
            assert c.dc_ranges() == (3, 3227)
        c.data_costs(M.Settings(**kw))
        p = c.get_profile()
        table = c.costs_download()
        c.set_option("stats", 1)
        c.data_costs(M.Settings(**kw))
        return {k: v[1] for k, v in p.items() if k.startswith("dc_")}, table, c.costs_download()
    finally:
        c.close()


@pytest.mark.parametrize("case", list(STAGE_CASES))
def test_every_stage_is_recorded_as_often_as_before_the_split(case):
    counts, table, table_stats = _stage_counts(case)
    assert counts == STAGE_COUNTS[case]
    _same_table(table_stats, table)                                   # the STATS instantiation of every kernel computes the same table


# the same for postprocess_face_infos on a caller's infos: dc_postprocess, dc_phase2, dc_phase3 as mvs_postprocess_face_infos runs them,
# but on a context of the test's (tests/tools/dc_postprocess_ctx.hip).  Read off the same parent build.
POSTPROCESS_STAGE_COUNTS = {"none": dict(dc_post=2), "gauss_clamping": dict(dc_post=2)}   # histogram, percentile + costs


def _postprocess_on_context(mode_name, case_name="outlier_mix_lds"):
    """({stage: times recorded} of one pass after a warm-up pass, its table and statistics, the table of the same pass with stats = 1)"""
    import postprocess_model as PM
    tool = C.CDLL(os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools", "libdc_postprocess_ctx.so"))
    tool.test_dc_postprocess_on.restype = C.c_int
    V, ptr, view, q, col = PM.get_case(case_name).args()
    ptr = np.ascontiguousarray(ptr, np.uint32); n = int(ptr[-1])
    face = np.repeat(np.arange(len(ptr) - 1), np.diff(ptr.astype(np.int64)))
    src = ptr[face].astype(np.int64) + ptr[face + 1] - 1 - np.arange(n)       # every face's list reversed
    rv, rq, rc = np.ascontiguousarray(view[src], np.uint16), np.ascontiguousarray(q[src], np.float32), np.ascontiguousarray(col[src], np.float32)
    st = M.Settings(outlier_removal=mode_name)
    c = M.Context(0)

    def run():
        ds = M.viewsel.DcStats()
        rcode = tool.test_dc_postprocess_on(c.h, C.c_uint32(len(ptr) - 1), C.c_uint32(V), C.c_void_p(ptr.ctypes.data),
                                            C.c_void_p(rv.ctypes.data), C.c_void_p(rq.ctypes.data), C.c_void_p(rc.ctypes.data), C.byref(st), C.byref(ds))
        assert rcode == 0, c.L.mvs_last_error()
        return ds
    try:
        c.set_option("profile", 1)
        run(); c.get_profile()
        ds = run()
        p = c.get_profile()
        table = c.costs_download()
        c.set_option("stats", 1)
        run()
        return {k: v[1] for k, v in p.items() if k.startswith("dc_")}, table, ds, c.costs_download()
    finally:
        c.close()


@pytest.mark.parametrize("mode", [0, 2], ids=["none", "gauss_clamping"])
def test_postprocess_route_records_its_stages_as_before_the_split(mode):
    """crafted infos (tests/tools/postprocess_model.py) through dc_postprocess + phases 2 and 3 on a context with the profile on: the
    stage counts of the parent, the table of the plain reference bit for bit, the same table with stats = 1"""
    import postprocess_model as PM
    mode_name = dict(PM.MODES)[mode]
    counts, got, ds, got_stats = _postprocess_on_context(mode_name)
    assert counts == POSTPROCESS_STAGE_COUNTS[mode_name]
    col_ptr, view, cost, q, rc, mx, pct, _ = PM.reference_of("outlier_mix_lds", mode)
    assert got.nnz == len(view) == ds.nnz and np.array_equal(got.col_ptr, col_ptr) and np.array_equal(got.view_id, view)
    assert np.array_equal(got.cost.view(np.uint32), cost.view(np.uint32))
    assert np.float32(ds.max_quality).view(np.uint32) == np.float32(mx).view(np.uint32)
    assert np.float32(ds.percentile).view(np.uint32) == np.float32(pct).view(np.uint32)
    _same_table(got_stats, got)
