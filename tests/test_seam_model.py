"""Row f5 (global seam leveling) on the CPU: the library's ABI exports it, and the CPU model (tests/tools/seam_model.cpp) that the GPU
suite compares with bit for bit is checked here against independent numpy / scipy statements of the definition (DESIGN.md
section 4 "Global seam leveling")."""
import numpy as np
import pytest

import mvs_texturing_amd as M
import seam_model as SM
from conftest import get_scene

# calibrated on the model (tiny, five labelings, per-view offsets of up to 40 / 255): the mean absolute seam difference after the
# adjustment is 0.8 % .. 12.3 % of its value before; tests/test_gpu_seam_leveling.py keeps the same bound
PLANTED_RATIO = 0.25


@pytest.fixture(scope="module", autouse=True)
def _model_built():
    SM.build()


def test_library_exports_global_seam_leveling():
    L = M.load_library()
    for name in ("mvs_ctx_global_seam_leveling", "mvs_ctx_gsl_system", "mvs_gsl_default_params", "mvs_gsl_result_free", "mvs_gsl_system_free"):
        assert hasattr(L, name), name
    assert {"mvs_ctx_global_seam_leveling", "mvs_ctx_gsl_system", "mvs_gsl_default_params"} <= set(L._declared)
    p = M.default_gsl_params()
    assert (p.tolerance, p.max_iterations, p.lam) == (np.float32(1e-4), 1000, np.float32(0.1))
    assert hasattr(M.Context, "global_seam_leveling") and hasattr(M.Context, "gsl_system") and callable(M.global_seam_leveling)


def _numpy_layout(s, labels):
    """x rows, rings, A rows and the integer part of Lhs, written independently of the model"""
    F, NV = len(s.faces), len(s.verts)
    vf = [[] for _ in range(NV)]
    for f, tri in enumerate(s.faces.tolist()):
        for v in sorted(set(tri)):
            vf[v].append(f)
    xl = [sorted({int(labels[f]) for f in vf[v] if labels[f]}) for v in range(NV)]
    x_ptr = np.concatenate([[0], np.cumsum([len(l) for l in xl])]).astype(np.uint32)
    ring = [sorted({u for f in vf[v] for u in s.faces[f].tolist() if u != v}) for v in range(NV)]
    rows = {}
    for v in range(NV):
        for j, l1 in enumerate(xl[v]):
            for k in range(j + 1, len(xl[v])):
                l2 = xl[v][k]
                for u in ring[v]:
                    ef = [f for f in vf[v] if f in vf[u]]
                    pairs = [(a, b) for i, a in enumerate(ef) for b in ef[i + 1:] if sorted((labels[a], labels[b])) == [l1, l2]]
                    if pairs and np.linalg.norm(s.verts[u].astype(np.float32) - s.verts[v].astype(np.float32)) != 0:
                        rows[(v, j, k)] = True
                        break
    a_col = np.array([[x_ptr[v] + j, x_ptr[v] + k] for (v, j, k) in sorted(rows)], np.uint32).reshape(-1, 2)
    XR = int(x_ptr[-1])
    row_of = {(v, l): int(x_ptr[v]) + i for v in range(NV) for i, l in enumerate(xl[v])}
    ata = {}
    for a, b in a_col.tolist():
        ata[(a, a)] = ata.get((a, a), 0) + 1; ata[(b, b)] = ata.get((b, b), 0) + 1; ata[(a, b)] = -1; ata[(b, a)] = -1
    gam = {}
    for v in range(NV):
        for l in xl[v]:
            for u in ring[v]:
                if (u, l) in row_of:
                    i, c = row_of[(v, l)], row_of[(u, l)]
                    gam[(i, i)] = gam.get((i, i), 0) + 1; gam[(i, c)] = -1
    return x_ptr, np.array([l for x in xl for l in x], np.uint32), ring, a_col, ata, gam, XR


@pytest.mark.parametrize("name", ["first", "last", "random", "blocks", "random_with_unseen"])
def test_model_layout_equals_numpy(name):
    s = get_scene("tiny")
    labels = SM.crafted_labelings(s)[name]
    st, out, stats = SM.run_scene(s, labels)
    assert st == 0
    x_ptr, x_label, ring, a_col, ata, gam, XR = _numpy_layout(s, labels)
    assert np.array_equal(out["x_ptr"], x_ptr) and np.array_equal(out["x_label"], x_label)
    assert np.array_equal(out["ring"], np.array([u for r in ring for u in r], np.uint32))
    assert np.array_equal(out["a_col"].reshape(-1, 2), a_col)
    assert stats["x_rows"] == XR and stats["a_rows"] == len(a_col)
    assert stats["gamma_rows"] == sum(1 for (i, c) in gam if i != c) // 2
    g = np.float32(0.1) * np.float32(0.1)
    want = {}
    for key in set(ata) | set(gam):
        i, c = key
        if i == c:
            gs = np.float32(0)
            for _ in range(gam.get(key, 0)):
                gs = np.float32(gs + g)
            want[key] = np.float32(ata[key]) + gs if key in ata and key in gam else (np.float32(ata[key]) if key in ata else gs)
        else:
            want[key] = np.float32(ata[key]) if key in ata else np.float32(-g)
    ptr, col, val = out["lhs_ptr"], out["lhs_col"], out["lhs_val"]
    got = {(i, int(col[e])): val[e] for i in range(XR) for e in range(int(ptr[i]), int(ptr[i + 1]))}
    assert set(got) == set(want)
    assert all(np.float32(got[k]).view(np.uint32) == np.float32(want[k]).view(np.uint32) for k in want)
    assert all(np.all(np.diff(col[ptr[i]:ptr[i + 1]].astype(np.int64)) > 0) for i in range(XR))    # columns ascending
    assert stats["lhs_nnz_lower"] == sum(1 for (i, c) in want if c <= i)
    if name == "first":   # one label everywhere: no seam, Rhs = 0, no iteration
        assert stats["a_rows"] == 0 and stats["iterations"] == [0, 0, 0] and not np.any(out["x_adjust"])


@pytest.mark.parametrize("name", ["random", "blocks", "random_with_unseen"])
def test_model_solves_the_normal_equations(name):
    s = get_scene("tiny")
    st, out, stats = SM.run_scene(s, SM.crafted_labelings(s)[name])
    res = SM.normal_residual(out, stats["x_rows"])
    for c in range(3):
        assert res[c] <= 2.0 * float(stats["error"][c]) + 1e-6, (c, res, stats["error"])
        if stats["iterations"][c] < 1000:
            assert res[c] <= 2e-3
    # the mean is taken off: x_adjust sums to ~0 per channel, and corner k of face f carries its (vertex, label) row
    assert np.all(np.abs(out["x_adjust"].reshape(-1, 3).mean(0)) < 1e-5)
    labels = SM.crafted_labelings(s)[name]
    ca = out["corner_adjust"].reshape(-1, 3, 3)
    for f in range(0, len(s.faces), 7):
        for k in range(3):
            v = int(s.faces[f, k])
            if labels[f] == 0:
                assert not np.any(ca[f, k])
            else:
                r = int(out["x_ptr"][v]) + list(out["x_label"][out["x_ptr"][v]:out["x_ptr"][v + 1]]).index(labels[f])
                assert np.array_equal(ca[f, k], out["x_adjust"].reshape(-1, 3)[r])


@pytest.mark.parametrize("name", ["random", "blocks", "random_with_unseen"])
def test_model_recovers_planted_view_offsets(name):
    s = SM.planted_scene(get_scene("tiny"))
    st, out, stats = SM.run_scene(s, SM.crafted_labelings(get_scene("tiny"))[name])
    before, after = SM.seam_difference(out["a_col"], out["b"], out["x_adjust"])
    assert before > 0.05 and after <= PLANTED_RATIO * before, (before, after)


# caps inside, at the end of and just after the device's replays of 16 iterations, and tolerances on both sides of the default
CAPS = (0, 1, 15, 16, 17, 31, 32, 33)
TOLERANCES = (1e-2, 1e-7)


@pytest.mark.parametrize("name", ["random", "blocks"])
def test_model_under_iteration_caps_and_tolerances(name):
    s = get_scene("tiny")
    labels = SM.crafted_labelings(s)[name]
    st, base, bstats = SM.run_scene(s, labels)
    default = bstats["iterations"]
    assert st == 0 and min(default) > max(CAPS), default            # every cap binds on every channel
    capped = {}
    for cap in CAPS:
        st, out, stats = SM.run_scene(s, labels, max_iterations=cap)
        assert st == 0 and stats["iterations"] == [min(cap, d) for d in default], (cap, stats["iterations"])   # a capped iteration is counted
        capped[cap] = (out, stats)
    assert not np.any(capped[0][0]["x_raw"]) and np.all(capped[0][1]["error"] == 1)          # x0 = 0, r0 = Rhs
    assert np.all(capped[1][1]["error"] > bstats["error"]) and np.all(capped[1][1]["error"] < 1)
    assert np.all(capped[33][1]["error"] < capped[1][1]["error"])
    for a, b in zip(CAPS, CAPS[1:]):                                                         # one more iteration moves x
        assert not np.array_equal(capped[a][0]["x_raw"], capped[b][0]["x_raw"]), (a, b)
    its = {}
    for tol in TOLERANCES:
        st, out, stats = SM.run_scene(s, labels, tolerance=tol)
        assert st == 0 and max(stats["iterations"]) < 1000
        # the stop is |r|^2 < fl(tol tol) |Rhs|^2 in fp32: the error is below tol up to a few roundings
        assert np.all(stats["error"] <= tol * (1 + 1e-5)), (tol, stats["error"])
        its[tol] = stats["iterations"]
    assert all(a < d < b for a, d, b in zip(its[1e-2], default, its[1e-7])), (its, default)


def test_model_crafted_meshes_and_errors():
    for kw in (dict(), dict(fin=True), dict(zero_edge=True), dict(fin=True, zero_edge=True)):
        g = SM.grid_scene(**kw)
        st, out, stats = SM.run_scene(g, SM.grid_labels(g))
        assert st == 0 and stats["a_rows"] > 0, kw
        assert max(SM.normal_residual(out, stats["x_rows"])) <= 2e-3
    g = SM.grid_scene(outside=True)
    assert SM.run_scene(g, SM.grid_labels(g))[0] == 4                                 # a face outside its view
    g = SM.grid_scene()
    assert SM.run_scene(g, np.full(len(g.faces), 3, np.uint32))[0] == 4               # label > n_views
    st, out, stats = SM.run_scene(g, np.zeros(len(g.faces), np.uint32))
    assert st == 0 and stats["x_rows"] == 0 and len(out["x_adjust"]) == 0 and not np.any(out["corner_adjust"])
