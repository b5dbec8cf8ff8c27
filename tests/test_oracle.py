"""CPU tests of the ORACLE (the checker itself): golden fixtures, independent
numpy / scipy re-statements of its pieces, and the properties the reference
implies.  No GPU needed."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle_py as O
from conftest import get_scene
from util_cases import brute_force_optimum, energy_numpy, random_mrf
import util_cases as U

GOLD = os.path.join(os.path.dirname(__file__), "golden")


@pytest.mark.parametrize("name", ["c1", "bumpy"])
def test_golden_fixtures_reproduced(name):
    """the oracle still produces the committed vectors (and the scene generator still the same scene)"""
    import sys
    sys.path.insert(0, GOLD)
    from make_golden import MODES, scene_checksum
    g = np.load(os.path.join(GOLD, name + ".npz"))
    s = get_scene(name)
    assert scene_checksum(s) == str(g["scene_checksum"]), "synthetic scene drifted: regenerate goldens deliberately"
    for mode, kw in MODES.items():
        if mode + "/col_ptr" not in g:
            continue
        csr, st = O.data_costs(s, **kw)
        assert np.array_equal(csr.col_ptr, g[mode + "/col_ptr"])
        assert np.array_equal(csr.view_id, g[mode + "/view_id"])
        assert np.array_equal(csr.quality.view(np.uint32), g[mode + "/quality"].view(np.uint32))
        assert np.array_equal(csr.cost.view(np.uint32), g[mode + "/cost"].view(np.uint32))
        culls = [st[k] for k in ("cull_backface", "cull_angle", "cull_outside", "cull_occluded", "cull_zero_quality", "nnz_pre")]
        assert culls == g[mode + "/culls"].tolist()
        if mode + "/labels" in g:
            labels, ms = O.view_selection(csr, s.adj_ptr, s.adj)
            assert np.array_equal(labels, g[mode + "/labels"])
            assert [ms["energy_fixed"], ms["cut_edges"], ms["sweeps"], ms["icm_iters"]] == g[mode + "/energy_fixed"].tolist()


def test_reference_properties_bumpy():
    """sorted columns, costs in [0,1], labels from the face's own column, 0 <=> empty column"""
    s = get_scene("bumpy")
    csr, st = O.data_costs(s)
    K = np.diff(csr.col_ptr)
    for i in np.nonzero(K > 1)[0][:2000]:
        v = csr.view_id[csr.col_ptr[i]:csr.col_ptr[i + 1]]
        assert (np.diff(v.astype(np.int64)) > 0).all()                      # calculate_data_costs.cpp:272
    assert csr.cost.min() >= 0.0 and csr.cost.max() <= 1.0                   # :295-296
    assert st["cull_outside"] > 0 and st["cull_occluded"] > 0 and st["cull_angle"] > 0
    labels, ms = O.view_selection(csr, s.adj_ptr, s.adj)
    assert ((labels == 0) == (K == 0)).all()                                 # view_selection.cpp:50-51
    e, cuts = O.energy(csr, s.adj_ptr, s.adj, labels)                        # rejects labels outside the column
    assert e == ms["energy_fixed"] and cuts == ms["cut_edges"] and e != 2 ** 64 - 1
    e2, c2 = energy_numpy(csr.col_ptr, csr.view_id, csr.cost, s.adj_ptr, s.adj, labels)
    assert e2 == e and c2 == cuts


def test_bvh_equals_brute_force():
    """the any-hit boolean does not depend on the acceleration structure"""
    for name in ("tiny", "bumpy", "spiky"):
        s = get_scene(name)
        a, sa = O.data_costs(s, brute=False)
        b, sb = O.data_costs(s, brute=True)
        assert np.array_equal(a.col_ptr, b.col_ptr) and np.array_equal(a.view_id, b.view_id)
        assert sa["cull_occluded"] == sb["cull_occluded"] and sa["cull_occluded"] > 0


def test_face_range_and_threads_do_not_change_results():
    s = get_scene("bumpy")
    full, _ = O.data_costs(s, n_threads=1)
    multi, _ = O.data_costs(s, n_threads=4)
    assert np.array_equal(full.col_ptr, multi.col_ptr) and np.array_equal(full.quality.view(np.uint32), multi.quality.view(np.uint32))
    part, _ = O.data_costs(s, face_range=(1000, 3000))
    a, b = full.col_ptr[1000], full.col_ptr[3000]
    assert np.array_equal(part.view_id, full.view_id[a:b])
    assert np.array_equal(part.quality.view(np.uint32), full.quality[a:b].view(np.uint32))   # qualities are local; costs depend on the global percentile


def test_image_prep_against_scipy():
    """validity mask = zero pixels 4-connected to a corner (texture_view.cpp:42-94); Sobel magnitude; erosion semantics"""
    from scipy import ndimage
    rng = np.random.default_rng(5)
    h, w = 61, 83
    img = rng.integers(1, 255, size=(h, w, 3), dtype=np.uint8)
    img[:9, :13] = 0; img[30:40, 20:50] = 0; img[h - 5:, w - 20:] = 0; img[5:9, 13:30] = 0   # corner blobs, an island, a tail
    L = O.load()
    mask = np.zeros((h, w), np.uint8); L.orc_validity_mask(img.ctypes.data, w, h, mask.ctypes.data)
    zero = img.sum(axis=2) == 0
    lab, _ = ndimage.label(zero, structure=[[0, 1, 0], [1, 1, 1], [0, 1, 0]])
    reach = np.zeros_like(zero)
    for cy, cx in ((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)):
        if zero[cy, cx]:
            reach |= lab == lab[cy, cx]
    assert np.array_equal(mask.astype(bool), ~reach)
    assert mask[35, 30] == 1          # the island is NOT reachable from a corner: stays valid
    gmi = np.zeros((h, w), np.uint8); L.orc_gradient_magnitude(img.ctypes.data, w, h, gmi.ctypes.data)
    lum = (0.30 * img[..., 0].astype(np.float64) + (np.float32(0.59) * img[..., 1].astype(np.float32)).astype(np.float64)
           + (np.float32(0.11) * img[..., 2].astype(np.float32)).astype(np.float64)).astype(np.uint8).astype(np.float64)
    gx = ndimage.correlate(lum, np.array([[-1, 0, 1], [-2, 0, 2], [-1, 0, 1]], float), mode="constant")
    gy = ndimage.correlate(lum, np.array([[-1, -2, -1], [0, 0, 0], [1, 2, 1]], float), mode="constant")
    ref = np.minimum(255.0, np.sqrt(gx * gx + gy * gy)).astype(np.uint8)
    ref[0, :] = ref[-1, :] = 0; ref[:, 0] = ref[:, -1] = 0
    assert np.array_equal(gmi, ref)
    er = mask.copy(); L.orc_erode_validity_mask(er.ctypes.data, w, h)
    inv = (mask == 0); inv[0, :] = inv[-1, :] = False; inv[:, 0] = inv[:, -1] = False   # only INTERIOR invalid pixels erode
    dil = ndimage.binary_dilation(inv, structure=np.ones((3, 3), bool))
    assert np.array_equal(er.astype(bool), mask.astype(bool) & ~dil)


def test_percentile_against_numpy_restatement():
    """Histogram::add_value / get_approx_percentile (histogram.cpp:27-63)"""
    rng = np.random.default_rng(11)
    q = (rng.random(50000).astype(np.float32) ** 3) * np.float32(7.5)
    mx = np.float32(q.max())
    L = O.load()
    got = L.orc_percentile(q.ctypes.data, len(q), C.c_float(mx), C.c_float(0.995))
    idx = np.floor((np.minimum(q, mx) / mx) * np.float32(9999)).astype(np.int64)
    bins = np.bincount(idx, minlength=10000)
    num = 0; ub = np.float32(0); ref = mx
    for i in range(10000):
        if np.float32(num) / np.float32(len(q)) > np.float32(0.995):
            ref = ub; break
        num += int(bins[i]); ub = np.float32(np.float32(i) / np.float32(9999)) * mx
    assert np.float32(got) == np.float32(ref)


def test_outlier_detection_matches_numpy_linear_algebra():
    """photometric_outlier_detection (calculate_data_costs.cpp:35-129): damping multiplies the quality by
    exp(-0.5 * 0.2 * d^T Sigma^-1 d); compare against numpy's inverse on a face with many views"""
    s = get_scene("bumpy")
    none, _ = O.data_costs(s, data_term="area", outlier_removal="none")
    damp, _ = O.data_costs(s, data_term="area", outlier_removal="gauss_damping")
    clamp, _ = O.data_costs(s, data_term="area", outlier_removal="gauss_clamping")
    assert damp.nnz <= none.nnz and clamp.nnz <= none.nnz
    # damping never increases a quality, clamping keeps or removes entries
    for i in np.nonzero(np.diff(none.col_ptr) >= 6)[0][:200]:
        qn = dict(zip(none.view_id[none.col_ptr[i]:none.col_ptr[i + 1]], none.quality[none.col_ptr[i]:none.col_ptr[i + 1]]))
        for v, q in zip(damp.view_id[damp.col_ptr[i]:damp.col_ptr[i + 1]], damp.quality[damp.col_ptr[i]:damp.col_ptr[i + 1]]):
            assert q <= qn[v] * (1 + 1e-6)
        for v, q in zip(clamp.view_id[clamp.col_ptr[i]:clamp.col_ptr[i + 1]], clamp.quality[clamp.col_ptr[i]:clamp.col_ptr[i + 1]]):
            assert q == qn[v]


def test_8bit_message_storage():
    """the solver stores messages as 8-bit codes over [0, 1/rho]: the oracle's conversion equals a numpy restatement --
    code = rne(fma(old, alpha, raw_s)), raw_s = raw * ((1 - alpha) * (255 / lam)), saturated at 255, products in fp32, the fma evaluated
    exactly in fp64 and rounded once -- codes cover 0 .. 255, the undamped stored value (code * lam / 255) is within half a
    step of the input, storing a stored value again is the identity, and full damping towards a code reproduces it"""
    L = O.load()
    L.orc_msg_code.argtypes = [C.c_float, C.c_float, C.c_float, C.c_uint32]; L.orc_msg_code.restype = C.c_uint32
    rng = np.random.default_rng(0)
    f32 = np.float32
    for rho in (f32(0.8), f32(1.0), f32(0.6667), f32(0.5)):
        lam = f32(1.0) / rho
        scale, step = f32(255.0) / lam, lam / f32(255.0)
        x = np.concatenate([rng.random(3000).astype(np.float32) * lam, f32([0, lam, lam / 2, step / 2, step * 0.49, step * 254.5, step * 1.5, step * 2.5, 1e-9])]).astype(np.float32)
        for alpha in (f32(0.0), f32(0.2), f32(0.35)):
            old = rng.integers(0, 256, len(x)).astype(np.uint32)
            code = np.array([L.orc_msg_code(C.c_float(float(v)), C.c_float(float(rho)), C.c_float(float(alpha)), int(o)) for v, o in zip(x, old)], dtype=np.uint32)
            oms = (f32(1.0) - alpha) * scale
            t1 = (x * oms).astype(np.float32)                                           # fp32 product
            v = (old.astype(np.float64) * np.float64(alpha) + t1.astype(np.float64)).astype(np.float32)   # exact in fp64, one rounding = fma
            ref = np.minimum(np.rint(v), 255).astype(np.uint32)                         # round to nearest even
            assert np.array_equal(code, ref)
            if alpha == 0:
                assert code.max() == 255 and code.min() == 0
                val = code.astype(np.float32) * step
                assert (np.abs(val - x) <= step * 0.5 * (1 + 1e-3) + 1e-7).all()
                again = np.array([L.orc_msg_code(C.c_float(float(v)), C.c_float(float(rho)), C.c_float(0.0), 0) for v in val], dtype=np.uint32)
                assert np.array_equal(again, code)


def test_solver_quality_small_instances():
    """the DEFINED-HERE solver: never worse than plain ICM, optimal or near-optimal on tiny instances"""
    worse = 0
    for seed in range(12):
        col_ptr, view_id, cost, adj_ptr, adj = random_mrf(9, 5, 3, 3, seed)
        csr = O.CsrNp(9, 5, col_ptr, view_id, cost)
        labels, ms = O.view_selection(csr, adj_ptr, adj)
        e, cuts = energy_numpy(col_ptr, view_id, cost, adj_ptr, adj, labels)
        assert e == ms["energy_fixed"]
        opt = brute_force_optimum(col_ptr, view_id, cost, adj_ptr, adj)
        assert e / 2 ** 32 >= opt - 1e-6
        if e / 2 ** 32 > opt * 1.05 + 1e-6:
            worse += 1
        icm = O.icm_baseline(csr, adj_ptr, adj)
        ei, _ = O.energy(csr, adj_ptr, adj, icm)
        assert e <= ei
    assert worse <= 2


def test_solver_beats_icm_on_scene_and_is_deterministic():
    s = get_scene("bumpy")
    csr, _ = O.data_costs(s)
    l1, m1 = O.view_selection(csr, s.adj_ptr, s.adj, n_threads=1)
    l2, m2 = O.view_selection(csr, s.adj_ptr, s.adj, n_threads=4)
    assert np.array_equal(l1, l2) and m1["energy_fixed"] == m2["energy_fixed"]
    icm = O.icm_baseline(csr, s.adj_ptr, s.adj)
    ei, _ = O.energy(csr, s.adj_ptr, s.adj, icm)
    assert m1["energy_fixed"] < ei


def test_guards():
    """calculate_data_costs.cpp:317-318"""
    s = get_scene("tiny")
    L = O.load()
    m = O.mesh_struct(s); views = O.view_structs(s); st = O.settings_struct()
    out = O.Csr(); stats = O.DcStats()
    rc = L.orc_data_costs(C.byref(m), views, 70000, C.byref(st), 0, 0, 0, 1, C.byref(out), C.byref(stats))
    assert rc == 2


def _f1_meshes():
    """meshes for the row-f1 stages: manifold, open boundary, duplicated faces, a non-manifold fan, degenerate faces"""
    s = get_scene("tiny")
    out = {"manifold": (s.verts, s.faces)}
    out["open"] = (s.verts, s.faces[: len(s.faces) // 2].copy())
    dup = np.concatenate([s.faces, s.faces[5:9], s.faces[40:41][:, [1, 2, 0]], s.faces[41:42][:, [0, 2, 1]]])
    out["duplicates"] = (s.verts, np.ascontiguousarray(dup))
    nv = len(s.verts)
    extra_v = np.array([[0.0, 0.0, 2.0], [0.0, 0.3, 2.2], [0.2, -0.2, 2.1]], dtype=np.float32)
    a, b = s.faces[0][0], s.faces[0][1]
    fan = np.array([[a, b, nv], [b, a, nv + 1], [a, b, nv + 2]], dtype=np.uint32)          # 5 faces on the edge (a, b)
    out["fan"] = (np.ascontiguousarray(np.concatenate([s.verts, extra_v])), np.ascontiguousarray(np.concatenate([s.faces, fan])))
    deg = np.array([[a, a, b], [a, b, a], [nv - 1, nv - 1, nv - 1]], dtype=np.uint32)
    out["degenerate"] = (s.verts, np.ascontiguousarray(np.concatenate([s.faces, deg])))
    # triangle soup, a quarter of the faces with a repeated vertex: the reference's edge query (a, a) returns every face at a
    rng = np.random.default_rng(3)
    soup = rng.integers(0, 40, (150, 3)).astype(np.uint32)
    m = rng.random(150) < 0.25; soup[m, 1] = soup[m, 0]
    m = rng.random(150) < 0.05; soup[m, 2] = soup[m, 0]
    out["soup"] = (rng.standard_normal((40, 3)).astype(np.float32), np.ascontiguousarray(soup))
    return out


def test_adjacency_restatement_properties():
    """build_adjacency_graph.cpp:16-53 + UniGraph::add_edge: symmetric, no self loops, list order = smaller ids ascending then edge order;
    around a face with a repeated vertex a: adjacent to every face at a (the reference's query for the "edge" (a, a))"""
    for name, (verts, faces) in _f1_meshes().items():
        adj_ptr, adj = O.build_adjacency(faces)
        F = len(faces)
        pairs = set()
        for i in range(F):
            nb = adj[adj_ptr[i]:adj_ptr[i + 1]].tolist()
            assert len(set(nb)) == len(nb) and i not in nb, name
            small = [g for g in nb if g < i]
            if name not in ("degenerate", "soup"):       # a face with a repeated vertex finds neighbours that do not find it: no such order
                assert small == sorted(small) and nb[:len(small)] == small, name
            for g in nb:
                pairs.add((i, g))
                assert len(set(faces[i].tolist()) & set(faces[g].tolist())) >= 2 or name in ("degenerate", "soup"), name
        assert all((g, i) in pairs for i, g in pairs), name
    s = get_scene("tiny")
    ap, ad = O.build_adjacency(s.faces)
    assert np.array_equal(ap, s.adj_ptr) and np.array_equal(ad, s.adj)      # the scene generator restates the same semantics independently


def test_prepare_mesh_restatement():
    """prepare_mesh.cpp:14-70: the LAST copy of a duplicated face survives, order is kept, normals = normalised (b-a)x(c-a)"""
    m = _f1_meshes()
    verts, faces = m["duplicates"]
    f2, n2 = O.prepare_mesh(verts, faces)
    F0 = len(get_scene("tiny").faces)
    assert len(f2) == F0                                                     # 6 duplicates removed, the later copies kept
    keep = [i for i in range(len(faces)) if not any(set(faces[i].tolist()) == set(faces[g].tolist()) for g in range(i + 1, len(faces)))]
    assert np.array_equal(f2, faces[keep])
    a, b, c = verts[f2[:, 0]], verts[f2[:, 1]], verts[f2[:, 2]]
    ref = np.cross(b - a, c - a); ref /= np.linalg.norm(ref, axis=1, keepdims=True)
    assert np.allclose(n2, ref, atol=2e-6)
    verts, faces = m["degenerate"]
    f3, n3 = O.prepare_mesh(verts, faces)
    assert (n3[-1] == 0).all()                                               # zero-area face: zero normal, no NaN


def _adjacency_numpy(faces):
    """the neighbour SETS of a mesh without repeated-vertex faces: faces sharing an (unordered) edge, as sorted (face, neighbour) pairs"""
    F = len(faces)
    f = faces.astype(np.int64)
    e = np.concatenate([np.sort(f[:, [0, 1]], axis=1), np.sort(f[:, [1, 2]], axis=1), np.sort(f[:, [2, 0]], axis=1)])
    key = e[:, 0] << 32 | e[:, 1]
    own = np.tile(np.arange(F), 3)
    o = np.argsort(key, kind="stable"); key, own = key[o], own[o]
    first = np.searchsorted(key, key, side="left"); last = np.searchsorted(key, key, side="right")
    pairs = set()
    for d in range(1, int((last - first).max())):
        i = np.arange(len(key)); m = i + d < last
        a, b = own[i[m]], own[i[m] + d]
        ne = a != b
        pairs |= set(zip(a[ne].tolist(), b[ne].tolist())) | set(zip(b[ne].tolist(), a[ne].tolist()))
    return pairs


def test_row_f1_cases_past_one_tile_and_at_the_capacity_limits():
    """the oracle side of tests/test_gpu_mesh_stages.py: 20 480-face meshes (as built, repeated vertices, duplicates, open, each also
    permuted) and the fans / discs at the capacity limits of csrc/k_mesh.hip -- lists are symmetric and without self loops, equal as
    sets to an independent numpy edge match where no face repeats a vertex; the fans have the neighbour counts the limits are about"""
    big = U.f1_large_meshes(get_scene("spiky32"))
    assert len(big["built"][1]) == 20480 and len(big["built"][0]) == 10242
    cases = {k: v for k, v in big.items()}
    cases.update({k: (v[0], v[1]) for k, v in U.f1_limit_meshes().items()})
    deg = {}
    for name, (verts, faces) in cases.items():
        ap, ad = O.build_adjacency(faces)
        F = len(faces)
        src = np.repeat(np.arange(F), np.diff(ap.astype(np.int64)))
        assert not (src == ad).any(), name
        fwd = set(zip(src.tolist(), ad.tolist()))
        assert len(fwd) == len(ad) and all((g, i) in fwd for i, g in fwd), name
        if not (faces[:, 0] == faces[:, 1]).any() and not (faces[:, 1] == faces[:, 2]).any() and not (faces[:, 0] == faces[:, 2]).any():
            assert fwd == _adjacency_numpy(faces), name
        deg[name] = np.diff(ap.astype(np.int64))
        f2, n2 = O.prepare_mesh(verts, faces)
        assert len(f2) <= F and n2.shape == f2.shape, name
    assert (deg["built"] == 3).all() and deg["open"].min() < 3
    assert len(O.prepare_mesh(*big["duplicates"])[0]) == 20480 and len(O.prepare_mesh(*big["duplicates-permuted"])[0]) == 20480
    for tag in ("", "-general"):
        assert (deg["fan49" + tag][:49] == 48).all() and (deg["fan50" + tag][:50] == 49).all()
        assert deg["two_fans" + tag][48] == 96 and np.delete(deg["two_fans" + tag][:97], 48).max() == 48
    assert (deg["fan97"] == 96).all()
    assert (deg["disc129"][:129] == 2).all() and (deg["disc130"][:130] == 2).all()


# Where the oracle alone misses the 2 ulp: the largest distance met, in units of 2^-23, of an oracle normal component from the float64
# normal (measured with the test below).  At 2^-40 the squares of the cross product's components (2^-170) underflow and at 2^40 they
# overflow (2^150) in float32: the length is 0 or infinite, the oracle -- and the device, bit for bit -- return the unnormalised cross
# product or the zero vector, a whole unit vector away.  The coordinates stay normal numbers, the squared length does not.
F1_NORMAL_ULPS = {"scale2^-40": 8387435.634032583, "scale2^40": 8387435.634032583}


def test_row_f1_normals_over_the_exponent_range():
    """the oracle side of the scaled meshes of tests/test_gpu_mesh_stages.py: the oracle's float32 normals (pinned to upstream) against
    a float64 cross product and normalise of the float32 edge vectors, per component, in ulps of a unit vector's components (2^-23;
    2 ulp = the atol = 2e-6 of test_prepare_mesh_restatement restated for unit vectors, eight times tighter).  Measured: 0.992 ulp at
    2^-20 and 2^20, 0.531 ulp translated by 2^20 -- and 8 387 435.634 ulp (0.99986, the whole vector) at 2^-40 and 2^40, see
    F1_NORMAL_ULPS: there the bound is that figure plus one ulp.  At 2^-70 even the cross products are denormal and no unit vector
    comes out of float32 at all: that case is compared between device and oracle only."""
    s = get_scene("tiny")
    for name, (verts, faces) in U.f1_scaled_meshes(s).items():
        f2, n2 = O.prepare_mesh(verts, faces)
        assert np.array_equal(f2, faces), name
        if name == "scale2^-70":
            continue
        ref = U.normals_float64(verts, faces)
        assert np.isfinite(ref).all(), name
        err = np.abs(n2.astype(np.float64) - ref).max() / 2.0 ** -23
        print("f1 normals %-14s max error %.3f ulp" % (name, err))
        assert err <= (F1_NORMAL_ULPS[name] + 1 if name in F1_NORMAL_ULPS else 2), (name, err)


def _f3_cases():
    """(adj_ptr, adj, labels, n_labels) for the row-f3 stage: mesh graphs with few / many labels, one giant
    component, isolated nodes, and a random multigraph with duplicate list entries and high degrees"""
    s = get_scene("tiny")
    F = s.n_faces
    rng = np.random.default_rng(5)
    out = {"three_labels": (s.adj_ptr, s.adj, rng.integers(0, 3, F).astype(np.uint32), 3),
           "noisy": (s.adj_ptr, s.adj, rng.integers(0, 40, F).astype(np.uint32), 41),
           "giant": (s.adj_ptr, s.adj, np.full(F, 2, np.uint32), 3)}
    bands = (np.arange(F) * 7 // F).astype(np.uint32)
    out["bands"] = (s.adj_ptr, s.adj, bands, 9)
    n = 500
    src = rng.integers(0, n, 1500); dst = rng.integers(0, n, 1500)
    lists = [[] for _ in range(n)]
    for a, b in zip(src.tolist(), dst.tolist()):
        if a != b:
            lists[a].append(b); lists[b].append(a)                       # duplicates stay in the lists
    ap = np.zeros(n + 1, np.uint32); ap[1:] = np.cumsum([len(l) for l in lists])
    ad = np.array([g for l in lists for g in l], dtype=np.uint32)
    out["multigraph"] = (ap, ad, rng.integers(0, 2, n).astype(np.uint32), 2)
    out["isolated"] = (np.zeros(6, np.uint32), np.zeros(0, np.uint32), np.array([1, 0, 1, 1, 0], np.uint32), 2)
    return out


def test_get_subgraphs_restatement():
    """uni_graph.cpp:21-55: each label's subgraphs in ascending order of their smallest face, members in BFS queue
    order -- against a pure-Python BFS and scipy's connected components"""
    import collections
    import scipy.sparse as sp
    from scipy.sparse.csgraph import connected_components
    for name, (adj_ptr, adj, labels, n_labels) in _f3_cases().items():
        label_ptr, comp_ptr, comp_faces = O.get_subgraphs(adj_ptr, adj, labels, n_labels)
        F = len(adj_ptr) - 1
        assert sorted(comp_faces.tolist()) == list(range(F)), name
        assert label_ptr[0] == 0 and label_ptr[-1] == len(comp_ptr) - 1 and comp_ptr[-1] == F, name
        want = []
        for L in range(n_labels):
            used = [False] * F
            for i in range(F):
                if labels[i] == L and not used[i]:
                    q = collections.deque([i]); used[i] = True; comp = []
                    while q:
                        u = q.popleft(); comp.append(u)
                        for v in adj[adj_ptr[u]:adj_ptr[u + 1]].tolist():
                            if labels[v] == L and not used[v]:
                                used[v] = True; q.append(v)
                    want.append((L, comp))
        got = []
        for L in range(n_labels):
            for c in range(label_ptr[L], label_ptr[L + 1]):
                got.append((L, comp_faces[comp_ptr[c]:comp_ptr[c + 1]].tolist()))
        assert got == want, name
        rows = np.repeat(np.arange(F), np.diff(adj_ptr.astype(np.int64)))
        keep = labels[rows] == labels[adj] if len(adj) else np.zeros(0, bool)
        g = sp.coo_matrix((np.ones(int(keep.sum())), (rows[keep], adj[keep].astype(np.int64))), shape=(F, F))
        ncc, _ = connected_components(g, directed=False)
        assert ncc == len(comp_ptr) - 1, name


def test_row_f3_cases_past_one_tile_and_one_chunk():
    """the oracle side of tests/test_gpu_mesh_stages.py: thousands of components, components far above the 256 nodes one BFS chunk
    holds, frontiers above 256 nodes with degrees around 20 and duplicate list entries, a star, a path, one label, 70 000 labels --
    against a plain-Python BFS; the cases are what they claim to be"""
    cases = U.f3_large_cases(get_scene("spiky32"))
    seen = {}
    for name, (adj_ptr, adj, labels, n_labels) in cases.items():
        label_ptr, comp_ptr, comp_faces = O.get_subgraphs(adj_ptr, adj, labels, n_labels)
        lp, cp, cf, widest = U.subgraphs_python(adj_ptr, adj, labels, n_labels)
        assert np.array_equal(label_ptr, lp) and np.array_equal(comp_ptr, cp) and np.array_equal(comp_faces, cf), name
        seen[name] = (len(comp_ptr) - 1, int(np.diff(comp_ptr.astype(np.int64)).max()), widest)
    assert seen["noisy40"][0] > 2048 and seen["sparse_labels"][0] > 2048
    assert seen["bands"][1] > 4 * 256 and seen["one_label"] [:2] == (1, 20480)
    assert seen["multigraph"][2] > 256 and seen["multigraph2"][2] > 256
    ap, ad = cases["multigraph"][:2]
    src = np.repeat(np.arange(3000), np.diff(ap.astype(np.int64)))
    assert len(ad) > 55000 and len(set(zip(src.tolist(), ad.tolist()))) < len(ad)                  # degrees around 20, duplicates kept
    assert seen["star"][:2] == (1, 1501) and seen["path"] == (1, 3000, 1)
    lp = O.get_subgraphs(*cases["sparse_labels"])[0]
    assert lp[5] == 0 and lp[69990] == lp[70000] == seen["sparse_labels"][0]


def test_energy_is_within_a_fraction_of_a_percent_of_the_lp_lower_bound():
    """Parity with mapMAP's LABELS cannot be pinned (the library is absent), so pin the QUALITY: a lower bound on the
    minimum energy (LP dual, MPLP in fp64, oracle.cpp orc_mrf_lower_bound) that no solver can beat.  The bound is valid
    (<= the brute-force optimum on tiny instances, where it is also tight) and the solver's labeling is within 0.1 % of
    it on the mesh scenes, 4 % on the 700-view scene where the LP itself is not tight (tests/tools/lower_bound.py: 0.27 %
    at BASELINE config 2 with 4000 rounds, 0.93 % at config 3 with 15 000)."""
    for seed in range(8):
        col_ptr, view_id, cost, adj_ptr, adj = random_mrf(9, 4, 3, 3, seed=40 + seed, p_empty=0.2)
        csr = O.CsrNp(9, 4, col_ptr, view_id, cost)
        opt = brute_force_optimum(col_ptr, view_id, cost, adj_ptr, adj)
        lb, trace = O.lower_bound(csr, adj_ptr, adj, iters=200)
        assert lb <= opt + 1e-9 and (np.diff(trace) >= -1e-9).all(), (seed, lb, opt)     # valid, and MPLP ascends monotonically
    for name, rounds, tol in (("tiny", 200, 1e-3), ("bumpy", 300, 1e-3), ("spiky32", 300, 1e-3), ("mixed", 200, 1e-3), ("manyviews", 300, 4e-2)):
        s = get_scene(name)
        dc, _ = O.data_costs(s)
        _, st = O.view_selection(dc, s.adj_ptr, s.adj)
        lb, _ = O.lower_bound(dc, s.adj_ptr, s.adj, iters=rounds)
        assert lb <= st["energy"] * (1 + 1e-12), name
        assert st["energy"] - lb <= tol * lb, (name, st["energy"], lb)
        e_icm = O.energy(dc, s.adj_ptr, s.adj, O.icm_baseline(dc, s.adj_ptr, s.adj))[0] / 2.0 ** 32
        assert e_icm - lb > 10 * (st["energy"] - lb) or st["energy"] - lb < 1e-6 * lb, name   # the bound separates a good labeling from a greedy one



def test_undistortion_models_row_f4():
    """row f4 (generate_texture_views.cpp:153-165; MVE's image_undistort_k2k4 / _vsfm are absent: DEFINED in oracle.cpp): zero
    first coefficient = copy; otherwise every output pixel samples the source at the distorted position of an independent fp64
    restatement (numpy) -- k2k4 factor 1 + rsq k2 + rsq^2 k4; vsfm: the root of k1 r^3 + r - r_u -- checked on an image whose
    red / green channels ARE the pixel coordinates, so the sampled value reveals the position"""
    h, w, flen = 96, 128, 0.8
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.stack([xx, yy, (xx + yy) // 2], -1).astype(np.uint8)
    assert np.array_equal(O.undistort(img, flen, 0.0, 0.5), img)
    for d0, d1 in ((-0.15, 0.04), (0.1, 0.02), (0.12, 0.0), (-0.1, 0.0)):
        out = O.undistort(img, flen, d0, d1)
        fx = (xx - w / 2.0) / max(w, h); fy = (yy - h / 2.0) / max(w, h)
        if d1 != 0.0:
            rsq = (fx * fx + fy * fy) / flen ** 2
            factor = 1.0 + rsq * d0 + rsq * rsq * d1
        else:
            ru = np.sqrt(fx * fx + fy * fy) / flen
            rd = ru.copy()
            for _ in range(60):
                rd = rd - (d0 * rd ** 3 + rd - ru) / (3 * d0 * rd ** 2 + 1)
            assert np.abs(d0 * rd ** 3 + rd - ru).max() < 1e-12
            factor = np.where(ru > 0, rd / np.maximum(ru, 1e-300), 1.0)
        sx = fx * factor * max(w, h) + w / 2.0; sy = fy * factor * max(w, h) + h / 2.0
        inside = (sx >= -0.5) & (sx <= w - 0.5) & (sy >= -0.5) & (sy <= h - 0.5)
        assert np.array_equal((out == 0).all(axis=2) & ~inside, ~inside)               # outside stays black
        m = inside & (sx > 1) & (sx < w - 2) & (sy > 1) & (sy < h - 2)
        assert np.abs(out[..., 0][m] - sx[m]).max() <= 0.51 and np.abs(out[..., 1][m] - sy[m]).max() <= 0.51   # bilinear of a ramp = the position, rounded
        assert m.mean() > 0.7


@pytest.mark.parametrize("kmax", [1, 5, 64])
def test_label_compression_restatement_against_numpy(kmax):
    """orc_prune_labels (the definition of the `max_labels` option): per face the kmax entries with the smallest (cost, view id)
    pairs, kept in ascending view order -- against a plain numpy lexsort, on a table full of cost ties"""
    rng = np.random.default_rng(7 + kmax)
    V = 300
    lens = np.concatenate([np.array([0, 1, kmax, kmax + 1, 130], dtype=np.int64), rng.integers(0, 120, size=60)])
    col_ptr = np.zeros(len(lens) + 1, dtype=np.uint32); col_ptr[1:] = np.cumsum(lens)
    view_id = np.concatenate([np.sort(rng.choice(V, size=int(n), replace=False)) for n in lens]).astype(np.uint16)
    cost = rng.choice(np.array([0.0, 0.25, 0.5, 0.50000006, 1.0], dtype=np.float32), size=int(col_ptr[-1])).astype(np.float32)
    got = O.prune_labels(O.CsrNp(len(lens), V, col_ptr, view_id, cost), kmax)
    exp_v, exp_c, exp_ptr = [], [], [0]
    for f in range(len(lens)):
        a, b = int(col_ptr[f]), int(col_ptr[f + 1])
        v, c = view_id[a:b], cost[a:b]
        keep = np.sort(np.lexsort((v, c))[:kmax])          # smallest (cost, view id) pairs, back in view order
        exp_v.append(v[keep]); exp_c.append(c[keep]); exp_ptr.append(exp_ptr[-1] + len(keep))
    assert np.array_equal(got.col_ptr, np.array(exp_ptr, dtype=np.uint32))
    assert np.array_equal(got.view_id, np.concatenate(exp_v)) and np.array_equal(got.cost.view(np.uint32), np.concatenate(exp_c).view(np.uint32))


def test_ray_predicate_agrees_with_exact_geometry_away_from_boundaries():
    """the occlusion predicate DEFINED by this repository (Moeller-Trumbore in fp32 with fused multiply-adds, oracle.cpp ray_tri)
    against an fp64 segment / triangle intersection: whenever the exact barycentrics and the exact distance are clear of
    their limits by 1e-4, the boolean is the geometric truth -- also for rays that start ON the triangle's plane neighbours
    (the reference's rays start at mesh vertices) and for both orientations of the triangle"""
    rng = np.random.default_rng(42)
    L = O.load()
    checked = hits = 0
    for _ in range(4000):
        tri = rng.uniform(-1, 1, size=(3, 3)).astype(np.float32)
        if rng.random() < 0.5:
            tri = tri[::-1].copy()                                   # flipped winding: det changes sign
        o = rng.uniform(-2, 2, size=3).astype(np.float32)
        p = rng.uniform(-2, 2, size=3).astype(np.float32)
        a, b, c = (tri[k].astype(np.float64) for k in range(3))
        e1, e2 = b - a, c - a
        d = p.astype(np.float64) - o.astype(np.float64)
        n = np.cross(e1, e2)
        den = float(np.dot(n, d))
        if abs(den) < 1e-3 or np.linalg.norm(n) < 1e-2:
            continue                                                 # nearly parallel or degenerate: not "away from boundaries"
        s = float(np.dot(n, a - o.astype(np.float64))) / den         # hit at o + s d, s in [0, 1] along the segment
        q = o.astype(np.float64) + s * d
        m = np.array([e1, e2]).T
        uv, *_ = np.linalg.lstsq(m, q - a, rcond=None)
        u, v = float(uv[0]), float(uv[1])
        margins = [u, v, 1.0 - u - v, s - 1e-4, 1.0 - s]
        if min(abs(x) for x in margins) < 1e-4:
            continue                                                 # too close to an edge of the triangle or an end of the segment
        truth = all(x > 0 for x in margins)
        verts = np.ascontiguousarray(tri, dtype=np.float32)
        faces = np.array([[0, 1, 2]], dtype=np.uint32)
        normals = np.zeros((1, 3), dtype=np.float32)
        mesh = O.Mesh(3, 1, verts.ctypes.data, faces.ctypes.data, normals.ctypes.data)
        got = L.orc_ray_occluded(None, C.byref(mesh), o.ctypes.data, p.ctypes.data, 1)
        assert bool(got) == truth, (tri, o, p, margins)
        checked += 1; hits += truth
    assert checked > 2500 and 100 < hits < checked - 100


# ---- the oracle half of the crafted ray scenes (tests/util_cases.py ray_*; the GPU half is tests/test_gpu_occlusion_rays.py): the
# ---- conditions that keep the GPU tests from passing vacuously

@pytest.mark.parametrize("name", list(U.ray_scenes()))
def test_crafted_ray_scenes_bvh_equals_brute_force_and_occlusion_decides(name):
    """every crafted ray scene: the oracle's BVH and its brute-force loop give the same pattern and counters, some pairs are culled as
    occluded and some survive, no pair is culled for zero quality (the need bits are derived from the pattern without the rays)"""
    s = U.ray_scenes()[name]()
    a, sa = O.data_costs(s, brute=False)
    b, sb = O.data_costs(s, brute=True)
    assert np.array_equal(a.col_ptr, b.col_ptr) and np.array_equal(a.view_id, b.view_id)
    for k in ("cull_backface", "cull_angle", "cull_outside", "cull_occluded", "cull_zero_quality", "nnz_pre"):
        assert sa[k] == sb[k], k
    assert sa["cull_occluded"] > 0 and a.nnz > 0 and sa["cull_zero_quality"] == 0
    nv, sn = O.data_costs(s, geometric_visibility_test=False)
    assert sn["cull_zero_quality"] == 0 and nv.nnz == a.nnz + sa["cull_occluded"]
    need = U.need_from_pass_pattern(s, nv.col_ptr, nv.view_id)
    occl = U.ray_truth(s, need)
    assert occl.any() and (need & ~occl).any()
    if name.startswith("strip"):
        assert not need[:, s.faces.max() + 1:].any()                       # vertices no face references need no ray
    if name == "octants":
        per_view = np.bincount(a.view_id, minlength=s.n_views)
        assert (per_view > 0).all() and occl.any(axis=1).all() and s.n_views == 8
        d = s.cams["pos"][:, None, :] - s.verts[None, :, :]                 # all rays towards one camera share their three signs
        assert (np.sign(d) == np.sign(s.cams["pos"])[:, None, :]).all() and len({tuple(r) for r in np.sign(s.cams["pos"])}) == 8
    if name == "fence":
        vid = {(int(x), int(y)): k for k, (x, y, z) in enumerate(s.verts[:81])}
        col = [vid[0, y] for y in range(-4, 4)]                                # the ground vertices in the wall's plane that camera 0 needs
        assert need[0, col].all() and (s.cams["pos"][0, 0] - s.verts[col, 0] == 0).all()
        # from (0, -1, 0) and (0, 0, 0) the segment to (0, 4, 3) runs through the wall's area (z = 1.2 / 0.75 at y = 1): in its plane, no hit
        assert not occl[0].any()
        # from behind the wall level with its edge y = 1: the hit lies ON the upright edge and counts
        assert occl[2, [vid[2, 1], vid[4, 1]]].all() and need[1, 81:].all() and not occl[1, 81:].any()
    if name == "confetti":
        assert np.nonzero(occl[0])[0].tolist() == sorted(U.CONFETTI_VERTS) and need[0, list(U.CONFETTI_VERTS)].all()
        assert not occl[1].any() and need[1].sum() > 81
        assert len(s.faces) == 141 and len(s.verts) == 120


def test_ray_terrace_has_exact_zero_components_and_boundary_rays():
    """ray_terrace as built: 136 faces on 90 vertices (a partial last need word); needed rays whose fp32 direction has one and two
    components exactly zero; the rays through the plate's rim, an inner edge, its centre vertex and a shared diagonal are needed, and
    the predicate's brute-force answers for them are recorded here (the GPU must reproduce them, whatever they are)"""
    s = U.ray_terrace()
    assert s.faces.shape == (136, 3) and s.verts.shape == (90, 3) and s.n_views == 10
    assert np.array_equal(s.verts[40], np.float32([0, 0, 0]))
    nv, sn = O.data_costs(s, geometric_visibility_test=False)
    need = U.need_from_pass_pattern(s, nv.col_ptr, nv.view_id)
    occl = U.ray_truth(s, need)
    d = s.cams["pos"][:, None, :] - s.verts[None, :, :]                     # fp32 subtraction, as make_ray forms it
    zeros = (d == 0).sum(axis=2)
    assert (need & (zeros == 1)).sum() >= 40 and (need[:5, :81] & (zeros[:5, :81] == 2)).sum() == 5   # the five vertices under cameras 0 - 4
    # both signs of the non-zero components beside a zero one, and a zero component on every axis but z (no camera is level with the ground)
    for a in (0, 1):
        assert (need & (d[:, :, a] == 0) & (d[:, :, 1 - a] > 0)).any() and (need & (d[:, :, a] == 0) & (d[:, :, 1 - a] < 0)).any()
    vid = {(int(x), int(y)): k for k, (x, y, z) in enumerate(s.verts[:81])}
    # camera 5 at (-2, 0, 2): from the origin the ray meets z = 0.5 at x = -0.5, the plate's rim
    assert need[5, vid[0, 0]] and np.array_equal(s.cams["pos"][5], np.float32([-2, 0, 2]))
    recorded = {"rim": bool(occl[5, vid[0, 0]]), "inner_edge": bool(occl[0, vid[0, 0]]), "centre_vertex": bool(occl[1, vid[1, 0]]),
                "diagonal": bool(occl[2, vid[2, 1]]), "inner_edge_2": bool(occl[3, vid[1, 1]]), "clear": bool(occl[4, vid[-3, -2]])}
    assert all(need[j, vid[xy]] for j, xy in ((0, (0, 0)), (1, (1, 0)), (2, (2, 1)), (3, (1, 1)), (4, (-3, -2))))
    # a hit ON an edge, a corner or the shared diagonal belongs to at least one of the triangles that meet there: the plate has no leak
    assert recorded == {"rim": recorded["rim"], "inner_edge": True, "centre_vertex": True, "diagonal": True, "inner_edge_2": True, "clear": False}
    assert recorded["rim"] is True, recorded
    assert need[9].sum() == 0                                                # level with the plate: the angle cull leaves that view no pair


# ---- crafted MRF instances (util_cases "crafted MRF instances"): every generator's own property, the oracle's per-sweep traces against
# ---- numpy restatements of the tracking energy, the keep-the-best rule and the ICM polish; tests/test_gpu_mrf_crafted.py runs the same
# ---- instances against the GPU

def _mrf_csr(case):
    return O.CsrNp(len(case.col_ptr) - 1, case.n_views, case.col_ptr, case.view_id, case.cost)


def test_crafted_mrf_generators_hold_their_properties():
    """the generators assert what they exist for themselves (classes per the documented rule, colours per the restated greedy colouring,
    tied minima, kinds of neighbouring lists); here they all run, and the planted entries are looked at once more from outside"""
    cases = U.crafted_cases()
    assert len(cases) == 6 + sum(len(U.small_range_counts(c)) for c in range(5))
    assert [U.small_range_counts(c) for c in range(5)] == [[1, 2, 3, 31, 32, 33], [1, 2, 3, 31, 32, 33], [1, 2, 3, 7, 8, 9], [1, 2, 3, 4, 5], [1, 2, 3]]
    for name, build in cases.items():
        case = build()
        F = len(case.col_ptr) - 1
        assert F <= 2500 and int(np.diff(case.col_ptr.astype(np.int64)).max()) <= 257, name
        assert len(case.adj_ptr) == F + 1 and case.view_id.max() < case.n_views
        for i in range(F):                                           # strictly ascending label lists, symmetric adjacency
            assert np.all(np.diff(case.view_id[case.col_ptr[i]:case.col_ptr[i + 1]].astype(np.int64)) > 0)
        src = np.repeat(np.arange(F), np.diff(case.adj_ptr.astype(np.int64)))
        assert sorted(zip(src.tolist(), case.adj.tolist())) == sorted(zip(case.adj.tolist(), src.tolist())), name
    for L, seed in U.TIED_CASES:
        case = U.tied_mrf(L, seed)
        codes = U.cost_codes(case.cost)
        step = np.nonzero((np.diff(codes.astype(np.int64)) == -1) & (np.nextafter(case.cost[1:], np.float32(2.0)) == case.cost[:-1]))[0]
        assert len(step) >= 20, "neighbouring floats on either side of a rounding point"
        same = np.nonzero((codes[:-1] == 0) & (codes[1:] == 0) & (case.cost[:-1] > 0) & (case.cost[1:] == 0))[0]
        assert len(same) >= 5, "equal codes, different costs"
    lo, hi = U.rounding_pair(0)
    assert 0 < lo < hi and U.cost_codes(lo) == 0 and U.cost_codes(hi) == 1 and np.nextafter(lo, np.float32(1)) == hi
    case = U.isolated_mrf()
    first = U.first_min_code_labels(case)
    exact = np.array([0 if a == b else int(case.view_id[a + int(np.argmin(case.cost[a:b]))]) + 1 for a, b in zip(case.col_ptr[:-1], case.col_ptr[1:])], np.uint32)
    assert int((first != exact).sum()) >= 10, "columns whose first smallest CODE is not their smallest cost"


TRACE_CASES = ("tied1", "tied15", "boundary", "isolated")          # the instances whose every sweep the GPU is compared on
TRACE_PARAMS = dict(max_sweeps=16, min_sweeps=16)                  # 16 sweeps: four damped ones


@pytest.mark.parametrize("name", TRACE_CASES)
def test_mrf_traces_agree_with_numpy_restatements(name):
    """the decode trace against restatements that owe the oracle nothing: every sweep's tracking energy = the 16-bit codes of the traced
    labels + 65535 per cut edge; the traced best labeling = the decode of the FIRST sweep that reached the smallest energy so far; the
    final labels = the restated ICM polish of the last best labeling (and that labeling itself without a polish); an instance without
    model edges decodes the first smallest code in every sweep"""
    case = U.crafted_cases()[name]()
    csr = _mrf_csr(case)
    labels, st, tr = O.view_selection_traced(csr, case.adj_ptr, case.adj, O.default_mrf_params(**TRACE_PARAMS), n_sweeps=16)
    assert st["sweeps"] == 16 and tr["lab"].shape == (16, csr.n_faces)
    kept = 0
    for s in range(16):
        assert U.tracking_energy_numpy(case, tr["lab"][s]) == int(tr["energy"][s]), "sweep %d" % (s + 1)
        if tr["energy"][s] < tr["energy"][kept]: kept = s
        assert np.array_equal(tr["best"][s], tr["lab"][kept]), "sweep %d: the kept labeling is not sweep %d's" % (s + 1, kept + 1)
    polished, its = U.icm_numpy(case, tr["best"][-1], 50)
    assert np.array_equal(labels, polished) and st["icm_iters"] == its
    assert energy_numpy(case.col_ptr, case.view_id, case.cost, case.adj_ptr, case.adj, labels) == (st["energy_fixed"], st["cut_edges"])
    l0, s0 = O.view_selection(csr, case.adj_ptr, case.adj, O.default_mrf_params(icm_iters=0, **TRACE_PARAMS))
    assert np.array_equal(l0, tr["best"][-1]) and s0["icm_iters"] == 0
    l1, s1 = O.view_selection(csr, case.adj_ptr, case.adj, O.default_mrf_params(**TRACE_PARAMS))
    assert np.array_equal(l1, labels) and s1 == {**st, "t_setup": s1["t_setup"], "t_solve": s1["t_solve"]}, "the trace changes what the solver computes"
    if name == "isolated":
        assert np.all(tr["lab"] == U.first_min_code_labels(case)[None, :])


def test_best_sweep_tie_instance_has_a_tied_sweep():
    """BEST_TIE_CASE under the "best_tie" parameters: some sweep's tracking energy EQUALS the best so far while its labeling differs from
    the kept one -- "keep the best" with `<=` for `<` would end on another labeling; without a polish nothing repairs that"""
    case = U.tied_mrf(*U.BEST_TIE_CASE)
    labels, st, tr = O.view_selection_traced(_mrf_csr(case), case.adj_ptr, case.adj, O.default_mrf_params(**U.CRAFTED_PARAMS["best_tie"]), n_sweeps=40)
    e = tr["energy"]
    assert st["sweeps"] == 40 and len(e) == 40
    tied = [s for s in range(1, 40) if e[s] == e[:s].min() and not np.array_equal(tr["lab"][s], tr["best"][s])]
    assert tied, "no sweep ties the best energy with another labeling: search another seed"
    assert np.array_equal(labels, tr["best"][-1]) and not np.array_equal(labels, tr["lab"][tied[-1]])
    assert int(e.min()) == U.tracking_energy_numpy(case, labels)


def test_plateau_parameters_run_every_sweep():
    """min_improvement = 0: `improvement < 0 * previous` is never true, so the stop rule's strict `<` runs all 40 sweeps on every crafted
    instance -- although each of them sits on a plateau (no improvement over a window) long before"""
    for name in ("tied1", "tied3", "tied15", "tied255", "boundary", "isolated"):
        case = U.crafted_cases()[name]()
        labels, st, tr = O.view_selection_traced(_mrf_csr(case), case.adj_ptr, case.adj, O.default_mrf_params(**U.CRAFTED_PARAMS["plateau"]), n_sweeps=40)
        best = np.minimum.accumulate(tr["energy"])
        assert st["sweeps"] == 40 and any(best[s] == best[s - 5] for s in range(6, 40)), name


# ---- region moves on crafted instances (util_cases "region moves on crafted instances"): the oracle's rounds against a third statement
# ---- written from the rule text (region_round_numpy), the instances' own properties, a witness per rule that the instances can tell the
# ---- rule from its inversion, and the tie counts the GPU tests rely on; tests/test_gpu_mrf_regions.py runs the same instances on the GPU

REGION_CASES = {**U.crafted_cases(), **U.region_cases()}
REGION_START = U.CRAFTED_REGION_PARAMS["start"]


@pytest.mark.parametrize("name", list(REGION_CASES))
def test_region_rounds_agree_with_the_rule_text_round_by_round(name):
    """from the argmin-unary labeling ("start": no sweep, a polish of zero iterations), for r = 1, 2, ..: the oracle's labels after r region
    rounds are the model's, its move count the model's, and its energy has dropped by exactly the sum of the gains of the regions the
    model moved; with region_rounds = 8 it runs as many rounds as the model finds moves in"""
    case = REGION_CASES[name]()
    csr = _mrf_csr(case)
    start = U.argmin_labels(case)
    l0, s0 = O.view_selection(csr, case.adj_ptr, case.adj, O.default_mrf_params(**{**REGION_START, "region_rounds": 0}))
    assert np.array_equal(l0, start) and (s0["region_rounds"], s0["region_moves"]) == (0, 0)
    assert energy_numpy(case.col_ptr, case.view_id, case.cost, case.adj_ptr, case.adj, start) == (s0["energy_fixed"], s0["cut_edges"])
    rounds = U.region_rounds_numpy(case, start, REGION_START["region_rounds"])
    energy, moves = s0["energy_fixed"], 0
    for r, (lab, moved, _) in enumerate(rounds, 1):
        lo, so = O.view_selection(csr, case.adj_ptr, case.adj, O.default_mrf_params(**{**REGION_START, "region_rounds": r}))
        energy -= sum(g for _, g in moved.values()); moves += len(moved)
        assert all(g > 0 for _, g in moved.values())
        assert np.array_equal(lo, lab), "round %d: %d labels differ from the model's, first at node %d" % (r, int((lo != lab).sum()), int(np.nonzero(lo != lab)[0][0]))
        assert (so["region_rounds"], so["region_moves"], so["energy_fixed"]) == (r, moves, energy), "round %d" % r
        assert energy_numpy(case.col_ptr, case.view_id, case.cost, case.adj_ptr, case.adj, lab)[0] == energy
    lo, so = O.view_selection(csr, case.adj_ptr, case.adj, O.default_mrf_params(**REGION_START))
    assert so["region_rounds"] == len(rounds) and so["region_moves"] == moves and so["energy_fixed"] == energy
    if rounds: assert np.array_equal(lo, rounds[-1][0])


# rule -> (instance, the inversion): the model with that ONE rule inverted ends round 1 on other labels -- an implementation that has the
# rule the other way round cannot pass on that instance
REGION_WITNESSES = [
    ("label_tie", "hub65_wnone_aligned", dict(label_tie="larger")), ("label_tie", "tied1", dict(label_tie="larger")),
    ("name_tie", "chain", dict(name_tie="larger")), ("name_tie", "tied1", dict(name_tie="larger")),
    ("name", "tied1", dict(name="position", order="reversed")), ("name", "chain", dict(name="position", order="reversed")),
    ("name", "tied3", dict(name="position", order="random")),
    ("zero_gain_moves", "large_zero", dict(zero_gain_moves=True)), ("zero_gain_moves", "tied1", dict(zero_gain_moves=True)),
    ("ignore_lacking", "large_lacking", dict(ignore_lacking=True)), ("ignore_lacking", "tied1", dict(ignore_lacking=True)),
]


@pytest.mark.parametrize("rule,name,inverted", REGION_WITNESSES, ids=["%s-%s" % (r, n) for r, n, _ in REGION_WITNESSES])
def test_region_rule_witnesses(rule, name, inverted):
    case = REGION_CASES[name]()
    start = U.argmin_labels(case)
    rules = dict(inverted)
    if "order" in rules: rules["order"] = U.table_orders(len(start))[rules["order"]]
    good = U.region_round_numpy(case, start)[0]
    bad = U.region_round_numpy(case, start, rules)[0]
    assert int((good != bad).sum()) > 0, "inverting %s changes nothing on %s" % (rule, name)
    if rule == "name":      # under the identity positions ARE names
        assert np.array_equal(U.region_round_numpy(case, start, dict(name="position", order=U.table_orders(len(start))["identity"]))[0], good)


def test_every_invertible_region_rule_has_a_witness():
    assert {r for r, _, _ in REGION_WITNESSES} == set(U.REGION_RULES)


def test_region_tie_material_of_the_crafted_instances():
    """conditions the GPU tests rest on, on tied1 from the argmin start (measured: 404 / 35 / 739 / 2834 and 408 tied edges in all; tied3:
    440 of 446 edges, 96 label ties): enough tied directed cut edges that positions in reversed order would decide differently from
    names, enough label ties, zero-gain candidates and lacking candidates; the hubs have nc candidates, region_large 700 faces in a region"""
    case = REGION_CASES["tied1"]()
    F = len(case.col_ptr) - 1
    cnt = U.region_round_numpy(case, U.argmin_labels(case), dict(order=U.table_orders(F)["reversed"]))[2]
    assert cnt["tied_edges_flipped"] >= 100 and cnt["label_ties"] >= 20 and cnt["zero_gain"] >= 100 and cnt["lacking"] >= 1000, cnt
    assert U.region_round_numpy(case, U.argmin_labels(case), dict(order=U.table_orders(F)["identity"]))[2]["tied_edges_flipped"] == 0
    assert max(U.region_round_numpy(c, U.argmin_labels(c))[2]["max_candidates"] for c in (b() for n, b in U.crafted_cases().items())) < 64, "the existing instances never reach the second chunk"
    for nc in U.REGION_HUB_NC:
        case = U.region_hub(nc, 0, "aligned")
        assert U.region_round_numpy(case, U.argmin_labels(case))[2]["max_candidates"] == nc
    case = U.region_large("moves")
    assert U.region_round_numpy(case, U.argmin_labels(case))[2]["max_region"] >= 700
    assert sorted(len(o) for o in U.table_orders(7).values()) == [7, 7, 7] and all(sorted(o.tolist()) == list(range(7)) for o in U.table_orders(7).values())
