"""Row f6 on the CPU: the model of the texture patches and TexturePatch::adjust_colors (tests/tools/patch_model.cpp, sequential, as
upstream's loop is written) against the pins recorded from upstream's own compiled adjust_colors (tests/golden/texture_patch_pins.npz),
against a numpy statement of the order-free rule the device uses, and against invariants of the definition (DESIGN.md section 4
"Texture patches"); plus the library's new exports.

What the crafted set shows about the crop's fill colour: a frame that starts at -1 has a magenta column, and upstream's loop DOES
make some of those pixels valid -- as near-only pixels (blending 64: a corner at pixel x in [0, 0.41) is within sqrt(2) of column -1).
It never makes them inside pixels (upstream asserts x != 0 && y != 0 there); both facts are asserted from the model's counters."""
import os

import numpy as np
import pytest

import mvs_texturing_amd as M
import patch_model as PM
import seam_model as SM
from conftest import get_scene

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "texture_patch_pins.npz")
U = float(2.0 ** -24)   # unit roundoff of fp32


@pytest.fixture(scope="module", autouse=True)
def _models_built():
    SM.build(); PM.build()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32).ravel()


def crafted_set():
    """name -> (scene, labels): grids with a fin, a zero-length edge and frames at -1; an island whose candidate is absorbed"""
    out = {}
    for name, kw in (("grid", dict()), ("grid_fin_zero", dict(fin=True, zero_edge=True)), ("grid9", dict(n=9, fin=True))):
        g = SM.grid_scene(**kw)
        out[name] = (g, SM.grid_labels(g))
    out["island"] = PM.island_scene()
    return out


# The label-1 patch's face list of PM.nested_scene(order) as blocks of whole regions, derived by hand from the merge loop (DESIGN.md
# section 4 item 3: "scan in order, a candidate whose box lies inside another's of its label is absorbed, its list appended"; the boxes
# nest outer > annulus > core; candidates c0 < c1 < c2 are `order`; i runs over the living candidates, j over all others, both ascending):
NESTED_LISTS = {
    # i = outer takes annulus, then core.
    ("outer", "annulus", "core"): ("outer", "annulus", "core"),
    # i = outer takes core (j = 1), then annulus (j = 2).
    ("outer", "core", "annulus"): ("outer", "core", "annulus"),
    # i = annulus: outer does not fit, core does -> [annulus, core]; i = outer takes that list whole (a chain, the absorber is later).
    ("annulus", "outer", "core"): ("outer", "annulus", "core"),
    # i = annulus takes core; core is dead; i = outer takes [annulus, core] (a chain, the absorber is later).
    ("annulus", "core", "outer"): ("outer", "annulus", "core"),
    # i = core takes nothing; i = outer takes core (j = 0, the absorber is later), then annulus (j = 2).
    ("core", "outer", "annulus"): ("outer", "core", "annulus"),
    # i = core takes nothing; i = annulus takes core (later); i = outer: core is dead, takes [annulus, core] (a chain, later).
    ("core", "annulus", "outer"): ("outer", "annulus", "core"),
}
NESTED_SIZES = {"outer": 176, "annulus": 80, "core": 2}   # faces: 2 (13^2 - 9^2), 2 (7^2 - 3^2), 2


def nested_set():
    """name -> (scene, labels): PM.nested_scene in the six candidate orders and PM.equal_box_scene"""
    out = {"nested_" + "_".join(o): PM.nested_scene(o)[:2] for o in PM.NESTED_ORDERS}        # lowest candidate first
    out["equal_boxes"] = PM.equal_box_scene()
    return out


def corner_values(scene, seed=11, amp=0.06):
    """per-corner adjustments as row f5 would hand them over: one value per (vertex, label), so faces of a patch agree on shared corners"""
    rng = np.random.default_rng(seed)
    per = rng.normal(0, amp, (len(scene.verts), len(scene.images) + 1, 3)).astype(np.float32)
    return per


def corner_adjust(scene, labels, seed=11):
    per = corner_values(scene, seed)
    ca = per[scene.faces.astype(np.int64), np.asarray(labels, np.int64)[:, None]]      # (F, 3, 3)
    ca[np.asarray(labels) == 0] = 0
    return np.ascontiguousarray(ca, np.float32)


def test_library_exports_and_ctypes_table():
    import ctypes as C
    assert os.path.exists(M.lib_path()), "build the library first (__graft_entry__.build)"
    raw = C.CDLL(M.lib_path())
    L = M.load_library()
    for name in ("mvs_ctx_texture_patches", "mvs_patch_default_params", "mvs_patch_set_free"):
        assert hasattr(raw, name), name
        assert name in L._declared and getattr(L, name).argtypes is not None, name
    p = M.default_patch_params()
    assert p.max_pixels == 0
    assert M.default_patch_params(max_pixels=5).max_pixels == 5
    assert callable(M.texture_patches) and callable(M.patch_view) and hasattr(M.Context, "texture_patches")


def test_model_equals_upstream_pins():
    z = np.load(GOLDEN)
    W, H = [int(v) for v in z["wh"]]
    n = int(z["n_cases"])
    assert n == 30
    seen = dict(inside_twice=0, near_then_inside=0, degenerate=0)
    for k in range(n):
        img = z["img%02d" % k].astype(np.float32) / np.float32(255.0)
        got, val, bl, cnt = PM.adjust_colors(W, H, img, z["tc%02d" % k], z["adj%02d" % k])
        assert np.array_equal(_bits(got), _bits(z["out%02d" % k])), k
        assert np.array_equal(val, z["val%02d" % k]) and np.array_equal(bl, z["bl%02d" % k]), k
        assert cnt["clamped"] == 0
        for key in seen:
            seen[key] += cnt[key]
        ri, rv, rb = PM.rule_adjust_colors(W, H, img, z["tc%02d" % k], z["adj%02d" % k])      # the rule against upstream directly
        assert np.array_equal(_bits(ri), _bits(z["out%02d" % k])) and np.array_equal(rv, z["val%02d" % k]) and np.array_equal(rb, z["bl%02d" % k]), k
    assert all(v > 0 for v in seen.values()), seen


def _rule_on_model(scene, arrays, ca):
    """the numpy rule patch by patch on the model's geometry: asserts image / validity / blending equal the model's"""
    P = len(arrays["label"])
    box = arrays["box"].reshape(-1, 4)
    for i in range(P):
        img, val, bl = PM.patch(arrays, i)
        e0, e1 = int(arrays["face_ptr"][i]), int(arrays["face_ptr"][i + 1])
        adj = ca[arrays["faces"][e0:e1]] if ca is not None else np.zeros((e1 - e0, 3, 3), np.float32)
        ri, rv, rb = PM.rule_adjust_colors(int(box[i, 2]), int(box[i, 3]), PM.crop(scene, int(arrays["label"][i]), box[i]),
                                           arrays["texcoords"].reshape(-1, 6)[e0:e1], adj)
        assert np.array_equal(rv, val) and np.array_equal(rb, bl), i
        assert np.array_equal(_bits(ri), _bits(img)), i


def test_model_equals_the_order_free_rule_and_the_cases_are_not_vacuous():
    total = {k: 0 for k in PM.COUNTERS}
    for name, (g, labels) in crafted_set().items():
        for ca in (corner_adjust(g, labels), None):
            st, arrays, stats, cnt = PM.run_scene(g, labels, ca)
            assert st == 0, name
            _rule_on_model(g, arrays, ca)
        for k in total:
            total[k] += cnt[k]
        assert cnt["clamped"] == 0 and cnt["magenta_inside"] == 0, (name, cnt)
    assert total["absorbed"] >= 1, total              # a candidate absorbed by the merge
    assert total["inside_twice"] >= 1, total          # a pixel inside two faces of one list
    assert total["near_then_inside"] >= 1, total      # a pixel a near face reached before an inside face
    assert total["degenerate"] >= 1, total            # a face adjust_colors skips
    assert total["frame_negative"] >= 1, total        # a patch whose frame starts at -1
    assert total["magenta"] >= 1 and total["magenta_near"] >= 1, total   # ... its fill colour reaches near-only pixels, never inside ones


def test_nested_scene_as_the_grid_is_built():
    g, labels, region = PM.nested_scene()
    assert len(g.faces) == 338
    st, arrays, stats, cnt = PM.run_scene(g, labels)
    assert st == 0 and stats["patches"] == 2 and stats["merged"] == 3 and stats["pixels"] == 10840
    assert arrays["face_ptr"].tolist() == [0, 258, 338] and arrays["label"].tolist() == [1, 2]
    assert arrays["box"].reshape(-1, 4)[0, :2].tolist() == [-1, -1] and cnt["frame_negative"] == 1
    p = M.synth.permute_scene(g, seed=5)                              # a random renumbering gives the same patches
    st, shuffled, sstats, _ = PM.run_scene(p, labels[p.face_perm])
    assert all(sstats[k] == stats[k] for k in PM.STATS) and np.array_equal(shuffled["box"], arrays["box"]) and np.array_equal(shuffled["face_ptr"], arrays["face_ptr"])


def _blocks(ids):
    """the runs of equal values in ids: [(value, length)]"""
    ids = np.asarray(ids)
    cut = np.flatnonzero(np.diff(ids)) + 1
    return [(int(ids[a]), int(b - a)) for a, b in zip(np.r_[0, cut], np.r_[cut, len(ids)])]


def check_nested_list(order, region, arrays):
    """the label-1 patch's face list (the model's or the library's) is NESTED_LISTS[order], region by region; the label-2 patch lists the
    outer ring, then the inner one, whichever came first"""
    assert arrays["label"].tolist() == [1, 2] and arrays["face_ptr"].tolist() == [0, 258, 338], order
    faces = arrays["faces"]
    want = [(PM.NESTED_REGIONS.index(r), NESTED_SIZES[r]) for r in NESTED_LISTS[tuple(order)]]
    assert _blocks(region[faces[:258]]) == want, (order, _blocks(region[faces[:258]]))
    assert _blocks(region[faces[258:]]) == [(3, 64), (4, 16)], order


def test_nested_orders_give_the_lists_derived_by_hand():
    assert set(NESTED_LISTS) == set(PM.NESTED_ORDERS) and len(PM.NESTED_ORDERS) == 6
    for order in PM.NESTED_ORDERS:
        g, labels, region = PM.nested_scene(order)
        lowest = [int(np.flatnonzero(region == PM.NESTED_REGIONS.index(r)).min()) for r in order]
        assert lowest == sorted(lowest) and lowest[0] == 0, (order, lowest)      # the candidate order asked for
        st, arrays, stats, _ = PM.run_scene(g, labels)
        assert st == 0 and stats["patches"] == 2 and stats["merged"] == 3 and stats["pixels"] == 10840, (order, stats)
        check_nested_list(order, region, arrays)


def test_nested_set_reaches_chains_later_absorbers_and_equal_boxes():
    total = {k: 0 for k in PM.COUNTERS}
    for name, (g, labels) in nested_set().items():
        for ca in (corner_adjust(g, labels), None):
            st, arrays, stats, cnt = PM.run_scene(g, labels, ca)
            assert st == 0, name
            _rule_on_model(g, arrays, ca)
        for k in total:
            total[k] += cnt[k]
        assert cnt["clamped"] == 0 and cnt["magenta_inside"] == 0, (name, cnt)
        if name == "equal_boxes":
            box = arrays["box"].reshape(-1, 4)
            assert cnt["equal_boxes"] >= 1 and stats["patches"] == 2 and np.array_equal(box[0], box[1]), (cnt, box)
    assert total["chain"] >= 2, total                 # an absorbed candidate that had absorbed others: cand_pos sums several offsets
    assert total["absorber_later"] >= 2, total        # the absorber comes after what it absorbs (j < i)
    assert total["equal_boxes"] >= 1, total           # two candidates with the same box: the earlier one absorbs
    print("nested set counters:", total)


def _strictly_inside(tc):
    """(ys, xs) of the integer pixels certainly inside the triangle tc (3, 2) in fp32: float64 barycentrics above the fp32 evaluation
    error -- each numerator is a sum of two products of differences (relative error u each), so it is off by at most
    4 u (|t1| + |t2|) <= 8 u (s + 2)^2 for a triangle of extent s and a pixel of its range; gamma = 1 - alpha - beta adds both and 2 u"""
    t = tc.astype(np.float64)
    s = float(np.ptp(t, axis=0).max())
    det = (t[0, 0] - t[2, 0]) * (t[1, 1] - t[2, 1]) - (t[0, 1] - t[2, 1]) * (t[1, 0] - t[2, 0])
    if det == 0:
        return np.zeros(0, int), np.zeros(0, int)
    m = 2 * 8 * U * (s + 2) ** 2 / abs(det) + 4 * U
    x0, y0 = np.floor(t.min(0)).astype(int); x1, y1 = np.ceil(t.max(0)).astype(int)
    Y, X = np.meshgrid(np.arange(y0, y1 + 1), np.arange(x0, x1 + 1), indexing="ij")
    a = ((t[1, 1] - t[2, 1]) * (X - t[2, 0]) + (t[2, 0] - t[1, 0]) * (Y - t[2, 1])) / det
    b = ((t[2, 1] - t[0, 1]) * (X - t[2, 0]) + (t[0, 0] - t[2, 0]) * (Y - t[2, 1])) / det
    ok = (a > m) & (b > m) & (1 - a - b > m)
    return Y[ok], X[ok]


def check_invariants(scene, labels, arrays, stats, zero_arrays=None):
    """the invariants of the definition on one patch set (the model's or the library's host arrays).  zero_arrays: the set computed with
    no adjustment, when `arrays` was computed with one (unused here; see test_constant_adjustment)"""
    val, bl, img = arrays["validity"], arrays["blending"], arrays["image"].reshape(-1, 3)
    assert set(np.unique(val)) <= {0, 255} and set(np.unique(bl)) <= {0, 64, 255}
    assert np.array_equal(bl == 0, val == 0)
    assert not np.any(img[val == 0])
    assert stats["pixels"] == len(val) == int(arrays["pix_ptr"][-1]) and stats["valid_pixels"] == int((val == 255).sum())
    assert stats["near_pixels"] == int((bl == 64).sum()) and stats["listed_faces"] == int((np.asarray(labels) != 0).sum())
    assert sorted(arrays["faces"].tolist()) == np.nonzero(np.asarray(labels))[0].tolist()          # every labelled face listed once
    box = arrays["box"].reshape(-1, 4)
    eps = np.float32(np.finfo(np.float32).eps)
    for i in range(len(arrays["label"])):
        pimg, pval, pbl = PM.patch(arrays, i)
        assert np.all(np.asarray(labels)[arrays["faces"][arrays["face_ptr"][i]:arrays["face_ptr"][i + 1]]] == arrays["label"][i])
        for e in range(int(arrays["face_ptr"][i]), int(arrays["face_ptr"][i + 1])):
            tc = arrays["texcoords"].reshape(-1, 3, 2)[e]
            u, v = tc[1] - tc[0], tc[2] - tc[0]
            if np.float32(0.5) * np.abs(np.float32(u[0] * v[1]) - np.float32(u[1] * v[0])) < eps:
                continue
            ys, xs = _strictly_inside(tc)
            assert np.all(pbl[ys, xs] == 255), (i, e)


@pytest.mark.parametrize("name", ["tiny", "bumpy", "grid", "grid_fin_zero", "island", "nested_annulus_core_outer", "equal_boxes"])
def test_invariants_and_patch_counts(name):
    if name in ("tiny", "bumpy"):
        s = get_scene(name)
        cases = SM.crafted_labelings(s)
        if name == "bumpy":
            cases = {k: cases[k] for k in ("random", "random_with_unseen")}
    elif name == "equal_boxes" or name.startswith("nested_"):
        s, labels = nested_set()[name]
        cases = {"crafted": labels}
    else:
        s, labels = crafted_set()[name]
        cases = {"crafted": labels}
        if name == "grid":
            cases.update(SM.crafted_labelings(s))
    for lname, labels in cases.items():
        st, zero, zstats, _ = PM.run_scene(s, labels, None)
        assert st == 0
        sst = SM.run_scene(s, labels, max_iterations=0)[2]
        assert zstats["patches"] == sst["patches"] and zstats["merged"] == sst["merged"], (lname, zstats, sst)
        check_invariants(s, labels, zero, zstats)
        # zero adjustments leave valid pixels equal to the crop
        box = zero["box"].reshape(-1, 4)
        for i in range(len(zero["label"])):
            pimg, pval, _ = PM.patch(zero, i)
            cr = PM.crop(s, int(zero["label"][i]), box[i])
            assert np.array_equal(_bits(pimg[pval == 255]), _bits(cr[pval == 255])), (lname, i)
        st, adj, astats, _ = PM.run_scene(s, labels, corner_adjust(s, labels))
        check_invariants(s, labels, adj, astats)
        for k in ("validity", "blending", "texcoords", "faces", "box", "pix_ptr", "face_ptr", "label"):
            assert np.array_equal(adj[k], zero[k]), k          # the adjustment changes the image only


def constant_bound(c, w, image_c):
    """|image_c - crop - c| for adj = fl(fl(fl(c a) + fl(c b)) + fl(c g)), g = fl(fl(1 - a) - b), image_c = fl(crop + adj), u = 2^-24:
    exactly a + b + (1 - a - b) = 1, so adj - c = c (g - g_exact) + the roundings: |g - g_exact| <= u (|1 - a| + |g|) (two
    subtractions), three products u |c| (|a| + |b| + |g|), the first sum u |c| (|a| + |b|), the second u |c| (|a| + |b| + |g|), the
    final add u |image_c|; (1 + 2^-20) covers the second-order terms of at most five nested roundings ((1 + u)^5 - 1 - 5 u < 2^-20 * 5 u)."""
    a, b, g = [np.abs(w[..., k].astype(np.float64)) for k in range(3)]
    one_minus_a = np.abs(1.0 - w[..., 0].astype(np.float64))
    s = a + b + g
    return (abs(float(c)) * U * (one_minus_a + g + s + (a + b) + s) + U * np.abs(image_c.astype(np.float64))) * (1 + 2.0 ** -20)


def check_constant_adjustment(scene, labels, run):
    """run(corner_adjust) -> arrays.  A constant c on all corners moves every valid pixel by c up to constant_bound."""
    zero = run(None)
    c = np.float32([0.0625, -0.03, 0.11])
    ca = np.zeros((len(scene.faces), 3, 3), np.float32); ca[:] = c
    got = run(ca)
    assert np.array_equal(got["validity"], zero["validity"]) and np.array_equal(got["blending"], zero["blending"])
    box = zero["box"].reshape(-1, 4)
    checked = 0
    for i in range(len(zero["label"])):
        e0, e1 = int(zero["face_ptr"][i]), int(zero["face_ptr"][i + 1])
        w, h = int(box[i, 2]), int(box[i, 3])
        _, rv, _, idx, wts = PM.rule_adjust_colors(w, h, np.zeros((h, w, 3), np.float32), zero["texcoords"].reshape(-1, 6)[e0:e1],
                                                   np.zeros((e1 - e0, 3, 3), np.float32), return_weights=True)
        gi, gv, _ = PM.patch(got, i); zi, _, _ = PM.patch(zero, i)
        assert np.array_equal(rv, gv)
        ok = gv == 255
        for ch in range(3):
            err = np.abs(gi[..., ch].astype(np.float64) - zi[..., ch].astype(np.float64) - float(c[ch]))
            assert np.all(err[ok] <= constant_bound(c[ch], wts, gi[..., ch])[ok]), (i, ch, float(err[ok].max()))
        checked += int(ok.sum())
    assert checked > 0


@pytest.mark.parametrize("name", ["tiny", "grid_fin_zero", "island"])
def test_constant_adjustment(name):
    if name == "tiny":
        s = get_scene(name); labels = SM.crafted_labelings(s)["random"]
    else:
        s, labels = crafted_set()[name]
    check_constant_adjustment(s, labels, lambda ca: PM.run_scene(s, labels, ca)[1])


def test_labeling_errors_of_the_model():
    g = SM.grid_scene()
    assert PM.run_scene(g, np.full(len(g.faces), 3, np.uint32))[0] == 4
    o = SM.grid_scene(outside=True)
    assert PM.run_scene(o, SM.grid_labels(o))[0] == 4
    st, arrays, stats, _ = PM.run_scene(g, np.zeros(len(g.faces), np.uint32))
    assert st == 0 and stats["patches"] == 0 and stats["pixels"] == 0 and len(arrays["image"]) == 0
