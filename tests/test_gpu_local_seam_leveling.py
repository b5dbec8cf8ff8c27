"""Row f7 on the GPU: Context.local_seam_leveling equals the CPU model (tests/tools/blend_model.cpp: upstream's loops, the solve of
DESIGN.md section 4 "Local seam leveling") bit for bit on image, validity and the prepared blending mask and on every counter -- the
suite's scenes (labels from the library's own view selection, patches from its rows f5 and f6), shuffled meshes, the crafted sets of
tests/test_local_seam_model.py, the nested set of tests/test_patch_model.py (merge chains, equal boxes) and config 2; with the default parameters and with max_iterations = 0 (the state before the solve);
the patch sets of tests/golden/local_seam_pins.npz against what upstream's compiled local_seam_leveling left for them; and the
edge sets of tests/test_local_seam_model.py (skipped pairs, sanitized pixels, an idle channel, the ladder of unknown counts) with
iteration caps, tolerances and strip widths moved, on the LDS path and in global memory."""
import numpy as np
import pytest

import mvs_texturing_amd as M
import blend_model as BM
import patch_model as PM
import seam_model as SM
from conftest import get_scene
from test_patch_model import nested_set
from test_local_seam_model import EDGE_REACHES, crafted_sets, edge_sets, ladder_sets, mid_cap, pin_cases, unknown_counts

pytestmark = pytest.mark.gpu

KEYS = ("image", "validity", "blending")


@pytest.fixture(scope="module", autouse=True)
def _models_built():
    SM.build(); PM.build(); BM.build()


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


def _raw(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32).ravel() if a.dtype == np.float32 else a.ravel()


def _same(got, want, what=""):
    for k in KEYS:
        assert got[k].size == want[k].size and np.array_equal(_raw(got[k]), _raw(want[k])), (what, k)


def _compare(s, labels, pa, ctx=None, what="", **params):
    """one GPU run on the patch set pa against the model; returns (gpu arrays, gpu stats, model arrays, model stats)"""
    st, want, wst, _ = BM.run_scene(s, labels, pa, **params)
    assert st == 0
    c = ctx or _ctx(s)
    try:
        got, gst = c.local_seam_leveling(s.adj_ptr, s.adj, np.ascontiguousarray(labels, np.uint32), pa, M.default_lsl_params(**params))
    finally:
        if ctx is None:
            c.close()
    _same(got, want, what)
    for k in BM.STATS:
        assert gst[k] == wst[k], (what, k, gst[k], wst[k])
    assert np.float32(gst["error_max"]).view(np.uint32) == np.float32(wst["error_max"]).view(np.uint32), (what, gst["error_max"], wst["error_max"])
    return got, gst, want, wst


def _pipeline_patches(s, labels):
    """rows f5 and f6 of the library on the host"""
    c = _ctx(s)
    gsl, _ = c.global_seam_leveling(s.adj_ptr, s.adj, labels)
    pa, _ = c.texture_patches(s.adj_ptr, s.adj, labels, gsl["corner_adjust"])
    c.close()
    return pa


@pytest.mark.parametrize("name", ["tiny", "bumpy", "oddw", "mixed", "spiky", "close", "manyviews"])
def test_scenes_equal_the_model(name):
    s = get_scene(name)
    labels = _library_labels(name, s)
    pa = _pipeline_patches(s, labels)
    got, gst, _, _ = _compare(s, labels, pa, what=name)
    assert gst["strip_pixels"] > 0 and gst["seam_edges"] > 0 and gst["iterations_total"] > 0 and gst["hit_max_iterations"] == 0
    assert gst["outside_frame"] == 0 and gst["demoted"] == 0 and gst["skipped_pairs"] == 0, gst
    _compare(s, labels, pa, what=name + "/no solve", max_iterations=0)


@pytest.mark.parametrize("name", ["tiny", "bumpy"])
def test_shuffled_scenes_equal_the_model(name):
    s = get_scene(name)
    p = M.synth.permute_scene(s, seed=7)
    labels = _library_labels(name, s)[p.face_perm]
    _compare(p, labels, _pipeline_patches(p, labels), what=name + "/shuffled")


def test_crafted_sets_equal_the_model():
    for name, (g, labels, pa) in crafted_sets().items():
        got, gst, _, _ = _compare(g, labels, pa, what=name)
        assert gst["hit_max_iterations"] == 0
        _compare(g, labels, pa, what=name + "/no solve", max_iterations=0)
        if name == "outside_frame":
            assert gst["outside_frame"] > 0
        if name == "demoted":
            assert gst["demoted"] > 0


def test_nested_set_equals_the_model():
    """patches whose lists were merged through chains, in all six candidate orders, and two patches of one frame: rows f5 and f6 of the
    library give the set, this row equals its model on it"""
    for name, (g, labels) in nested_set().items():
        pa = _pipeline_patches(g, labels)
        assert len(pa["label"]) == 2, name
        got, gst, _, _ = _compare(g, labels, pa, what=name)
        assert gst["strip_pixels"] > 0 and gst["seam_edges"] > 0 and gst["hit_max_iterations"] == 0, (name, gst)
        _compare(g, labels, pa, what=name + "/no solve", max_iterations=0)


def test_upstream_pins_on_the_gpu():
    """the recorded patch sets fed to the GPU directly, no solve: upstream's own arrays"""
    n = 0
    for name, m, labels, pa, want in pin_cases():
        c = M.Context(0)
        c.set_mesh(m.verts, m.faces, np.zeros((len(m.faces), 3), np.float32))
        got, gst = c.local_seam_leveling(m.adj_ptr, m.adj, labels, pa, M.default_lsl_params(max_iterations=0))
        c.close()
        _same(got, want, name)
        assert gst["outside_frame"] == 0 and gst["demoted"] == 0 and gst["skipped_pairs"] == 0
        n += 1
    assert n == 20


def test_global_memory_path_equals_the_model_and_the_lds_path():
    g, labels, pa = crafted_sets()["three_labels_and_unseen"]
    lds, lst, want, _ = _compare(g, labels, pa, what="lds")
    assert lst["patches_global"] == 0 and lst["patches_lds"] == len(pa["label"])
    need = []                                                    # a patch's solver image: 12 B per pixel + 16 B per unknown
    for i in range(len(pa["label"])):
        _, _, mask = BM.patch(pa, want, i)
        unknowns = BM.solve(mask, BM.patch(pa, pa, i)[0], BM.patch(pa, pa, i)[0], max_iterations=0)[3][0]
        need.append(12 * mask.size + 16 * unknowns)
    order = np.argsort(need)
    assert need[order[-1]] > need[order[-2]]
    mixed, mst, _, _ = _compare(g, labels, pa, what="mixed", lds_bytes=need[order[-1]] - 1)    # the threshold moved below the largest patch
    assert mst["patches_global"] == 1 and mst["patches_lds"] == len(need) - 1 and mst["pixels_global"] == BM.patch(pa, want, order[-1])[2].size
    _same(mixed, lds, "that patch's bits in global memory == its bits in LDS")
    glob, gst, _, _ = _compare(g, labels, pa, what="global", lds_bytes=0)
    assert gst["patches_lds"] == 0 and gst["patches_global"] == len(need)
    _same(glob, lds, "all global == lds")
    g, labels, pa = crafted_sets()["wide"]                       # patches of 12 000 pixels: global memory under the default threshold
    _, wst, _, _ = _compare(g, labels, pa, what="wide")
    assert wst["patches_global"] >= 1


def test_edge_sets_equal_the_model():
    """the sets of edge_sets(): a skipped pair (one shared vertex, once and twice), the sanitize pass converting pixels, an idle
    channel, black views and the ladder of unknown counts -- with the default parameters and before the solve"""
    for name, (g, labels, pa) in edge_sets().items():
        c = _ctx(g)
        got, gst, want, wst = _compare(g, labels, pa, ctx=c, what=name)
        assert gst["hit_max_iterations"] == 0 and gst["outside_frame"] == 0 and gst["demoted"] == 0, (name, gst)
        raw, rst, before, _ = _compare(g, labels, pa, ctx=c, what=name + "/no solve", max_iterations=0)
        c.close()
        kind, key = EDGE_REACHES.get(name, (None, None))
        if kind == "stats":
            assert gst[key] > 0 and rst[key] == gst[key], (name, key, gst)
        elif key == "sanitized":     # no counter on the device: pixels the writes left at 128 that its prepared mask holds as 255
            assert int(((before["blend_writes"] == 128) & (raw["blending"] == 255)).sum()) > 0, name
            assert int(((before["blend_writes"] == 128) & (got["blending"] == 255)).sum()) > 0, name
        else:
            assert gst["skipped_pairs"] == 0, (name, gst)
        if name == "black":
            assert gst["iterations_total"] == 0 and gst["strip_pixels"] > 0 and gst["error_max"] == 0.0
        if name == "const_channel":      # the idle channel: its unknowns keep the bits the writes left, the other two move
            st, alone, _, _ = BM.run_scene(g, labels, pa)
            assert np.all(alone["iters"][:, 1] == 0) and np.all(alone["iters"][:, [0, 2]] > 0)
            u = raw["blending"] == 255
            assert np.array_equal(_raw(got["image"].reshape(-1, 3)[u, 1]), _raw(raw["image"].reshape(-1, 3)[u, 1]))
            assert not np.array_equal(_raw(got["image"].reshape(-1, 3)[u, 0]), _raw(raw["image"].reshape(-1, 3)[u, 0]))


def _both_paths(g, labels, pa, ctx, what, **params):
    """one run under the default LDS threshold and one in global memory: each equals the model, and they equal each other"""
    lds, lst, want, wst = _compare(g, labels, pa, ctx=ctx, what=what, **params)
    glob, gst, _, _ = _compare(g, labels, pa, ctx=ctx, what=what + "/global", lds_bytes=0, **params)
    assert gst["patches_lds"] == 0 and gst["patches_global"] == lst["patches_lds"] + lst["patches_global"], (what, lst, gst)
    _same(glob, lds, what + ": global == lds")
    for k in ("iterations_total", "iterations_max", "hit_max_iterations"):
        assert gst[k] == lst[k], (what, k)
    assert np.float32(gst["error_max"]).view(np.uint32) == np.float32(lst["error_max"]).view(np.uint32), what
    return lst, want


def test_unknown_ladder_on_both_paths():
    """1, 2, 255 .. 257, 1023 .. 1025, 2047 .. 2049 and 4158 unknowns in a patch: the tails of the tree's lanes and of the workgroup"""
    seen = []
    for name, (g, labels, pa) in ladder_sets().items():
        c = _ctx(g)
        lst, _ = _both_paths(g, labels, pa, c, name)
        c.close()
        counts = unknown_counts(g, labels, pa)
        assert lst["patches_lds"] == len(counts) and lst["patches_global"] == 0 and lst["strip_pixels"] == sum(counts), (name, lst)
        seen += counts
    assert {1, 2, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049} <= set(seen) and any(n > 4096 and n % 1024 for n in seen), seen


def test_iteration_caps_on_both_paths():
    """max_iterations of 1, 2, 5 and half the set's converged count: the capped iteration is counted and leaves p alone"""
    sets = {k: crafted_sets()[k] for k in ("grid", "wide")}
    sets.update({k: v for k, v in edge_sets().items() if k == "const_channel" or k.startswith("unknown_ladder")})
    for name, (g, labels, pa) in sets.items():
        st, base, bst, _ = BM.run_scene(g, labels, pa)
        assert st == 0 and bst["hit_max_iterations"] == 0
        caps = [1, 2, 5, mid_cap(base["iters"])]
        if name == "const_channel":      # between the two moving channels of patch 0: one idle, one capped, one converged
            a, b = sorted(int(v) for v in base["iters"][0, [0, 2]])
            assert base["iters"][0, 1] == 0 and 0 < a < b
            caps.append((a + b + 1) // 2)
        c = _ctx(g)
        for cap in caps:
            lst, want = _both_paths(g, labels, pa, c, "%s/cap %d" % (name, cap), max_iterations=cap)
            assert np.array_equal(want["iters"], np.minimum(base["iters"], cap)), (name, cap)
            assert lst["hit_max_iterations"] == int((base["iters"] >= cap).any(1).sum()), (name, cap, lst)
            if bst["iterations_max"] > cap:
                assert lst["hit_max_iterations"] > 0 and lst["iterations_max"] == cap, (name, cap, lst)
            if name == "const_channel":
                assert len(set(want["iters"][0].tolist())) == (3 if cap == caps[-1] else 2), (cap, want["iters"])
        _compare(g, labels, pa, ctx=c, what=name + "/after the caps")
        c.close()


def test_tolerances_equal_the_model():
    for name in ("grid", "wide"):
        g, labels, pa = crafted_sets()[name]
        c = _ctx(g)
        its = [_compare(g, labels, pa, ctx=c, what="%s/tolerance %g" % (name, tol), tolerance=tol)[1]["iterations_max"] for tol in (1e-3, 1e-5, 1e-6)]
        c.close()
        assert 0 < its[0] < its[1] < its[2], (name, its)


def test_strip_widths_equal_the_model():
    for name in ("wide", "grid"):
        g, labels, pa = crafted_sets()[name]
        c = _ctx(g)
        strips = {}
        for sw in (0, 1, 3, 250):
            strips[sw] = _compare(g, labels, pa, ctx=c, what="%s/strip_width %d" % (name, sw), strip_width=sw)[1]["strip_pixels"]
        assert strips[0] == 0 and strips[1] < strips[3] < strips[250], (name, strips)          # width 0: no strip, nothing to solve
        with pytest.raises(M.MvsError) as e:
            c.local_seam_leveling(g.adj_ptr, g.adj, labels, pa, M.default_lsl_params(strip_width=251))
        assert e.value.status == 1                                        # MVS_ERR_INVALID
        _compare(g, labels, pa, ctx=c, what=name + "/after the refused width")
        c.close()


def _device_host(dev, dtype):
    """a DevArray of the context copied to the host through torch (no copy on the device)"""
    import torch
    dt = np.dtype(dtype)
    n = dev.shape[0]
    if n == 0:
        return np.zeros(0, dt)

    class _Dev:
        __cuda_array_interface__ = {"shape": (n * dt.itemsize,), "typestr": "|u1", "data": (dev.data_ptr(), False), "version": 2}
    return torch.as_tensor(_Dev(), device="cuda").cpu().numpy().view(dt)


def test_host_and_device_inputs_outputs_and_repeat():
    import torch
    s = get_scene("bumpy")
    labels = _library_labels("bumpy", s)
    pa = _pipeline_patches(s, labels)
    c = _ctx(s)
    a, ast, _, _ = _compare(s, labels, pa, ctx=c, what="host")
    b, _ = c.local_seam_leveling(s.adj_ptr, s.adj, labels, pa)
    _same(b, a, "repeat")
    gsl, _ = c.global_seam_leveling(s.adj_ptr, s.adj, labels, on_device=True)
    dev, _ = c.texture_patches(s.adj_ptr, s.adj, labels, gsl["corner_adjust"], on_device=True)
    d, dst = c.local_seam_leveling(s.adj_ptr, s.adj, labels, dev)                 # row f6's device output passed straight in
    _same(d, a, "device patches")
    assert dst["strip_pixels"] == ast["strip_pixels"]
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x, np.uint32).view(np.int32)).cuda()
    e, est = c.local_seam_leveling(t(s.adj_ptr), t(s.adj), t(labels), dev, on_device=True)
    c.synchronize()
    host = {k: _device_host(e[k], dt) for k, dt in (("image", np.float32), ("validity", np.uint8), ("blending", np.uint8))}
    _same(host, a, "device inputs and outputs")
    assert est["ms_total"] > 0 and est["ms_solve"] > 0
    again, _ = c.texture_patches(s.adj_ptr, s.adj, labels, gsl["corner_adjust"])   # the input was not modified
    for k in pa:
        assert np.array_equal(_raw(again[k]), _raw(pa[k])), k
    c.close()
    merged = dict(pa); merged.update(a)
    i0 = int(np.argmax(np.diff(pa["pix_ptr"].astype(np.int64))))
    img, val, bl = M.patch_view(merged, i0)
    assert img.shape == (int(pa["box"][i0, 3]), int(pa["box"][i0, 2]), 3) and val.shape == bl.shape == img.shape[:2]
    assert set(np.unique(bl)) <= {0, 64, 128, 255}


def test_errors_leave_the_context_usable():
    g, labels, pa = crafted_sets()["grid"]
    c = _ctx(g)
    bad = labels.copy(); bad[int(pa["faces"][0])] = 3 - bad[int(pa["faces"][0])]
    with pytest.raises(M.MvsError) as e:
        c.local_seam_leveling(g.adj_ptr, g.adj, bad, pa)
    assert e.value.status == 4
    pb = dict(pa); f = pa["faces"].copy(); f[0] = len(g.faces); pb["faces"] = f
    with pytest.raises(M.MvsError) as e:
        c.local_seam_leveling(g.adj_ptr, g.adj, labels, pb)
    assert e.value.status == 4
    pc = dict(pa); tc = pa["texcoords"].copy(); tc.reshape(-1)[0] = np.inf; pc["texcoords"] = tc
    with pytest.raises(M.MvsError) as e:
        c.local_seam_leveling(g.adj_ptr, g.adj, labels, pc)
    assert e.value.status == 7
    _compare(g, labels, pa, ctx=c, what="after the errors")
    empty, _ = c.texture_patches(g.adj_ptr, g.adj, np.zeros(len(g.faces), np.uint32))     # all labels 0: an empty set
    got, gst = c.local_seam_leveling(g.adj_ptr, g.adj, np.zeros(len(g.faces), np.uint32), empty)
    assert got["image"].shape == (0, 3) and gst["seam_edges"] == 0 and gst["strip_pixels"] == 0
    c.close()
    with pytest.raises(M.MvsError) as e:                                  # no mesh
        M.Context(0).local_seam_leveling(g.adj_ptr, g.adj, labels, pa)
    assert e.value.status == 6


def test_module_level_entry():
    s = get_scene("tiny")
    labels = _library_labels("tiny", s)
    got, gst = M.local_seam_leveling(s, labels)
    pa = _pipeline_patches(s, labels)
    st, want, wst, _ = BM.run_scene(s, labels, pa)
    _same(got, want)
    assert gst["strip_pixels"] == wst["strip_pixels"] and np.array_equal(got["pix_ptr"], pa["pix_ptr"])


def test_config2_equals_the_model():
    s = M.synth.make_scene(**M.synth.CONFIGS[2])
    labels = _library_labels("config2", s)
    pa = _pipeline_patches(s, labels)
    got, gst, _, _ = _compare(s, labels, pa, what="config 2")
    assert gst["strip_pixels"] > 0 and gst["hit_max_iterations"] == 0
    assert gst["outside_frame"] == 0 and gst["demoted"] == 0, gst
    _compare(s, labels, pa, what="config 2/no solve", max_iterations=0)
