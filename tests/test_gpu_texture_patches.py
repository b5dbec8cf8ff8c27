"""Row f6 on the GPU: Context.texture_patches equals the CPU model (tests/tools/patch_model.cpp, upstream's sequential loop) bit for
bit on every array of mvs_patch_set -- labels, frames, lists, texture coordinates, pixel offsets, images, both masks -- and on the
counts, on the suite's scenes (labels from the library's own view selection, adjustments from its own global seam leveling, and
none), shuffled meshes, the crafted and nested sets of tests/test_patch_model.py (merge chains in every candidate order, equal boxes),
crafted labelings on the scenes where chains occur by themselves, and config 2; plus the checks of that file on the GPU's output."""
import numpy as np
import pytest

import mvs_texturing_amd as M
import patch_model as PM
import seam_model as SM
from conftest import get_scene
from test_patch_model import check_constant_adjustment, check_invariants, check_nested_list, corner_adjust, crafted_set, nested_set

pytestmark = pytest.mark.gpu

KEYS = ("label", "box", "face_ptr", "faces", "texcoords", "pix_ptr", "image", "validity", "blending")
COUNTS = ("patches", "merged", "listed_faces", "degenerate_faces", "pixels", "valid_pixels", "near_pixels")


@pytest.fixture(scope="module", autouse=True)
def _models_built():
    SM.build(); PM.build()


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


def _compare(s, labels, ca=None, ctx=None, what=""):
    """one GPU run against the model; returns (gpu arrays, gpu stats, the model's counters)"""
    st, want, wst, cnt = PM.run_scene(s, labels, ca)
    assert st == 0
    c = ctx or _ctx(s)
    try:
        got, gst = c.texture_patches(s.adj_ptr, s.adj, np.ascontiguousarray(labels, np.uint32), ca)
    finally:
        if ctx is None:
            c.close()
    _same(got, want, what)
    for k in COUNTS:
        assert gst[k] == wst[k], (what, k, gst[k], wst[k])
    return got, gst, cnt


# which side of the 512-pixel split between tp_mark_kernel and tp_mark_big_kernel a scene's list entries fall on (patch_model.entry_pixels
# on the model's output under the labels of the reference's own view selection, which the library's equal): both, at least 77 entries
# on either side, except that manyviews' faces cover a few pixels of its 160 x 120 views (ranges of at most 81 pixels) and bigfoot's
# thousands of its 1024 x 768 views (at least 1548)
SPLIT_SIDES = {"manyviews": ("small",), "bigfoot": ("big",)}


@pytest.mark.parametrize("name", ["tiny", "bumpy", "oddw", "mixed", "spiky", "close", "manyviews", "bigfoot"])
def test_scenes_equal_the_model(name):
    s = get_scene(name)
    labels = _library_labels(name, s)
    c = _ctx(s)
    gsl, _ = c.global_seam_leveling(s.adj_ptr, s.adj, labels)
    c.close()
    assert np.any(gsl["corner_adjust"])
    got, gst, _ = _compare(s, labels, gsl["corner_adjust"], what=name + "/gsl")
    assert gst["valid_pixels"] > 0 and gst["near_pixels"] > 0
    n = PM.entry_pixels(PM.run_scene(s, labels)[1])                       # from the model's texcoords and frames
    sides = {"small": int(((n > 0) & (n <= 512)).sum()), "big": int((n > 512).sum())}
    print("%s: entries of <= 512 / > 512 pixels: %d / %d, the largest %d" % (name, sides["small"], sides["big"], int(n.max())))
    for side in SPLIT_SIDES.get(name, ("small", "big")):
        assert sides[side] > 0, (name, sides)
    if name == "bigfoot":
        assert int(n.max()) > 20 * 256                                    # many strides of a block of tp_mark_big_kernel
    zero, zst, _ = _compare(s, labels, None, what=name + "/none")
    check_invariants(s, labels, zero, zst)
    for k in KEYS:
        if k != "image":
            assert np.array_equal(got[k], zero[k]), k


@pytest.mark.parametrize("name", ["tiny", "bumpy"])
def test_shuffled_scenes_equal_the_model(name):
    s = get_scene(name)
    p = M.synth.permute_scene(s, seed=7)
    labels = _library_labels(name, s)[p.face_perm]
    _compare(p, labels, corner_adjust(p, labels), what=name + "/shuffled")


def test_crafted_set_equals_the_model():
    total = {k: 0 for k in PM.COUNTERS}
    for name, (g, labels) in crafted_set().items():
        got, gst, cnt = _compare(g, labels, corner_adjust(g, labels), what=name)
        check_invariants(g, labels, got, gst)
        _compare(g, labels, None, what=name + "/none")
        for k in total:
            total[k] += cnt[k]
    for k in ("absorbed", "inside_twice", "near_then_inside", "degenerate", "frame_negative"):
        assert total[k] >= 1, total
    s = get_scene("tiny")
    for lname, labels in SM.crafted_labelings(s).items():
        got, gst, _ = _compare(s, labels, corner_adjust(s, labels), what="tiny/" + lname)
        if lname == "random":
            assert gst["merged"] > 0
        if lname == "first":                                              # an entry on either side of the split, to the pixel
            n = PM.entry_pixels(got)
            assert (n == 512).any() and (n == 513).any()
    g = SM.grid_scene()
    c = _ctx(g)                                                           # all labels 0: an empty set
    got, gst = c.texture_patches(g.adj_ptr, g.adj, np.zeros(len(g.faces), np.uint32))
    assert gst["patches"] == 0 and gst["pixels"] == 0 and got["image"].shape == (0, 3) and got["pix_ptr"].tolist() == [0]
    c.close()


def test_nested_set_equals_the_model():
    """chains of absorptions in all six candidate orders and two candidates with one box: every array and count, with adjustments and
    without; the label-1 list of the DEVICE against the literal order derived by hand (tests/test_patch_model.py NESTED_LISTS)"""
    total = {k: 0 for k in PM.COUNTERS}
    for name, (g, labels) in nested_set().items():
        got, gst, cnt = _compare(g, labels, corner_adjust(g, labels), what=name)
        check_invariants(g, labels, got, gst)
        _compare(g, labels, None, what=name + "/none")
        for k in total:
            total[k] += cnt[k]
        assert gst["patches"] == 2 and gst["merged"] == 3, (name, gst)
    for order in PM.NESTED_ORDERS:
        g, labels, region = PM.nested_scene(order)
        c = _ctx(g)
        got, _ = c.texture_patches(g.adj_ptr, g.adj, labels)
        c.close()
        check_nested_list(order, region, got)
    assert total["chain"] >= 2 and total["absorber_later"] >= 2 and total["equal_boxes"] >= 1, total
    assert total["clamped"] == 0 and total["magenta_inside"] == 0, total


@pytest.mark.parametrize("name", ["spiky", "oddw"])
def test_crafted_labelings_where_chains_occur(name):
    """the scenes on which random labelings build chains by themselves (an absorbed candidate that had absorbed others)"""
    s = get_scene(name)
    total = {k: 0 for k in PM.COUNTERS}
    for lname, labels in SM.crafted_labelings(s).items():
        _, gst, cnt = _compare(s, labels, corner_adjust(s, labels), what=name + "/" + lname)
        for k in total:
            total[k] += cnt[k]
    print("%s: chain %d, absorber_later %d, equal_boxes %d, absorbed %d" % (name, total["chain"], total["absorber_later"], total["equal_boxes"], total["absorbed"]))
    assert total["chain"] >= 1 and total["absorber_later"] >= 1, total
    assert total["clamped"] == 0, total


def test_constant_adjustment_on_the_gpu():
    g, labels = crafted_set()["grid_fin_zero"]
    c = _ctx(g)
    check_constant_adjustment(g, labels, lambda ca: c.texture_patches(g.adj_ptr, g.adj, labels, ca)[0])
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
    fresh = _ctx(s)                                                       # no seam leveling on this context
    ca = corner_adjust(s, labels)
    a, ast = fresh.texture_patches(s.adj_ptr, s.adj, labels, ca)
    fresh.close()
    c = _ctx(s)
    gsl, _ = c.global_seam_leveling(s.adj_ptr, s.adj, labels, on_device=True)
    after_gsl, _ = c.texture_patches(s.adj_ptr, s.adj, labels, ca)         # after a seam leveling: the same bits
    _same(after_gsl, a, "after seam leveling")
    b, _ = c.texture_patches(s.adj_ptr, s.adj, labels, ca)
    _same(b, a, "repeat")
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x, np.uint32).view(np.int32)).cuda()
    d, _ = c.texture_patches(dev(s.adj_ptr), dev(s.adj), dev(labels), torch.from_numpy(ca).cuda())
    _same(d, a, "device inputs")
    e, est = c.texture_patches(s.adj_ptr, s.adj, labels, ca, on_device=True)
    c.synchronize()
    dt = dict(label=np.uint32, box=np.int32, face_ptr=np.uint32, faces=np.uint32, texcoords=np.float32, pix_ptr=np.uint64, image=np.float32,
              validity=np.uint8, blending=np.uint8)
    host = {k: _device_host(e[k], dt[k]) for k in KEYS}
    _same(host, a, "device outputs")
    assert est["pixels"] == ast["pixels"] and est["ms_total"] > 0
    # the device output of seam leveling fed straight back in
    gsl, _ = c.global_seam_leveling(s.adj_ptr, s.adj, labels, on_device=True)
    f, _ = c.texture_patches(s.adj_ptr, s.adj, labels, gsl["corner_adjust"])
    gh, _ = c.global_seam_leveling(s.adj_ptr, s.adj, labels)
    c.close()
    st, want, _, _ = PM.run_scene(s, labels, gh["corner_adjust"])
    _same(f, want, "device corner_adjust")
    i0 = int(np.argmax(np.diff(a["pix_ptr"].astype(np.int64))))
    img, val, bl = M.patch_view(a, i0)
    assert img.shape == (int(a["box"][i0, 3]), int(a["box"][i0, 2]), 3) and val.shape == bl.shape == img.shape[:2]
    assert np.shares_memory(img, a["image"]) and np.shares_memory(val, a["validity"])


def test_errors_leave_the_context_usable():
    g = SM.grid_scene()
    c = _ctx(g)
    with pytest.raises(M.MvsError) as e:
        c.texture_patches(g.adj_ptr, g.adj, np.full(len(g.faces), 3, np.uint32))
    assert e.value.status == 4
    o = SM.grid_scene(outside=True)
    c2 = _ctx(o)
    with pytest.raises(M.MvsError) as e:
        c2.texture_patches(o.adj_ptr, o.adj, SM.grid_labels(o))
    assert e.value.status == 4
    c2.close()
    labels = SM.grid_labels(g)
    _, want, wst, _ = PM.run_scene(g, labels)
    with pytest.raises(M.MvsError) as e:                                  # the cap: refused before the pixel arrays exist, counts filled
        c.texture_patches(g.adj_ptr, g.adj, labels, params=M.default_patch_params(max_pixels=wst["pixels"] - 1))
    assert e.value.status == 7 and e.value.stats["pixels"] == wst["pixels"] and e.value.stats["patches"] == wst["patches"]
    got, _ = c.texture_patches(g.adj_ptr, g.adj, labels, params=M.default_patch_params(max_pixels=wst["pixels"]))   # exactly the cap passes
    _same(got, want, "at the cap")
    _compare(g, labels, corner_adjust(g, labels), ctx=c)
    c.close()
    with pytest.raises(M.MvsError) as e:                                  # no mesh, no views
        M.Context(0).texture_patches(g.adj_ptr, g.adj, labels)
    assert e.value.status == 6


def test_module_level_entry():
    s = get_scene("tiny")
    labels = _library_labels("tiny", s)
    got, gst = M.texture_patches(s, labels)
    st, want, wst, _ = PM.run_scene(s, labels)
    _same(got, want)
    assert gst["pixels"] == wst["pixels"]


def test_config2_equals_the_model():
    s = M.synth.make_scene(**M.synth.CONFIGS[2])
    labels = _library_labels("config2", s)
    c = _ctx(s)
    gsl, _ = c.global_seam_leveling(s.adj_ptr, s.adj, labels)
    got, gst = c.texture_patches(s.adj_ptr, s.adj, labels, gsl["corner_adjust"])
    c.close()
    st, want, wst, _ = PM.run_scene(s, labels, gsl["corner_adjust"])
    assert st == 0
    _same(got, want, "config 2")
    for k in COUNTS:
        assert gst[k] == wst[k], (k, gst[k], wst[k])
    assert gst["patches"] > 0 and gst["valid_pixels"] > 0 and gst["near_pixels"] > 0
