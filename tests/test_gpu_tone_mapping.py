"""Tone mapping `gamma` on the GPU (DESIGN.md section 4 "Tone mapping"; csrc/tone.h, k_tone.hip and the gamma instantiations of rows f5, f6,
f8 and f10).  (a) Context.gamma_correct gives the host twin's bits; (b) row f6 is the texel table at the crop's bytes, then the model's
adjust_colors; (c) with a PERMUTED byte / 255 table set through the harness entry, rows f5 and f6 under tone_mapping = 1 on images I equal
tone_mapping = 0 on the permuted images -- and the existing CPU models on those --, so every texel read goes through the table; (d) row
f5's right-hand side moves and its solution still solves the normal equations; (e) row f8 equals the `none` run and the atlas model on the
set whose image went through the host twin; (f) an unknown mode is refused; (g) M.texture_model end to end; (h) the debug model's files do
not depend on the mode.  Labels come from the library's own view selection, as in the neighbouring files."""
import copy
import os

import numpy as np
import pytest

import mvs_texturing_amd as M
import atlas_model as AM
import patch_model as PM
import png_decode as PD
import seam_model as SM
from conftest import get_scene
from test_atlas_model import crafted_sets
from test_gpu_seam_leveling import _bits, _ctx, _library_labels

pytestmark = pytest.mark.gpu

P22 = np.float32(2.2)
PINV = np.float32(1.0) / np.float32(2.2)
PATCH_KEYS = ("label", "box", "face_ptr", "faces", "texcoords", "pix_ptr", "image", "validity", "blending")
GSL_KEYS = ("x_ptr", "x_label", "x_adjust", "corner_adjust")
SYS_KEYS = ("lhs_ptr", "lhs_col", "lhs_val", "rhs", "a_col", "b", "x_raw")
GAMMA = dict(tone_mapping=1)


@pytest.fixture(scope="module", autouse=True)
def _models_built():
    SM.build(); PM.build(); AM.build()


def _raw(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32).ravel() if a.dtype == np.float32 else a.ravel()


def _same(got, want, keys, what=""):
    for k in keys:
        assert got[k].size == want[k].size and np.array_equal(_raw(got[k]), _raw(want[k])), (what, k)


def _same_floats(got, want, what=""):
    """bit for bit, a NaN comparing as a NaN"""
    got, want = np.asarray(got, np.float32).ravel(), np.asarray(want, np.float32).ravel()
    nan = np.isnan(want)
    assert got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(_bits(got[~nan]), _bits(want[~nan])), what


# ---- (a) the route on its own ----

@pytest.mark.parametrize("which", ["2.2", "inv"])
def test_gamma_correct_on_the_device_equals_the_host_twin(which):
    import torch
    p = P22 if which == "2.2" else PINV
    rng = np.random.default_rng(31)
    specials = np.array([0x7FC00000, 0x7F800001, 0xFFC12345, 0xBF800000, 0x80000001, 0xFF800000, 0, 0x80000000, 0x7F800000, 0x3F800000, 1, 0x007FFFFF,
                         0x00800000, 0x7F7FFFFF], np.uint32).view(np.float32)
    x = np.concatenate([np.arange(256, dtype=np.float32) / np.float32(255.0), specials,
                        rng.integers(0, 1 << 32, 65536, dtype=np.uint64).astype(np.uint32).view(np.float32)])
    want = M.gamma_correct(x, p)
    assert np.isnan(want).any() and np.isinf(want).any() and (np.abs(x) < np.finfo(np.float32).tiny).sum() > 100
    c = M.Context(0)
    for n in (1, 255, 257, 65537, len(x)):
        _same_floats(c.gamma_correct(x[:n], p), want[:n], ("host", n))
        t = torch.from_numpy(x[:n].copy()).cuda()
        assert c.gamma_correct(t, p) is t
        _same_floats(t.cpu().numpy(), want[:n], ("device", n))
        u = torch.from_numpy(x[:n + 1].copy()).cuda()[1:]                 # not 16-byte aligned: the scalar path alone
        c.gamma_correct(u, p)
        _same_floats(u.cpu().numpy(), want[1:n + 1], ("device, unaligned", n))
    table = c.gamma_correct(M.tone_table("none"), P22)
    assert np.array_equal(_bits(table), _bits(M.tone_table("gamma")))
    with pytest.raises(M.MvsError) as e:
        c.gamma_correct(x[:4], -1.0)
    assert e.value.status == 1
    assert c.gamma_correct(np.zeros(0, np.float32), p).shape == (0,)
    c.close()


# ---- (b) row f6 ----

def _crop_bytes(s, label, box):
    return np.rint(PM.crop(s, int(label), box) * np.float32(255.0)).astype(np.uint8)


def _check_patches_against_the_table(s, labels, what):
    table = M.tone_table("gamma")
    c = _ctx(s)
    none, nst = c.texture_patches(s.adj_ptr, s.adj, labels)
    got, gst = c.texture_patches(s.adj_ptr, s.adj, labels, params=M.default_patch_params(**GAMMA))
    gsl, _ = c.global_seam_leveling(s.adj_ptr, s.adj, labels, M.default_gsl_params(**GAMMA))
    adj, _ = c.texture_patches(s.adj_ptr, s.adj, labels, gsl["corner_adjust"], M.default_patch_params(**GAMMA))
    c.close()
    _same(got, none, [k for k in PATCH_KEYS if k != "image"], what)
    _same(adj, none, [k for k in PATCH_KEYS if k not in ("image", "validity", "blending")], what)
    for k in ("patches", "pixels", "valid_pixels", "near_pixels"):
        assert gst[k] == nst[k], (what, k)
    ca = gsl["corner_adjust"].reshape(-1, 3, 3)
    assert np.any(ca)
    differs = False
    for i in range(len(got["label"])):
        w, h = int(got["box"][i, 2]), int(got["box"][i, 3])
        lin = table[_crop_bytes(s, got["label"][i], got["box"][i])]       # the crop in bytes, fill included, through the table
        img, val, _ = M.patch_view(got, i)
        want = np.where(val[..., None] == 255, lin, np.float32(0))
        assert np.array_equal(_bits(img), _bits(want)), (what, i)
        differs = differs or not np.array_equal(_bits(img), _bits(M.patch_view(none, i)[0]))
        a, b = int(got["face_ptr"][i]), int(got["face_ptr"][i + 1])
        mi, mv, mb, _ = PM.adjust_colors(w, h, lin, adj["texcoords"][a:b], ca[adj["faces"][a:b]])
        gi, gv, gb = M.patch_view(adj, i)
        assert np.array_equal(_bits(gi), _bits(mi)) and np.array_equal(gv, mv) and np.array_equal(gb, mb), (what, i)
    assert differs, what


@pytest.mark.parametrize("name", ["tiny", "bumpy"])
def test_patches_are_the_table_at_the_crops_bytes(name):
    s = get_scene(name)
    _check_patches_against_the_table(s, _library_labels(name, s), name)


def test_the_fill_of_the_crop_goes_through_the_table():
    """frames that start at -1: the magenta column of the crop is table[255], table[0], table[255] -- under a table that does not map
    255 to 1 and 0 to 0 as well"""
    g = SM.grid_scene()
    labels = SM.grid_labels(g)
    assert PM.run_scene(g, labels)[3]["magenta"] > 0
    _check_patches_against_the_table(g, labels, "grid")
    table = np.linspace(0.25, 0.75, 256).astype(np.float32)              # fill = (0.75, 0.25, 0.75)
    c = _ctx(g)
    c.set_tone_table(table)
    got, _ = c.texture_patches(g.adj_ptr, g.adj, labels, params=M.default_patch_params(**GAMMA))
    c.close()
    seen = 0
    for i in range(len(got["label"])):
        by = _crop_bytes(g, got["label"][i], got["box"][i])
        img, val, _ = M.patch_view(got, i)
        assert np.array_equal(_bits(img), _bits(np.where(val[..., None] == 255, table[by], np.float32(0)))), i
        if int(got["box"][i, 0]) < 0:
            col = val[:, 0] == 255
            seen += int(col.sum())
            assert np.all(img[:, 0][col] == np.float32([0.75, 0.25, 0.75]))
    assert seen > 0


# ---- (c) rows f5 and f6 through a permuted table ----

def _permuted(s, seed=41):
    rng = np.random.default_rng(seed)
    pi = np.arange(256)
    pi[1:255] = 1 + rng.permutation(254)
    t = copy.copy(s)
    t.images = [np.ascontiguousarray(pi[im].astype(np.uint8)) for im in s.images]
    return pi, (pi.astype(np.float32) / np.float32(255.0)).astype(np.float32), t


def _rows_f5_f6(c, s, labels, tone):
    gsl, gst = c.global_seam_leveling(s.adj_ptr, s.adj, labels, M.default_gsl_params(tone_mapping=tone))
    system = c.gsl_system()
    pa, _ = c.texture_patches(s.adj_ptr, s.adj, labels, gsl["corner_adjust"], M.default_patch_params(tone_mapping=tone))
    flat, _ = c.texture_patches(s.adj_ptr, s.adj, labels, None, M.default_patch_params(tone_mapping=tone))
    return gsl, gst, system, pa, flat


@pytest.mark.parametrize("name", ["tiny", "bumpy", "grid"])
def test_every_texel_read_goes_through_the_table(name):
    if name == "grid":
        s = SM.grid_scene(); labels = SM.grid_labels(s)                  # frames leave the view: the fill is read as well
    else:
        s = get_scene(name); labels = _library_labels(name, s)
    pi, table, t = _permuted(s)
    assert table[0] == 0 and table[255] == 1 and not np.array_equal(pi, np.arange(256))
    c = _ctx(s)
    c.set_tone_table(table)
    a = _rows_f5_f6(c, s, labels, 1)
    c.close()
    c = _ctx(t)
    b = _rows_f5_f6(c, t, labels, 0)
    c.close()
    _same(a[0], b[0], GSL_KEYS, name)
    assert a[1]["iterations"] == b[1]["iterations"] and np.array_equal(_bits(a[1]["error"]), _bits(b[1]["error"]))
    assert a[1]["iterations"] != [0, 0, 0]
    _same(a[2], b[2], SYS_KEYS, name)
    _same(a[3], b[3], PATCH_KEYS, name)
    _same(a[4], b[4], PATCH_KEYS, name)
    if name != "bumpy":                                                   # ... and the CPU models as they are, on the permuted images
        st, want, wst = SM.run_scene(t, labels)
        assert st == 0
        for k in GSL_KEYS:
            assert np.array_equal(_raw(a[0][k]), _raw(want[k])), k
        assert np.array_equal(_bits(a[2]["b"]), _bits(want["b"])) and np.array_equal(_bits(a[2]["rhs"]), _bits(want["rhs"]))
        assert a[1]["iterations"] == wst["iterations"]
        st, pw, _, _ = PM.run_scene(t, labels, a[0]["corner_adjust"])
        assert st == 0
        _same(a[3], pw, PATCH_KEYS, name + "/model")


def test_the_default_table_is_the_gamma_table():
    s = get_scene("tiny")
    labels = _library_labels("tiny", s)
    c = _ctx(s)
    default = _rows_f5_f6(c, s, labels, 1)
    c.set_tone_table(M.tone_table("gamma"))
    explicit = _rows_f5_f6(c, s, labels, 1)
    c.set_tone_table(M.tone_table("none"))
    plain = _rows_f5_f6(c, s, labels, 1)
    none = _rows_f5_f6(c, s, labels, 0)                                   # mode 0 never reads the table
    c.set_tone_table(None)
    restored = _rows_f5_f6(c, s, labels, 1)
    c.close()
    for other in (explicit, restored):
        _same(default[0], other[0], GSL_KEYS); _same(default[2], other[2], SYS_KEYS); _same(default[3], other[3], PATCH_KEYS)
    _same(plain[0], none[0], GSL_KEYS); _same(plain[3], none[3], PATCH_KEYS)
    assert not np.array_equal(_bits(default[3]["image"]), _bits(none[3]["image"]))


# ---- (d) row f5 under gamma ----

def test_seam_leveling_moves_and_still_solves_its_system():
    s = get_scene("bumpy")
    labels = _library_labels("bumpy", s)
    c = _ctx(s)
    c.global_seam_leveling(s.adj_ptr, s.adj, labels)
    none = c.gsl_system()
    c.global_seam_leveling(s.adj_ptr, s.adj, labels, M.default_gsl_params(**GAMMA))
    gamma = c.gsl_system()
    c.close()
    assert not np.array_equal(_bits(gamma["rhs"]), _bits(none["rhs"]))
    _same(gamma, none, ("lhs_ptr", "lhs_col", "lhs_val", "a_col"))        # the structure does not depend on colour
    s = get_scene("tiny")
    for name in ("random", "blocks", "random_with_unseen"):
        labels = SM.crafted_labelings(s)[name]
        c = _ctx(s)
        got, gst = c.global_seam_leveling(s.adj_ptr, s.adj, labels, M.default_gsl_params(**GAMMA))
        sysg = c.gsl_system()
        c.close()
        _, full, _ = SM.run_scene(s, labels)                              # the full symmetric Lhs of the same structure
        arrays = dict(lhs_ptr=full["lhs_ptr"], lhs_col=full["lhs_col"], lhs_val=full["lhs_val"], rhs=sysg["rhs"].ravel(), x_raw=sysg["x_raw"].ravel())
        assert not np.array_equal(_bits(sysg["rhs"]), _bits(full["rhs"]))
        res = SM.normal_residual(arrays, gst["x_rows"])
        for ch in range(3):
            assert res[ch] <= 2.0 * float(gst["error"][ch]) + 1e-6 and (gst["iterations"][ch] == 1000 or res[ch] <= 2e-3)


# ---- (e) row f8 ----

ATLAS_KEYS = tuple(AM.ARRAYS)


def _check_atlases(pa, ctx, what, device_too=False):
    """tone_mapping = 1 on pa == tone_mapping = 0 on pa with its image through the host twin == the atlas model on that"""
    corrected = dict(pa)
    corrected["image"] = M.gamma_correct(np.ascontiguousarray(pa["image"], np.float32), PINV)
    st, want, wst, _, _ = AM.run(corrected)
    assert st == 0
    got, gst = ctx.texture_atlases(pa, M.default_atlas_params(**GAMMA))
    none, nst = ctx.texture_atlases(corrected)
    _same(got, want, ATLAS_KEYS, what + "/model")
    _same(got, none, ATLAS_KEYS, what + "/none")
    for k in AM.STATS:
        assert gst[k] == wst[k] == nst[k], (what, k)
    again, _ = ctx.texture_atlases(pa, M.default_atlas_params(**GAMMA))
    _same(again, got, ATLAS_KEYS, what + "/repeat")
    if device_too:
        import torch
        signed = {np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}
        flat = {k: np.ascontiguousarray(pa[k], dt).reshape(-1) for k, dt in AM.PATCH_ARRAYS.items()}
        dev = {k: torch.from_numpy(v.view(signed.get(v.dtype, v.dtype))).cuda() for k, v in flat.items()}
        d, _ = ctx.texture_atlases(dev, M.default_atlas_params(**GAMMA))
        _same(d, got, ATLAS_KEYS, what + "/device")
    return got, none


@pytest.mark.parametrize("name", sorted(crafted_sets()))
def test_crafted_atlas_sets(name):
    c = M.Context(0)
    pa = crafted_sets()[name]
    got, _ = _check_atlases(pa, c, name, device_too=name == "small")
    plain, _ = c.texture_atlases(pa)
    assert not np.array_equal(got["image"], plain["image"]), name
    c.close()


@pytest.mark.parametrize("name", ["tiny", "bumpy"])
def test_pipeline_patches_through_the_atlases(name):
    s = get_scene(name)
    labels = _library_labels(name, s)
    c = _ctx(s)
    gsl, _ = c.global_seam_leveling(s.adj_ptr, s.adj, labels, M.default_gsl_params(**GAMMA))
    pa, _ = c.texture_patches(s.adj_ptr, s.adj, labels, gsl["corner_adjust"], M.default_patch_params(**GAMMA))
    lsl, _ = c.local_seam_leveling(s.adj_ptr, s.adj, labels, pa)
    pa = dict(pa); pa.update(image=lsl["image"], validity=lsl["validity"])
    _check_atlases(pa, c, name, device_too=True)
    c.close()


def test_special_values_and_sizes_around_the_compose_chunk():
    rng = np.random.default_rng(51)
    pa = AM.craft(rng, [(2, 2), (31, 33), (32, 32), (25, 41)], hole=0.2)   # 4, 1023, 1024 and 1025 pixels: the chunk is 1024
    assert sorted(np.diff(pa["pix_ptr"].astype(np.int64)).tolist()) == [4, 1023, 1024, 1025]
    c = M.Context(0)
    _check_atlases(pa, c, "sizes", device_too=True)
    odd = AM.craft(rng, [(40, 30), (17, 23), (3, 3)], hole=0.0)
    img = np.ascontiguousarray(odd["image"], np.float32).reshape(-1)
    vals = np.array([-0.5, -1e-30, 1.0000001, 1.5, 7.0, np.nan, -0.0, 0.0, np.inf, -np.inf, 1e-45, 1e-40, 1.1754942e-38, 0.5, 1.0], np.float32)
    img[:] = vals[rng.integers(0, len(vals), img.size)]
    img[:len(vals)] = vals
    odd["image"] = img
    got, _ = _check_atlases(odd, c, "special values", device_too=True)
    # the first patch's first pixels, channel by channel: NaN and the negatives give 0, +inf and everything above 1 give 255
    place = got["patch_pos"].reshape(-1, 2)[0] + (int(got["atlas_size"][0]) >> 7)
    first = M.atlas_view(got, 0)[place[1], place[0]:place[0] + 5].reshape(-1)
    assert first.tolist() == [0, 0, 255, 255, 255, 0, 0, 0, 255, 0, 0, 0, 0, 186, 255]
    c.close()


# ---- (f) refusal ----

def test_an_unknown_mode_is_refused_and_the_context_stays_usable():
    s = get_scene("tiny")
    labels = _library_labels("tiny", s)
    c = _ctx(s)
    gsl, _ = c.global_seam_leveling(s.adj_ptr, s.adj, labels)
    pa, _ = c.texture_patches(s.adj_ptr, s.adj, labels, gsl["corner_adjust"])
    at, _ = c.texture_atlases(pa)
    for call in (lambda: c.global_seam_leveling(s.adj_ptr, s.adj, labels, M.default_gsl_params(tone_mapping=2)),
                 lambda: c.texture_patches(s.adj_ptr, s.adj, labels, gsl["corner_adjust"], M.default_patch_params(tone_mapping=2)),
                 lambda: c.debug_patches(s.adj_ptr, s.adj, labels, params=M.default_patch_params(tone_mapping=2)),
                 lambda: c.texture_atlases(pa, M.default_atlas_params(tone_mapping=2)),
                 lambda: c.texture_atlases(pa, M.default_atlas_params(tone_mapping=0xFFFFFFFF))):
        with pytest.raises(M.MvsError) as e:
            call()
        assert e.value.status == 1 and "tone_mapping" in str(e.value)
    g2, _ = c.global_seam_leveling(s.adj_ptr, s.adj, labels)
    p2, _ = c.texture_patches(s.adj_ptr, s.adj, labels, g2["corner_adjust"])
    a2, _ = c.texture_atlases(p2)
    c.close()
    _same(g2, gsl, GSL_KEYS); _same(p2, pa, PATCH_KEYS); _same(a2, at, ATLAS_KEYS)


# ---- (g) end to end, (h) the debug model ----

def _files(d):
    return {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d))}


def test_texture_model_end_to_end(tmp_path):
    s = get_scene("tiny")
    labels = _library_labels("tiny", s)
    normals = M.vertex_normals(s.verts, s.faces)
    for mode in ("none", "gamma"):
        os.makedirs(tmp_path / mode)
        M.texture_model(s, labels, str(tmp_path / mode / "m"), normals, tone_mapping=mode)
    none, gamma = _files(tmp_path / "none"), _files(tmp_path / "gamma")
    assert sorted(none) == sorted(gamma) and "m.obj" in gamma and "m.mtl" in gamma
    assert gamma["m.obj"] == none["m.obj"] and gamma["m.mtl"] == none["m.mtl"]   # sizes, packing and coordinates do not depend on colour
    # the rows one by one with the mode set
    c = _ctx(s)
    gsl, _ = c.global_seam_leveling(s.adj_ptr, s.adj, labels, M.default_gsl_params(**GAMMA))
    pa, _ = c.texture_patches(s.adj_ptr, s.adj, labels, gsl["corner_adjust"], M.default_patch_params(**GAMMA))
    lsl, _ = c.local_seam_leveling(s.adj_ptr, s.adj, labels, pa)
    pa = dict(pa); pa.update(image=lsl["image"], validity=lsl["validity"])
    at, _ = c.texture_atlases(pa, M.default_atlas_params(**GAMMA))
    c.close()
    module, _ = M.texture_atlases(s, labels, tone_mapping="gamma")
    _same(module, at, ATLAS_KEYS, "module-level texture_atlases")
    pngs = [f for f in gamma if f.endswith(".png")]
    assert len(pngs) == len(at["atlas_size"]) >= 1
    differs = False
    for a in range(len(pngs)):
        f = "m_material%04d_map_Kd.png" % a
        assert np.array_equal(PD.decode(gamma[f])[0], M.atlas_view(at, a)), f
        differs = differs or not np.array_equal(PD.decode(none[f])[0], M.atlas_view(at, a))
    assert differs
    # the other module-level calls pass the mode on
    g, _ = M.global_seam_leveling(s, labels, tone_mapping="gamma")
    _same(g, gsl, GSL_KEYS, "module-level global_seam_leveling")
    p, _ = M.texture_patches(s, labels, gsl["corner_adjust"], tone_mapping="gamma")
    l, _ = M.local_seam_leveling(s, labels, tone_mapping="gamma")
    assert np.array_equal(_bits(l["image"]), _bits(lsl["image"])) and np.array_equal(l["validity"], lsl["validity"])
    assert not np.array_equal(_bits(p["image"]), _bits(M.texture_patches(s, labels, gsl["corner_adjust"])[0]["image"]))


def test_the_debug_model_does_not_depend_on_the_mode(tmp_path):
    s = get_scene("tiny")
    labels = _library_labels("tiny", s)
    for mode in ("none", "gamma"):
        os.makedirs(tmp_path / mode)
        M.view_selection_model(s, labels, str(tmp_path / mode / "m"), tone_mapping=mode)
    none, gamma = _files(tmp_path / "none"), _files(tmp_path / "gamma")
    assert len(none) >= 3 and none == gamma
    # the patch values themselves do move: the table at the bytes of the rule
    c = _ctx(s)
    a, _ = c.debug_patches(s.adj_ptr, s.adj, labels)
    b, _ = c.debug_patches(s.adj_ptr, s.adj, labels, params=M.default_patch_params(**GAMMA))
    c.close()
    by = np.rint(a["image"] * np.float32(255.0)).astype(np.uint8)
    assert np.array_equal(_bits(by.astype(np.float32) / np.float32(255.0)), _bits(a["image"]))
    assert np.array_equal(_bits(b["image"]), _bits(M.tone_table("gamma")[by]))
    _same(a, b, [k for k in PATCH_KEYS if k != "image"])
    g = SM.grid_scene()                                                   # frames that leave the view: the fill through the table and back
    gl = SM.grid_labels(g)
    for mode in ("none", "gamma"):
        os.makedirs(tmp_path / ("grid_" + mode))
        M.view_selection_model(g, gl, str(tmp_path / ("grid_" + mode) / "m"), tone_mapping=mode)
    assert _files(tmp_path / "grid_none") == _files(tmp_path / "grid_gamma")
