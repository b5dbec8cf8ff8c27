"""Row f9 on the GPU: Context.build_model / save_model and M.texture_model write, byte for byte, what the CPU model (tests/tools/obj_model.cpp:
upstream's loops with std::ostringstream << std::fixed << std::setprecision(6), DESIGN.md section 4 "Model output") writes -- on the
float grid and 2^20 random bit patterns, on vertex counts around the 256-line blocks of the write kernel and on blocks whose text takes
several passes through its staging buffer, on indices that change their digit count, on text-only atlas sets, on upstream's recorded
files, and on the suite's scenes through rows f5 - f9 -- and every refusal of item 6."""
import os

import numpy as np
import pytest

import mvs_texturing_amd as M
import obj_model as OM
from conftest import get_scene
from test_atlas_model import crafted_sets
from test_obj_model import pins

pytestmark = pytest.mark.gpu

FLT_MAX = np.finfo(np.float32).max


@pytest.fixture(scope="module", autouse=True)
def _model_built():
    OM.build()


def _mesh_ctx(verts, faces=None):
    """a context holding a crafted mesh (no views): faces default to one face of vertex 0; face normals are not read by row f9"""
    verts = np.ascontiguousarray(verts, np.float32).reshape(-1, 3)
    faces = np.zeros((1, 3), np.uint32) if faces is None else np.ascontiguousarray(faces, np.uint32).reshape(-1, 3)
    c = M.Context(0)
    c.set_mesh(verts, faces, np.zeros((max(len(faces), 1), 3), np.float32))
    return c, verts, faces


def _device_host(dev, dtype=np.uint8):
    """a DevArray of the context copied to the host through torch (no copy on the device)"""
    import torch
    dt = np.dtype(dtype)
    n = dev.shape[0]
    if n == 0:
        return np.zeros(0, dt)

    class _Dev:
        __cuda_array_interface__ = {"shape": (n * dt.itemsize,), "typestr": "|u1", "data": (dev.data_ptr(), False), "version": 2}
    return torch.as_tensor(_Dev(), device="cuda").cpu().numpy().view(dt)


def _check_sections(out, st, A):
    """section_ptr / section_bytes against the text itself and the stats"""
    obj = out["obj"]
    sp, sb = out["section_ptr"].astype(np.int64), out["section_bytes"].astype(np.int64)
    assert len(sp) == len(sb) == A + 5 and sp[0] == sb[0] == 0 and sb[-1] == len(obj) and sp[-1] == obj.count(b"\n")
    starts = np.concatenate([[0], np.flatnonzero(np.frombuffer(obj, np.uint8) == 10) + 1])        # byte offset of every line, and the end
    assert np.array_equal(starts[sp], sb)
    for i, k in enumerate(M.viewsel.MODEL_SECTIONS[:4]):
        assert st["lines"][k] == sp[i + 1] - sp[i] and st["bytes"][k] == sb[i + 1] - sb[i], k
    assert st["lines"]["groups"] == sp[-1] - sp[4] and st["bytes"]["groups"] == sb[-1] - sb[4]
    prefix = (b"mtllib ", b"v ", b"vt ", b"vn ") + (b"usemtl ",) * A
    for i, p in enumerate(prefix):
        if sb[i + 1] > sb[i]:
            assert obj.startswith(p, sb[i]), i


def _compare(c, verts, faces, atlases=None, normals=None, name="model", what=""):
    atlases = OM.EMPTY_ATLASES if atlases is None else atlases
    want_obj, want_mtl = OM.run(verts, faces, atlases, normals, name)
    out, st = c.build_model(atlases, normals, name)
    assert out["obj"] == want_obj, what
    assert out["mtl"] == want_mtl, what
    assert st["mtl_bytes"] == len(want_mtl)
    _check_sections(out, st, len(atlases["face_ptr"]) - 1)
    return out, st


def test_floats_grid_and_random_bit_patterns():
    rng = np.random.default_rng(5)
    bits = np.concatenate([OM.float_grid(), rng.integers(0, 1 << 32, 1 << 20, dtype=np.uint64).astype(np.uint32)])
    x = bits.view(np.float32)
    c, verts, faces = _mesh_ctx(OM.pad3(x))
    out, st = _compare(c, verts, faces, what="floats")
    c.close()
    assert OM.v_lines_to_floats(out["obj"])[:64] == OM.snprintf_floats(bits[:9])[:64]               # (the model itself is held to snprintf by tests/test_obj_model.py)
    finite = np.isfinite(x)
    assert st["wide_values"] == int((finite & (np.abs(x) >= np.float32(2.0 ** 64))).sum()) > 0
    assert st["nonfinite_values"] == int((~finite).sum()) > 0
    assert st["lines"]["v"] == len(verts) and st["lines"]["vt"] == st["lines"]["vn"] == st["lines"]["groups"] == 0


@pytest.mark.parametrize("nv", [1, 255, 256, 257, 20000])
def test_block_seams(nv):
    """the header is line 0, so vertex 255 is the first line of the second block; 20 000 lines are 79 blocks"""
    rng = np.random.default_rng(nv)
    verts = (rng.normal(0, 1, (nv, 3)) * 10.0 ** rng.integers(-7, 9, (nv, 3))).astype(np.float32)
    c, verts, faces = _mesh_ctx(verts)
    _compare(c, verts, faces, what=nv)
    c.close()


def test_blocks_of_longest_lines_take_several_passes():
    """every line of several consecutive blocks is 146 bytes (three times -FLT_MAX): 256 of them are 37 376 bytes, more than the write
    kernel's staging buffer holds at once"""
    verts = np.full((256 * 5 + 77, 3), -FLT_MAX, np.float32)
    c, verts, faces = _mesh_ctx(verts)
    out, st = _compare(c, verts, faces, what="longest")
    c.close()
    lines = out["obj"].split(b"\n")[1:-1]
    assert set(len(s) + 1 for s in lines) == {146}
    assert st["wide_values"] == verts.size


def test_alternating_shortest_and_longest_lines():
    """a `v` line is at least 29 bytes (three values of 8 bytes, "0.000000"; 30 with one "-0.000000") and at most 146: 30 and
    146 alternate here, so the lines that fit the staging buffer end at a different place in every pass"""
    verts = np.zeros((256 * 4 + 31, 3), np.float32)
    verts[1::2] = -FLT_MAX
    verts[::2, 1] = -0.0
    c, verts, faces = _mesh_ctx(verts)
    out, _ = _compare(c, verts, faces, what="alternating")
    c.close()
    lens = [len(s) + 1 for s in out["obj"].split(b"\n")[1:-1]]
    assert lens[:4] == [30, 146, 30, 146] and b"v 0.000000 -0.000000 0.000000\n" in out["obj"]


def test_indices_change_their_digit_count():
    """100 001 vertices: vertex and texcoord indices cross 9|10, 99|100, ..., 99 999|100 000, the second atlas's behind its tc_ptr offset"""
    rng = np.random.default_rng(11)
    NV = 100001
    verts = rng.normal(0, 2, (NV, 3)).astype(np.float32)
    faces = ((np.arange(NV, dtype=np.int64)[:, None] + np.array([0, 1, 2])) % NV).astype(np.uint32)
    n0 = 99990
    atl = dict(face_ptr=np.array([0, n0, NV], np.uint32), faces=np.arange(NV, dtype=np.uint32), tc_ptr=np.array([0, n0, NV + 7], np.uint32),
               texcoords_merged=rng.uniform(0, 1, (NV + 7, 2)).astype(np.float32), texcoord_ids=np.zeros((NV, 3), np.uint32))
    atl["texcoord_ids"][:n0] = (np.arange(n0)[:, None] + np.array([0, 1, 2])) % n0
    atl["texcoord_ids"][n0:] = (np.arange(NV - n0)[:, None] + np.array([0, 5, 17])) % (NV + 7 - n0)
    c, verts, faces = _mesh_ctx(verts, faces)
    normals = M.vertex_normals(verts, faces)
    out, st = _compare(c, verts, faces, atl, normals, what="digits")
    for text in (b"f 9/9/9 10/10/10 11/11/11\n", b"f 99/99/99 100/100/100 ", b"f 99999/99999/99999 100000/100004/100000 100001/99998/100001\n", b"/99990/", b"f 99991/99991/99991 99992/99996/99992 "):
        assert text in out["obj"], text
    out2, _ = _compare(c, verts, faces, atl, None, what="digits without normals")
    assert b"vn " not in out2["obj"] and b"f 9/9 10/10 11/11\n" in out2["obj"] and out2["section_ptr"][3] == out2["section_ptr"][4]
    c.close()
    cnt = OM.parse_obj(out["obj"])
    assert cnt == dict(v=NV, vt=NV + 7, vn=NV, usemtl=2, f=NV)
    assert st["lines"]["groups"] == NV + 2


def test_ten_thousand_and_one_empty_atlases():
    A = 10001
    atl = dict(OM.EMPTY_ATLASES, face_ptr=np.zeros(A + 1, np.uint32), tc_ptr=np.zeros(A + 1, np.uint32))
    c, verts, faces = _mesh_ctx(np.arange(12, dtype=np.float32))
    out, st = _compare(c, verts, faces, atl, name="many", what="empty atlases")
    c.close()
    assert out["obj"].endswith(b"usemtl material9999\nusemtl material10000\n") and out["mtl"].endswith(b"map_Kd many_material10000_map_Kd.png\n")
    assert st["lines"]["groups"] == A


@pytest.mark.parametrize("name", ["some_faceless", "mixed_sizes"])
def test_text_only_sets_from_row_f8(name):
    """row f8's arrays for two crafted patch sets (an atlas set with faceless patches; two atlases: tc_ptr offsets), then text only"""
    pa = crafted_sets()[name]
    rng = np.random.default_rng(3)
    F = int(np.asarray(pa["faces"]).max()) + 1
    c, verts, faces = _mesh_ctx(rng.normal(0, 1, (F + 2, 3)), rng.integers(0, F + 2, (F, 3)))
    arrays, _ = c.texture_atlases(pa)
    atl = {k: arrays[k] for k in ("face_ptr", "faces", "tc_ptr", "texcoords_merged", "texcoord_ids")}      # no image, no atlas_size
    _compare(c, verts, faces, atl, M.vertex_normals(verts, faces), what=name)
    if name == "mixed_sizes":
        assert len(atl["face_ptr"]) == 3 and atl["tc_ptr"][1] > 0
    c.close()


def test_upstream_pins_on_the_device():
    seen = 0
    for name, v, f, n, atl, prefix, obj, mtl in pins():
        c, v, f = _mesh_ctx(v, f)
        out, _ = c.build_model(atl, n, prefix.rsplit("/", 1)[-1])
        c.close()
        assert out["obj"] == obj, name
        assert out["mtl"] == mtl, name
        seen += 1
    assert seen == 6


_labels_cache = {}


def _library_labels(name, s):
    if name not in _labels_cache:
        c = M.Context(0)
        c.set_mesh(s.verts, s.faces, s.normals); c.set_views(s.cams, s.images)
        c.data_costs(M.Settings())
        _labels_cache[name], _ = c.view_selection(s.adj_ptr, s.adj)
        c.close()
    return _labels_cache[name]


@pytest.mark.parametrize("name", ["tiny", "bumpy"])
@pytest.mark.parametrize("shuffled", [False, True])
def test_scenes_through_texture_model(name, shuffled, tmp_path):
    s = get_scene(name)
    labels = _library_labels(name, s)
    if shuffled:
        s = M.synth.permute_scene(s, seed=7)
        labels = labels[s.face_perm]
    normals = M.vertex_normals(s.verts, s.faces)
    os.makedirs(tmp_path / "out.dir")
    prefix = str(tmp_path / "out.dir" / ("scene_" + name))
    st = M.texture_model(s, labels, prefix, normals)
    arrays, _ = M.texture_atlases(s, labels)                       # row f8's host arrays
    want_obj, want_mtl = OM.run(s.verts, s.faces, arrays, normals, "scene_" + name)
    obj = open(prefix + ".obj", "rb").read()
    assert obj == want_obj and open(prefix + ".mtl", "rb").read() == want_mtl
    A = len(arrays["atlas_size"])
    assert A >= 1 and sorted(os.listdir(tmp_path / "out.dir")) == sorted(["scene_%s.obj" % name, "scene_%s.mtl" % name] + ["scene_%s_material%04d_map_Kd.png" % (name, a) for a in range(A)])
    for a in range(A):
        img, _ = OM.decode_png(open("%s_material%04d_map_Kd.png" % (prefix, a), "rb").read())
        assert np.array_equal(img, M.atlas_view(arrays, a)), a
    cnt = OM.parse_obj(obj)                                         # the grammar of item 1, every index within its section's count
    assert cnt == dict(v=len(s.verts), vt=len(arrays["texcoords_merged"]), vn=len(s.verts), usemtl=A, f=len(arrays["faces"]))
    assert st["bytes"]["header"] + st["bytes"]["v"] + st["bytes"]["vt"] + st["bytes"]["vn"] + st["bytes"]["groups"] == len(obj)
    assert st["ms_measure"] > 0 and st["ms_scan"] > 0 and st["ms_write"] > 0 and st["ms_png"] > 0


def test_compressed_pngs_hold_the_same_pixels(tmp_path):
    s = get_scene("tiny")
    labels = _library_labels("tiny", s)
    c = M.Context(0)
    arrays, _ = M.texture_atlases(s, labels, ctx=c)
    try:
        c.save_model(arrays, str(tmp_path / "z"), params=M.default_model_params(png_level=6))
    except M.MvsError as e:
        assert e.status == 7 and "libz" in str(e)                   # MVS_ERR_UNSUPPORTED where libz.so.1 does not resolve
        return
    finally:
        c.close()
    for a in range(len(arrays["atlas_size"])):
        img, _ = OM.decode_png(open(str(tmp_path / ("z_material%04d_map_Kd.png" % a)), "rb").read())
        assert np.array_equal(img, M.atlas_view(arrays, a))


def test_host_and_device_inputs_outputs_and_repeat():
    import torch
    s = get_scene("tiny")
    labels = _library_labels("tiny", s)
    c = M.Context(0)
    arrays, _ = M.texture_atlases(s, labels, ctx=c)
    normals = M.vertex_normals(s.verts, s.faces)
    a, ast = _compare(c, s.verts, s.faces, arrays, normals, what="host")
    b, _ = c.build_model(arrays, normals)
    assert b["obj"] == a["obj"] and b["mtl"] == a["mtl"]
    dev = {k: torch.from_numpy(np.ascontiguousarray(arrays[k]).reshape(-1).view(np.int32 if arrays[k].dtype == np.uint32 else arrays[k].dtype)).cuda()
           for k in ("face_ptr", "faces", "tc_ptr", "texcoords_merged", "texcoord_ids")}
    dn = torch.from_numpy(normals).cuda()
    torch.cuda.synchronize()
    d, dst = c.build_model(dev, dn)
    assert d["obj"] == a["obj"] and d["mtl"] == a["mtl"]
    e, est = c.build_model(dev, dn, on_device=True)
    c.synchronize()
    assert _device_host(e["obj"]).tobytes() == a["obj"] and _device_host(e["mtl"]).tobytes() == a["mtl"]
    assert np.array_equal(e["section_bytes"], a["section_bytes"]) and np.array_equal(e["section_ptr"], a["section_ptr"])
    for k in ("lines", "bytes", "mtl_bytes", "wide_values", "nonfinite_values"):
        assert est[k] == ast[k], k
    n, _ = c.build_model(arrays, None)
    assert b"vn " not in n["obj"] and n["obj"].split(b"\n")[-2].count(b"/") == 3 and OM.parse_obj(n["obj"])["vn"] == 0
    assert n["obj"] == OM.run(s.verts, s.faces, arrays, None)[0]
    c.close()


def _good_and_bad():
    rng = np.random.default_rng(4)
    verts = rng.normal(0, 1, (30, 3)).astype(np.float32); faces = rng.integers(0, 30, (20, 3)).astype(np.uint32)
    good = OM.crafted_atlases(rng, 20, [8, 0, 12], [10, 0, 9])
    bad = {}
    x = {k: v.copy() for k, v in good.items()}; x["faces"][5] = 20; bad["face id == n_faces"] = x
    x = {k: v.copy() for k, v in good.items()}; x["texcoord_ids"][3, 1] = 10; bad["texcoord id == its atlas's count"] = x
    x = {k: v.copy() for k, v in good.items()}; x["texcoord_ids"][19, 2] = 9; bad["texcoord id of the last atlas"] = x
    x = {k: v.copy() for k, v in good.items()}; x["face_ptr"][0] = 1; bad["face_ptr starts at 1"] = x
    x = {k: v.copy() for k, v in good.items()}; x["face_ptr"][-1] = 19; bad["face_ptr ends before the total"] = x
    x = {k: v.copy() for k, v in good.items()}; x["face_ptr"][1] = 13; x["face_ptr"][2] = 8; bad["face_ptr descends"] = x
    x = {k: v.copy() for k, v in good.items()}; x["tc_ptr"][0] = 2; bad["tc_ptr starts at 2"] = x
    x = {k: v.copy() for k, v in good.items()}; x["tc_ptr"][-1] = 18; bad["tc_ptr ends before the total"] = x
    return verts, faces, good, bad


def test_refusals_and_a_good_call_after_each():
    verts, faces, good, bad = _good_and_bad()
    c = M.Context(0)
    with pytest.raises(M.MvsError) as e:
        c.build_model(good)
    assert e.value.status == 6                                      # MVS_ERR_STATE: no mesh
    c.set_mesh(verts, faces, np.zeros((20, 3), np.float32))
    want = OM.run(verts, faces, good)
    for what, atl in bad.items():
        with pytest.raises(M.MvsError) as e:
            c.build_model(atl)
        assert e.value.status == 1, what                            # MVS_ERR_INVALID
        out, _ = c.build_model(good)
        assert (out["obj"], out["mtl"]) == want, what
    with pytest.raises(M.MvsError) as e:
        c.build_model(good, name="n" * 256)
    assert e.value.status == 1
    c.close()


def test_max_bytes_refuses_with_stats_filled():
    verts, faces, good, _ = _good_and_bad()
    c = M.Context(0)
    c.set_mesh(verts, faces, np.zeros((20, 3), np.float32))
    obj, mtl = OM.run(verts, faces, good)
    with pytest.raises(M.MvsError) as e:
        c.build_model(good, params=M.default_model_params(max_bytes=len(obj) - 1))
    assert e.value.status == 7                                      # MVS_ERR_UNSUPPORTED, after the measuring pass
    st = e.value.stats
    assert sum(st["bytes"].values()) == len(obj) and st["lines"]["v"] == 30 and st["lines"]["groups"] == 23 and st["mtl_bytes"] == len(mtl)
    out, _ = c.build_model(good, params=M.default_model_params(max_bytes=len(obj)))
    assert out["obj"] == obj
    c.close()


def test_write_png_from_the_library(tmp_path):
    rng = np.random.default_rng(1)
    img = rng.integers(0, 256, (37, 53, 3), dtype=np.uint8)
    M.write_png(tmp_path / "a.png", img)
    got, _ = OM.decode_png(open(tmp_path / "a.png", "rb").read())
    assert np.array_equal(got, img)
    with pytest.raises(M.MvsError):
        M.write_png(tmp_path / "missing" / "a.png", img)
