"""Row f11 on the GPU: Context.build_glb / save_glb and M.texture_model(format="glb" | "both") give, byte for byte, the file that the numpy
restatement of DESIGN.md section 4 "Model output" item 8 (tests/tools/glb_model.py) describes -- on seams written out by hand, on crafted
atlas sets either side of the kernels' 256-thread blocks, with heavy and with hardly any merging, with coordinates above 2^16 and with
10 001 empty atlases, on the suite's scene with the PNGs of save_model embedded -- and every refusal of the item."""
import os

import numpy as np
import pytest

import glb_model as GM
import mvs_texturing_amd as M
import obj_model as OM
from conftest import get_scene

pytestmark = pytest.mark.gpu

VERTS6 = np.array([[0, 0, 0], [1, 0, 0.25], [0, 1, -0.0], [1, 1, 2], [2, 1, -3], [2, 2, 1e-30]], np.float32)
FACES6 = np.array([[0, 1, 2], [2, 1, 3], [3, 4, 5]], np.uint32)
NORMALS6 = np.array([[0, 0, 1], [0, 1, 0], [1, 0, 0], [0, 0, -1], [0, -1, 0], [-0.0, 0.6, 0.8]], np.float32)


def _mesh_ctx(verts, faces):
    verts = np.ascontiguousarray(verts, np.float32).reshape(-1, 3); faces = np.ascontiguousarray(faces, np.uint32).reshape(-1, 3)
    c = M.Context(0)
    c.set_mesh(verts, faces, np.zeros((max(len(faces), 1), 3), np.float32))
    return c


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _check_corners(prims, verts, faces, atl, normals):
    """corner c expanded from the file has the position bits of verts[v(c)], the uv bits of texcoords_merged[g(c)], the normal bits of normals[v(c)]"""
    v, g, atlas = GM.corners(faces, atl)
    merged = np.ascontiguousarray(atl["texcoords_merged"], np.float32).reshape(-1, 2)
    assert sorted(set(atlas.tolist())) == [p["material"] for p in prims]
    for p in prims:
        sel = atlas == p["material"]
        pos, uv, nrm = GM.expand(p)
        assert np.array_equal(_bits(pos), _bits(verts[v[sel]])) and np.array_equal(_bits(uv), _bits(merged[g[sel]]))
        assert (nrm is None) == (normals is None)
        if normals is not None:
            assert np.array_equal(_bits(nrm), _bits(normals[v[sel]]))


def _compare(c, verts, faces, atl, normals=None, pngs=None, params=None, what=""):
    """build_glb against the restatement: the BIN bytes, the JSON, the stats and every corner; returns (file, parsed, stats)"""
    want = GM.restate(verts, faces, atl, normals, pngs)
    data, st = c.build_glb(atl, normals, params)
    got = GM.parse_glb(data)
    assert got["bin"] == want["bin"], what
    assert GM.json_equal(got["json"], want["json"]), what
    assert st["vertices"] == want["vertices"] and st["indices"] == 3 * len(atl["faces"]) and st["primitives"] == len(got["primitives"]), what
    assert st["file_bytes"] == len(data) and st["nonfinite_values"] == 0 and st["json_bytes"] + (8 + len(got["bin"]) if got["bin"] else 0) + 20 == len(data)
    assert st["geometry_bytes"] + st["image_bytes"] == len(got["bin"])
    _check_corners(got["primitives"], np.asarray(verts, np.float32).reshape(-1, 3), faces, atl, None if normals is None else np.asarray(normals, np.float32).reshape(-1, 3))
    return data, got, st


def _one_atlas(faces, ids, n_coords, rng=None):
    merged = np.arange(2 * n_coords, dtype=np.float32).reshape(n_coords, 2) / np.float32(2 * n_coords)
    return dict(face_ptr=np.array([0, len(faces)], np.uint32), faces=np.array(faces, np.uint32), tc_ptr=np.array([0, n_coords], np.uint32), texcoords_merged=merged,
                texcoord_ids=np.array(ids, np.uint32).reshape(-1, 3))


# ---- seams written out by hand ----

def test_shared_edge_with_equal_and_with_different_coordinates():
    c = _mesh_ctx(VERTS6, FACES6)
    atl = _one_atlas([0, 1], [[0, 1, 2], [2, 1, 3]], 4)             # faces (0 1 2) and (2 1 3): the shared vertices 1 and 2 keep their coordinates
    _, g, st = _compare(c, VERTS6, FACES6, atl, NORMALS6)
    p = g["primitives"][0]
    assert st["vertices"] == 4 and p["indices"].tolist() == [0, 1, 2, 2, 1, 3] and np.array_equal(_bits(p["POSITION"]), _bits(VERTS6[:4]))
    atl = _one_atlas([0, 1], [[0, 1, 2], [4, 5, 3]], 6)             # vertex 2 through coordinate 4, vertex 1 through coordinate 5
    _, g, st = _compare(c, VERTS6, FACES6, atl, NORMALS6)
    p = g["primitives"][0]
    assert st["vertices"] == 6 and p["indices"].tolist() == [0, 1, 2, 4, 5, 3]
    assert np.array_equal(_bits(p["POSITION"]), _bits(VERTS6[[0, 1, 2, 3, 2, 1]])) and np.array_equal(_bits(p["NORMAL"]), _bits(NORMALS6[[0, 1, 2, 3, 2, 1]]))
    assert np.array_equal(p["TEXCOORD_0"], atl["texcoords_merged"])
    c.close()


def test_a_vertex_used_by_two_atlases_is_in_both_primitives():
    c = _mesh_ctx(VERTS6, FACES6)
    atl = dict(face_ptr=np.array([0, 1, 2], np.uint32), faces=np.array([0, 1], np.uint32), tc_ptr=np.array([0, 3, 6], np.uint32),
               texcoords_merged=np.linspace(0, 1, 12, dtype=np.float32).reshape(6, 2), texcoord_ids=np.array([[0, 1, 2], [0, 1, 2]], np.uint32))
    _, g, st = _compare(c, VERTS6, FACES6, atl)
    p = g["primitives"]
    assert st["vertices"] == 6 and [q["material"] for q in p] == [0, 1] and p[0]["indices"].tolist() == p[1]["indices"].tolist() == [0, 1, 2]
    assert np.array_equal(_bits(p[0]["POSITION"]), _bits(VERTS6[[0, 1, 2]])) and np.array_equal(_bits(p[1]["POSITION"]), _bits(VERTS6[[2, 1, 3]]))
    assert np.array_equal(p[1]["TEXCOORD_0"], atl["texcoords_merged"][3:])
    acc = g["json"]["accessors"]
    assert acc[0]["min"] == [0, 0, 0] and str(acc[0]["min"][2]) == "-0.0" and acc[0]["max"] == [1, 1, 0.25] and acc[3]["min"] == [0, 0, 0] and acc[3]["max"] == [1, 1, 2]
    c.close()


def test_one_coordinate_used_by_two_vertices_and_one_pair_used_twice():
    c = _mesh_ctx(VERTS6, FACES6)
    atl = _one_atlas([0], [[0, 0, 1]], 2)                           # vertices 0 and 1 both read coordinate 0: two split vertices
    _, g, st = _compare(c, VERTS6, FACES6, atl)
    p = g["primitives"][0]
    assert st["vertices"] == 3 and p["indices"].tolist() == [0, 1, 2] and np.array_equal(p["TEXCOORD_0"], atl["texcoords_merged"][[0, 0, 1]])
    assert np.array_equal(_bits(p["POSITION"]), _bits(VERTS6[[0, 1, 2]]))
    atl = _one_atlas([2, 2], [[0, 1, 2], [0, 1, 2]], 3)             # the same face listed twice: its three pairs once
    _, g, st = _compare(c, VERTS6, FACES6, atl)
    p = g["primitives"][0]
    assert st["vertices"] == 3 and p["indices"].tolist() == [0, 1, 2, 0, 1, 2] and np.array_equal(_bits(p["POSITION"]), _bits(VERTS6[[3, 4, 5]]))
    c.close()


# ---- crafted sets ----

CRAFTED = {
    # name: (vertices, mesh faces, faces per atlas, coordinates per atlas); 85 and 86 faces are 255 and 258 corners, either side of a block
    "heavy_merging": (12, 900, [0, 1, 85, 86, 3000], [0, 2, 7, 9, 40]),
    "hardly_any_merging": (4000, 3500, [0, 1, 85, 86, 3000], [0, 3, 255, 258, 9000]),
    "coordinates_above_2_16": (70000, 30000, [10, 4000], [20, 140000]),
    "empty_atlases_around_one_face": (9, 3, [0] * 5000 + [1] + [0] * 5001, [0] * 5000 + [3] + [0] * 5001),
}


@pytest.mark.parametrize("name", sorted(CRAFTED))
@pytest.mark.parametrize("with_normals", [False, True])
def test_crafted_sets(name, with_normals):
    import torch
    nv, nf, per_atlas, coords = CRAFTED[name]
    rng = np.random.default_rng(len(name))
    verts = (rng.normal(0, 1, (nv, 3)) * 10.0 ** rng.integers(-3, 4, (nv, 3))).astype(np.float32)
    faces = rng.integers(0, nv, (nf, 3)).astype(np.uint32)
    normals = rng.normal(0, 1, (nv, 3)).astype(np.float32) if with_normals else None
    atl = OM.crafted_atlases(rng, nf, per_atlas, coords)
    c = _mesh_ctx(verts, faces)
    data, g, st = _compare(c, verts, faces, atl, normals, what=name)
    assert len(g["primitives"]) == sum(1 for n in per_atlas if n) and len(g["json"]["materials"]) == len(per_atlas)
    if name == "coordinates_above_2_16":
        assert int(atl["texcoord_ids"].max()) > 1 << 16 and st["vertices"] > 1 << 13
    if name == "heavy_merging":
        assert st["vertices"] < st["indices"] // 4
    again, _ = c.build_glb(atl, normals)                            # a second call: the same bytes
    assert again == data
    dev = {k: torch.from_numpy(np.ascontiguousarray(atl[k]).reshape(-1).view(np.int32 if atl[k].dtype == np.uint32 else atl[k].dtype)).cuda() for k in atl}
    dn = torch.from_numpy(normals).cuda() if with_normals else None
    torch.cuda.synchronize()
    from_device, _ = c.build_glb(dev, dn)                           # device inputs: the same bytes
    assert from_device == data
    c.close()


def test_save_glb_writes_the_bytes_of_build_glb(tmp_path):
    rng = np.random.default_rng(2)
    verts = rng.normal(0, 1, (50, 3)).astype(np.float32); faces = rng.integers(0, 50, (40, 3)).astype(np.uint32)
    atl = OM.crafted_atlases(rng, 40, [30, 0, 100], [25, 0, 70])
    c = _mesh_ctx(verts, faces)
    data, _ = c.build_glb(atl)
    st = c.save_glb(atl, tmp_path / "m.glb")
    c.close()
    assert open(tmp_path / "m.glb", "rb").read() == data and st["file_bytes"] == len(data) and sorted(os.listdir(tmp_path)) == ["m.glb"]
    assert st["ms_keys"] > 0 and st["ms_sort"] > 0 and st["ms_number"] > 0 and st["ms_indices"] > 0 and st["ms_gather"] > 0


# ---- the suite's scene ----

_cache = {}


def _tiny():
    """the scene, its labels from the library, vertex normals and row f8's host arrays"""
    if not _cache:
        s = get_scene("tiny")
        c = M.Context(0)
        c.set_mesh(s.verts, s.faces, s.normals); c.set_views(s.cams, s.images)
        c.data_costs(M.Settings())
        labels, _ = c.view_selection(s.adj_ptr, s.adj)
        c.close()
        arrays, _ = M.texture_atlases(s, labels)
        _cache.update(s=s, labels=labels, normals=M.vertex_normals(s.verts, s.faces), arrays=arrays)
    return _cache["s"], _cache["labels"], _cache["normals"], _cache["arrays"]


def _files(d):
    return {n: open(os.path.join(d, n), "rb").read() for n in sorted(os.listdir(d))}


def test_texture_model_formats(tmp_path):
    s, labels, normals, arrays = _tiny()
    for fmt in ("obj", "both", "glb"):
        os.makedirs(tmp_path / fmt)
    st_obj = M.texture_model(s, labels, str(tmp_path / "obj" / "m"), normals)
    st_both = M.texture_model(s, labels, str(tmp_path / "both" / "m"), normals, format="both")
    st_glb = M.texture_model(s, labels, str(tmp_path / "glb" / "m"), normals, format="glb")
    obj, both, glb = _files(tmp_path / "obj"), _files(tmp_path / "both"), _files(tmp_path / "glb")
    A = len(arrays["atlas_size"])
    assert A >= 1 and sorted(obj) == sorted(["m.obj", "m.mtl"] + ["m_material%04d_map_Kd.png" % a for a in range(A)])
    assert sorted(glb) == ["m.glb"]                                 # no .obj, no .mtl, no loose PNG
    assert {k: v for k, v in both.items() if k != "m.glb"} == obj and both["m.glb"] == glb["m.glb"]
    assert isinstance(st_both, tuple) and st_both[0]["bytes"] == st_obj["bytes"] and st_both[1]["file_bytes"] == st_glb["file_bytes"] == len(glb["m.glb"])
    pngs = [obj["m_material%04d_map_Kd.png" % a] for a in range(A)]
    got = GM.parse_glb(glb["m.glb"])
    assert got["images"] == pngs                                    # the files of save_model, byte for byte
    want = GM.restate(s.verts, s.faces, arrays, normals, pngs)
    assert got["bin"] == want["bin"] and GM.json_equal(got["json"], want["json"])
    _check_corners(got["primitives"], s.verts, s.faces, arrays, normals)
    assert st_glb["vertices"] == want["vertices"] and st_glb["ms_png"] > 0


def _libz_loads():
    """whether png_io.h will find zlib: it tries these two names in this order"""
    import ctypes
    for name in ("libz.so.1", "libz.so"):
        try:
            ctypes.CDLL(name)
            return True
        except OSError:
            pass
    return False


HAVE_LIBZ = _libz_loads()
LEGS = [pytest.param("png_device_1", id="png_device_1"),
        pytest.param("png_level_1", id="png_level_1", marks=pytest.mark.skipif(not HAVE_LIBZ, reason="libz.so.1 does not load here"))]


@pytest.mark.parametrize("leg", LEGS)
def test_embedded_pngs_follow_the_params(leg, tmp_path):
    s, labels, normals, arrays = _tiny()
    params = M.default_model_params(png_device=1) if leg == "png_device_1" else M.default_model_params(png_level=1)
    c = _mesh_ctx(s.verts, s.faces)
    c.save_model(arrays, str(tmp_path / "m"), normals, params)
    A = len(arrays["atlas_size"])
    pngs = [open(str(tmp_path / ("m_material%04d_map_Kd.png" % a)), "rb").read() for a in range(A)]
    _, got, _ = _compare(c, s.verts, s.faces, arrays, normals, pngs, params, what=leg)
    c.close()
    assert got["images"] == pngs
    for a in range(A):
        if leg == "png_level_1":
            assert np.array_equal(OM.decode_png(pngs[a])[0], M.atlas_view(arrays, a))
        assert len(pngs[a]) < 3 * int(arrays["atlas_size"][a]) ** 2  # compressed: the default's stored blocks are larger than the pixels


@pytest.mark.skipif(HAVE_LIBZ, reason="libz.so.1 loads here: png_level 1 is not refused")
def test_png_level_without_libz_is_refused_by_both_routes(tmp_path):
    s, labels, normals, arrays = _tiny()
    params = M.default_model_params(png_level=1)
    c = _mesh_ctx(s.verts, s.faces)
    for call in (lambda: c.save_model(arrays, str(tmp_path / "m"), normals, params), lambda: c.build_glb(arrays, normals, params)):
        with pytest.raises(M.MvsError) as e:
            call()
        assert e.value.status == 7 and "libz" in str(e.value)       # MVS_ERR_UNSUPPORTED
    _compare(c, s.verts, s.faces, {k: arrays[k] for k in ("face_ptr", "faces", "tc_ptr", "texcoords_merged", "texcoord_ids")}, normals)
    c.close()


def test_texture_model_refuses_an_unknown_format(tmp_path):
    s, labels, normals, _ = _tiny()
    with pytest.raises(ValueError, match="format"):
        M.texture_model(s, labels, str(tmp_path / "m"), normals, format="gltf")
    assert os.listdir(tmp_path) == []


# ---- refusals ----

def _good_and_bad():
    rng = np.random.default_rng(4)
    verts = rng.normal(0, 1, (30, 3)).astype(np.float32); faces = rng.integers(0, 29, (20, 3)).astype(np.uint32)   # vertex 29 is in no face
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


def test_refusals_of_build_model_and_a_good_call_after_each():
    verts, faces, good, bad = _good_and_bad()
    c = M.Context(0)
    with pytest.raises(M.MvsError) as e:
        c.build_glb(good)
    assert e.value.status == 6                                      # MVS_ERR_STATE: no mesh
    c.set_mesh(verts, faces, np.zeros((20, 3), np.float32))
    want, _, _ = _compare(c, verts, faces, good)
    for what, atl in bad.items():
        with pytest.raises(M.MvsError) as e:
            c.build_glb(atl)
        assert e.value.status == 1, what                            # MVS_ERR_INVALID
        assert c.build_glb(good)[0] == want, what
    c.close()
    wild = faces.copy(); wild[7, 1] = 30                            # a mesh face that names vertex n_verts
    c = _mesh_ctx(verts, wild)
    with pytest.raises(M.MvsError) as e:
        c.build_glb(good)
    assert e.value.status == 1 and "vertex" in str(e.value)
    c.close()


@pytest.mark.parametrize("normals_too", [False, True])
def test_non_finite_values_are_refused_at_referenced_vertices_only(normals_too):
    verts, faces, good, _ = _good_and_bad()
    normals = np.ones((30, 3), np.float32)
    used = np.unique(faces[good["faces"]])
    v_used = int(used[0])
    assert 29 not in used
    for value in (np.inf, -np.inf, np.nan):
        x, n = verts.copy(), normals.copy()
        (n if normals_too else x)[29, 1] = value                    # unreferenced: accepted, and not in the file
        c = _mesh_ctx(x, faces)
        data, _, st = _compare(c, x, faces, good, n)
        (n if normals_too else x)[v_used, 2] = value                # referenced
        c.close()
        c = _mesh_ctx(x, faces)
        with pytest.raises(M.MvsError) as e:
            c.build_glb(good, n)
        assert e.value.status == 7                                  # MVS_ERR_UNSUPPORTED
        want = GM.restate(x, faces, good, n)
        assert e.value.stats["nonfinite_values"] == want["nonfinite"] >= 1 and e.value.stats["vertices"] == want["vertices"] == st["vertices"]
        if normals_too:                                             # without the normals the same mesh is fine
            _compare(c, x, faces, good)
        c.close()


def test_size_refusals_with_stats_filled():
    verts, faces, good, _ = _good_and_bad()
    c = _mesh_ctx(verts, faces)
    data, g, st = _compare(c, verts, faces, good)
    for cap, stage in ((len(data) - 1, "whole file"), (st["geometry_bytes"] + 27, "after the numbering")):
        with pytest.raises(M.MvsError) as e:
            c.build_glb(good, params=M.default_model_params(max_bytes=cap))
        assert e.value.status == 7, stage                           # MVS_ERR_UNSUPPORTED
        es = e.value.stats
        assert es["vertices"] == st["vertices"] and es["indices"] == 60 and es["primitives"] == 2 and es["geometry_bytes"] == st["geometry_bytes"], stage
        assert es["file_bytes"] == (len(data) if stage == "whole file" else 28 + st["geometry_bytes"]), stage
        assert (es["json_bytes"] > 0) == (stage == "whole file")
        assert c.build_glb(good, params=M.default_model_params(max_bytes=len(data)))[0] == data, stage
    # 2^32 - 1 bytes: the indices of 357 913 941 faces alone are more (the arrays are untouched zero pages: the call refuses before it reads them)
    L = 357913941
    huge = dict(face_ptr=np.array([0, L], np.uint32), faces=np.zeros(L, np.uint32), tc_ptr=np.array([0, 1], np.uint32), texcoords_merged=np.zeros((1, 2), np.float32),
                texcoord_ids=np.zeros((L, 3), np.uint32))
    with pytest.raises(M.MvsError) as e:
        c.build_glb(huge)
    assert e.value.status == 7 and e.value.stats["indices"] == 3 * L
    assert c.build_glb(good)[0] == data
    c.close()


def test_png_parameters_are_refused_as_save_model_refuses_them():
    verts, faces, good, _ = _good_and_bad()
    rng = np.random.default_rng(9)
    size = np.array([4, 8, 4], np.uint32)
    pix = np.concatenate([[0], np.cumsum(size.astype(np.uint64) ** 2)]).astype(np.uint64)
    atl = dict(good, atlas_size=size, atlas_pix_ptr=pix, image=rng.integers(0, 256, (int(pix[-1]), 3), dtype=np.uint8))
    c = _mesh_ctx(verts, faces)
    pngs = [bytes(M.encode_png_rle(M.atlas_view(atl, a))) for a in range(3)]
    data, got, _ = _compare(c, verts, faces, atl, None, pngs, M.default_model_params(png_device=1))
    for kw in (dict(png_level=10), dict(png_level=-1), dict(png_device=2), dict(png_device=1, png_level=1)):
        with pytest.raises(M.MvsError) as e:
            c.build_glb(atl, params=M.default_model_params(**kw))
        assert e.value.status == 1, kw
        assert c.build_glb(atl, params=M.default_model_params(png_device=1))[0] == data, kw
    x = dict(atl, atlas_size=np.array([4, 8, 5], np.uint32))        # a size that disagrees with atlas_pix_ptr
    with pytest.raises(M.MvsError) as e:
        c.build_glb(x)
    assert e.value.status == 1
    text_only, _, _ = _compare(c, verts, faces, good)               # and the text-only set: no images, no textures, no samplers
    assert not {"images", "textures", "samplers"} & set(GM.parse_glb(text_only)["json"])
    c.close()
