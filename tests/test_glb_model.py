"""Row f11 without a GPU: the numpy restatement of DESIGN.md section 4 "Model output" item 8 (tests/tools/glb_model.py) against vertices
and indices written out by hand, the strict .glb parser on the restatement's own files, and the parser's rejections."""
import os
import struct

import numpy as np
import pytest

import glb_model as GM
import mvs_texturing_amd as M

VERTS = np.array([[0, 0, 0], [1, 0, 0], [1, 1, -0.0], [0, 1, 0.5]], np.float32)
MESH_FACES = np.array([[0, 1, 2], [0, 2, 3]], np.uint32)
MERGED = np.array([[0.1, 0.1], [0.9, 0.1], [0.9, 0.9], [0.1, 0.9], [0.5, 0.5]], np.float32)


def _two_triangles(seam):
    """one atlas, both faces; with `seam` the second face reads vertex 0 through coordinate 4 instead of coordinate 0"""
    ids = np.array([[0, 1, 2], [4 if seam else 0, 2, 3]], np.uint32)
    return dict(face_ptr=np.array([0, 2], np.uint32), faces=np.array([0, 1], np.uint32), tc_ptr=np.array([0, 5], np.uint32), texcoords_merged=MERGED, texcoord_ids=ids)


def test_two_triangles_by_hand():
    r = GM.restate(VERTS, MESH_FACES, _two_triangles(False))
    p = GM.parse_glb(GM.assemble(r["json"], r["bin"]))["primitives"]
    assert r["vertices"] == 4 and len(p) == 1 and p[0]["material"] == 0
    assert p[0]["indices"].tolist() == [0, 1, 2, 0, 2, 3]
    assert np.array_equal(p[0]["POSITION"].view(np.uint32), VERTS.view(np.uint32))
    assert np.array_equal(p[0]["TEXCOORD_0"], MERGED[:4]) and "NORMAL" not in p[0]
    # the seam splits vertex 0: pairs in ascending coordinate are (0, v0) (1, v1) (2, v2) (3, v3) (4, v0)
    normals = np.array([[0, 0, 1], [0, 1, 0], [1, 0, 0], [0, 0, -1]], np.float32)
    r = GM.restate(VERTS, MESH_FACES, _two_triangles(True), normals)
    g = GM.parse_glb(GM.assemble(r["json"], r["bin"]))
    p = g["primitives"]
    assert r["vertices"] == 5 and p[0]["indices"].tolist() == [0, 1, 2, 4, 2, 3]
    assert np.array_equal(p[0]["POSITION"].view(np.uint32), VERTS[[0, 1, 2, 3, 0]].view(np.uint32))
    assert np.array_equal(p[0]["TEXCOORD_0"], MERGED) and np.array_equal(p[0]["NORMAL"], normals[[0, 1, 2, 3, 0]])
    acc = g["json"]["accessors"]
    assert acc[0]["min"] == [0.0, 0.0, 0.0] and acc[0]["max"] == [1.0, 1.0, 0.5]
    assert str(acc[0]["min"][2]) == "-0.0"                          # -0 < +0 in the order of the integer images
    assert [a["count"] for a in acc] == [5, 5, 5, 6] and len(r["bin"]) == 5 * 32 + 24
    assert g["json"]["materials"] == [{"name": "material0000", "pbrMetallicRoughness": {"metallicFactor": 0, "roughnessFactor": 1}}]
    assert "images" not in g["json"] and "textures" not in g["json"] and "samplers" not in g["json"]
    pos, uv, nrm = GM.expand(p[0])
    v, gc, _ = GM.corners(MESH_FACES, _two_triangles(True))
    assert np.array_equal(pos, VERTS[v]) and np.array_equal(uv, MERGED[gc]) and np.array_equal(nrm, normals[v])


def test_two_atlases_images_and_an_empty_atlas():
    """vertex 0 and vertex 2 are used by atlas 0 and by atlas 2; atlas 1 has no faces: a material and an image, no primitive"""
    atl = dict(face_ptr=np.array([0, 1, 1, 2], np.uint32), faces=np.array([0, 1], np.uint32), tc_ptr=np.array([0, 3, 3, 6], np.uint32),
               texcoords_merged=np.linspace(0, 1, 12, dtype=np.float32).reshape(6, 2), texcoord_ids=np.array([[0, 1, 2], [2, 1, 0]], np.uint32))
    pngs = [GM.PNG_SIG + bytes([a]) * (5 + a) for a in range(3)]
    r = GM.restate(VERTS, MESH_FACES, atl, None, pngs)
    g = GM.parse_glb(GM.assemble(r["json"], r["bin"]))
    p = g["primitives"]
    assert [q["material"] for q in p] == [0, 2] and r["first"].tolist() == [0, 3, 3, 6]
    assert p[0]["indices"].tolist() == [0, 1, 2] and p[1]["indices"].tolist() == [2, 1, 0]
    assert np.array_equal(p[0]["POSITION"], VERTS[[0, 1, 2]]) and np.array_equal(p[1]["POSITION"], VERTS[[3, 2, 0]])
    assert g["images"] == pngs and len(g["json"]["materials"]) == 3 and g["json"]["materials"][1]["pbrMetallicRoughness"]["baseColorTexture"] == {"index": 1}
    assert g["json"]["images"][0]["bufferView"] == 3 and g["json"]["buffers"][0]["byteLength"] == len(r["bin"]) - 1   # 8 + 7 bytes: one byte of padding
    # no face at all: no meshes, no nodes, the scene is {}
    none = dict(atl, face_ptr=np.zeros(4, np.uint32), faces=np.zeros(0, np.uint32), texcoord_ids=np.zeros((0, 3), np.uint32))
    r = GM.restate(VERTS, MESH_FACES, none, None, pngs)
    g = GM.parse_glb(GM.assemble(r["json"], r["bin"]))
    assert g["primitives"] == [] and g["json"]["scenes"] == [{}] and "meshes" not in g["json"] and g["images"] == pngs
    r = GM.restate(VERTS, MESH_FACES, none)
    assert r["bin"] == b"" and "buffers" not in r["json"] and GM.parse_glb(GM.assemble(r["json"], r["bin"]))["images"] == []


def test_parser_rejections():
    r = GM.restate(VERTS, MESH_FACES, _two_triangles(True))
    good = GM.assemble(r["json"], r["bin"])
    GM.parse_glb(good)
    with pytest.raises(AssertionError, match="length"):             # the header's length field
        GM.parse_glb(good[:8] + struct.pack("<I", len(good) + 4) + good[12:])
    with pytest.raises(AssertionError, match="length"):             # a file cut short
        GM.parse_glb(good[:-4])
    n_json = struct.unpack_from("<I", good, 12)[0]
    text = good[20:20 + n_json].rstrip(b" ")
    assert len(text) % 4, "the case needs a JSON text that takes padding"
    unpadded = struct.pack("<II", len(text), GM.JSON_CHUNK) + text + good[20 + n_json:]
    with pytest.raises(AssertionError):                             # an unpadded chunk
        GM.parse_glb(struct.pack("<III", GM.MAGIC, 2, 12 + len(unpadded)) + unpadded)
    with pytest.raises(AssertionError, match="padding"):            # padded with zeros instead of spaces
        GM.parse_glb(good[:20] + good[20:20 + n_json].rstrip(b" ").ljust(n_json, b"\0") + good[20 + n_json:])
    bad = bytearray(r["bin"])
    bad[-4:] = struct.pack("<I", 5)                                 # the last index: 5 vertices, so 5 is out of range
    with pytest.raises(AssertionError, match="index out of range"):
        GM.parse_glb(GM.assemble(r["json"], bytes(bad)))
    j = dict(r["json"], accessors=[dict(a) for a in r["json"]["accessors"]])
    j["accessors"][0]["min"] = [0.0, 0.0, 0.0]                      # +0 where the data's minimum is -0
    with pytest.raises(AssertionError, match="min"):
        GM.parse_glb(GM.assemble(j, r["bin"]))
    j = dict(r["json"], bufferViews=[dict(v) for v in r["json"]["bufferViews"]])
    j["bufferViews"][2]["byteLength"] += 4
    with pytest.raises(AssertionError, match="outside the buffer"):
        GM.parse_glb(GM.assemble(j, r["bin"]))


def test_entry_points_are_declared():
    if not os.path.exists(M.lib_path()):
        pytest.skip("HIP library not built (run __graft_entry__.build())")
    L = M.load_library()
    for name in ("mvs_ctx_build_glb", "mvs_ctx_save_glb", "mvs_glb_free"):
        assert name in L._declared and getattr(L, name).argtypes is not None, name
    assert hasattr(M.Context, "build_glb") and hasattr(M.Context, "save_glb")
    st = M.viewsel.GlbStats()
    assert C_sizeof(st) == 8 * 8 + 8 * 4 and C_sizeof(M.viewsel.Glb()) == 16      # mvs_glb_stats, mvs_glb of include/mvs_viewsel.h


def C_sizeof(x):
    import ctypes
    return ctypes.sizeof(x)


def test_texture_model_checks_its_format_before_anything_runs():
    """no scene is read and no context is made for a format that is not "obj", "glb" or "both" """
    import inspect
    assert inspect.signature(M.texture_model).parameters["format"].default == "obj"
    for bad in ("gltf", "OBJ", "", None):
        with pytest.raises(ValueError, match="format"):
            M.texture_model(None, None, "unused", format=bad)
