"""Row f11 under glb_quantize = 1 without a GPU: the numpy restatement of DESIGN.md section 4 "Model output" item 10
(tests/tools/glb_quant_model.py) against itself and against the definition -- every file it builds passes the strict readers, every part
and index range starts at a multiple of 4, min / max are the stored integers' own, dequantised values lie within the item's bounds, and
the rounding cases come out as exact arithmetic says."""
import ctypes
import os
from fractions import Fraction

import numpy as np
import pytest

import glb_model as GM
import glb_quant_model as QM
import mvs_texturing_amd as M
import obj_model as OM

VERTS = np.array([[0, 0, 0], [1, 0, 0], [1, 1, -0.0], [0, 1, 0.5]], np.float32)
MESH_FACES = np.array([[0, 1, 2], [0, 2, 3]], np.uint32)
MERGED = np.array([[0.1, 0.1], [0.9, 0.1], [0.9, 0.9], [0.1, 0.9], [0.5, 0.5]], np.float32)
NORMALS = np.array([[0, 0, 1], [0, 1, 0], [1, 0, 0], [0, 0, -1]], np.float32)


def _file(r):
    return GM.assemble(r["json"], r["bin"])


def _check_file(verts, faces, atl, normals, r):
    """the file of a restatement through the strict readers, its alignment, and every corner dequantised within the item's bounds"""
    g = QM.parse_glb(_file(r))
    for v in g["json"].get("bufferViews", []):
        assert v["byteOffset"] % 4 == 0
    for a in g["json"].get("accessors", []):
        assert a["byteOffset"] % 4 == 0
    verts = np.ascontiguousarray(verts, np.float32).reshape(-1, 3)
    merged = np.ascontiguousarray(atl["texcoords_merged"], np.float32).reshape(-1, 2)
    v, gc, atlas = GM.corners(faces, atl)
    assert sorted(set(atlas.tolist())) == [p["material"] for p in g["primitives"]]
    for p in g["primitives"]:
        sel = atlas == p["material"]
        pos, uv, nrm = QM.expand(g, p)
        x = verts[v[sel]].astype(np.float64)
        assert np.all(np.abs(pos - x) <= QM.position_bound(x, g["translation"].astype(np.float64)[None, :], g["scale"]))
        assert np.all(np.abs(uv - merged[gc[sel]].astype(np.float64)) <= QM.TEXCOORD_BOUND)
        assert (nrm is None) == (normals is None)
        if normals is not None:
            n = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)[v[sel]].astype(np.float64)
            l = np.sqrt((n * n).sum(1))
            unit = n / np.where(l == 0, 1.0, l)[:, None]
            assert np.all(np.abs(nrm - unit) <= QM.NORMAL_BOUND)
    return g


def _two_triangles(seam):
    ids = np.array([[0, 1, 2], [4 if seam else 0, 2, 3]], np.uint32)
    return dict(face_ptr=np.array([0, 2], np.uint32), faces=np.array([0, 1], np.uint32), tc_ptr=np.array([0, 5], np.uint32), texcoords_merged=MERGED, texcoord_ids=ids)


def test_two_triangles_by_hand():
    atl = _two_triangles(True)
    r = QM.restate(VERTS, MESH_FACES, atl, NORMALS)
    g = _check_file(VERTS, MESH_FACES, atl, NORMALS, r)
    p = g["primitives"][0]
    # pairs (0, v0) (1, v1) (2, v2) (3, v3) (4, v0); the grid: lo = (0, 0, -0), E = 1, S = 1 / 65535
    assert r["vertices"] == 5 and p["indices"].tolist() == [0, 1, 2, 4, 2, 3] and p["index_bytes"] == 2 and r["index16_primitives"] == 1
    assert p["POSITION"].tolist() == [[0, 0, 0], [65535, 0, 0], [65535, 65535, 0], [0, 65535, 32768], [0, 0, 0]]   # 0.5 * 65535 + 0.5 = 32768
    assert p["NORMAL"].tolist() == [[0, 0, 127], [0, 127, 0], [127, 0, 0], [0, 0, -127], [0, 0, 127]]
    assert p["TEXCOORD_0"].tolist() == [[int(Fraction(float(u)) * 65535 + Fraction(1, 2)) for u in row] for row in MERGED]
    node = g["json"]["nodes"][0]
    assert node["translation"] == [0.0, 0.0, 0.0] and str(node["translation"][2]) == "-0.0" and node["scale"] == [1.0 / 65535.0] * 3
    acc = g["json"]["accessors"]
    assert acc[0]["min"] == [0, 0, 0] and acc[0]["max"] == [65535, 65535, 32768]
    assert [a["count"] for a in acc] == [5, 5, 5, 6] and [a["componentType"] for a in acc] == [5123, 5123, 5120, 5123]
    assert len(r["bin"]) == 5 * 16 + 12 and [v.get("byteStride") for v in g["json"]["bufferViews"]] == [8, 4, 4, None]
    assert r["zero_normals"] == 0 and r["texcoords_out_of_range"] == 0
    # without normals: 12 bytes per vertex
    r = QM.restate(VERTS, MESH_FACES, atl)
    _check_file(VERTS, MESH_FACES, atl, None, r)
    assert len(r["bin"]) == 5 * 12 + 12


def test_two_atlases_share_one_grid_and_a_one_face_atlas_is_padded():
    """vertex 0 and vertex 2 are in atlas 0 and in atlas 2: the same stored triple in both primitives; atlas 0's one face takes 6 index
    bytes and 2 of padding, so that atlas 2's indices start at byte 8; images behind the geometry as in item 8"""
    atl = dict(face_ptr=np.array([0, 1, 1, 2], np.uint32), faces=np.array([0, 1], np.uint32), tc_ptr=np.array([0, 3, 3, 6], np.uint32),
               texcoords_merged=np.linspace(0, 1, 12, dtype=np.float32).reshape(6, 2), texcoord_ids=np.array([[0, 1, 2], [2, 1, 0]], np.uint32))
    pngs = [GM.PNG_SIG + bytes([a]) * (5 + a) for a in range(3)]
    r = QM.restate(VERTS, MESH_FACES, atl, None, pngs)
    g = _check_file(VERTS, MESH_FACES, atl, None, r)
    p = g["primitives"]
    assert [q["material"] for q in p] == [0, 2] and p[0]["indices"].tolist() == [0, 1, 2] and p[1]["indices"].tolist() == [2, 1, 0]
    assert p[0]["POSITION"][0].tolist() == p[1]["POSITION"][2].tolist() and p[0]["POSITION"][2].tolist() == p[1]["POSITION"][1].tolist()   # v0, v2
    acc = g["json"]["accessors"]
    assert [acc[2]["byteOffset"], acc[5]["byteOffset"]] == [0, 8] and g["json"]["bufferViews"][2]["byteLength"] == 16
    assert acc[0]["max"] == [65535, 65535, 0] and acc[3]["min"] == [0, 0, 0] and acc[3]["max"] == [65535, 65535, 32768]   # per primitive, of the stored integers
    assert g["images"] == pngs and g["json"]["images"][0]["bufferView"] == 3 and g["json"]["materials"][1]["pbrMetallicRoughness"]["baseColorTexture"] == {"index": 1}
    want8 = GM.restate(VERTS, MESH_FACES, atl, None, pngs)
    assert g["json"]["materials"] == want8["json"]["materials"] and g["json"]["textures"] == want8["json"]["textures"]
    # JPEG files: the mime type changes, nothing else
    jpgs = [QM.JPEG_SIG + bytes([a]) * (3 + a) for a in range(3)]
    g = QM.parse_glb(_file(QM.restate(VERTS, MESH_FACES, atl, None, jpgs, "image/jpeg")))
    assert g["images"] == jpgs and {im["mimeType"] for im in g["json"]["images"]} == {"image/jpeg"}
    # no face at all: no meshes, no nodes, the scene is {} -- and still the extension
    none = dict(atl, face_ptr=np.zeros(4, np.uint32), faces=np.zeros(0, np.uint32), texcoord_ids=np.zeros((0, 3), np.uint32))
    g = QM.parse_glb(_file(QM.restate(VERTS, MESH_FACES, none, None, pngs)))
    assert g["primitives"] == [] and g["json"]["scenes"] == [{}] and g["images"] == pngs


@pytest.mark.parametrize("with_normals", [False, True])
def test_random_sets_within_the_bounds(with_normals):
    for seed, (nv, nf, per_atlas, coords) in enumerate([(12, 900, [0, 1, 85, 86, 3000], [0, 2, 7, 9, 40]), (4000, 3500, [0, 1, 85, 86, 3000], [0, 3, 255, 258, 9000])]):
        rng = np.random.default_rng(seed)
        verts = (rng.normal(0, 1, (nv, 3)) * 10.0 ** rng.integers(-3, 4, (nv, 3))).astype(np.float32)
        faces = rng.integers(0, nv, (nf, 3)).astype(np.uint32)
        normals = (rng.normal(0, 1, (nv, 3)) * 10.0 ** rng.integers(-10, 10, (nv, 1))).astype(np.float32) if with_normals else None
        atl = OM.crafted_atlases(rng, nf, per_atlas, coords)
        r = QM.restate(verts, faces, atl, normals)
        g = _check_file(verts, faces, atl, normals, r)
        assert r["index16_primitives"] == len(g["primitives"]) == 4
        want8 = GM.restate(verts, faces, atl, normals)
        assert r["vertices"] == want8["vertices"]
        assert len(r["bin"]) == r["vertices"] * (16 if with_normals else 12) + sum((6 * n + 3) // 4 * 4 for n in per_atlas)


def test_index_widths_follow_the_vertex_counts():
    """65 535 vertices: 16 bits (the largest index is 65 534); 65 536: 32 bits; a wide primitive between two narrow ones"""
    def strip(n):                                                   # n vertices, n - 2 faces, every pair its own coordinate
        return np.stack([np.arange(n - 2), np.arange(1, n - 1), np.arange(2, n)], 1).astype(np.uint32)
    for counts, widths in (([65535], [2]), ([65536], [4]), ([300, 65536, 5], [2, 4, 2])):
        nv = max(counts)
        verts = np.random.default_rng(1).normal(0, 1, (nv, 3)).astype(np.float32)
        faces = strip(nv)
        listed = [np.arange(n - 2, dtype=np.uint32) for n in counts]
        atl = dict(face_ptr=np.concatenate([[0], np.cumsum([len(x) for x in listed])]).astype(np.uint32), faces=np.concatenate(listed),
                   tc_ptr=np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32),
                   texcoords_merged=np.random.default_rng(2).uniform(0, 1, (sum(counts), 2)).astype(np.float32),
                   texcoord_ids=np.concatenate([strip(n) for n in counts]))
        r = QM.restate(verts, faces, atl)
        g = QM.parse_glb(_file(r))
        assert [p["index_bytes"] for p in g["primitives"]] == widths and [len(p["POSITION"]) for p in g["primitives"]] == counts
        assert r["index16_primitives"] == widths.count(2)
        assert [int(p["indices"].max()) for p in g["primitives"]] == [n - 1 for n in counts]
        view = g["json"]["bufferViews"][2]
        assert view["byteLength"] == sum((w * 3 * (n - 2) + 3) // 4 * 4 for w, n in zip(widths, counts))


def test_degenerate_grids():
    one = np.array([[3.5, -2.0, 1e-40]] * 3, np.float32)            # E == 0 (a subnormal among the values)
    atl = dict(face_ptr=np.array([0, 1], np.uint32), faces=np.array([0], np.uint32), tc_ptr=np.array([0, 1], np.uint32),
               texcoords_merged=np.array([[0.25, 0.75]], np.float32), texcoord_ids=np.zeros((1, 3), np.uint32))
    r = QM.restate(one, np.array([[0, 1, 2]], np.uint32), atl)
    g = _check_file(one, np.array([[0, 1, 2]], np.uint32), atl, None, r)
    assert g["scale"] == 1.0 and not g["primitives"][0]["POSITION"].any() and np.array_equal(g["translation"].view(np.uint32), one[0].view(np.uint32))
    tri = dict(face_ptr=np.array([0, 1], np.uint32), faces=np.array([0], np.uint32), tc_ptr=np.array([0, 3], np.uint32),
               texcoords_merged=np.array([[0, 0], [1, 0], [0, 1]], np.float32), texcoord_ids=np.array([[0, 1, 2]], np.uint32))
    f = np.array([[0, 1, 2]], np.uint32)
    fmax = np.finfo(np.float32).max
    for verts in (np.array([[0, 0, 7], [2, 0, 7], [0, 1, 7]], np.float32),                      # planar: one axis of extent 0
                  np.array([[-0.0, 0, 0], [0.0, 1, 0], [0.0, 0, 1]], np.float32),              # lo = -0
                  np.array([[-fmax, 0, 0], [fmax, 1e-45, 0], [0, -1e-45, fmax]], np.float32)):  # +-FLT_MAX beside subnormals
        r = QM.restate(verts, f, tri)
        g = _check_file(verts, f, tri, None, r)
        assert np.isfinite(g["scale"]) and g["scale"] > 0
    assert str(QM.restate(np.array([[-0.0, 0, 0], [0.0, 1, 0], [0.0, 0, 1]], np.float32), f, tri)["json"]["nodes"][0]["translation"][0]) == "-0.0"


def test_rounding_cases():
    ks = np.array([0, 1, 2, 100, 255, 256, 32766, 32767, 32768, 65533, 65534])
    # positions exactly halfway between two steps round up: lo = 0, hi = 65535, so S = 1 and x = k + 0.5 lies between k and k + 1
    pos = np.concatenate([[[0, 0, 0], [65535, 0, 0]], np.stack([ks + 0.5, np.zeros(len(ks)), np.zeros(len(ks))], 1)]).astype(np.float32)
    assert np.array_equal(pos[2:, 0].astype(np.float64), ks + 0.5)                # (exact in float32)
    lo, E, S = QM.grid(pos)
    assert E == 65535.0 and S == 1.0
    assert QM.quantise_positions(pos, lo, E)[2:, 0].tolist() == (ks + 1).tolist()
    # texture coordinates: 0, 1 and the float32 nearest (k + 0.5) / 65535, which is a little above or below the tie -- exact arithmetic decides
    u = np.concatenate([[0.0, -0.0, 1.0], (ks + 0.5) / 65535.0]).astype(np.float32)
    want = [int(Fraction(float(x)) * 65535 + Fraction(1, 2)) for x in u]
    assert QM.quantise_texcoords(u).tolist() == want and want[:3] == [0, 0, 65535]
    assert {w - k for w, k in zip(want[3:], ks.tolist())} == {0, 1}               # both sides of the tie occur
    assert np.all(np.abs(np.array(want) / 65535.0 - u.astype(np.float64)) <= QM.TEXCOORD_BOUND)
    bad = np.array([-2.0 ** -30, np.nextafter(np.float32(1), np.float32(2)), np.nan, np.inf, 0.5], np.float32)
    assert QM.texcoords_storable(bad).tolist() == [False, False, False, False, True]
    # normals: a component at +-(k + 0.5) / 127 of the length goes away from zero or towards it as float64 lands, symmetrically in the sign,
    # and within the bound either way
    kn = np.arange(0, 127)
    c = (kn + 0.5) / 127.0
    n = np.stack([c, np.sqrt(1.0 - c * c), np.zeros(len(c))], 1).astype(np.float32)
    q, zero = QM.quantise_normals(n)
    qm, _ = QM.quantise_normals(-n)
    assert not zero.any() and np.array_equal(qm, -q)
    assert np.all((q[:, 0] == kn) | (q[:, 0] == kn + 1))
    unit = n.astype(np.float64) / np.sqrt((n.astype(np.float64) ** 2).sum(1))[:, None]
    assert np.all(np.abs(q / 127.0 - unit) <= QM.NORMAL_BOUND)
    # exact ties of c = (x / l) * 127: x / l = 1 / 2 (l a power of two times x) gives 63.5, away from zero: +-64
    q, _ = QM.quantise_normals(np.array([[1, 0, 0], [-1, 0, 0], [0, 0, 0], [2.0 ** -60, 0, 0], [0, -2.0 ** 60, 0]], np.float32))
    assert q.tolist() == [[127, 0, 0], [-127, 0, 0], [0, 0, 0], [127, 0, 0], [0, -127, 0]]
    half = np.array([[0.5, np.sqrt(0.75), 0]], np.float64)
    assert abs(QM.quantise_normals(half.astype(np.float32))[0][0, 0]) in (63, 64)


def test_reader_rejections():
    atl = _two_triangles(True)
    r = QM.restate(VERTS, MESH_FACES, atl, NORMALS)
    QM.parse_glb(_file(r))
    j = dict(r["json"]); j.pop("extensionsRequired")
    with pytest.raises(AssertionError, match="extension"):
        QM.parse_glb(_file(dict(r, json=j)))
    j = dict(r["json"], accessors=[dict(a) for a in r["json"]["accessors"]]); j["accessors"][0]["max"] = [65535, 65535, 32767]
    with pytest.raises(AssertionError, match="max"):
        QM.parse_glb(_file(dict(r, json=j)))
    j = dict(r["json"], accessors=[dict(a) for a in r["json"]["accessors"]]); del j["accessors"][1]["normalized"]
    with pytest.raises(AssertionError, match="normalized"):
        QM.parse_glb(_file(dict(r, json=j)))
    bad = bytearray(r["bin"]); bad[6] = 1                           # a byte of POSITION's stride padding
    with pytest.raises(AssertionError, match="padding"):
        QM.parse_glb(_file(dict(r, bin=bytes(bad))))
    bad = bytearray(r["bin"]); bad[-2:] = (5).to_bytes(2, "little")  # the last index: 5 vertices
    with pytest.raises(AssertionError, match="index out of range"):
        QM.parse_glb(_file(dict(r, bin=bytes(bad))))
    with pytest.raises(AssertionError, match="length"):             # the container is still glb_model's business
        QM.parse_glb(_file(r)[:-4])
    assert GM.json.__name__ == "json" and GM.PNG_SIG.startswith(b"\x89PNG")   # the reader leaves glb_model as it found it


def test_json_equal_compares_the_translation_as_float32_bits():
    r = QM.restate(VERTS + np.float32(0.1), MESH_FACES, _two_triangles(False))
    import json
    text = json.dumps(r["json"])
    j = json.loads(text)
    j["nodes"][0]["translation"] = [float("%.9g" % x) for x in j["nodes"][0]["translation"]]     # as the library prints them
    assert j["nodes"][0]["translation"] != r["json"]["nodes"][0]["translation"] and QM.json_equal(j, r["json"])
    j["nodes"][0]["scale"][0] = float(np.nextafter(j["nodes"][0]["scale"][0], 1.0))
    assert not QM.json_equal(j, r["json"])


def test_parameter_and_stats_structs():
    assert ctypes.sizeof(M.viewsel.ModelParams) == 32 and M.viewsel.ModelParams.glb_quantize.offset == 28
    assert ctypes.sizeof(M.viewsel.GlbStats) == 96                   # mvs_glb_stats keeps its size: the route's own stats are a struct beside it
    qs = M.viewsel.GlbQuantStats()
    assert ctypes.sizeof(qs) == 32                                   # mvs_glb_quant_stats of include/mvs_viewsel.h
    for k in ("ms_bounds", "zero_normals", "texcoords_out_of_range", "index16_primitives"):
        assert hasattr(qs, k), k
    if not os.path.exists(M.lib_path()):
        pytest.skip("HIP library not built (run __graft_entry__.build())")
    L = M.load_library()
    assert "mvs_ctx_glb_quant_stats" in L._declared and L.mvs_ctx_glb_quant_stats.argtypes is not None
    assert M.default_model_params().glb_quantize == 0 and M.default_model_params(glb_quantize=1).glb_quantize == 1
