"""Row f11 under glb_quantize = 1 on the GPU: Context.build_glb / save_glb and M.texture_model(format="both") give the file that the numpy
restatement of DESIGN.md section 4 "Model output" item 10 (tests/tools/glb_quant_model.py) describes -- the BIN chunk byte for byte, the
JSON value for value -- on seams written out by hand, either side of the gather's 256-pair blocks, at every index width, on degenerate
grids, at the rounding ties, with zero and with tiny and huge normals, through every refusal of the item and on the suite's scene."""
import os

import numpy as np
import pytest

import glb_model as GM
import glb_quant_model as QM
import mvs_texturing_amd as M
import obj_model as OM
from conftest import get_scene

pytestmark = pytest.mark.gpu

VERTS6 = np.array([[0, 0, 0], [1, 0, 0.25], [0, 1, -0.0], [1, 1, 2], [2, 1, -3], [2, 2, 1e-30]], np.float32)
FACES6 = np.array([[0, 1, 2], [2, 1, 3], [3, 4, 5]], np.uint32)
NORMALS6 = np.array([[0, 0, 1], [0, 1, 0], [1, 0, 0], [0, 0, -1], [0, -1, 0], [-0.0, 0.6, 0.8]], np.float32)
F32_MAX = float(np.finfo(np.float32).max)


def _quant(**kw):
    return M.default_model_params(glb_quantize=1, **kw)


def _mesh_ctx(verts, faces):
    verts = np.ascontiguousarray(verts, np.float32).reshape(-1, 3); faces = np.ascontiguousarray(faces, np.uint32).reshape(-1, 3)
    c = M.Context(0)
    c.set_mesh(verts, faces, np.zeros((max(len(faces), 1), 3), np.float32))
    return c


def _compare(c, verts, faces, atl, normals=None, images=None, params=None, mime="image/png", what=""):
    """build_glb against the restatement: the BIN bytes, the JSON and the stats; returns (file, parsed, stats, restatement)"""
    want = QM.restate(verts, faces, atl, normals, images, mime)
    data, st = c.build_glb(atl, normals, params or _quant())
    got = QM.parse_glb(data)
    assert got["bin"] == want["bin"], what
    assert QM.json_equal(got["json"], want["json"]), what
    assert st["vertices"] == want["vertices"] and st["indices"] == 3 * len(atl["faces"]) and st["primitives"] == len(got["primitives"]), what
    assert st["file_bytes"] == len(data) and st["nonfinite_values"] == 0 and st["texcoords_out_of_range"] == 0
    assert st["json_bytes"] + (8 + len(got["bin"]) if got["bin"] else 0) + 20 == len(data) and st["geometry_bytes"] + st["image_bytes"] == len(got["bin"])
    assert st["zero_normals"] == want["zero_normals"] and st["index16_primitives"] == want["index16_primitives"], what
    return data, got, st, want


def _both(c, verts, faces, atl, normals, what=""):
    """with and without normals"""
    _compare(c, verts, faces, atl, None, what=what)
    return _compare(c, verts, faces, atl, normals, what=what)


def _one_atlas(faces, ids, n_coords):
    merged = np.arange(2 * n_coords, dtype=np.float32).reshape(n_coords, 2) / np.float32(2 * n_coords)
    return dict(face_ptr=np.array([0, len(faces)], np.uint32), faces=np.array(faces, np.uint32), tc_ptr=np.array([0, n_coords], np.uint32), texcoords_merged=merged,
                texcoord_ids=np.array(ids, np.uint32).reshape(-1, 3))


def _strip(n):
    """n vertices in n - 2 faces"""
    return np.stack([np.arange(n - 2), np.arange(1, n - 1), np.arange(2, n)], 1).astype(np.uint32)


def _strips(counts, seed=0):
    """(verts, mesh faces, atlas set, normals): atlas a is the strip over vertices 0 .. counts[a] - 1 with a coordinate of its own per vertex,
    so that it has counts[a] glTF vertices and the atlases share their vertices"""
    rng = np.random.default_rng(seed)
    nv = max(counts)
    verts = (rng.normal(0, 1, (nv, 3)) * 10.0 ** rng.integers(-2, 3, (nv, 3))).astype(np.float32)
    normals = (rng.normal(0, 1, (nv, 3)) * 10.0 ** rng.integers(-5, 6, (nv, 1))).astype(np.float32)
    listed = [np.arange(n - 2, dtype=np.uint32) for n in counts]
    atl = dict(face_ptr=np.concatenate([[0], np.cumsum([len(x) for x in listed])]).astype(np.uint32), faces=np.concatenate(listed),
               tc_ptr=np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32), texcoords_merged=rng.uniform(0, 1, (sum(counts), 2)).astype(np.float32),
               texcoord_ids=np.concatenate([_strip(n) for n in counts]))
    return verts, _strip(nv), atl, normals


# ---- seams written out by hand ----

def test_shared_edge_with_equal_and_with_different_coordinates():
    c = _mesh_ctx(VERTS6, FACES6)
    atl = _one_atlas([0, 1], [[0, 1, 2], [2, 1, 3]], 4)
    _, g, st, _ = _both(c, VERTS6, FACES6, atl, NORMALS6)
    p = g["primitives"][0]
    assert st["vertices"] == 4 and p["indices"].tolist() == [0, 1, 2, 2, 1, 3] and p["index_bytes"] == 2
    atl = _one_atlas([0, 1], [[0, 1, 2], [4, 5, 3]], 6)             # vertex 2 through coordinate 4, vertex 1 through coordinate 5
    _, g, st, _ = _both(c, VERTS6, FACES6, atl, NORMALS6)
    p = g["primitives"][0]
    assert st["vertices"] == 6 and p["indices"].tolist() == [0, 1, 2, 4, 5, 3]
    assert p["POSITION"][4].tolist() == p["POSITION"][2].tolist() and p["POSITION"][5].tolist() == p["POSITION"][1].tolist()
    assert p["NORMAL"][4].tolist() == p["NORMAL"][2].tolist() == [127, 0, 0]
    c.close()


def test_a_vertex_used_by_two_atlases_has_one_stored_triple():
    c = _mesh_ctx(VERTS6, FACES6)
    atl = dict(face_ptr=np.array([0, 1, 2], np.uint32), faces=np.array([0, 1], np.uint32), tc_ptr=np.array([0, 3, 6], np.uint32),
               texcoords_merged=np.linspace(0, 1, 12, dtype=np.float32).reshape(6, 2), texcoord_ids=np.array([[0, 1, 2], [0, 1, 2]], np.uint32))
    _, g, st, want = _both(c, VERTS6, FACES6, atl, NORMALS6)
    p = g["primitives"]
    assert st["vertices"] == 6 and [q["material"] for q in p] == [0, 1] and p[0]["indices"].tolist() == p[1]["indices"].tolist() == [0, 1, 2]
    # atlas 0 holds vertices 0 1 2, atlas 1 vertices 2 1 3: the shared ones are the same integers in both, on the one grid of the file
    assert p[0]["POSITION"][2].tolist() == p[1]["POSITION"][0].tolist() and p[0]["POSITION"][1].tolist() == p[1]["POSITION"][1].tolist()
    assert g["scale"] == 2.0 / 65535.0 and g["translation"].tolist() == [0, 0, 0] and str(g["json"]["nodes"][0]["translation"][2]) == "-0.0"
    acc = g["json"]["accessors"]
    assert acc[0]["min"] == [0, 0, 0] and acc[0]["max"] == [32768, 32768, 8192] and acc[4]["max"] == [32768, 32768, 65535]
    assert acc[3]["byteOffset"] == 0 and acc[7]["byteOffset"] == 8   # 6 index bytes and 2 of padding in front of the second primitive
    c.close()


def test_one_coordinate_used_by_two_vertices_and_one_pair_used_twice():
    c = _mesh_ctx(VERTS6, FACES6)
    atl = _one_atlas([0], [[0, 0, 1]], 2)
    _, g, st, _ = _both(c, VERTS6, FACES6, atl, NORMALS6)
    p = g["primitives"][0]
    assert st["vertices"] == 3 and p["indices"].tolist() == [0, 1, 2] and p["TEXCOORD_0"][0].tolist() == p["TEXCOORD_0"][1].tolist()
    atl = _one_atlas([2, 2], [[0, 1, 2], [0, 1, 2]], 3)
    _, g, st, _ = _both(c, VERTS6, FACES6, atl, NORMALS6)
    assert st["vertices"] == 3 and g["primitives"][0]["indices"].tolist() == [0, 1, 2, 0, 1, 2]
    c.close()


# ---- block edges ----

@pytest.mark.parametrize("counts", [[255], [256], [257], [100, 300], [3, 511, 258]], ids=str)
def test_block_edges(counts):
    """255 / 256 / 257 pairs in one atlas; borders of atlases inside a gather block; odd totals, which leave TEXCOORD_0 and NORMAL off
    16-byte alignment"""
    verts, faces, atl, normals = _strips(counts, seed=sum(counts))
    c = _mesh_ctx(verts, faces)
    data, g, st, _ = _both(c, verts, faces, atl, normals)
    assert st["vertices"] == sum(counts) and [len(p["POSITION"]) for p in g["primitives"]] == counts
    assert c.build_glb(atl, normals, _quant())[0] == data           # a second call: the same bytes
    c.close()


def test_crafted_sets_with_merging_and_device_inputs():
    import torch
    rng = np.random.default_rng(11)
    nv, nf = 4000, 3500
    verts = (rng.normal(0, 1, (nv, 3)) * 10.0 ** rng.integers(-3, 4, (nv, 3))).astype(np.float32)
    faces = rng.integers(0, nv, (nf, 3)).astype(np.uint32)
    normals = rng.normal(0, 1, (nv, 3)).astype(np.float32)
    atl = OM.crafted_atlases(rng, nf, [0, 1, 85, 86, 3000], [0, 3, 255, 258, 9000])
    c = _mesh_ctx(verts, faces)
    data, g, st, _ = _both(c, verts, faces, atl, normals)
    dev = {k: torch.from_numpy(np.ascontiguousarray(atl[k]).reshape(-1).view(np.int32 if atl[k].dtype == np.uint32 else atl[k].dtype)).cuda() for k in atl}
    dn = torch.from_numpy(normals).cuda()
    torch.cuda.synchronize()
    assert c.build_glb(dev, dn, _quant())[0] == data
    assert st["ms_bounds"] > 0 and st["ms_gather"] > 0 and st["ms_indices"] > 0
    plain, pst = c.build_glb(atl, normals)                          # the default route beside it: item 8's file, no bounds pass
    assert GM.parse_glb(plain)["bin"] == GM.restate(verts, faces, atl, normals)["bin"] and pst["ms_bounds"] == 0 and pst["index16_primitives"] == 0
    c.close()


# ---- index width ----

@pytest.mark.parametrize("counts,widths", [([65535], [2]), ([65536], [4]), ([300, 65536, 5], [2, 4, 2]), ([3, 4], [2, 2])], ids=str)
def test_index_width(counts, widths):
    verts, faces, atl, normals = _strips(counts, seed=len(counts))
    c = _mesh_ctx(verts, faces)
    _, g, st, _ = _both(c, verts, faces, atl, normals)
    c.close()
    assert [p["index_bytes"] for p in g["primitives"]] == widths and st["index16_primitives"] == widths.count(2)
    assert [int(p["indices"].max()) for p in g["primitives"]] == [n - 1 for n in counts]
    if counts == [3, 4]:                                            # one face: 6 index bytes and 2 of padding in front of the next primitive
        acc = g["json"]["accessors"]
        assert [acc[3]["byteOffset"], acc[7]["byteOffset"]] == [0, 8] and g["json"]["bufferViews"][3]["byteLength"] == 8 + 12


# ---- degenerate grids ----

TRI = dict(face_ptr=np.array([0, 1], np.uint32), faces=np.array([0], np.uint32), tc_ptr=np.array([0, 3], np.uint32),
           texcoords_merged=np.array([[0, 0], [1, 0], [0, 1]], np.float32), texcoord_ids=np.array([[0, 1, 2]], np.uint32))
GRIDS = {
    "one_point": np.array([[3.5, -2.0, 1e-40]] * 3, np.float32),                               # E == 0: three pairs on one point
    "planar": np.array([[0, 0, 7], [2, 0, 7], [0, 1, 7]], np.float32),
    "lo_is_minus_zero": np.array([[-0.0, 0, 0], [0.0, 1, 0], [0.0, 0, 1]], np.float32),
    "flt_max_and_subnormals": np.array([[-F32_MAX, 0, 0], [F32_MAX, 1e-45, 0], [0, -1e-45, F32_MAX]], np.float32),
    "subnormal_extent": np.array([[0, 0, 0], [1e-45, 0, 0], [3e-45, 2e-45, 1e-45]], np.float32),
}


@pytest.mark.parametrize("name", sorted(GRIDS))
def test_degenerate_grids(name):
    verts, f = GRIDS[name], np.array([[0, 1, 2]], np.uint32)
    c = _mesh_ctx(verts, f)
    _, g, st, want = _both(c, verts, f, TRI, np.array([[0, 0, 1]] * 3, np.float32), what=name)
    c.close()
    if name == "one_point":
        assert g["scale"] == 1.0 and not g["primitives"][0]["POSITION"].any() and st["vertices"] == 3
        assert np.array_equal(g["translation"].view(np.uint32), verts[0].view(np.uint32))
    if name == "lo_is_minus_zero":
        assert str(g["json"]["nodes"][0]["translation"][0]) == "-0.0" and g["primitives"][0]["POSITION"][:, 0].tolist() == [0, 0, 0]
    if name == "planar":
        assert g["primitives"][0]["POSITION"].tolist() == [[0, 0, 0], [65535, 0, 0], [0, 32768, 0]]
    pos, _, _ = QM.expand(g, g["primitives"][0])
    x = verts.astype(np.float64)
    assert np.all(np.abs(pos - x) <= QM.position_bound(x, g["translation"].astype(np.float64)[None, :], g["scale"])), name


# ---- rounding ----

def test_rounding_ties():
    ks = np.array([0, 1, 2, 100, 255, 256, 32766, 32767, 32768, 65533, 65534])
    n = len(ks) + 2
    verts = np.concatenate([[[0, 0, 0], [65535, 0, 0]], np.stack([ks + 0.5, np.zeros(len(ks)), np.zeros(len(ks))], 1)]).astype(np.float32)
    u = np.concatenate([[0.0, 1.0], (ks + 0.5) / 65535.0]).astype(np.float32)
    kn = np.arange(n) * 9 % 127                                     # normal components at (k + 0.5) / 127 of the length, either sign
    cn = (kn + 0.5) / 127.0 * np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
    normals = (np.stack([cn, np.sqrt(1.0 - cn * cn), np.zeros(n)], 1) * 3.0).astype(np.float32)
    faces = _strip(n)
    atl = dict(face_ptr=np.array([0, n - 2], np.uint32), faces=np.arange(n - 2, dtype=np.uint32), tc_ptr=np.array([0, n], np.uint32),
               texcoords_merged=np.stack([u, u[::-1]], 1), texcoord_ids=faces)
    c = _mesh_ctx(verts, faces)
    _, g, _, _ = _both(c, verts, faces, atl, normals)
    c.close()
    p = g["primitives"][0]
    assert g["scale"] == 1.0 and p["POSITION"][2:, 0].tolist() == (ks + 1).tolist()                  # halves round up
    assert p["TEXCOORD_0"][:2, 0].tolist() == [0, 65535] and set((p["TEXCOORD_0"][2:, 0] - ks).tolist()) == {0, 1}
    n64 = normals.astype(np.float64)
    assert np.all(np.abs(p["NORMAL"] / 127.0 - n64 / np.sqrt((n64 * n64).sum(1))[:, None]) <= QM.NORMAL_BOUND)
    assert np.all((np.abs(p["NORMAL"][:, 0]) == kn) | (np.abs(p["NORMAL"][:, 0]) == kn + 1)) and np.all(p["NORMAL"][:, 0] * cn >= 0)


# ---- normals ----

def test_normals_axes_zero_and_extreme_lengths():
    verts, f = VERTS6, FACES6[:2]                                   # vertices 0 .. 3 are referenced, 4 and 5 are not
    atl = _one_atlas([0, 1], [[0, 1, 2], [2, 1, 3]], 4)
    c = _mesh_ctx(verts, FACES6)
    for normals, stored, zeros in (
            (np.array([[1, 0, 0], [0, -1, 0], [0, 0, 1], [-1, 0, 0], [0, 0, 0], [0, 0, 0]], np.float32), [[127, 0, 0], [0, -127, 0], [0, 0, 127], [-127, 0, 0]], 0),
            (np.array([[0, 0, 0], [0, 1, 0], [-0.0, 0, -0.0], [1, 1, 0], [0, 0, 0], [0, 0, 0]], np.float32), [[0, 0, 0], [0, 127, 0], [0, 0, 0], [90, 90, 0]], 2),
            (np.array([[2.0 ** -60, 0, 0], [0, 2.0 ** 60, 0], [3 * 2.0 ** -60, 4 * 2.0 ** -60, 0], [0, -3 * 2.0 ** 60, 4 * 2.0 ** 60], [1, 0, 0], [1, 0, 0]], np.float32),
             [[127, 0, 0], [0, 127, 0], [76, 102, 0], [0, -76, 102]], 0)):
        _, g, st, _ = _compare(c, verts, FACES6, atl, normals)
        assert g["primitives"][0]["NORMAL"].tolist() == stored and st["zero_normals"] == zeros
    c.close()


# ---- refusals ----

def _good_and_used():
    rng = np.random.default_rng(4)
    verts = rng.normal(0, 1, (30, 3)).astype(np.float32); faces = rng.integers(0, 29, (20, 3)).astype(np.uint32)   # vertex 29 is in no face
    good = OM.crafted_atlases(rng, 20, [8, 0, 12], [10, 0, 9])
    ids = good["texcoord_ids"]
    used = set((good["tc_ptr"][np.repeat([0, 2], [8, 12])][:, None] + ids).reshape(-1).tolist())
    unused = sorted(set(range(19)) - used)
    assert unused, "the case needs a coordinate that no corner names"
    return verts, faces, good, sorted(used), unused


@pytest.mark.parametrize("value", [-2.0 ** -30, float(np.nextafter(np.float32(1), np.float32(2))), float("nan")], ids=["minus_2^-30", "above_1", "nan"])
def test_texture_coordinates_outside_0_1_are_refused_at_referenced_pairs_only(value):
    verts, faces, good, used, unused = _good_and_used()
    c = _mesh_ctx(verts, faces)
    data, _, st, _ = _compare(c, verts, faces, good)
    x = dict(good, texcoords_merged=good["texcoords_merged"].copy())
    x["texcoords_merged"][unused[0], 1] = value                     # unreferenced: accepted, and not in the file
    assert _compare(c, verts, faces, x)[0] == data
    x["texcoords_merged"][used[0], 0] = value; x["texcoords_merged"][used[-1], :] = value
    with pytest.raises(M.MvsError) as e:
        c.build_glb(x, params=_quant())
    assert e.value.status == 7 and "texture coordinate" in str(e.value)                  # MVS_ERR_UNSUPPORTED
    want = QM.restate(verts, faces, x)
    es = e.value.stats
    assert es["texcoords_out_of_range"] == want["texcoords_out_of_range"] >= 3 and es["vertices"] == st["vertices"] and es["geometry_bytes"] == st["geometry_bytes"]
    assert es["index16_primitives"] == 2 and es["nonfinite_values"] == 0
    GM.parse_glb(c.build_glb(x)[0])                                 # the float route stores them as they are
    assert c.build_glb(good, params=_quant())[0] == data            # and a good call afterwards
    c.close()


def test_other_refusals_and_a_good_call_after_each():
    verts, faces, good, used, _ = _good_and_used()
    c = _mesh_ctx(verts, faces)
    data, _, st, _ = _compare(c, verts, faces, good)
    plain, pst = c.build_glb(good)
    for q in (2, -1):
        with pytest.raises(M.MvsError) as e:
            c.build_glb(good, params=M.default_model_params(glb_quantize=q))
        assert e.value.status == 1 and "glb_quantize" in str(e.value)                    # MVS_ERR_INVALID
        assert c.build_glb(good, params=_quant())[0] == data
    # max_bytes between the two sizes: the quantised file passes, the float file does not
    assert len(data) < len(plain) and st["geometry_bytes"] < pst["geometry_bytes"]
    cap = (len(data) + len(plain)) // 2
    assert c.build_glb(good, params=_quant(max_bytes=cap))[0] == data
    with pytest.raises(M.MvsError) as e:
        c.build_glb(good, params=M.default_model_params(max_bytes=cap))
    assert e.value.status == 7
    for cap, stage in ((len(data) - 1, "whole file"), (st["geometry_bytes"] + 27, "after the numbering")):   # on the sizes this layout has
        with pytest.raises(M.MvsError) as e:
            c.build_glb(good, params=_quant(max_bytes=cap))
        assert e.value.status == 7 and e.value.stats["geometry_bytes"] == st["geometry_bytes"], stage
        assert e.value.stats["file_bytes"] == (len(data) if stage == "whole file" else 28 + st["geometry_bytes"]), stage
    assert c.build_glb(good, params=_quant(max_bytes=len(data)))[0] == data
    c.close()
    # the non-finite refusal of item 8 runs first: the gather, which counts texture coordinates, is not reached
    x = verts.copy(); x[int(np.unique(faces[good["faces"]])[0]), 2] = np.inf
    bad_tc = dict(good, texcoords_merged=good["texcoords_merged"].copy()); bad_tc["texcoords_merged"][used[0], 0] = 2.0
    c = _mesh_ctx(x, faces)
    with pytest.raises(M.MvsError) as e:
        c.build_glb(bad_tc, params=_quant())
    assert e.value.status == 7 and "finite" in str(e.value) and e.value.stats["nonfinite_values"] >= 1 and e.value.stats["texcoords_out_of_range"] == 0
    n = np.ones((30, 3), np.float32); n[int(np.unique(faces[good["faces"]])[0]), 0] = np.nan
    c.close()
    c = _mesh_ctx(verts, faces)
    with pytest.raises(M.MvsError) as e:
        c.build_glb(good, n, _quant())
    assert e.value.status == 7 and "finite" in str(e.value) and e.value.stats["nonfinite_values"] == QM.restate(verts, faces, good, n)["nonfinite"] >= 1
    assert c.build_glb(good, params=_quant())[0] == data
    c.close()


# ---- end to end ----

def test_save_glb_writes_the_bytes_of_build_glb(tmp_path):
    verts, faces, atl, normals = _strips([40, 300], seed=5)
    c = _mesh_ctx(verts, faces)
    data, _ = c.build_glb(atl, normals, _quant())
    st = c.save_glb(atl, tmp_path / "m.glb", normals, _quant())
    c.close()
    assert open(tmp_path / "m.glb", "rb").read() == data and st["file_bytes"] == len(data) and sorted(os.listdir(tmp_path)) == ["m.glb"]


_cache = {}


def _tiny():
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


def test_texture_model_on_the_suites_scene(tmp_path):
    s, labels, normals, arrays = _tiny()
    os.makedirs(tmp_path / "q"); os.makedirs(tmp_path / "f")
    st_q = M.texture_model(s, labels, str(tmp_path / "q" / "m"), normals, format="both", params=M.default_model_params(glb_quantize=1, image_format=1))
    st_f = M.texture_model(s, labels, str(tmp_path / "f" / "m"), normals, format="both", params=M.default_model_params(glb_quantize=0, image_format=1))
    q, f = _files(tmp_path / "q"), _files(tmp_path / "f")
    A = len(arrays["atlas_size"])
    assert A >= 1 and sorted(q) == sorted(["m.obj", "m.mtl", "m.glb"] + ["m_material%04d_map_Kd.jpg" % a for a in range(A)])
    assert {k: v for k, v in q.items() if k != "m.glb"} == {k: v for k, v in f.items() if k != "m.glb"}     # row f9 does not read the field
    jpgs = [q["m_material%04d_map_Kd.jpg" % a] for a in range(A)]
    got = QM.parse_glb(q["m.glb"])
    assert got["images"] == jpgs
    want = QM.restate(s.verts, s.faces, arrays, normals, jpgs, "image/jpeg")
    assert got["bin"] == want["bin"] and QM.json_equal(got["json"], want["json"])
    # every corner, expanded and dequantised from the file, against its vertex, coordinate and unit normal
    verts = np.ascontiguousarray(s.verts, np.float32).reshape(-1, 3); merged = np.ascontiguousarray(arrays["texcoords_merged"], np.float32).reshape(-1, 2)
    v, gc, atlas = GM.corners(s.faces, arrays)
    n64 = np.ascontiguousarray(normals, np.float32).reshape(-1, 3).astype(np.float64)
    length = np.sqrt((n64 * n64).sum(1))
    unit = n64 / np.where(length == 0, 1.0, length)[:, None]
    for p in got["primitives"]:
        sel = atlas == p["material"]
        pos, uv, nrm = QM.expand(got, p)
        x = verts[v[sel]].astype(np.float64)
        assert np.all(np.abs(pos - x) <= QM.position_bound(x, got["translation"].astype(np.float64)[None, :], got["scale"]))
        assert np.all(np.abs(uv - merged[gc[sel]].astype(np.float64)) <= QM.TEXCOORD_BOUND)
        assert np.all(np.abs(nrm - unit[v[sel]]) <= QM.NORMAL_BOUND)
    # the default parameters' file names no extension
    gq, gf = st_q[1], st_f[1]
    jf = f["m.glb"][20:20 + int.from_bytes(f["m.glb"][12:16], "little")]
    assert b"extensions" not in jf and b"KHR_mesh_quantization" in q["m.glb"][20:20 + int.from_bytes(q["m.glb"][12:16], "little")]
    # the size: 16 of 32 bytes per vertex, 2 of 4 per index; the margin is the padding behind the primitives
    assert gq["vertices"] == gf["vertices"] and gq["image_bytes"] == gf["image_bytes"] and gf["geometry_bytes"] == 32 * gf["vertices"] + 4 * gf["indices"]
    if all(len(p["POSITION"]) <= 65535 for p in got["primitives"]):
        assert gq["index16_primitives"] == gq["primitives"] and gq["geometry_bytes"] <= 0.55 * gf["geometry_bytes"]
    else:
        face_ptr = np.asarray(arrays["face_ptr"], np.int64)
        _, ioff = QM.index_layout(want["first"], face_ptr)
        assert gq["geometry_bytes"] == 16 * gq["vertices"] + int(ioff[-1])
