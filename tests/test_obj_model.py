"""Row f9 without a GPU: the CPU model (tests/tools/obj_model.cpp, DESIGN.md section 4 "Model output") writes the bytes upstream's compiled
build_model + ObjModel::save + MaterialLib::save_to_files left for the recorded cases (tests/golden/obj_model_pins.npz); its float lines
equal printf("%.6f") on the grid of exponents, mantissas and ties; the recorded files parse with the grammar of item 1; the library
exports the entry points."""
import os

import numpy as np
import pytest

import mvs_texturing_amd as M
import obj_model as OM

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "obj_model_pins.npz")
PINS = ("one_atlas", "three_atlases", "faceless_atlas", "ties_negative_zeros", "digit_counts", "prefix_with_directories")
ATLAS_KEYS = ("face_ptr", "faces", "tc_ptr", "texcoords_merged", "texcoord_ids")


@pytest.fixture(scope="module", autouse=True)
def _model_built():
    OM.build()


def pins():
    """(name, verts, faces, normals, atlas-set dict, prefix, upstream's .obj bytes, upstream's .mtl bytes)"""
    z = np.load(GOLDEN)
    for name in PINS:
        g = lambda k: z[name + "/" + k]
        yield name, g("verts"), g("mesh_faces"), g("normals"), {k: g(k) for k in ATLAS_KEYS}, g("prefix").tobytes().decode(), g("obj").tobytes(), g("mtl").tobytes()


def test_model_equals_upstream_on_the_pins():
    seen = 0
    for name, v, f, n, atl, prefix, obj, mtl in pins():
        got_obj, got_mtl = OM.run(v, f, atl, n, name=prefix.rsplit("/", 1)[-1])
        assert got_obj == obj, name
        assert got_mtl == mtl, name
        seen += 1
    assert seen == len(PINS)


def test_pins_cover_what_they_are_named_for():
    cases = {p[0]: p for p in pins()}
    assert len(cases["one_atlas"][4]["face_ptr"]) == 2 and len(cases["three_atlases"][4]["face_ptr"]) == 4
    fp = cases["faceless_atlas"][4]["face_ptr"]
    assert (np.diff(fp.astype(np.int64)) == 0).any() and cases["faceless_atlas"][6].count(b"usemtl ") == len(fp) - 1
    ties = cases["ties_negative_zeros"][6]
    for text in (b"v 0.007812 0.023438 -0.000000\n", b" -0.000000", b"340282346638528859811704183484516925440.000000", b"18446744073709551616.000000", b"999999.937500"):
        assert text in ties
    digits = cases["digit_counts"][6]
    for text in (b"f 9/", b"f 10/", b"f 99/", b"f 100/", b"f 999/", b"f 1000/", b"/9/", b"/10/", b"/99/", b"/100/", b"/999/", b"/1000/"):
        assert text in digits
    name, *_rest, prefix, obj, mtl = cases["prefix_with_directories"]
    assert "/" in prefix and obj.startswith(b"mtllib scene_v1.mtl\n") and b"map_Kd scene_v1_material0001_map_Kd.png\n" in mtl and b"/" not in mtl


def test_pins_parse_with_the_grammar():
    for name, v, f, n, atl, prefix, obj, mtl in pins():
        cnt = OM.parse_obj(obj)
        A = len(atl["face_ptr"]) - 1
        assert cnt == dict(v=len(v), vt=int(atl["tc_ptr"][-1]), vn=len(n), usemtl=A, f=int(atl["face_ptr"][-1])), name
        assert mtl.count(b"\n") == 8 * A


def test_model_floats_equal_snprintf_on_the_grid():
    bits = OM.float_grid()
    assert len(bits) == 2 * 256 * 67 + 2 * 13 * 4096
    got = OM.format_floats(bits.view(np.float32))
    want = OM.snprintf_floats(bits)
    assert got == want
    lines = got.split(b"\n")
    x = np.array([0.0078125, 0.0234375, -1e-7, np.finfo(np.float32).max], np.float32)
    assert OM.format_floats(x) == b"0.007812\n0.023438\n-0.000000\n340282346638528859811704183484516925440.000000\n"
    assert max(len(s) for s in lines) == 47


def test_model_without_normals_and_without_atlases():
    v = np.array([[0, 0.5, -0.25], [1, 2, 3]], np.float32)
    obj, mtl = OM.run(v, np.zeros((0, 3), np.uint32), OM.EMPTY_ATLASES, None, name="n")
    assert obj == b"mtllib n.mtl\nv 0.000000 0.500000 -0.250000\nv 1.000000 2.000000 3.000000\n" and mtl == b""
    rng = np.random.default_rng(2)
    atl = OM.crafted_atlases(rng, 1, [1], [3])
    obj, _ = OM.run(np.zeros((3, 3), np.float32), np.array([[0, 1, 2]], np.uint32), atl, None, name="n")
    last = obj.split(b"\n")[-2]
    assert last.startswith(b"f ") and last.count(b"/") == 3 and b"vn " not in obj
    assert OM.parse_obj(obj)["f"] == 1


def test_library_exports_the_entry_points():
    if not os.path.exists(M.lib_path()):
        pytest.skip("HIP library not built")
    L = M.load_library()
    for name in ("mvs_ctx_build_model", "mvs_ctx_save_model", "mvs_write_png", "mvs_model_default_params", "mvs_model_text_free"):
        assert name in L._declared and hasattr(L, name)
    p = M.default_model_params()
    assert (p.max_bytes, p.png_level) == (0, 0)
