"""Row f10 on the GPU: the view-selection debug model (DESIGN.md section 4 "Debug model").  Context.debug_embeddings equals the numpy
restatement (tests/tools/debug_model.py, itself held to upstream's recorded images) on mixed sizes in one call, so that images start
at odd byte offsets; Context.debug_patches has row f6's geometry bit for bit, the masks of TexturePatch's constructor and the crop of
the materialised debug images as pixels, and leaves the real images alone; view_selection_model writes what the CPU models of rows
f8 and f9 write for that patch set, and every labelled face's texel carries its view's colour."""
import os

import numpy as np
import pytest

import atlas_model as AM
import debug_model as DM
import mvs_texturing_amd as M
import obj_model as OM
import patch_model as PM
import seam_model as SM
from conftest import get_scene
from test_debug_embeddings import PIN_IDS, PIN_SHAPES
from test_patch_model import crafted_set, nested_set

pytestmark = pytest.mark.gpu

GEOMETRY = ("label", "box", "face_ptr", "faces", "texcoords", "pix_ptr")
KEYS = GEOMETRY + ("image", "validity", "blending")
SIZES = PIN_SHAPES + [(1, 1), (64, 64), (300, 7)]
IDS = PIN_IDS + [3, 368, 999]
UNSUPPORTED = 7


@pytest.fixture(scope="module", autouse=True)
def _models_built():
    SM.build(); PM.build(); AM.build(); OM.build()


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


def _same(got, want, keys, what=""):
    for k in keys:
        assert got[k].size == want[k].size and np.array_equal(_raw(got[k]), _raw(want[k])), (what, k)


# ---- 1. debug_embeddings ----
@pytest.mark.parametrize("first_position", [0, 143, 144])
@pytest.mark.parametrize("with_ids", [True, False])
def test_embeddings_equal_the_restatement(first_position, with_ids):
    import torch
    ids = IDS if with_ids else None
    want = DM.images(SIZES, ids, first_position)
    starts = 3 * np.cumsum([0] + [w * h for w, h in SIZES])
    assert (starts[1:-1] % 16 != 0).sum() >= 8                                        # images start off the 16-byte grid
    c = M.Context(0)
    got = c.debug_embeddings(SIZES, ids, first_position)
    assert np.array_equal(got, want)
    for shift in (0, 5):                                                              # a device buffer on and off a 16-byte boundary
        buf = torch.full((len(want) + 16 + shift,), 0xAB, dtype=torch.uint8, device="cuda")
        c.debug_embeddings(SIZES, ids, first_position, out=buf[shift:shift + len(want)])
        c.synchronize()
        host = buf.cpu().numpy()
        assert np.array_equal(host[shift:shift + len(want)], want), shift
        assert (host[:shift] == 0xAB).all() and (host[shift + len(want):] == 0xAB).all()   # nothing written around it
    c.close()


def test_embeddings_edges_and_refusal():
    c = M.Context(0)
    assert c.debug_embeddings(np.zeros((0, 2), np.int32)).size == 0                   # n = 0
    assert c.debug_embeddings([(0, 5), (7, 0)]).size == 0                             # images without pixels
    got = c.debug_embeddings([(0, 9), (14, 7), (5, 0), (1, 1)], [1, 23, 4, 5], 7)     # ... between others
    assert np.array_equal(got, np.concatenate([DM.image(14, 7, 23, 8).ravel(), DM.image(1, 1, 5, 10).ravel()]))
    with pytest.raises(M.MvsError) as e:
        c.debug_embeddings([(14, 7), (14, 7)], [999, 1000])
    assert e.value.status == UNSUPPORTED
    with pytest.raises(M.MvsError) as e:
        c.debug_embeddings([(14, 7)], None, 1000)                                     # the position is the id
    assert e.value.status == UNSUPPORTED
    assert np.array_equal(c.debug_embeddings([(14, 7)], [999], 1000), DM.image(14, 7, 999, 1000).ravel())   # the context stays usable
    c.close()


# ---- 2. debug_patches ----
def _check_patches(s, labels, view_ids=None, what="", expect_magenta=False):
    labels = np.ascontiguousarray(labels, np.uint32)
    c = _ctx(s)
    try:
        before, bst = c.texture_patches(s.adj_ptr, s.adj, labels)
        got, st = c.debug_patches(s.adj_ptr, s.adj, labels, view_ids)
        after, _ = c.texture_patches(s.adj_ptr, s.adj, labels)
        sizes = [(im.shape[1], im.shape[0]) for im in s.images]
        packed = c.debug_embeddings(sizes, view_ids)                                  # the materialised debug images of this context's views
    finally:
        c.close()
    _same(before, after, KEYS, what + ": the real images changed")
    _same(got, before, GEOMETRY, what)
    n = got["validity"].size
    assert n == before["validity"].size and (got["validity"] == 255).all() and (got["blending"] == 0).all()
    assert st["valid_pixels"] == st["pixels"] == n and st["near_pixels"] == 0 and st["degenerate_faces"] == 0 and st["ms_mark"] == 0
    for k in ("patches", "merged", "listed_faces", "pixels"):
        assert st[k] == bst[k], (what, k)
    if n:
        assert st["ms_resolve"] > 0
    assert np.array_equal(packed, DM.images(sizes, view_ids))
    off = 3 * np.cumsum([0] + [w * h for w, h in sizes])
    views = [packed[off[v]:off[v + 1]].reshape(h, w, 3) for v, (w, h) in enumerate(sizes)]
    magenta = 0
    for p in range(len(got["label"])):
        img, _, _ = M.patch_view(got, p)
        want = DM.crop(views[int(got["label"][p]) - 1], got["box"][p])
        assert np.array_equal(img.view(np.uint32), want.view(np.uint32)), (what, p)
        if got["box"][p, 0] < 0:
            assert (img[:, 0] == np.array([1, 0, 1], np.float32)).all(), (what, p)
            magenta += 1
    if expect_magenta:
        assert magenta > 0, what
    return got


@pytest.mark.parametrize("name", ["tiny", "oddw", "mixed"])
def test_scene_patches(name):
    s = get_scene(name)
    labels = _library_labels(name, s)
    got = _check_patches(s, labels, what=name)
    assert len(got["label"]) > 1 and len(set(got["label"].tolist())) > 1
    w = got["box"][:, 2]
    assert (w % 4 != 0).any() and (np.diff(got["pix_ptr"].astype(np.int64)) > 1024).any()   # four-pixel seams inside rows, more than one chunk
    ids = 7 + 3 * np.arange(len(s.images), dtype=np.uint32)                              # ids that differ from the positions
    _check_patches(s, labels, ids, what=name + "/ids")


def test_crafted_and_nested_sets():
    for name, (g, labels) in crafted_set().items():
        _check_patches(g, labels, what=name, expect_magenta=name.startswith("grid"))
    for name, (g, labels) in nested_set().items():
        _check_patches(g, labels, what=name)


def test_empty_set_and_refusals():
    g = SM.grid_scene()
    c = _ctx(g)
    got, st = c.debug_patches(g.adj_ptr, g.adj, np.zeros(len(g.faces), np.uint32))
    assert all(got[k].size == 0 for k in KEYS if k not in ("face_ptr", "pix_ptr")) and st["patches"] == st["pixels"] == 0
    labels = SM.grid_labels(g)
    with pytest.raises(M.MvsError) as e:
        c.debug_patches(g.adj_ptr, g.adj, labels, np.full(len(g.images), 1000, np.uint32))
    assert e.value.status == UNSUPPORTED
    with pytest.raises(M.MvsError) as e:
        c.debug_patches(g.adj_ptr, g.adj, labels, params=M.default_patch_params(max_pixels=10))
    assert e.value.status == UNSUPPORTED and e.value.stats["pixels"] > 10
    bad = labels.copy(); bad[0] = len(g.images) + 1
    with pytest.raises(M.MvsError) as e:
        c.debug_patches(g.adj_ptr, g.adj, bad)
    assert e.value.status == 4                                                        # MVS_ERR_LABELING, as row f6
    got, _ = c.debug_patches(g.adj_ptr, g.adj, labels)                                # the context stays usable
    assert len(got["label"]) > 0
    c.close()
    c = M.Context(0)
    with pytest.raises(M.MvsError) as e:
        c.debug_patches(g.adj_ptr, g.adj, labels)
    assert e.value.status == 6                                                        # MVS_ERR_STATE: no mesh, no views
    c.close()


def test_shuffled_tiny_has_the_same_patches():
    s = get_scene("tiny")
    labels = _library_labels("tiny", s)
    p = M.synth.permute_scene(s, seed=7)
    a = _check_patches(s, labels, what="tiny")
    b = _check_patches(p, labels[p.face_perm], what="tiny/shuffled")

    def patches(arr, perm):                                                           # label, frame, the caller's ORIGINAL face ids, the pixels
        out = []
        for i in range(len(arr["label"])):
            f = arr["faces"][arr["face_ptr"][i]:arr["face_ptr"][i + 1]]
            out.append((int(arr["label"][i]), tuple(arr["box"][i].tolist()), tuple(sorted((f if perm is None else perm[f]).tolist())), M.patch_view(arr, i)[0].tobytes()))
        return sorted(out)
    assert patches(a, None) == patches(b, p.face_perm)


# ---- 3. end to end ----
def _end_to_end_cases():
    s = get_scene("tiny")
    yield "tiny", s, _library_labels("tiny", s)
    for name, (g, labels) in nested_set().items():
        yield name, g, labels


def test_view_selection_model_files(tmp_path):
    for name, s, labels in _end_to_end_cases():
        labels = np.ascontiguousarray(labels, np.uint32)
        normals = M.vertex_normals(s.verts, s.faces)
        d = tmp_path / name
        os.makedirs(d)
        prefix = str(d / "m")
        c = _ctx(s)
        st = M.view_selection_model(s, labels, prefix, vertex_normals=normals, ctx=c)
        patches, _ = c.debug_patches(s.adj_ptr, s.adj, labels)
        dev_atlases, _ = c.texture_atlases(patches)                                   # the library's own atlases, for the centroid check
        c.close()
        rc, arrays, _, _, _ = AM.run(patches)
        assert rc == 0
        A = len(arrays["atlas_size"])
        want_obj, want_mtl = OM.run(s.verts, s.faces, arrays, normals, "m_view_selection")
        obj = open(prefix + "_view_selection.obj", "rb").read()
        assert obj == want_obj and open(prefix + "_view_selection.mtl", "rb").read() == want_mtl, name
        assert b"mtllib m_view_selection.mtl\n" in obj and b"map_Kd m_view_selection_material0000_map_Kd.png" in want_mtl
        assert A >= 1 and sorted(os.listdir(d)) == sorted(["m_view_selection.obj", "m_view_selection.mtl"] + ["m_view_selection_material%04d_map_Kd.png" % a for a in range(A)])
        pngs = []
        for a in range(A):
            img, _ = OM.decode_png(open("%s_view_selection_material%04d_map_Kd.png" % (prefix, a), "rb").read())
            assert np.array_equal(img, AM.atlas_view(arrays, a)), (name, a)
            pngs.append(img)
        assert st["patches"]["patches"] == len(patches["label"]) and st["atlases"]["atlases"] == A and st["model"]["bytes"]["v"] > 0
        # through none of the models: the texel under the centroid of every labelled face carries its view's colour
        seen = 0
        for a in range(A):
            size = int(dev_atlases["atlas_size"][a])
            for e in range(int(dev_atlases["face_ptr"][a]), int(dev_atlases["face_ptr"][a + 1])):
                f = int(dev_atlases["faces"][e])
                tc = dev_atlases["texcoords_merged"][int(dev_atlases["tc_ptr"][a]) + dev_atlases["texcoord_ids"][e].astype(np.int64)]
                x, y = np.floor(tc.astype(np.float64).mean(0) * size + 0.5).astype(int)
                bg, fg = M.debug_view_style(int(labels[f]) - 1)
                texel = tuple(int(v) for v in pngs[a][y, x])
                assert texel in (bg, fg), (name, f, int(labels[f]), texel, bg)
                seen += texel == bg
        assert int((labels > 0).sum()) == sum(int(n) for n in np.diff(dev_atlases["face_ptr"])) and seen > 0.25 * (labels > 0).sum()


def test_texture_model_keyword_leaves_the_textured_model_alone(tmp_path):
    s = get_scene("tiny")
    labels = _library_labels("tiny", s)
    normals = M.vertex_normals(s.verts, s.faces)
    os.makedirs(tmp_path / "a"); os.makedirs(tmp_path / "b")
    M.texture_model(s, labels, str(tmp_path / "a" / "t"), normals)
    M.texture_model(s, labels, str(tmp_path / "b" / "t"), normals, view_selection_model=True)
    plain = sorted(os.listdir(tmp_path / "a"))
    both = sorted(os.listdir(tmp_path / "b"))
    assert not any("view_selection" in n for n in plain)
    assert [n for n in both if "view_selection" not in n] == plain and "t_view_selection.obj" in both and "t_view_selection.mtl" in both
    for n in plain:
        assert open(tmp_path / "a" / n, "rb").read() == open(tmp_path / "b" / n, "rb").read(), n
    c = _ctx(s)
    c.view_selection_model(s.adj_ptr, s.adj, labels, str(tmp_path / "a" / "t"), vertex_normals=normals)
    c.close()
    for n in both:
        assert open(tmp_path / "a" / n, "rb").read() == open(tmp_path / "b" / n, "rb").read(), n
