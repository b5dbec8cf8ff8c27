"""Row f7 on the CPU: the model of local seam leveling (tests/tools/blend_model.cpp: upstream's loops in upstream's order, the solve of
DESIGN.md section 4 "Local seam leveling" item 9) against numpy statements of the order-free rules the device uses, against the Poisson
system of item 8 assembled independently and solved directly in fp64 (the accuracy ceiling), and against invariants of the
definition; plus the library's new exports.

Accuracy, measured with scripts/lsl_accuracy.py over the cases of accuracy_cases() (profiles/lsl_accuracy.json): the largest
|model - fp64 direct| over all unknowns and channels is 4.6e-5 at the default tolerance 1e-6 (6.3e-4 at 1e-5) (ceiling 2^-11 = 4.9e-4, half of it
2.4e-4); an fp32 SuperLU solve of the same systems is off by at most 3.3e-6.

tests/golden/local_seam_pins.npz: 20 crafted patch sets (two to four patches at seams; three labels at a vertex, seams against
label 0, non-manifold edges, a line of length 0, crossing lines, patches narrower and wider than two strips) with the image,
validity and prepared blending mask upstream's own compiled tex::local_seam_leveling left for them with an empty poisson_blend
(DESIGN.md section 4 "Local seam leveling", "How the rule is held to upstream").  Data only."""
import json
import os

import numpy as np
import pytest

import mvs_texturing_amd as M
import blend_model as BM
import patch_model as PM
import seam_model as SM
from conftest import get_scene
from test_patch_model import corner_adjust, crafted_set

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "local_seam_pins.npz")
CEILING = 2.0 ** -11     # an eighth of the 1 / 255 step the atlas quantises to


@pytest.fixture(scope="module", autouse=True)
def _models_built():
    SM.build(); PM.build(); BM.build()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32).ravel()


def patches_of(scene, labels, adjust=True):
    st, pa, _, _ = PM.run_scene(scene, labels, corner_adjust(scene, labels) if adjust else None)
    assert st == 0
    return pa


def three_view_grid(**kw):
    """SM.grid_scene with a third identical camera (its own image): three labels can meet at a vertex"""
    g = SM.grid_scene(**kw)
    rng = np.random.default_rng(17)
    H, W = g.images[0].shape[:2]
    g.cams = {k: np.concatenate([v, v[:1]]) for k, v in g.cams.items()}
    g.images = list(g.images) + [np.ascontiguousarray(rng.integers(0, 256, (H, W, 3)).astype(np.uint8))]
    return g


def crafted_sets():
    """name -> (scene, labels, patch set): the situations the definition names.  Patch sets come from the patch model (row f6) on
    crafted grids; the last three are edited by hand."""
    out = {}
    for name, (g, labels) in crafted_set().items():          # two patches at one seam; a fin (non-manifold edge); an absorbed island
        out[name] = (g, labels, patches_of(g, labels))
    g = three_view_grid(n=7)                                  # three labels around one vertex, a strip of label 0 beside them
    x = g.verts[g.faces[:, 0], 0]; y = g.verts[g.faces[:, 0], 1]
    labels = np.where(y < np.median(y), np.where(x < np.median(x), 1, 2), 3).astype(np.uint32)
    labels[x > np.quantile(x, 0.8)] = 0
    out["three_labels_and_unseen"] = (g, labels, patches_of(g, labels))
    g = SM.grid_scene(n=8, W=200, H=120, fin=True)            # patches ~100 pixels wide: an inner region and its 128 ring
    labels = SM.grid_labels(g)
    fin = len(g.faces) - 1                                    # the fin against both its neighbours: its edge is a seam edge twice
    labels[fin] = 3 - labels[g.adj[g.adj_ptr[fin]]]
    out["wide"] = (g, labels, patches_of(g, labels))
    g = SM.grid_scene(n=6)                                    # a seam edge shorter than a pixel: a line of length 0
    labels = SM.grid_labels(g)
    pairs = [sorted(set(g.faces[f].tolist()) & set(g.faces[a].tolist())) for f in range(len(g.faces)) for a in g.adj[g.adj_ptr[f]:g.adj_ptr[f + 1]]
             if f < a and labels[f] != labels[a]]
    a, b = pairs[len(pairs) // 2]
    verts = g.verts.copy(); verts[b] = verts[a] + np.float32([0.0, 0.2 / 50.0, 0.0]); g.verts = np.ascontiguousarray(verts)
    out["short_edge"] = (g, labels, patches_of(g, labels))
    g, labels = crafted_set()["grid"]                         # a vertex moved out of its frame: writes outside
    pa = patches_of(g, labels)
    tc = pa["texcoords"].reshape(-1, 3, 2).copy()
    box = pa["box"].reshape(-1, 4)
    e0 = int(pa["face_ptr"][1])
    hit = np.isclose(tc[:e0, :, 0], tc[:e0, :, 0].max())       # patch 0's right-most column of vertices (the seam) moved beyond the frame
    tc[:e0, :, 0][hit] = box[0, 2] + 3.0
    pa = dict(pa); pa["texcoords"] = tc.reshape(-1)
    out["outside_frame"] = (g, labels, pa)
    g, labels = crafted_set()["grid"]                         # 255s on the frame's edge and beside mask 0: demoted
    pa = dict(patches_of(g, labels))
    val = pa["validity"].copy(); bl = pa["blending"].copy()
    w, h = int(box[0, 2]), int(box[0, 3])
    v0 = val[:w * h].reshape(h, w); b0 = bl[:w * h].reshape(h, w)
    v0[0, :] = 255; b0[0, :] = 255                             # a valid row on the frame's edge
    near = np.argwhere(b0 == 64)
    for yy, xx in near[len(near) // 2:len(near) // 2 + 6]:
        v0[yy, xx] = 0; b0[yy, xx] = 0                         # holes in the near ring: inside pixels next to mask 0
    pa["validity"] = val; pa["blending"] = bl
    out["demoted"] = (g, labels, pa)
    return out


LADDER_BASE = dict(n=6, W=128, H=80)     # two patches of about 80 x 82 pixels and 4091 / 4158 unknowns: both fit the LDS tier
LADDER = ((1, 2), (255, 256), (257, 1023), (1024, 1025), (2047, 2048), (2049, None))      # unknowns wanted per patch; None: all of them
# what each set of edge_sets() is made to reach: ("stats" | "counters", name), or None where the solve's own arrays say it
EDGE_REACHES = {"skipped_pair": ("stats", "skipped_pairs"), "skipped_pair_twice": ("stats", "skipped_pairs"),
                "sanitized_vertex": ("counters", "sanitized"), "sanitized_input": ("counters", "sanitized")}


def _with_adjacency(g, f, a):
    """a copy of the scene with one symmetric adjacency entry f <-> a appended to both faces' lists"""
    import copy
    lists = [g.adj[g.adj_ptr[i]:g.adj_ptr[i + 1]].tolist() for i in range(len(g.faces))]
    lists[f].append(a); lists[a].append(f)
    s = copy.copy(g)
    s.adj_ptr = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.uint32)
    s.adj = np.array([x for l in lists for x in l], np.uint32)
    return s


def _with_images(g, edit):
    import copy
    s = copy.copy(g)
    s.images = [np.ascontiguousarray(edit(im.copy())) for im in g.images]
    return s


def unknown_pixels(mask):
    """flat row-major indices of the unknowns of a prepared mask (h, w): 255, off the frame's edge, no 4-neighbour of mask 0"""
    m = np.asarray(mask)
    u = np.zeros(m.shape, bool)
    u[1:-1, 1:-1] = (m[1:-1, 1:-1] == 255) & (m[1:-1, :-2] != 0) & (m[1:-1, 2:] != 0) & (m[:-2, 1:-1] != 0) & (m[2:, 1:-1] != 0)
    return np.flatnonzero(u.ravel())


def unknown_counts(scene, labels, pa, **params):
    """per patch, from the model's prepared mask through its per-patch entry"""
    st, out, _, _ = BM.run_scene(scene, labels, pa, max_iterations=0, **params)
    assert st == 0
    return [BM.solve(BM.patch(pa, out, i)[2], BM.patch(pa, pa, i)[0], BM.patch(pa, pa, i)[0], max_iterations=0)[3][0] for i in range(len(pa["label"]))]


def _ladder_set(g, labels, pa, wanted):
    """the patch set with all but the first wanted[i] unknowns (row-major) of patch i fixed: their input blending becomes 64, which
    item 7 passes through, item 8 keeps as a fixed value and no neighbour is demoted by (64 is not 0)"""
    st, out, _, _ = BM.run_scene(g, labels, pa, max_iterations=0)
    assert st == 0
    pa = dict(pa); bl = pa["blending"].copy()
    for i, n in enumerate(wanted):
        if n is None:
            continue
        idx = unknown_pixels(BM.patch(pa, out, i)[2])
        assert len(idx) >= n, (i, len(idx), n)
        bl[int(pa["pix_ptr"][i]) + idx[n:]] = 64
    pa["blending"] = bl
    return pa


def edge_sets():
    """name -> (scene, labels, patch set): the situations of the definition that crafted_sets() does not reach -- a listed pair that
    shares one vertex (once, and twice through a face with a repeated vertex id), the sanitize pass of item 7 converting pixels (after
    a vertex moved into the strip, and from a 128 in the input), a channel that is idle from the start beside two that iterate, black
    views, and patches whose unknown counts sit on and beside the edges of the reduction tree (LADDER)."""
    out = {}
    g, labels = crafted_set()["grid"]
    pa = patches_of(g, labels)
    faces = g.faces.astype(np.int64)
    sets = [set(f.tolist()) for f in faces]
    near = lambda f: set(g.adj[g.adj_ptr[f]:g.adj_ptr[f + 1]].tolist())
    f, a = next((f, a) for f in range(len(faces)) for a in range(f + 1, len(faces))
                if labels[f] and labels[a] and labels[f] != labels[a] and len(sets[f] & sets[a]) == 1 and a not in near(f))
    out["skipped_pair"] = (_with_adjacency(g, f, a), labels, pa)
    # a face (va, va, vb) on an edge inside one label region whose end va lies on the seam, listed against a face of the other label
    # that holds va and not vb: upstream's double loop collects va twice
    import copy
    labels_at = lambda v: {int(labels[k]) for k in range(len(faces)) if v in sets[k]}
    va, vb = next((int(u), int(v)) for tri in faces for u in tri for v in tri if u != v and len(labels_at(u)) == 2 and len(labels_at(v)) == 1)
    inner = labels_at(vb).pop()
    other = next(k for k in range(len(faces)) if va in sets[k] and labels[k] != inner)
    d = copy.copy(g)
    d.faces = np.ascontiguousarray(np.concatenate([g.faces, np.array([[va, va, vb]], g.faces.dtype)]))
    d.normals = np.ascontiguousarray(np.concatenate([g.normals, g.normals[:1]]))
    d.adj_ptr, d.adj = SM.face_adjacency(d.faces)
    dl = np.concatenate([labels, [inner]]).astype(np.uint32)
    out["skipped_pair_twice"] = (_with_adjacency(d, other, len(faces)), dl, patches_of(d, dl))
    # one seam vertex of patch 0 moved to the middle of its frame (every corner of it in the patch's list): its pixel and the ends of its
    # lines land among 255s
    box = pa["box"].reshape(-1, 4)
    e0 = int(pa["face_ptr"][1])
    ids = faces[pa["faces"][:e0]]
    seam = sorted(set(ids.ravel().tolist()) & set(faces[pa["faces"][e0:]].ravel().tolist()))
    for v in seam:                                              # the first seam vertex whose lines then run diagonally somewhere: a 128 between four 255s
        tc = pa["texcoords"].reshape(-1, 3, 2).copy()
        tc[:e0][ids == v] = np.float32([box[0, 2] / 2.0, box[0, 3] / 2.0])
        pv = dict(pa); pv["texcoords"] = tc.reshape(-1)
        if BM.run_scene(g, labels, pv, max_iterations=0)[3]["sanitized"] > 0:
            break
    out["sanitized_vertex"] = (g, labels, pv)
    # a single 128 in the input whose four neighbours stay 255 after the writes
    st, res, _, _ = BM.run_scene(g, labels, pa, max_iterations=0)
    assert st == 0
    bw = BM.patch(pa, dict(image=res["after_writes"], validity=pa["validity"], blending=res["blend_writes"]), 0)[2]
    ok = np.zeros(bw.shape, bool)
    ok[1:-1, 1:-1] = (bw[1:-1, 1:-1] == 255) & (bw[1:-1, :-2] == 255) & (bw[1:-1, 2:] == 255) & (bw[:-2, 1:-1] == 255) & (bw[2:, 1:-1] == 255)
    pi = dict(pa); bl = pa["blending"].copy()
    bl[np.flatnonzero(ok.ravel())[int(ok.sum()) // 2]] = 128      # patch 0 starts at pixel 0
    pi["blending"] = bl
    out["sanitized_input"] = (g, labels, pi)

    def green77(im):
        im[..., 1] = 77
        return im
    c = _with_images(g, green77)                                # channel 1 constant: no seam in it, so it never iterates
    out["const_channel"] = (c, labels, patches_of(c, labels, adjust=False))
    b = _with_images(g, lambda im: np.zeros_like(im))
    out["black"] = (b, labels, patches_of(b, labels, adjust=False))
    g = SM.grid_scene(**LADDER_BASE)
    labels = SM.grid_labels(g)
    pa = patches_of(g, labels)
    for wanted in LADDER:
        out["unknown_ladder_%s_%s" % wanted] = (g, labels, _ladder_set(g, labels, pa, wanted))
    return out


def ladder_sets():
    return {k: v for k, v in edge_sets().items() if k.startswith("unknown_ladder")}


def suite_sets():
    """(name, scene, labels, patch set) on suite scenes with crafted labelings (the library's own labels need a GPU)"""
    for name, keys in (("tiny", ("random", "blocks", "random_with_unseen")), ("bumpy", ("blocks",))):
        s = get_scene(name)
        cases = SM.crafted_labelings(s)
        for k in keys:
            yield name + "/" + k, s, cases[k], patches_of(s, cases[k])


def accuracy_cases():
    for name, (g, labels, pa) in crafted_sets().items():
        if name not in ("outside_frame", "demoted"):
            yield name, g, labels, pa
    yield from suite_sets()


def measure_accuracy(scene, labels, pa, **params):
    """(worst |model - fp64 direct|, worst |fp32 SuperLU - fp64 direct|, unknowns, the model's stats) over the set's patches"""
    import scipy.sparse.linalg as spl
    st, out, stats, _ = BM.run_scene(scene, labels, pa, **params)
    assert st == 0
    worst, worst32, unknowns = 0.0, 0.0, 0
    for i in range(len(pa["label"])):
        img, _, mask = BM.patch(pa, out, i)
        orig, _, _ = BM.patch(pa, pa, i)
        after = BM.patch(pa, dict(image=out["after_writes"], validity=out["validity"], blending=out["blend_writes"]), i)[0]
        A, rhs, idx = BM.poisson_system(mask, orig, after)
        if len(idx) == 0:
            continue
        x64 = spl.spsolve(A.tocsc(), rhs)
        x64 = x64.reshape(len(idx), 3)
        got = img.reshape(-1, 3)[idx].astype(np.float64)
        worst = max(worst, float(np.abs(got - x64).max()))
        lu = spl.splu(A.astype(np.float32).tocsc())
        x32 = np.stack([lu.solve(rhs[:, c].astype(np.float32)) for c in range(3)], 1).astype(np.float64)
        worst32 = max(worst32, float(np.abs(x32 - x64).max()))
        unknowns += len(idx)
    return worst, worst32, unknowns, stats


class _Mesh:
    pass


def pin_cases():
    """(name, mesh (verts count, faces, adjacency), labels, patch set, upstream's image / validity / mask) of every recorded case.  The
    input image is stored as bytes: the recorded patches came from u8 crops with zero adjustments, image = u8 / 255.0f exactly; the
    output as the pixels upstream changed."""
    z = np.load(GOLDEN)
    for name in [str(n) for n in z["names"]]:
        g = lambda k: z[name + "/" + k]
        m = _Mesh()
        m.verts = np.zeros((int(g("n_verts")), 3), np.float32); m.faces = g("mesh_faces").reshape(-1, 3); m.adj_ptr = g("adj_ptr"); m.adj = g("adj")
        pa = {k: g(k) for k in ("label", "box", "face_ptr", "faces", "texcoords", "pix_ptr", "validity", "blending")}
        pa["image"] = g("image_u8").astype(np.float32) / np.float32(255.0)
        img = pa["image"].reshape(-1, 3).copy()
        img[g("out_changed")] = g("out_values")
        yield name, m, g("labels"), pa, dict(image=img, validity=g("out_validity"), blending=g("out_mask"))


def test_model_equals_upstream_pins():
    total = {k: 0 for k in BM.COUNTERS}
    n = invalid_writes = 0
    for name, m, labels, pa, want in pin_cases():
        st, out, stats, cnt = BM.run_scene(m, labels, pa, max_iterations=0)
        assert st == 0, name
        assert np.array_equal(_bits(out["image"]), _bits(want["image"])), name
        assert np.array_equal(out["validity"], want["validity"]) and np.array_equal(out["blending"], want["blending"]), name
        assert stats["outside_frame"] == 0 and stats["demoted"] == 0 and stats["skipped_pairs"] == 0, (name, stats)
        assert cnt["clamped_idx"] == 0, name
        invalid_writes += stats["invalid_writes"]
        img, bl = rule_writes(m, labels, pa)                    # the order-free rules against upstream directly
        assert np.array_equal(_bits(img), _bits(want["image"])), name
        box = pa["box"].reshape(-1, 4)
        for i in range(len(pa["label"])):
            a, b = int(pa["pix_ptr"][i]), int(pa["pix_ptr"][i + 1]); shape = (int(box[i, 3]), int(box[i, 2]))
            mask = BM.rule_prepare_mask(pa["validity"][a:b].reshape(shape), bl[a:b].reshape(shape))
            assert np.array_equal(mask.ravel(), want["blending"][a:b]), (name, i)
            assert np.array_equal(np.where(mask.ravel() == 64, 0, pa["validity"][a:b]), want["validity"][a:b]), (name, i)
        for k in total:
            total[k] += cnt[k]
        n += 1
    assert n == 20
    assert invalid_writes > 0        # one pin (a fin beside label 0) has lines over pixels of validity 0: upstream, built without asserts, writes them
    for k in ("overwrites", "zero_lines", "label0_seams", "duplicate_edges", "vertices_3", "inner_pixels", "ring_pixels"):
        assert total[k] >= 1, (k, total)                         # every listed situation occurs among the pins


def test_library_exports_and_ctypes_table():
    import ctypes as C
    assert os.path.exists(M.lib_path()), "build the library first (__graft_entry__.build)"
    raw = C.CDLL(M.lib_path())
    L = M.load_library()
    for name in ("mvs_ctx_local_seam_leveling", "mvs_lsl_default_params", "mvs_lsl_result_free"):
        assert hasattr(raw, name), name
        assert name in L._declared and getattr(L, name).argtypes is not None, name
    p = M.default_lsl_params()
    assert p.strip_width == 20 and p.max_iterations == BM.DEFAULTS["max_iterations"] and p.lds_bytes == BM.DEFAULTS["lds_bytes"]
    assert p.tolerance == np.float32(BM.DEFAULTS["tolerance"])
    assert M.default_lsl_params(max_iterations=0).max_iterations == 0
    assert callable(M.local_seam_leveling) and hasattr(M.Context, "local_seam_leveling")


def rule_writes(scene, labels, pa):
    """items 1 - 6 in numpy / Python from the definition's order-free form: every pixel takes the LAST write of its patch's sequence
    (vertex pixels, vertices ascending; then lines, seam edges in order).  Returns (image, blending) after the writes."""
    f32 = np.float32
    a = BM.flat(pa)
    faces = np.asarray(scene.faces, np.int64)
    box = a["box"].reshape(-1, 4); tc = a["texcoords"].reshape(-1, 3, 2)
    P = len(a["label"])
    img = a["image"].reshape(-1, 3).copy(); bl = a["blending"].copy()
    src = a["image"].reshape(-1, 3)

    def linear(p, x, y):
        w, h, base = int(box[p, 2]), int(box[p, 3]), int(a["pix_ptr"][p])
        x = min(f32(x), f32(w - 1)); x = max(x, f32(0)); y = min(f32(y), f32(h - 1)); y = max(y, f32(0))
        fx, fy = int(x), int(y); fx1, fy1 = min(fx + 1, w - 1), min(fy + 1, h - 1)
        w1 = f32(x - f32(fx)); w0 = f32(f32(1) - w1); w3 = f32(y - f32(fy)); w2 = f32(f32(1) - w3)
        v1, v2, v3, v4 = src[base + fy * w + fx], src[base + fy * w + fx1], src[base + fy1 * w + fx], src[base + fy1 * w + fx1]
        return f32(f32(f32(v1 * f32(w0 * w2)) + f32(v2 * f32(w1 * w2))) + f32(v3 * f32(w0 * w3))) + f32(v4 * f32(w1 * w3))

    proj = {}                                                   # (vertex, patch) -> projection, first entry first
    for p in range(P):
        for e in range(int(a["face_ptr"][p]), int(a["face_ptr"][p + 1])):
            for k in range(3):
                proj.setdefault((int(faces[a["faces"][e], k]), p), (tc[e, k], set()))[1].add(int(a["faces"][e]))
    by_vertex = {}
    for (v, p) in sorted(proj):
        by_vertex.setdefault(v, []).append(p)
    writes = [[] for _ in range(P)]                             # per patch: (x, y, colour) in sequence
    for v in sorted(by_vertex):
        if len(by_vertex[v]) <= 1:
            continue
        s = np.zeros(3, f32); wsum = f32(0)
        for p in by_vertex[v]:
            q = proj[(v, p)][0]
            s = f32(s + f32(linear(p, q[0], q[1]) * f32(1))); wsum = f32(wsum + f32(1))
        col = f32(s / wsum)
        for p in by_vertex[v]:
            q = proj[(v, p)][0]
            writes[p].append((int(f32(q[0] + f32(0.5))), int(f32(q[1] + f32(0.5))), col))
    lab = np.asarray(labels)
    for node in range(len(faces)):
        for adj in scene.adj[scene.adj_ptr[node]:scene.adj_ptr[node + 1]]:
            adj = int(adj)
            if node > adj or lab[node] == lab[adj]:
                continue
            shared = [int(u) for u in faces[node] for t in faces[adj] if u == t]
            if len(shared) != 2 or shared[0] == shared[1]:
                continue
            v1, v2 = min(shared), max(shared)
            eps = [p for p in by_vertex.get(v1, []) if (v2, p) in proj and proj[(v1, p)][1] & proj[(v2, p)][1]]
            mx = f32(1)
            for p in eps:
                d = proj[(v1, p)][0] - proj[(v2, p)][0]
                mx = max(mx, f32(np.sqrt(f32(f32(d[0] * d[0]) + f32(d[1] * d[1])))))
            n = int(np.ceil(f32(mx * f32(2))))
            cols = np.zeros((n, 3), f32)
            for j in range(n):
                t = f32(f32(j) / f32(n - 1))
                s = np.zeros(3, f32); wsum = f32(0)
                for p in eps:
                    p1, p2 = proj[(v1, p)][0], proj[(v2, p)][0]
                    q = f32(f32(p1 * t) + f32(f32(f32(1) - t) * p2))
                    s = f32(s + f32(linear(p, q[0], q[1]) * f32(1))); wsum = f32(wsum + f32(1))
                cols[j] = f32(s / wsum)
            for p in eps:
                p1, p2 = proj[(v1, p)][0], proj[(v2, p)][0]
                x0, y0, x1, y1 = int(f32(p1[0] + f32(0.5))), int(f32(p1[1] + f32(0.5))), int(f32(p2[0] + f32(0.5))), int(f32(p2[1] + f32(0.5)))
                length = f32(np.sqrt(f32(f32(f32(x1 - x0) * f32(x1 - x0)) + f32(f32(y1 - y0) * f32(y1 - y0)))))
                dx, dy = abs(x1 - x0), abs(y1 - y0)
                sx, sy = (1 if x0 < x1 else -1), (1 if y0 < y1 else -1)
                err, x, y = dx - dy, x0, y0
                while True:
                    tdx, tdy = f32(x1 - x), f32(y1 - y)
                    t = f32(f32(np.sqrt(f32(f32(tdx * tdx) + f32(tdy * tdy)))) / length) if length != 0 else f32(0.5)
                    if t < 1 and n > 1:
                        idx = min(int(np.floor(f32(t * f32(n - 1)))), n - 2)
                        col = f32(f32(f32(f32(1) - t) * cols[idx]) + f32(t * cols[idx + 1]))
                    else:
                        col = cols[n - 1]
                    writes[p].append((x, y, col))
                    if x == x1 and y == y1:
                        break
                    e2 = 2 * err
                    if e2 > -dy:
                        err -= dy; x += sx
                    if e2 < dx:
                        err += dx; y += sy
    for p in range(P):
        w, h, base = int(box[p, 2]), int(box[p, 3]), int(a["pix_ptr"][p])
        last = {}
        for (x, y, col) in writes[p]:
            if 0 <= x < w and 0 <= y < h:
                last[(x, y)] = col                              # the last write of the sequence stays
        for (x, y), col in last.items():
            img[base + y * w + x] = col; bl[base + y * w + x] = 128
    return img, bl


def test_model_equals_the_order_free_rules_and_the_cases_are_not_vacuous():
    total = {k: 0 for k in BM.COUNTERS}
    stats_total = {k: 0 for k in BM.STATS}
    for name, (g, labels, pa) in crafted_sets().items():
        st, out, stats, cnt = BM.run_scene(g, labels, pa, max_iterations=0)
        assert st == 0, name
        img, bl = rule_writes(g, labels, pa)                    # items 1 - 6: last write wins
        assert np.array_equal(_bits(img), _bits(out["after_writes"])), name
        assert np.array_equal(bl, out["blend_writes"]), name
        assert np.array_equal(_bits(out["image"]), _bits(out["after_writes"])), name      # no solve: the image after the writes
        for i in range(len(pa["label"])):                       # item 7: the distance form == upstream's erosion loops
            _, val, _ = BM.patch(pa, pa, i)
            blw = BM.patch(pa, dict(image=out["after_writes"], validity=pa["validity"], blending=out["blend_writes"]), i)[2]
            mask = BM.patch(pa, out, i)[2]
            assert np.array_equal(BM.rule_prepare_mask(val, blw), mask), (name, i)
            assert np.array_equal(BM.prepare_mask(val, blw), mask), (name, i)
            for sw in (0, 3):
                assert np.array_equal(BM.rule_prepare_mask(val, blw, sw), BM.prepare_mask(val, blw, sw)), (name, i, sw)
        assert np.array_equal(out["validity"], np.where(out["blending"] == 64, 0, BM.flat(pa)["validity"])), name      # item 10
        assert stats["iterations_total"] == 0 and stats["written_pixels"] == int((out["blend_writes"] == 128).sum())      # row f6 leaves no 128
        for k in total:
            total[k] += cnt[k]
        for k in stats_total:
            stats_total[k] += stats[k]
        if name not in ("outside_frame", "demoted"):
            assert stats["outside_frame"] == 0 and stats["demoted"] == 0 and stats["skipped_pairs"] == 0, (name, stats)
        assert cnt["clamped_idx"] == 0
    for k in ("overwrites", "zero_lines", "label0_seams", "duplicate_edges", "vertices_3", "inner_pixels", "ring_pixels"):
        assert total[k] >= 1, (k, total)
    g, labels, pa = crafted_sets()["outside_frame"]
    assert BM.run_scene(g, labels, pa, max_iterations=0)[2]["outside_frame"] > 0
    g, labels, pa = crafted_sets()["demoted"]
    assert BM.run_scene(g, labels, pa, max_iterations=0)[2]["demoted"] > 0


def test_counters_are_zero_on_suite_scenes():
    for name, s, labels, pa in suite_sets():
        st, out, stats, cnt = BM.run_scene(s, labels, pa)
        assert st == 0
        assert stats["outside_frame"] == 0 and stats["demoted"] == 0 and stats["skipped_pairs"] == 0, (name, stats)
        assert stats["hit_max_iterations"] == 0 and stats["strip_pixels"] > 0 and stats["seam_edges"] > 0, (name, stats)
        assert cnt["clamped_idx"] == 0


@pytest.mark.parametrize("case", ["crafted", "suite"])
def test_accuracy_against_the_fp64_direct_solve(case):
    """the largest |model - fp64 direct| over all unknowns and channels stays below 2^-11"""
    cases = [c for c in accuracy_cases() if ("/" in c[0]) == (case == "suite")]
    assert cases
    for name, g, labels, pa in cases:
        worst, worst32, unknowns, stats = measure_accuracy(g, labels, pa)
        print("accuracy %-28s unknowns %7d  model %.3e  fp32 LU %.3e  iterations max %d" % (name, unknowns, worst, worst32, stats["iterations_max"]))
        assert unknowns > 0 and stats["hit_max_iterations"] == 0, name
        assert worst <= CEILING, (name, worst)


def test_accuracy_file():
    with open(os.path.join(ROOT, "profiles", "lsl_accuracy.json")) as f:
        acc = json.load(f)
    assert acc["worst_model"] < 2.0 ** -12 and acc["tolerance"] == BM.DEFAULTS["tolerance"]
    assert acc["max_iterations"] == BM.DEFAULTS["max_iterations"] >= 4 * acc["iterations_max_measured"]


def test_fixed_pixels_keep_their_bits_and_patches_do_not_couple():
    for name, (g, labels, pa) in crafted_sets().items():
        st, out, stats, _ = BM.run_scene(g, labels, pa)
        assert st == 0 and stats["hit_max_iterations"] == 0, (name, stats)
        fixed = out["blending"] != 255
        assert np.array_equal(_bits(out["image"][fixed]), _bits(out["after_writes"][fixed])), name
        assert stats["strip_pixels"] + stats["demoted"] == int((out["blending"] == 255).sum()), name
        assert stats["fixed_pixels"] == int(np.isin(out["blending"], (64, 128)).sum()), name
        for i in range(len(pa["label"])):                       # the per-patch entry on one patch alone == its bits inside the set
            img, _, mask = BM.patch(pa, out, i)
            orig = BM.patch(pa, pa, i)[0]
            after = BM.patch(pa, dict(image=out["after_writes"], validity=out["validity"], blending=out["blending"]), i)[0]
            x, it, err, _ = BM.solve(mask, orig, after)
            assert np.array_equal(_bits(x), _bits(img)), (name, i)
            assert np.array_equal(it, out["iters"][i]) and np.array_equal(_bits(err), _bits(out["err"][i])), (name, i)


def mid_cap(iters):
    """a cap in the middle of a set's converged iteration counts (at least 1)"""
    return max(1, int(np.max(iters)) // 2)


def test_edge_sets_equal_the_order_free_rules_and_reach_their_situations():
    """The second variant of the skipped pair needs a face with a repeated vertex id, (va, va, vb): the row f6 model accepts that mesh
    (status 0; the face joins the patch of its edge's label), so both variants are kept."""
    sets = edge_sets()
    for name, (g, labels, pa) in sets.items():
        st, out, stats, cnt = BM.run_scene(g, labels, pa, max_iterations=0)
        assert st == 0, name
        img, bl = rule_writes(g, labels, pa)
        assert np.array_equal(_bits(img), _bits(out["after_writes"])), name
        assert np.array_equal(bl, out["blend_writes"]), name
        assert np.array_equal(_bits(out["image"]), _bits(out["after_writes"])), name
        for i in range(len(pa["label"])):
            _, val, _ = BM.patch(pa, pa, i)
            blw = BM.patch(pa, dict(image=out["after_writes"], validity=pa["validity"], blending=out["blend_writes"]), i)[2]
            mask = BM.patch(pa, out, i)[2]
            assert np.array_equal(BM.rule_prepare_mask(val, blw), mask), (name, i)
            assert np.array_equal(BM.prepare_mask(val, blw), mask), (name, i)
        assert np.array_equal(out["validity"], np.where(out["blending"] == 64, 0, BM.flat(pa)["validity"])), name
        assert stats["outside_frame"] == 0 and stats["demoted"] == 0 and cnt["clamped_idx"] == 0, (name, stats)
        if name in EDGE_REACHES:
            kind, key = EDGE_REACHES[name]
            assert (stats if kind == "stats" else cnt)[key] > 0, (name, key)
        else:
            assert stats["skipped_pairs"] == 0 and cnt["sanitized"] == 0, (name, stats, cnt)
    base = BM.run_scene(*crafted_sets()["grid"], max_iterations=0)[2]
    for name in ("skipped_pair", "skipped_pair_twice"):               # the listed pair is skipped, not taken as an edge
        stats = BM.run_scene(*sets[name], max_iterations=0)[2]
        assert stats["skipped_pairs"] == 1 and stats["seam_edges"] == base["seam_edges"], (name, stats)
    g, labels, pa = sets["skipped_pair_twice"]
    assert len(set(g.faces[-1].tolist())) == 2 and len(g.faces) - 1 in pa["faces"]
    assert BM.run_scene(*sets["sanitized_input"], max_iterations=0)[3]["sanitized"] == 1
    # the sanitized pixels are 255 in the prepared mask and unknowns of the solve
    for name in ("sanitized_vertex", "sanitized_input"):
        st, out, stats, cnt = BM.run_scene(*sets[name], max_iterations=0)
        assert int(((out["blend_writes"] == 128) & (out["blending"] == 255)).sum()) == cnt["sanitized"], name


def test_const_channel_and_black_views_idle_in_different_ways():
    sets = edge_sets()
    g, labels, pa = sets["const_channel"]
    st, out, stats, _ = BM.run_scene(g, labels, pa)
    assert st == 0 and stats["hit_max_iterations"] == 0
    assert np.all(out["iters"][:, 1] == 0) and np.all(out["iters"][:, [0, 2]] > 0), out["iters"]
    assert np.all(out["err"][:, 1] > 0)                              # |rhs|^2 is not 0 (rounding): the channel stops on |r0|^2 < threshold
    assert np.all(out["iters"][:, 0] != out["iters"][:, 2])          # a cap between the two leaves one capped and one converged
    g, labels, pa = sets["black"]
    st, out, stats, _ = BM.run_scene(g, labels, pa)
    assert st == 0 and stats["iterations_total"] == 0 and stats["strip_pixels"] > 0 and stats["error_max"] == 0.0      # |rhs|^2 = 0
    assert np.array_equal(_bits(out["image"]), _bits(pa["image"]))


def test_unknown_ladder_reaches_the_edges_of_the_reduction_tree():
    """1 and 2 unknowns, and the counts on and beside 256 (the LDS variant's threads), 1024 (the tree's lanes) and 2048; one count
    above 4096 that is no multiple of 1024"""
    got = []
    for name, (g, labels, pa) in ladder_sets().items():
        counts = unknown_counts(g, labels, pa)
        st, out, stats, _ = BM.run_scene(g, labels, pa)
        assert st == 0 and stats["strip_pixels"] == sum(counts) and stats["demoted"] == 0, name
        assert stats["patches_lds"] == len(counts) and stats["patches_global"] == 0, (name, stats)      # every patch fits the LDS tier
        got += counts
    for n in (1, 2, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049):
        assert n in got, (n, got)
    assert any(n > 4096 and n % 1024 for n in got), got


def _fixed_and_uncoupled(name, g, labels, pa, **params):
    """fixed pixels keep their bits; the per-patch entry on one patch alone == its bits inside the set.  Returns (arrays, stats)."""
    st, out, stats, _ = BM.run_scene(g, labels, pa, **params)
    assert st == 0, name
    fixed = out["blending"] != 255
    assert np.array_equal(_bits(out["image"][fixed]), _bits(out["after_writes"][fixed])), name
    assert stats["strip_pixels"] + stats["demoted"] == int((out["blending"] == 255).sum()), name
    assert stats["fixed_pixels"] == int(np.isin(out["blending"], (64, 128)).sum()), name
    for i in range(len(pa["label"])):
        img, _, mask = BM.patch(pa, out, i)
        orig = BM.patch(pa, pa, i)[0]
        after = BM.patch(pa, dict(image=out["after_writes"], validity=out["validity"], blending=out["blending"]), i)[0]
        x, it, err, _ = BM.solve(mask, orig, after, **params)
        assert np.array_equal(_bits(x), _bits(img)), (name, i, params)
        assert np.array_equal(it, out["iters"][i]) and np.array_equal(_bits(err), _bits(out["err"][i])), (name, i, params)
    return out, stats


def test_caps_bind_and_patches_do_not_couple_under_them():
    sets = dict(edge_sets())
    sets.update({k: crafted_sets()[k] for k in ("grid", "wide")})
    bound = 0
    for name, (g, labels, pa) in sets.items():
        base, bst = _fixed_and_uncoupled(name, g, labels, pa)
        assert bst["hit_max_iterations"] == 0, (name, bst)
        for cap in (1, 2, mid_cap(base["iters"])):
            out, stats = _fixed_and_uncoupled(name, g, labels, pa, max_iterations=cap)
            assert np.array_equal(out["iters"], np.minimum(base["iters"], cap)), (name, cap)      # the breaking iteration is not counted
            want = int((base["iters"] >= cap).any(1).sum())
            assert stats["hit_max_iterations"] == want, (name, cap, stats)
            bound += want
            if name != "black" and cap == 1 and bst["iterations_max"] > 1:
                assert stats["hit_max_iterations"] > 0 and stats["error_max"] > bst["error_max"], (name, stats)
    assert bound > 0


def test_tolerance_shortens_the_solve():
    for name in ("grid", "wide"):
        g, labels, pa = crafted_sets()[name]
        it = [BM.run_scene(g, labels, pa, tolerance=t)[2]["iterations_max"] for t in (1e-3, 1e-5, 1e-6)]
        assert 0 < it[0] < it[1] < it[2], (name, it)


def test_line_index_clamp_cannot_fire():
    """item 6: idx = floor(fl(t * float(n - 1))) for t < 1.  The largest such t is 1 - 2^-24, and for every sample count n from 2 to
    2^25 (the device refuses more than 2^22 samples on one edge) the product stays below n - 1 in fp32: the clamp to n - 2 is dead."""
    t = np.nextafter(np.float32(1), np.float32(0))
    assert t < 1 and t.dtype == np.float32
    step = 1 << 22
    for lo in range(1, 1 << 25, step):
        m = np.arange(lo, min(lo + step, 1 << 25), dtype=np.int64)      # n - 1
        prod = t * m.astype(np.float32)
        assert prod.dtype == np.float32
        assert np.all(np.floor(prod).astype(np.int64) <= m - 1), lo


def _constant_scene(colour):
    import copy
    s = copy.copy(get_scene("tiny"))
    s.images = [np.ascontiguousarray(np.broadcast_to(np.uint8(colour), im.shape)) for im in s.images]
    return s


def test_black_and_constant_views():
    labels = SM.crafted_labelings(get_scene("tiny"))["random"]
    s = _constant_scene((0, 0, 0))
    pa = patches_of(s, labels, adjust=False)
    st, out, stats, _ = BM.run_scene(s, labels, pa)
    assert st == 0 and stats["iterations_total"] == 0 and stats["strip_pixels"] > 0
    assert np.array_equal(_bits(out["image"]), _bits(pa["image"]))
    colour = (200, 31, 97)
    s = _constant_scene(colour)
    pa = patches_of(s, labels, adjust=False)
    assert np.all(pa["box"].reshape(-1, 4)[:, :2] >= 0)          # frames inside the views: no crop fill
    st, out, stats, _ = BM.run_scene(s, labels, pa)
    assert st == 0 and stats["hit_max_iterations"] == 0
    c = np.float32(colour) / np.float32(255.0)
    valid = out["validity"] == 255
    assert valid.any() and float(np.abs(out["image"][valid].astype(np.float64) - c.astype(np.float64)).max()) <= 2.0 ** -12


def seam_step(pa, arrays, scene, labels):
    """mean |colour in patch A - colour in patch B| at the midpoints of the seam edges two patches share: the mean over the valid
    pixels of the 3 x 3 block around the midpoint's pixel in each patch"""
    a = BM.flat(pa)
    faces = np.asarray(scene.faces, np.int64)
    box = a["box"].reshape(-1, 4); tc = a["texcoords"].reshape(-1, 3, 2)
    img = np.asarray(arrays["image"]).reshape(-1, 3); val = np.asarray(arrays["validity"])
    proj = {}
    for p in range(len(a["label"])):
        for e in range(int(a["face_ptr"][p]), int(a["face_ptr"][p + 1])):
            for k in range(3):
                proj.setdefault((int(faces[a["faces"][e], k]), p), tc[e, k])
    edges = {}
    for p in range(len(a["label"])):
        for e in range(int(a["face_ptr"][p]), int(a["face_ptr"][p + 1])):
            f = faces[a["faces"][e]]
            for u, v in ((f[0], f[1]), (f[1], f[2]), (f[2], f[0])):
                edges.setdefault((min(u, v), max(u, v)), set()).add(p)
    steps = []
    for (u, v), ps in edges.items():
        if len(ps) != 2:
            continue
        cols = []
        for p in ps:
            m = (proj[(u, p)] + proj[(v, p)]) / 2
            x, y = int(m[0] + 0.5), int(m[1] + 0.5)
            w, h, base = int(box[p, 2]), int(box[p, 3]), int(a["pix_ptr"][p])
            pix = [base + yy * w + xx for yy in range(max(y - 1, 0), min(y + 2, h)) for xx in range(max(x - 1, 0), min(x + 2, w))]
            pix = [i for i in pix if val[i] == 255]
            if pix:
                cols.append(img[pix].astype(np.float64).mean(0))
        if len(cols) == 2:
            steps.append(np.abs(cols[0] - cols[1]).mean())
    assert steps
    return float(np.mean(steps))


def test_planted_offsets_shrink_across_the_seam():
    g = SM.grid_scene(n=8, W=200, H=120)
    g.images = [np.ascontiguousarray(np.full_like(g.images[0], 90)), np.ascontiguousarray(np.full_like(g.images[0], 150))]   # one scene, a per-view offset
    labels = SM.grid_labels(g)
    pa = patches_of(g, labels, adjust=False)
    st, out, stats, _ = BM.run_scene(g, labels, pa)
    assert st == 0
    before = seam_step(pa, pa, g, labels)
    after = seam_step(pa, out, g, labels)
    assert before > 0.2 and after < 0.25 * before, (before, after)


def test_labeling_errors_of_the_model():
    g, labels, pa = crafted_sets()["grid"]
    bad = labels.copy(); bad[int(pa["faces"][0])] = 3 - bad[int(pa["faces"][0])]
    assert BM.run_scene(g, bad, pa)[0] == 4
    pb = dict(pa); f = pa["faces"].copy(); f[0] = len(g.faces); pb["faces"] = f
    assert BM.run_scene(g, labels, pb)[0] == 4
    empty = PM.run_scene(g, np.zeros(len(g.faces), np.uint32))[1]
    st, out, stats, _ = BM.run_scene(g, np.zeros(len(g.faces), np.uint32), empty)
    assert st == 0 and len(out["validity"]) == 0 and stats["seam_edges"] == 0
