"""View masks on the device (run with -m gpu on an MI355X): a masked pixel is an invalid pixel, and nothing else changes (DESIGN.md section 4
"View input" item 10).
  T1  every bit the image preparation leaves behind under masks -- mask words, tile summary, the "no mask" flag, both data terms --
      against orc_validity_mask AND keep, then orc_erode_validity_mask; gradient bytes and unmasked views as without masks
  T2  area term: (original images, mask = not R) gives the oracle's table and labels on the images with R painted black, bit for bit
  T3  gradient term, interior blobs: the surviving pairs from float64 projections, their qualities and costs
  T4  every route to the same masks gives the same bits and table; clearing restores the unmasked table
  T5  masks under a lens: keep bits against oracle.undistort of the 0 / 255 replica; batches; ingest.run with device_undistort on and off
  T6  refusals; the outlier modes run under masks
Widths and heights of 1 are not views (every view input refuses an image below 2 x 2), so the smallest sizes here are 2."""
import os
import re
import threading

import numpy as np
import pytest

import mvs_texturing_amd as M
import oracle_py as O
import util_cases as U
import util_view_masks as VM

pytestmark = pytest.mark.gpu
MVS_ERR_INVALID, MVS_ERR_STATE = 1, 6      # include/mvs_viewsel.h
TERMS = ("gmi", "area")
LENSES = ((0.9, -0.2, 0.05), (1.3, 0.15, -0.03), (0.8, 0.1, 0.0), (1.1, -0.12, 0.0), (0.5, -0.5, 0.0), (0.5, 0.6, 0.0), (0.6, 0.9, 0.7), (1.0, 0.0, 0.3))


class _Read:
    def __init__(self, c, n):
        self.flags = c.prep_mask_flags()
        self.views = [c.prep_products(j) for j in range(n)]
        self.table = c.costs_download()
        self.keep = [c.view_keep_bits(j) for j in range(n)]


def _pass(s, term, masks=None, outlier="none", **options):
    c = M.Context(0)
    try:
        for k, v in options.items():
            c.set_option(k, v)
        c.set_mesh(s.verts, s.faces, s.normals); c.set_views(s.cams, s.images, masks=masks)
        stats = c.mask_stats if masks is not None else None
        c.data_costs(M.Settings(data_term=term, outlier_removal=outlier))
        r = _Read(c, s.n_views)
        r.stats = stats
        return r
    finally:
        c.close()


def _same_table(a, b):
    assert np.array_equal(a.col_ptr, b.col_ptr) and np.array_equal(a.view_id, b.view_id)
    assert np.array_equal(a.cost.view(np.uint32), b.cost.view(np.uint32))


def _check_products(read, s, masks, term, plain):
    """every mask word, summary word and flag of every view against the expected bits; gradient bytes against the unmasked pass `plain`"""
    want = [VM.expected_products(i, m, term) for i, m in zip(s.images, masks)]
    flags = np.array([0 if bits.all() else 1 for bits, _ in want], np.uint8)
    assert np.array_equal(read.flags, flags), [(j, int(g), int(w)) for j, (g, w) in enumerate(zip(read.flags, flags)) if g != w]
    for j, (p, (bits, tiles)) in enumerate(zip(read.views, want)):
        h, w = s.images[j].shape[:2]
        tag = (j, w, h, term)
        if term == "gmi":
            assert np.array_equal(p.gmi, plain.views[j].gmi), (tag, "gradient bytes moved")
        if masks[j] is None:
            assert read.keep[j] is None, tag
            assert plain.flags[j] == flags[j], tag
            if flags[j]:                                               # an unmasked view: the products of a context that never saw a mask
                assert np.array_equal(p.mask_words, plain.views[j].mask_words) and np.array_equal(p.summary_words, plain.views[j].summary_words), tag
        else:
            kb, kpad = read.keep[j]
            assert np.array_equal(kb, masks[j] != 0) and not kpad.any(), (tag, "keep words")
        if not flags[j]:
            continue
        got, pad = p.mask_bits()
        bad = np.argwhere(got != bits)
        assert len(bad) == 0, (tag, "%d wrong mask bits; (y, x, got) %s" % (len(bad), [(y, x, bool(got[y, x])) for y, x in bad[:8].tolist()]))
        assert not pad.any(), (tag, "padding bits set")
        assert np.array_equal(p.mask_words, U.pack_mask_words(bits)), tag
        t, tpad = p.summary_bits()
        assert np.array_equal(t, tiles) and not tpad.any(), (tag, "summary bits")
        assert np.array_equal(p.summary_words, U.pack_summary_words(tiles)), tag


# ---- T1. every bit ----

T1_SIZES = ((2, 2), (2, 33), (31, 2), (32, 3), (33, 33), (63, 2), (64, 3), (64, 33), (65, 33), (95, 3), (95, 33), (97, 67))


def _t1_scene(w, h):
    rng = np.random.default_rng(1000 * w + h)
    hostile = list(U.small_hostile_images(rng, w, h).values())
    hostile.append(np.ascontiguousarray(rng.integers(1, 255, (h, w, 3)).astype(np.uint8)))
    n = max(len(hostile), len(VM.MASK_PATTERNS))
    images = [hostile[k % len(hostile)] for k in range(n)] + hostile[:3]                 # ... and three views without a mask among them
    masks = [VM.mask_pattern(VM.MASK_PATTERNS[k % len(VM.MASK_PATTERNS)], w, h) for k in range(n)] + [None] * 3
    return U.prep_scene(images), masks


@pytest.mark.parametrize("size", T1_SIZES, ids=lambda s: "%dx%d" % s)
def test_every_bit(size):
    """every mask pattern on the hostile images of one size, three unmasked views mixed in; rows of a [h][w] byte mask start at every residue
    modulo 16 (odd widths with 33 rows), the last word of a row is partial; 32 x 3 and 64 x 3 / 64 x 33 take the vectorised image kernels"""
    w, h = size
    s, masks = _t1_scene(w, h)
    if w % 2 and h >= 16:
        assert {(y * w) % 16 for y in range(h)} == set(range(16))
    zeros = sum(int((m == 0).sum()) for m in masks if m is not None)
    for term in TERMS:
        plain = _pass(s, term)
        r = _pass(s, term, masks)
        assert r.stats["views_masked"] == len(masks) - 3 and r.stats["views_undistorted"] == 0
        assert r.stats["pixels"] == (len(masks) - 3) * w * h and r.stats["pixels_masked_out"] == zeros
        assert r.stats["device_bytes"] == 4 * (len(masks) - 3) * h * ((w + 31) // 32)
        _check_products(r, s, masks, term, plain)


def test_no_black_corner_anywhere_masked_views_go_round_the_shortcut():
    """no view has a black corner pixel: the flood has no seed; the views that carry a mask still get mask_final and the summary, the
    others drop their mask pointers as in a scene without masks -- black islands included"""
    rng = np.random.default_rng(77)
    imgs = [np.ascontiguousarray(rng.integers(1, 255, (h, w, 3)).astype(np.uint8)) for w, h in ((64, 48), (64, 48), (45, 37), (64, 48), (33, 9))]
    imgs[1][10:20, 10:30] = 0; imgs[3][5:9, 40:50] = 0                                    # islands: black, unreachable
    s = U.prep_scene(imgs)
    masks = [VM.mask_pattern("checker", 64, 48), None, VM.mask_pattern("interior", 45, 37), VM.mask_pattern("all_keep", 64, 48), VM.mask_pattern("col32", 33, 9)]
    for term in TERMS:
        plain = _pass(s, term)
        assert not plain.flags.any()
        r = _pass(s, term, masks)
        assert r.flags.tolist() == [1, 0, 1, 0, 1]
        _check_products(r, s, masks, term, plain)
    for j in (1, 3):                                                                      # one masked view among five: a checkerboard, then a mask that keeps everything
        one = [None] * 5; one[j] = masks[0] if j == 1 else masks[3]
        r = _pass(s, "gmi", one)
        _check_products(r, s, one, "gmi", _pass(s, "gmi"))


# ---- T2. exact against the oracle: area term, painted black = masked ----

@pytest.fixture(scope="module")
def small():
    s = VM.small_scene()
    R = VM.corner_regions(s)
    return s, R, [np.ascontiguousarray(np.where(r, 0, 255).astype(np.uint8)) for r in R]


def _table_and_labels(c, s, settings):
    c.data_costs(settings)
    t = c.costs_download()
    labels, ms = c.view_selection(s.adj_ptr, s.adj)
    return t, labels, ms


def test_mask_equals_painting_black_area_term(small):
    s, R, masks = small
    painted = M.synth.Scene(); painted.__dict__.update(s.__dict__)
    painted.images = [np.ascontiguousarray(np.where(r[:, :, None], 0, i).astype(np.uint8)) for i, r in zip(s.images, R)]
    ref, _ = O.data_costs(painted, data_term="area")
    lo, so = O.view_selection(ref, s.adj_ptr, s.adj)
    st = M.Settings(data_term="area")
    c = M.Context(0)
    try:
        c.set_mesh(s.verts, s.faces, s.normals); c.set_views(s.cams, s.images)
        full, _, _ = _table_and_labels(c, s, st)
        c.set_view_masks(masks)
        got, labels, ms = _table_and_labels(c, s, st)
    finally:
        c.close()
    print("pairs: unmasked %d, masked %d, oracle on the painted images %d" % (full.nnz, got.nnz, ref.nnz))
    assert got.nnz <= 0.95 * full.nnz, (got.nnz, full.nnz)                                 # the mask decides something
    _same_table(got, ref)
    assert np.array_equal(labels, lo) and ms["energy_fixed"] == so["energy_fixed"]


# ---- T3. gradient term, interior blobs ----

@pytest.fixture(scope="module")
def blobs():
    s = VM.small_scene()
    masks = VM.interior_blobs(s)
    ref, _ = O.data_costs(s, data_term="gmi")
    bits = [VM.expected_products(i, m, "gmi")[0] for i, m in zip(s.images, masks)]
    survives, decided = VM.surviving_pairs(s, ref, bits)
    assert (~decided).sum() <= 0.01 * ref.nnz
    return s, masks, ref, survives, decided


def _pair_keys(col_ptr, view_id, n_views):
    face = np.repeat(np.arange(len(col_ptr) - 1, dtype=np.int64), np.diff(col_ptr.astype(np.int64)))
    return face * n_views + view_id.astype(np.int64)


def test_interior_blobs_gradient_term(blobs):
    s, masks, ref, survives, decided = blobs
    r = _pass(s, "gmi", masks)
    got = r.table
    kref, kgot = _pair_keys(ref.col_ptr, ref.view_id, s.n_views), _pair_keys(got.col_ptr, got.view_id, s.n_views)
    pos = np.searchsorted(kref, kgot)
    assert (pos < len(kref)).all() and np.array_equal(kref[pos], kgot)                     # every pair is a pair of the unmasked table
    assert np.array_equal(got.quality.view(np.uint32), ref.quality[pos].view(np.uint32))   # ... with the same quality bits
    present = np.zeros(ref.nnz, bool); present[pos] = True
    print("pairs: unmasked %d, masked %d, undecided %d" % (ref.nnz, got.nnz, int((~decided).sum())))
    assert np.array_equal(present[decided], survives[decided])
    col_ptr, view_id, q, cost = VM.masked_table_from(ref, present)                         # the costs of exactly the pairs the device kept
    assert np.array_equal(col_ptr, got.col_ptr) and np.array_equal(view_id, got.view_id)
    assert np.array_equal(cost.view(np.uint32), got.cost.view(np.uint32))


@pytest.mark.parametrize("mode", ["gauss_damping", "gauss_clamping"])
def test_outlier_modes_run_under_masks(blobs, mode):
    """the mean colours are not masked, so exactness is not claimed: the pattern is a subset of the gradient term's masked pattern"""
    s, masks, ref, survives, decided = blobs
    base = _pass(s, "gmi", masks).table
    got = _pass(s, "gmi", masks, outlier=mode).table
    kb, kg = _pair_keys(base.col_ptr, base.view_id, s.n_views), _pair_keys(got.col_ptr, got.view_id, s.n_views)
    assert got.nnz > 0 and np.isin(kg, kb).all()


# ---- T4. routes agree ----

def _bits_and_table(c, s, st=None):
    c.data_costs(st or M.Settings())
    return [c.prep_products(j).mask_words for j in range(s.n_views)], c.prep_mask_flags(), c.costs_download()


def _same_run(a, b):
    assert np.array_equal(a[1], b[1])
    for j, (x, y) in enumerate(zip(a[0], b[0])):
        if a[1][j]:
            assert np.array_equal(x, y), j
    _same_table(a[2], b[2])


def test_routes_agree(blobs):
    import torch
    s, masks, ref, _, _ = blobs
    c = M.Context(0)
    try:
        c.set_mesh(s.verts, s.faces, s.normals)
        c.set_views(s.cams, s.images)
        plain = _bits_and_table(c, s)
        _same_table(plain[2], ref)
        c.set_views(s.cams, s.images, masks=masks)
        a = _bits_and_table(c, s)
        assert a[2].nnz < plain[2].nnz
        c.set_views(s.cams, s.images); c.set_view_masks(masks)                            # the entry on its own, behind the views
        _same_run(_bits_and_table(c, s), a)
        dev = [torch.from_numpy(m).to("cuda:0") for m in masks]                           # device-resident masks
        odd = torch.zeros(masks[0].size + 16, dtype=torch.uint8, device="cuda:0")         # ... one of them 5 bytes off every alignment
        odd[5:5 + masks[0].size] = dev[0].reshape(-1); dev[0] = odd[5:5 + masks[0].size].view(masks[0].shape)
        assert dev[0].data_ptr() % 16 == 5
        c.set_view_masks(dev)
        _same_run(_bits_and_table(c, s), a)
        c.set_option("dc_range_pairs", (s.n_faces // 3 + 1) * s.n_views)                  # three ranges of faces: the walk prepares the views once
        c.set_view_masks(masks)
        _same_run(_bits_and_table(c, s), a)
        assert c.dc_ranges()[0] == 3
        c.set_option("dc_range_pairs", 0)
        c.set_view_masks([None] * s.n_views)                                              # cleared: the unmasked table, bit for bit
        _same_run(_bits_and_table(c, s), plain)
        c.set_view_masks(masks); c.set_view_masks(None)
        _same_run(_bits_and_table(c, s), plain)
        c.set_view_masks(masks); c.set_views(s.cams, s.images)                            # a later view input clears them too
        _same_run(_bits_and_table(c, s), plain)
        assert all(c.view_keep_bits(j) is None for j in range(s.n_views))
    finally:
        c.close()


def test_jpeg_route_agrees(blobs):
    s, masks, _, _, _ = blobs
    files = [M.encode_jpeg(i, quality=90, subsampling=1) for i in s.images]                # 4:2:0
    pixels = [M.decode_jpeg(f) for f in files]
    c = M.Context(0)
    try:
        c.set_mesh(s.verts, s.faces, s.normals)
        c.set_views(s.cams, pixels, masks=masks)
        a = _bits_and_table(c, s)
        c.set_views_jpeg(s.cams, files, masks=masks)
        assert c.mask_stats["views_masked"] == s.n_views
        _same_run(_bits_and_table(c, s), a)
        c.set_views_jpeg(s.cams, files); c.set_view_masks(masks)
        _same_run(_bits_and_table(c, s), a)
    finally:
        c.close()


def test_two_logical_shards_give_the_one_context_labels(blobs):
    import torch
    s, masks, _, _, _ = blobs
    dev = torch.device("cuda:0")
    c0 = M.Context(0)
    try:
        c0.set_mesh(s.verts, s.faces, s.normals); c0.set_views(s.cams, s.images, masks=masks)
        c0.data_costs(M.Settings()); t0 = c0.costs_download()
        lab0, st0 = c0.view_selection(s.adj_ptr, s.adj)
    finally:
        c0.close()
    tap, tad = torch.from_numpy(s.adj_ptr.view(np.int32)).to(dev), torch.from_numpy(s.adj.view(np.int32)).to(dev)
    torch.cuda.synchronize()
    P = 2
    comms = M.shard.Comm.local(P, [0, 0])
    out, err = [None] * P, [None] * P

    def rank_main(r):
        try:
            torch.cuda.set_device(0)
            c = M.Context(0); c.set_mesh(s.verts, s.faces, s.normals); c.set_views(s.cams, s.images, masks=masks)   # images are replicated and so are masks
            sh = M.shard.Shard(c, comms[r], None, tap, tad)
            own = sh.own_faces()
            labels = torch.zeros(max(len(own), 1), dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            _, nnz = sh.data_costs(M.Settings())
            ms = sh.view_selection(labels); c.synchronize()
            out[r] = (own, labels.cpu().numpy().view(np.uint32)[:len(own)], nnz, ms)
            sh.close(); c.close()
        except Exception as e:  # noqa: BLE001
            err[r] = e
            comms[r].abort()
            raise
    th = [threading.Thread(target=rank_main, args=(r,), daemon=True) for r in range(P)]
    for t in th: t.start()
    for t in th: t.join(timeout=120)
    assert not any(t.is_alive() for t in th), "a rank is blocked"
    assert all(e is None for e in err), err
    for cm in comms: cm.close()
    labels = np.zeros(s.n_faces, np.uint32)
    for own, lab, nnz, ms in out:
        labels[own] = lab
        assert nnz == t0.nnz
    assert np.array_equal(labels, lab0) and out[0][3]["energy_fixed"] == st0["energy_fixed"]


# ---- T5. masks under a lens ----

LENS_SIZES = ((33, 5), (64, 48), (95, 7))


@pytest.fixture(scope="module")
def lens_cases():
    rng = np.random.default_rng(31)
    cases = [(size, lens) for size in LENS_SIZES for lens in LENSES]
    images = [np.ascontiguousarray(rng.integers(1, 255, (h, w, 3)).astype(np.uint8)) for (w, h), _ in cases]
    masks = []
    for k, ((w, h), _) in enumerate(cases):
        m = VM.mask_pattern(("checker", "interior", "col31", "blob_at_black", "border_top", "col_last", "corner_br", "all_keep")[k % 8], w, h)
        m[rng.random((h, w)) < 0.08] = 0
        masks.append(m)
    lens = np.array([l for _, l in cases], np.float32)
    want = [VM.keep_bits_under_lens(m, l) for m, (_, l) in zip(masks, cases)]
    return U.prep_scene(images), cases, masks, lens, want


def _check_keep(c, want):
    for j, w in enumerate(want):
        bits, pad = c.view_keep_bits(j)
        bad = np.argwhere(bits != w)
        assert len(bad) == 0 and not pad.any(), (j, w.shape, "%d wrong keep bits %s" % (len(bad), bad[:6].tolist()))


def test_keep_bits_under_the_eight_lenses(lens_cases):
    s, cases, masks, lens, want = lens_cases
    n = len(cases)
    moved = sum(not np.array_equal(w, m != 0) for w, m, (_, l) in zip(want, masks, cases) if l[1] != 0.0)
    assert moved >= n - 6                                                                  # the lenses move bits (the oracle side)
    c = M.Context(0)
    try:
        c.set_mesh(s.verts, s.faces, s.normals)
        c.set_views(s.cams, s.images, lens=lens, masks=masks)
        st = c.mask_stats
        assert st["views_masked"] == n and st["views_undistorted"] == sum(1 for _, l in cases if l[1] != 0.0) == n - 3 and st["batches"] == 1
        assert st["pixels_masked_out"] == sum(int((~w).sum()) for w in want)
        _check_keep(c, want)
        c.data_costs(M.Settings(data_term="area"))                                          # ... and they reach the validity mask
        for j in (0, 9, 23):
            bits = VM.expected_products(c.view_image(j), want[j].astype(np.uint8), "area")[0]
            if not bits.all():
                assert np.array_equal(c.prep_products(j).mask_bits()[0], bits), j
        # staging at the refusal boundary: the cap is the largest mask, 64 x 48 -- each of those a batch of its own, the small ones in groups
        sizes = [((w * h + 15) // 16) * 16 for (w, h), _ in cases]
        cap = max(sizes)
        batches, room = 0, 0
        for b in sizes:
            if batches == 0 or room + b > cap:
                batches, room = batches + 1, 0
            room += b
        assert batches >= 9
        c.set_views_jpeg(s.cams, [None] * n, params=M.default_jpegdec_params(max_scratch_bytes=cap), images=s.images)
        st = c.set_view_masks(masks, lens=lens)
        assert st["batches"] == batches and st["staging_bytes"] == cap
        _check_keep(c, want)
        # one byte less: the first 64 x 48 view does not fit alone and is refused with its number
        c.set_views_jpeg(s.cams, [None] * n, params=M.default_jpegdec_params(max_scratch_bytes=cap - 1), images=s.images)
        with pytest.raises(M.MvsError) as e:
            c.set_view_masks(masks, lens=lens)
        m = re.search(r"view (\d+) needs (\d+) bytes of staging, max_scratch_bytes is (\d+)", str(e.value))
        assert e.value.status == MVS_ERR_INVALID and m and (int(m.group(1)), int(m.group(2)), int(m.group(3))) == (len(LENSES), cap, cap - 1), str(e.value)
        assert all(c.view_keep_bits(j) is None for j in range(n))                          # a refusal leaves the context without masks
    finally:
        c.close()


def test_ingest_run_device_undistort_on_and_off(tmp_path):
    """a masked, distorted scene folder: the mask goes in in the camera's frame with the view's lens, or is undistorted on the host by the
    same rule -- the same .spt and .vec"""
    from PIL import Image
    from conftest import get_scene
    from mvs_texturing_amd import ingest
    s = get_scene("tiny")
    d = str(tmp_path / "scene"); mesh = str(tmp_path / "mesh.ply")
    ingest.save_scene_folder(s, d, mesh)
    h, w = s.images[0].shape[:2]
    yy, xx = np.mgrid[0:h, 0:w]
    for j, dist in {0: (-0.2, 0.05), 3: (-0.12, 0.0)}.items():
        p = os.path.join(d, "view_%04d.cam" % j)
        cam = ingest.read_cam_file(p); cam.dist[:] = dist; ingest.write_cam_file(p, cam)
    for j in (0, 2, 3):
        m = np.full((h, w), 255, np.uint8); m[(xx - w * 0.5) ** 2 + (yy - h * 0.45) ** 2 < (30 + 8 * j) ** 2] = 0; m[:, :25 + j] = 0
        Image.fromarray(m).save(os.path.join(d, "view_%04d.mask.png" % j))
    outs = {}
    for key, kw in (("host", {}), ("device", dict(device_undistort=True)), ("nomask", dict(masks=False))):
        prefix = str(tmp_path / key)
        ingest.run(d, mesh, prefix, **dict(dict(masks=True), **kw))
        outs[key] = (open(prefix + "_data_costs.spt", "rb").read(), open(prefix + "_labeling.vec", "rb").read())
    assert outs["host"] == outs["device"]
    assert outs["host"][0] != outs["nomask"][0]                                            # the masks decided something


# ---- T6. refusals ----

def test_refusals(blobs):
    s, masks, _, _, _ = blobs
    n = s.n_views
    good = np.array([(0.9, 0.0, 0.0)] * n, np.float32)
    c = M.Context(0)
    try:
        with pytest.raises(M.MvsError) as e:                                               # called without views
            c.set_view_masks(masks)
        assert e.value.status == MVS_ERR_STATE and "no views" in str(e.value)
        c.set_mesh(s.verts, s.faces, s.normals); c.set_views(s.cams, s.images)
        with pytest.raises(M.MvsError) as e:                                               # wrong n_views
            c.set_view_masks(masks[:-1])
        assert e.value.status == MVS_ERR_INVALID and "n_views is %d" % (n - 1) in str(e.value) and "has %d views" % n in str(e.value)
        for row, view, why in (((np.nan, 0.1, 0.0), 2, "must be finite"), ((0.9, np.inf, 0.0), 2, "must be finite"), ((0.9, 0.1, 0.0, 5), 4, "reserved must be 0"),
                               ((0.0, 0.1, 0.0), 1, "positive focal length")):
            bad = np.zeros((n, 4), np.float32); bad[:, :3] = good; bad[view, :len(row)] = row
            c.set_view_masks(masks)                                                         # masks are there ...
            with pytest.raises(M.MvsError) as e:
                c.set_view_masks(masks, lens=bad)
            assert e.value.status == MVS_ERR_INVALID and "view %d" % view in str(e.value) and why in str(e.value), str(e.value)
            assert e.value.stats["views_masked"] == 0
            assert all(c.view_keep_bits(j) is None for j in range(n))                      # ... and gone after the refusal
        with pytest.raises(AssertionError):                                                # the binding checks the size before the library sees the pointer
            c.set_view_masks([masks[0][:-1]] + masks[1:])
        c.set_view_masks(masks)                                                             # still usable
        c.data_costs(M.Settings())
        assert c.costs_download().nnz > 0
    finally:
        c.close()
