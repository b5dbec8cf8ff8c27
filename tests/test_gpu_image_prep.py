"""The image preparation (csrc/k_prep.hip) byte by byte and bit by bit (run with -m gpu on an MI355X): after one data-cost pass per context and
setting, what the kernels wrote is read back (mvs_ctx_prep_products, building-blocks library) and EVERY byte of the gradient-magnitude image,
every bit of the validity mask (plain for the area term, eroded for the gradient term, padding bits included), every word of the 32 x 32 tile
summary and the "this view has no mask" flag of the device view table are held against the oracle's orc_validity_mask / orc_erode_validity_mask /
orc_gradient_magnitude (pinned to upstream's texture_view.cpp in tests/test_reference_pins.py) and against the numpy restatement of the summary's
definition (tests/util_cases.py tile_summary_numpy, pinned to upstream's valid_pixel in tests/test_image_prep_host.py).  The crafted images are
tests/util_cases.py's; the shapes are the smallest at which each kernel's index arithmetic can go wrong.  Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import mvs_texturing_amd as M
import oracle_py as O
import util_cases as U

pytestmark = pytest.mark.gpu
MVS_ERR_INVALID, MVS_ERR_STATE = 1, 6      # include/mvs_viewsel.h
TERMS = ("gmi", "area")
_REF = {}


def _ref(img):
    """the oracle's products of one image, computed once: plain and eroded mask (bool), gradient magnitude (u8), tile summaries of both masks"""
    k = id(img)
    if k not in _REF:
        L = O.load()
        h, w = img.shape[:2]
        plain = np.zeros((h, w), np.uint8); L.orc_validity_mask(O._ptr(img), w, h, O._ptr(plain))
        eroded = plain.copy(); L.orc_erode_validity_mask(O._ptr(eroded), w, h)
        gmi = np.zeros((h, w), np.uint8); L.orc_gradient_magnitude(O._ptr(img), w, h, O._ptr(gmi))
        plain, eroded = plain.astype(bool), eroded.astype(bool)
        assert not (eroded & ~plain).any()
        _REF[k] = dict(img=img, area=plain, gmi_mask=eroded, gmi=gmi, area_sum=U.tile_summary_numpy(plain), gmi_sum=U.tile_summary_numpy(eroded))
    return _REF[k]


class _Read:
    """everything one pass left behind: flags, per-view products, the cost table"""
    def __init__(self, c, n):
        self.flags = c.prep_mask_flags()
        self.views = [c.prep_products(j) for j in range(n)]
        self.table = c.costs_download()


def _pass(c, s, term, images=None):
    c.set_mesh(s.verts, s.faces, s.normals); c.set_views(s.cams, images if images is not None else s.images)
    c.data_costs(M.Settings(data_term=term))
    return _Read(c, s.n_views)


def _fresh(s, term, images=None, **options):
    c = M.Context(0)
    try:
        for k, v in options.items():
            c.set_option(k, v)
        return _pass(c, s, term, images)
    finally:
        c.close()


def _check(read, s, term, names=None):
    """every product of every view of one pass against the oracle"""
    names = names or ["view %d" % j for j in range(s.n_views)]
    refs = [_ref(i) for i in s.images]
    want_flags = np.array([0 if r[term if term == "area" else "gmi_mask"].all() else 1 for r in refs], np.uint8)
    # flag 0 for EVERY view whose oracle mask is all ones (mask_trivial_kernel / the no-seed shortcut), flag 1 for every other
    assert np.array_equal(read.flags, want_flags), [(n, int(g), int(w)) for n, g, w in zip(names, read.flags, want_flags) if g != w]
    for j, (p, r, name) in enumerate(zip(read.views, refs, names)):
        h, w = s.images[j].shape[:2]
        tag = (name, w, h, term)
        assert (p.width, p.height) == (w, h) and p.mask_words.shape == (h, (w + 31) // 32), tag
        if term == "gmi":
            bad = np.argwhere(p.gmi != r["gmi"])
            assert len(bad) == 0, (tag, "%d wrong gradient bytes; (y, x, got, want) %s" % (len(bad), [(y, x, int(p.gmi[y, x]), int(r["gmi"][y, x])) for y, x in bad[:6].tolist()]))
        else:
            assert p.gmi is None, tag
        if not read.flags[j]:
            continue                                                   # (the oracle's mask is all ones: asserted above)
        want = r["area" if term == "area" else "gmi_mask"]
        bits, pad = p.mask_bits()
        bad = np.argwhere(bits != want)
        assert len(bad) == 0, (tag, "%d wrong mask bits; (y, x, got) %s" % (len(bad), [(y, x, bool(bits[y, x])) for y, x in bad[:8].tolist()]))
        assert not pad.any(), (tag, "padding bits set", np.argwhere(pad)[:8].tolist())
        assert np.array_equal(p.mask_words, U.pack_mask_words(want)), tag
        tiles, tpad = p.summary_bits()
        wsum = r["area_sum" if term == "area" else "gmi_sum"]
        assert p.summary_words.shape == ((h + 31) // 32, 2 * ((p.mask_words.shape[1] + 63) // 64)), tag
        bad = np.argwhere(tiles != wsum)
        assert len(bad) == 0, (tag, "%d wrong summary bits; (ty, tx, got) %s" % (len(bad), [(y, x, bool(tiles[y, x])) for y, x in bad[:8].tolist()]))
        assert not tpad.any(), (tag, "summary bits of tiles behind the last one are set")
        assert np.array_equal(p.summary_words, U.pack_summary_words(wsum)), tag


def _same(a, b):
    """two read-backs are the same: flags, gradient bytes, and the words of every view that still has a mask"""
    assert np.array_equal(a.flags, b.flags)
    for j, (p, q) in enumerate(zip(a.views, b.views)):
        assert (p.gmi is None) == (q.gmi is None) and (p.gmi is None or np.array_equal(p.gmi, q.gmi)), j
        if a.flags[j]:
            assert np.array_equal(p.mask_words, q.mask_words) and np.array_equal(p.summary_words, q.summary_words), j
    assert np.array_equal(a.table.col_ptr, b.table.col_ptr) and np.array_equal(a.table.view_id, b.table.view_id)
    assert np.array_equal(a.table.cost.view(np.uint32), b.table.cost.view(np.uint32))


def _table_equals_oracle(read, s, term):
    ref, _ = O.data_costs(s, data_term=term)
    assert np.array_equal(read.table.col_ptr, ref.col_ptr) and np.array_equal(read.table.view_id, ref.view_id)
    assert np.array_equal(read.table.cost.view(np.uint32), ref.cost.view(np.uint32))
    return ref


_SCENES = {}


def _scene(name):
    """the contexts' scenes, built once: (scene, view names)"""
    if name in _SCENES:
        return _SCENES[name]
    rng = np.random.default_rng(4242)
    imgs, names = [], []

    def add(n, i):
        names.append(n); imgs.append(i)
    if name == "vector":        # a.: widths multiple of 32 only -- the vectorised kernels; the grids are sized by the largest view
        for w in (32, 64, 1024, 1056):
            add("w%d" % w, U.noise_blob(rng, w, 35, 9, 7))
        for h in (2, 3, 15, 16, 17, 18, 33):                          # the FUSE_ROWS = 16 seams, the halo rows, h - 1 on a tile's first and last row
            add("h%d" % h, U.noise_blob(rng, 64, h, 5, min(h, 4)))
            add("h%d wide" % h, U.noise_blob(rng, 1056, h, 40, min(h, 6)))
        add("sobel pairs", U.sobel_pairs_image(1056))
        img = U.noise_blob(rng, 2080, 34, 12, 10, lo=1)               # tiles tx >= 64: the summary's second ballot wave, msum_stride = 4
        img[0:20, 2050:2071] = 0; img[0, 2050:2080] = 0               # a notch from the top border, flooded from the corner (2079, 0)
        add("notch", np.ascontiguousarray(img))
    elif name == "generic":     # b.: one width that is no multiple of 32 sends every view down the generic kernels
        for w in (2, 3, 5, 31, 33, 63, 65, 66, 129, 130):             # 64-pixel tiles of gmi_kernel, 32-bit mask words, w - 1 on a word's first and last bit
            add("w%d" % w, U.noise_blob(rng, w, 6, max(1, min(3, w - 1)), 3))
        for h in (2, 3, 4, 5, 9):                                     # 4-row tiles and mask blocks
            add("h%d" % h, U.noise_blob(rng, 33, h, 4, min(h, 3)))
            add("h%d w130" % h, U.noise_blob(rng, 130, h, 35, min(h, 3)))
        add("64x5", U.noise_blob(rng, 64, 5, 33, 3))
        add("sobel pairs", U.sobel_pairs_image(1057))
    elif name == "small_b":     # g.: fewer and smaller views than "generic"
        for w, h in ((33, 4), (5, 9), (64, 3)):
            add("%dx%d" % (w, h), U.noise_blob(rng, w, h, 2, 2))
    elif name == "no_seed":     # f.: no view has a black corner -- islands and a black border pixel that is no corner do not seed the flood
        a = rng.integers(1, 255, (48, 64, 3)).astype(np.uint8); a[10:20, 10:30] = 0; a[30:40, 40:50] = 0
        b = rng.integers(1, 255, (48, 64, 3)).astype(np.uint8); b[0, 5] = 0; b[20, 0] = 0; b[47, 62] = 0; b[10, 63] = 0
        c = rng.integers(1, 255, (37, 45, 3)).astype(np.uint8); c[1, 1] = 0
        for n, i in (("islands", a), ("border pixels", b), ("next to the corner", c), ("noise", rng.integers(1, 255, (48, 64, 3)).astype(np.uint8))):
            add(n, np.ascontiguousarray(i))
    elif name == "one_seed":    # f.: exactly one of five views has a black corner pixel
        for k in range(5):
            i = rng.integers(1, 255, (48, 64, 3)).astype(np.uint8); i[20:25, 20:25] = 0
            if k == 3: i[47, 63] = 0
            add("view %d" % k, np.ascontiguousarray(i))
    elif name == "checker":
        add("checker", U.hostile_images(rng, 64, 48)["checker"])
        add("checker odd", U.hostile_images(rng, 64, 47)["checker"])
    elif name.startswith("hostile"):                                   # d.: the eight flood-fill-breaking patterns
        w, h = (320, 240) if name == "hostile_fast" else (97, 67)
        for n, i in U.hostile_images(rng, w, h).items():
            add(n, i)
    elif name.startswith("small"):                                     # d.: the small patterns at one size
        w, h = (int(x) for x in name.split("_")[1].split("x"))
        for n, i in U.small_hostile_images(rng, w, h).items():
            add(n, i)
    elif name.startswith("tiles"):                                     # e.: rims on the summary's tile grid
        w, h = (int(x) for x in name.split("_")[1].split("x"))
        add("tile_rims", U.hostile_images(rng, w, h)["tile_rims"])
        for bx, by in ((31, 31), (32, 32), (33, 33), (31, 33), (33, 31), (32, 5), (5, 32)):
            add("rim %d %d" % (bx, by), U.rim_blob(rng, w, h, bx, by))
        for corner in ("tr", "bl", "br"):                              # the shared column / row 32 t + 32 is the tile's ONLY invalid one
            for b in (31, 32, 33, 34):
                add("rim %s %d" % (corner, b), U.rim_blob(rng, w, h, b, b, corner))
    else:
        raise KeyError(name)
    _SCENES[name] = (U.prep_scene(imgs), names)
    return _SCENES[name]


# ---- a. the vectorised paths ----

def test_vectorised_paths_fused_and_two_pass():
    """lum_sobel_kernel (prep_fused = 1), lum_zero_kernel + sobel4_kernel (prep_fused = 0) and the word-parallel mask kernels on views of 21
    sizes in ONE context: strip seam x = 1023 | 1024 with a partial second strip, tile rows 15 | 16, heights from 2, every Sobel argument,
    and tiles tx >= 64 with a zero summary bit among them"""
    s, names = _scene("vector")
    assert all(i.shape[1] % 32 == 0 for i in s.images)
    U.assert_sobel_pairs_coverage(s.images[names.index("sobel pairs")])            # the reference side holds every pair: only then compare
    notch = _ref(s.images[names.index("notch")])
    assert notch["gmi_sum"].shape == (2, 65) and not notch["gmi_sum"][0, 64] and notch["gmi_sum"][1, 64] and not notch["area_sum"][0, 64] and notch["gmi_sum"][0, 5]
    fused = _fresh(s, "gmi", prep_fused=1)
    _check(fused, s, "gmi", names)
    two = _fresh(s, "gmi", prep_fused=0)
    _check(two, s, "gmi", names)
    _same(fused, two)
    _check(_fresh(s, "area"), s, "area", names)


# ---- b. the generic paths ----

def test_generic_paths():
    """gmi_kernel, mask_zero_kernel and the mask kernels at widths 2 .. 130 and heights 2 .. 9, a 64 x 5 view forced down the generic path
    by its neighbours, and every Sobel argument at width 1057"""
    s, names = _scene("generic")
    assert any(i.shape[1] % 32 for i in s.images)
    U.assert_sobel_pairs_coverage(s.images[names.index("sobel pairs")])
    for term in TERMS:
        _check(_fresh(s, term), s, term, names)


# ---- c. misaligned device images ----

def test_misaligned_device_images_take_the_generic_path():
    """device-resident 64 x 8 images that start one byte into a larger tensor: (rgb & 3) != 0 sends the context down the generic kernels; the
    same images at offset 0 go through the vectorised ones -- the same bytes and bits either way, and the oracle's"""
    import torch
    rng = np.random.default_rng(7)
    imgs = [U.noise_blob(rng, 64, 8, 3 + 30 * k, 2 + 3 * k) for k in range(3)]
    s = U.prep_scene(imgs)
    n = 64 * 8 * 3
    dev = torch.device("cuda:0")
    reads = {}
    for off in (1, 0):
        big = [torch.zeros(n + 16, dtype=torch.uint8, device=dev) for _ in imgs]
        views = []
        for b, i in zip(big, s.images):
            b[off:off + n] = torch.from_numpy(i.reshape(-1)).to(dev)
            views.append(b[off:off + n].view(8, 64, 3))
            assert views[-1].data_ptr() % 4 == off and views[-1].is_contiguous()
        torch.cuda.synchronize()
        for term in TERMS:
            reads[off, term] = _fresh(s, term, images=views)
            _check(reads[off, term], s, term)
    for term in TERMS:
        _same(reads[1, term], reads[0, term])


# ---- d. hostile masks, every bit ----

HOSTILE_ERODE_PIXELS = {   # pattern -> (x, y, w, h): a pixel that is valid before the erosion and invalid after it, from the pattern's definition
    "vline31": lambda w, h: (32, 1), "vline32": lambda w, h: (31, 1),            # the kill crosses the 31 | 32 word boundary, both ways
    "blob_rim": lambda w, h: (w - 1, 1), "frame2": lambda w, h: (2, 2), "hline": lambda w, h: (1, 2) if h >= 4 and w >= 3 else None,
}


def _assert_erosion(s, names, w, h):
    """the eroded oracle mask differs from the plain one exactly where the pattern says it must"""
    for i, n in zip(s.images, names):
        r = _ref(i)
        assert (not np.array_equal(r["area"], r["gmi_mask"])) == U.erosion_bites(n, w, h), (n, w, h)
        px = HOSTILE_ERODE_PIXELS.get(n, lambda w, h: None)(w, h)
        if px:
            assert r["area"][px[1], px[0]] and not r["gmi_mask"][px[1], px[0]], (n, w, h, px)


@pytest.mark.parametrize("which", ["hostile_fast", "hostile_generic"])
def test_hostile_patterns_every_bit(which):
    """the eight flood-fill-breaking patterns at 320 x 240 (vectorised) and 97 x 67 (generic), both data terms"""
    s, names = _scene(which)
    w, h = s.images[0].shape[1], s.images[0].shape[0]
    assert sorted(names) == sorted(["all_black", "spiral", "frame_island", "serpentine", "diagonal", "checker", "corners", "tile_rims"])
    if which == "hostile_fast":
        # more than 17 steps = a second batch of 16 behind the first step and the first batch: counted on the CPU, by the numpy flood
        assert U.jacobi_flood_steps(s.images[names.index("spiral")], stop_after=17)[1] > 17
    _assert_erosion(s, names, w, h)
    assert not _ref(s.images[names.index("all_black")])["area"].any()
    isl = _ref(s.images[names.index("frame_island")])["area"]
    assert isl[h // 2, w // 2] and not isl[3, 3]
    for term in TERMS:
        _check(_fresh(s, term), s, term, names)


SMALL_SIZES = ((2, 2), (2, 5), (5, 2), (3, 3), (31, 3), (32, 2), (33, 4), (64, 3), (65, 66), (97, 67))
_NO_INTERIOR = {"frame1", "frame2", "blob_rim", "island"}
_WIDE = {"hline_break31", "hline_break32", "vline31", "vline32"}
SMALL_SKIPPED = {    # what each size cannot hold (tests/util_cases.py small_hostile_images says why)
    (2, 2): _NO_INTERIOR | _WIDE | {"hline"}, (2, 5): _NO_INTERIOR | _WIDE, (5, 2): _NO_INTERIOR | _WIDE | {"hline"},
    (3, 3): _WIDE | {"frame2"}, (31, 3): _WIDE | {"frame2"}, (32, 2): _NO_INTERIOR | _WIDE | {"hline"},
    (33, 4): {"frame2", "hline_break32", "vline32"}, (64, 3): {"frame2"}, (65, 66): set(), (97, 67): set(),
}


@pytest.mark.parametrize("size", SMALL_SIZES, ids=lambda s: "%dx%d" % s)
def test_small_patterns_every_bit(size):
    """borders, frames, lines across and along the 31 | 32 word boundary, rims at w - 2 / h - 2, an island: every pattern the size can hold,
    both data terms; 32 x 2 and 64 x 3 take the vectorised kernels, the others the generic ones"""
    w, h = size
    s, names = _scene("small_%dx%d" % size)
    assert set(U.SMALL_HOSTILE) - set(names) == SMALL_SKIPPED[size]
    _assert_erosion(s, names, w, h)
    for n in ("hline_break31", "hline_break32"):                       # nothing beyond the break is filled, everything before it is
        if n in names:
            m = _ref(s.images[names.index(n)])["area"]
            b = int(n[-2:])
            assert m[1, b:].all() and not m[1, :b].any()
    if "hline" in names and w > 64:
        assert U.jacobi_flood_steps(s.images[names.index("hline")])[1] >= (w + 31) // 32    # one word per step along row 1
    if "island" in names:
        assert _ref(s.images[names.index("island")])["area"].all()
    for term in TERMS:
        _check(_fresh(s, term), s, term, names)


# ---- e. the summary on the tile grid ----

@pytest.mark.parametrize("size", [(32, 32), (33, 33), (64, 64), (65, 65), (64, 33), (96, 97)], ids=lambda s: "%dx%d" % s)
def test_summary_on_the_tile_grid(size):
    """pixel column / row 32 t + 32 exists, does not exist, is exactly the last pixel -- under rims that end on columns and rows 31, 32, 33"""
    s, names = _scene("tiles_%dx%d" % size)
    sums = [_ref(i)["gmi_sum"] for i in s.images]
    if size[0] > 33 and size[1] > 33:
        assert any(t.any() and not t.all() for t in sums)              # both answers of a summary bit occur
    if size[0] >= 33:
        # a tile whose own 32 columns are valid in all its rows and whose bit is 0 all the same: the shared column 32 t + 32 decided it
        assert any(not _ref(i)["area_sum"][0, 0] and _ref(i)["area"][:33, :32].all() for i in s.images)
    if size[1] >= 33:                                                  # ... and the shared row
        assert any(not _ref(i)["area_sum"][0, 0] and _ref(i)["area"][:32, :33].all() for i in s.images)
    for term in TERMS:
        _check(_fresh(s, term), s, term, names)


# ---- f. the shortcuts ----

def test_no_black_corner_means_no_mask_at_all():
    """no view has a black corner pixel: the flood fill has no seed, every view drops its mask pointer -- black islands and black border pixels
    that are no corners included -- and the cull that consumes the decision gives the oracle's table"""
    s, names = _scene("no_seed")
    for term in TERMS:
        r = _fresh(s, term)
        assert not r.flags.any()
        _check(r, s, term, names)
        assert _table_equals_oracle(r, s, term).nnz > 0


def test_one_black_corner_among_five_views():
    s, names = _scene("one_seed")
    for term in TERMS:
        r = _fresh(s, term)
        assert r.flags.tolist() == [0, 0, 0, 1, 0]
        _check(r, s, term, names)
        bits = r.views[3].mask_bits()[0]
        assert not bits[47, 63] and bits.sum() == bits.size - 1       # a border pixel: erosion leaves the rest alone
        assert _table_equals_oracle(r, s, term).nnz > 0


def test_checker_keeps_its_mask_for_the_corner_pixels():
    s, names = _scene("checker")
    for term in TERMS:
        r = _fresh(s, term)
        assert r.flags.tolist() == [1, 1]
        _check(r, s, term, names)
        for p, img in zip(r.views, s.images):
            h, w = img.shape[:2]
            bits = p.mask_bits()[0]
            black = [(y, x) for y in (0, h - 1) for x in (0, w - 1) if img[y, x].sum() == 0]
            assert len(black) >= 2 and bits.sum() == bits.size - len(black) and not any(bits[y, x] for y, x in black)
        assert _table_equals_oracle(r, s, term).nnz > 0


# ---- g. stale state ----

def test_one_context_scene_after_scene():
    """scene A (gradient term), a smaller scene B (area term), A again, a scene without any seed, A again on ONE context: every read-back equals
    a fresh context's -- offsets recomputed, no reach bit carried over in the ping-pong buffers, any_seed / changed cleared"""
    seq = (("generic", "gmi"), ("small_b", "area"), ("generic", "gmi"), ("no_seed", "gmi"), ("generic", "area"), ("vector", "gmi"), ("small_b", "gmi"))
    fresh = {}
    c = M.Context(0)
    try:
        for name, term in seq:
            s, names = _scene(name)
            got = _pass(c, s, term)
            if (name, term) not in fresh:
                fresh[name, term] = _fresh(s, term)
            _same(got, fresh[name, term])
            _check(got, s, term, names)
    finally:
        c.close()


# ---- h. the entry point's contract ----

def test_entry_point_contract():
    s, _ = _scene("small_b")
    c = M.Context(0)
    try:
        L, n = c.L, C.c_uint64(0)
        call = lambda which, view, buf, cap: L.mvs_ctx_prep_products(c.h, which, view, buf, cap, C.byref(n))
        assert call(1, 0, None, 0) == MVS_ERR_STATE                    # no scene, no pass
        c.set_mesh(s.verts, s.faces, s.normals); c.set_views(s.cams, s.images)
        for which in range(4):
            assert call(which, 0, None, 0) == MVS_ERR_STATE            # a scene, no pass yet
        c.data_costs(M.Settings(data_term="area"))
        assert call(0, 0, None, 0) == MVS_ERR_STATE                    # the area term leaves no gradient image
        assert c.prep_products(0).gmi is None
        c.data_costs(M.Settings(data_term="gmi"))
        sizes = []
        for j, img in enumerate(s.images):
            h, w = img.shape[:2]
            wpr = (w + 31) // 32
            want = (w * h, 4 * h * wpr, 4 * ((h + 31) // 32) * 2 * ((wpr + 63) // 64), s.n_views)
            for which in range(4):
                assert call(which, j, None, 0) == 0 and n.value == want[which], (j, which, n.value)
                buf = np.full(want[which] + 8, 0xAB, np.uint8)
                assert call(which, j, buf.ctypes.data_as(C.c_void_p), want[which] - 1) == MVS_ERR_INVALID and (buf == 0xAB).all()
                assert call(which, j, buf.ctypes.data_as(C.c_void_p), want[which]) == 0 and (buf[want[which]:] == 0xAB).all()
            sizes.append(want)
        for which in range(3):
            assert call(which, s.n_views, None, 0) == MVS_ERR_INVALID
        assert call(3, 12345, None, 0) == 0 and n.value == s.n_views   # `view` is ignored for the flags
        assert call(4, 0, None, 0) == MVS_ERR_INVALID and call(-1, 0, None, 0) == MVS_ERR_INVALID
        c.set_views(s.cams, s.images)
        assert call(1, 0, None, 0) == MVS_ERR_STATE                    # new views, no pass over them yet
    finally:
        c.close()


def test_ranged_pass_is_served():
    """a pass that walks the faces in ranges prepares the views in its first range: the read-back is that of an unranged pass"""
    s0, names = _scene("one_seed")
    s = U.prep_scene(s0.images)
    s.faces = np.ascontiguousarray(np.repeat(s.faces, 4, axis=0)); s.normals = np.ascontiguousarray(np.repeat(s.normals, 4, axis=0))
    c = M.Context(0)
    try:
        c.set_option("dc_range_pairs", s.n_views)                      # one face x all views per range
        r = _pass(c, s, "gmi")
        assert c.dc_ranges()[0] == 4
    finally:
        c.close()
    _check(r, s, "gmi", names)
    _same(r, _fresh(s, "gmi"))
