"""View input on the GPU (DESIGN.md section 4 "View input"; csrc/k_jpegdec.hip): Context.decode_jpegs gives, byte for byte, what the host twin
of csrc/jpeg_dec.h gives (tests/test_jpeg_decode_host.py holds the twin to libjpeg-turbo and to a numpy statement, bit for bit) on the whole
Pillow-encoded set of tests/tools/jpeg_full_decode.py, in one call of many files and in calls of one file.

Self-synchronisation: the same check with option jpegdec_subseq_bytes at 16 and at 128 on a 64x64 noise image at quality 100 without
restart markers (more than 256 subsequences at 16 bytes: several windows, several launches; an FF 00 pair across a subsequence edge of the
raw data), a flat 256x256 image without restart markers (a periodic code stream, where a misaligned speculative decoder has the least reason
to fall into step: the result rests on the propagation rounds), a file whose restart segments are shorter than one subsequence, and a file
with a segment boundary inside a window.  Those conditions are computed from the file bytes, and the stats must agree.

Block edges: chroma planes that end 1, 7, 8 and 9 samples past a block and a 16-byte edge, widths with 3 W at every residue mod 16.

set_views_jpeg: the suite's small scene saved as JPEG gives the table and the labels of set_views on Pillow's decode of the same files, bit
for bit; set_views afterwards works as before; a size mismatch is refused and the context stays usable; a scratch cap that forces three
batches gives the same bytes; every refusal of the entropy data that the host cannot see arrives from the device with its reason."""
import re

import numpy as np
import pytest

import mvs_texturing_amd as M
import jpeg_full_decode as FD
from conftest import get_scene

pytestmark = pytest.mark.gpu

CASES = FD.pillow_cases()
NAMES = sorted(CASES)


@pytest.fixture(scope="module")
def ctx():
    c = M.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def twin():
    return {k: M.decode_jpeg(CASES[k]) for k in NAMES}


def _same(images, refs):
    assert len(images) == len(refs)
    for k, (a, b) in enumerate(zip(images, refs)):
        assert a.shape == b.shape and a.dtype == np.uint8, k
        assert np.array_equal(a, b), "image %d: %d bytes differ" % (k, int((a != b).sum()))


def test_all_files_in_one_call(ctx, twin):
    ctx.set_option("jpegdec_subseq_bytes", 128)
    images, st = ctx.decode_jpegs([CASES[k] for k in NAMES])
    _same(images, [twin[k] for k in NAMES])
    assert st["files"] == len(NAMES) and st["batches"] == 1 and st["file_bytes"] == sum(len(CASES[k]) for k in NAMES)
    parsed = [FD.decode(CASES[k]) for k in NAMES[::7]]
    _, st7 = ctx.decode_jpegs([CASES[k] for k in NAMES[::7]])
    assert st7["stuffed_bytes"] == sum(p["stuffed_bytes"] for p in parsed)
    assert st7["restart_segments"] == sum(p["segments"] for p in parsed)
    assert st7["blocks"] == sum(len(p["coefficients"]) for p in parsed)
    assert st7["entropy_bytes"] == sum(len(p["entropy"]) for p in parsed)


@pytest.mark.parametrize("name", NAMES[::5] + ["rst_blocks3_s2", "rst_rows1_s1", "gray_1x1", "gray_rst"])
def test_one_file_per_call(ctx, twin, name):
    ctx.set_option("jpegdec_subseq_bytes", 128)
    images, st = ctx.decode_jpegs([CASES[name]])
    _same(images, [twin[name]])
    assert st["files"] == 1


def test_on_device_output(ctx, twin):
    """the images left on the device: read through the deflate route, which takes device bytes and has a host twin"""
    names = NAMES[3::40]
    out, _ = ctx.decode_jpegs([CASES[k] for k in names], on_device=True)
    for k, (arr, h, w) in zip(names, out):
        assert (h, w, 3) == twin[k].shape and arr.shape == (h * w * 3,)
        assert ctx.deflate_rle(arr) == M.deflate_rle(twin[k].tobytes()), k


# ---- self-synchronisation ----
def _clean_segments(f):
    """the unstuffed restart segments of a file and its raw entropy bytes"""
    a, b = FD.entropy_range(f)
    raw = f[a:b]
    segs, cur, i = [], bytearray(), 0
    while i < len(raw):
        if raw[i] == 0xFF and raw[i + 1] == 0:
            cur.append(0xFF); i += 2
        elif raw[i] == 0xFF:
            segs.append(bytes(cur)); cur = bytearray(); i += 2
        else:
            cur.append(raw[i]); i += 1
    segs.append(bytes(cur))
    return segs, raw


def _subsequences(segs, S):
    return [max(1, -(-len(s) // S)) for s in segs]


@pytest.fixture(scope="module")
def sync_files():
    rs = np.random.RandomState(11)
    noise = rs.randint(0, 256, (64, 64, 3)).astype(np.uint8)
    out = {
        "noise": FD.pillow_file(noise, quality=100, subsampling=0),
        "flat": FD.pillow_file(np.full((256, 256, 3), (200, 30, 90), np.uint8), quality=90, subsampling=2),
        "short_segments": FD.pillow_file(FD.picture(48, 64), quality=90, subsampling=2, restart_marker_blocks=1),
        "boundary_in_window": FD.pillow_file(noise, quality=100, subsampling=0, restart_marker_rows=3),
    }
    return out


@pytest.mark.parametrize("S", (16, 128))
@pytest.mark.parametrize("name", ("noise", "flat", "short_segments", "boundary_in_window"))
def test_self_synchronisation(ctx, sync_files, name, S):
    f = sync_files[name]
    ref = M.decode_jpeg(f)
    assert np.array_equal(ref, FD.pillow_decode(f))
    segs, raw = _clean_segments(f)
    subs = _subsequences(segs, S)
    ctx.set_option("jpegdec_subseq_bytes", S)
    try:
        images, st = ctx.decode_jpegs([f])
    finally:
        ctx.set_option("jpegdec_subseq_bytes", 128)
    _same(images, [ref])
    assert st["subsequences"] == sum(subs) and st["restart_segments"] == len(segs)
    assert st["windows"] == -(-sum(subs) // 256)
    assert 1 <= st["sync_launches"] <= st["windows"] + 1 and 1 <= st["sync_rounds_max"] <= 256
    assert st["subseq_exact_after_pass1"] >= len(segs)          # a segment's first subsequence starts from the true state
    if name == "noise" and S == 16:
        assert len(segs) == 1 and sum(subs) > 256
        assert any(raw[i] == 0xFF and raw[i + 1] == 0 and (i + 1) % S == 0 for i in range(len(raw) - 1)), "no FF 00 pair across a subsequence edge"
        assert st["windows"] >= 2 and st["sync_launches"] >= 2 and st["stuffed_bytes"] > 0
    if name == "flat":
        assert len(segs) == 1 and sum(subs) >= (4 if S == 16 else 1)
    if name == "short_segments" and S == 128:
        assert len(segs) > 4 and max(len(s) for s in segs) < S and st["subsequences"] == len(segs)
        assert st["subseq_exact_after_pass1"] == len(segs) and st["sync_launches"] == 1
    if name == "boundary_in_window" and S == 16:
        starts = np.cumsum([0] + subs[:-1])
        assert st["windows"] >= 2 and any(s % 256 for s in starts[1:]), "no segment boundary inside a window"


def test_subsequence_option_is_checked(ctx):
    for bad in (12, 18, 132, 0):
        with pytest.raises(M.MvsError):
            ctx.set_option("jpegdec_subseq_bytes", bad)
    ctx.set_option("jpegdec_subseq_bytes", 128)


# ---- block edges ----
def test_block_and_store_edges(ctx):
    files = []
    for sub in (1, 2):
        for w in (33, 34, 45, 46, 47, 48, 49, 50):       # chroma planes of 17, 23, 24 and 25 samples across
            for h in (33, 46, 47, 50):                    # and (4:2:0) down
                files.append(FD.pillow_file(FD.picture(h, w, 20.0), quality=90, subsampling=sub))
    for sub in (0, 1, 2):
        for w in range(16, 32):                           # 3 W at every residue mod 16
            files.append(FD.pillow_file(FD.picture(9, w, 20.0), quality=90, subsampling=sub))
    assert {(3 * w) % 16 for w in range(16, 32)} == set(range(16))
    images, _ = ctx.decode_jpegs(files)
    refs = [M.decode_jpeg(f) for f in files]
    _same(images, refs)
    _same(refs, [FD.pillow_decode(f) for f in files])
    images, _ = ctx.decode_jpegs(files[::-1][5:])        # other offsets in the output, so other alignments of every image
    _same(images, refs[::-1][5:])


def test_idct_paths(ctx):
    f = FD.pillow_file(FD.idct_paths_image(), quality=100, subsampling=0)
    images, _ = ctx.decode_jpegs([f])
    _same(images, [M.decode_jpeg(f)])


# ---- refusals the host cannot see: they come from the device ----
@pytest.mark.parametrize("name", ("second_scan", "dnl", "marker_inside", "rst_swapped", "rst_removed", "rst_one_more", "invalid_code", "run_past_63", "dc_outside_int16",
                                  "segment_incomplete"))
def test_device_refusals(ctx, twin, name):
    f, why = FD.refusals()[name]
    good = CASES["35x50_s2_q90_o0_n40"]
    with pytest.raises(M.MvsError) as e:
        ctx.decode_jpegs([good, f])
    assert e.value.status == 1 and why in str(e.value) and "view 1" in str(e.value), str(e.value)
    assert e.value.stats["files"] == 2
    images, _ = ctx.decode_jpegs([good])
    _same(images, [twin["35x50_s2_q90_o0_n40"]])


def test_host_refusals_name_the_view(ctx):
    f, why = FD.refusals()["progressive"]
    with pytest.raises(M.MvsError) as e:
        ctx.decode_jpegs([CASES["8x8_s0_q90_o0_n0"], CASES["8x8_s1_q90_o0_n0"], f])
    assert why in str(e.value) and "view 2" in str(e.value)


# ---- batches ----
def _scratch_needs(ctx, files):
    needs = []
    for f in files:
        with pytest.raises(M.MvsError) as e:
            ctx.decode_jpegs([f], params=M.default_jpegdec_params(max_scratch_bytes=1))
        assert e.value.stats["files"] == 1 and e.value.stats["file_bytes"] == len(f)     # refused with the stats filled
        needs.append(int(re.search(r"needs (\d+) bytes of scratch", str(e.value)).group(1)))
    return needs


def _batches(needs, cap):
    n, total = 1, 0
    for v in needs:
        if total and total + v > cap:
            n += 1; total = 0
        total += v
    return n


def _cap_for(needs, batches):
    for cap in sorted({sum(needs[a:b]) for a in range(len(needs)) for b in range(a + 1, len(needs) + 1)}):
        if cap >= max(needs) and _batches(needs, cap) == batches:
            return cap
    raise AssertionError("no cap gives %d batches" % batches)


def test_three_batches(ctx, twin):
    names = NAMES[10:80:9]
    files = [CASES[k] for k in names]
    cap = _cap_for(_scratch_needs(ctx, files), 3)
    images, st = ctx.decode_jpegs(files, params=M.default_jpegdec_params(max_scratch_bytes=cap))
    assert st["batches"] == 3
    _same(images, [twin[k] for k in names])


# ---- set_views_jpeg ----
@pytest.fixture(scope="module")
def jpeg_scene():
    s = get_scene("tiny")
    files = [FD.pillow_file(img, quality=90, subsampling=2) for img in s.images]
    return s, files, [FD.pillow_decode(f) for f in files]


def _table_and_labels(c, s):
    c.data_costs(M.Settings())
    t = c.costs_download()
    labels, _ = c.view_selection(s.adj_ptr, s.adj)
    return t, labels


def _same_result(a, b):
    (ta, la), (tb, lb) = a, b
    assert np.array_equal(ta.col_ptr, tb.col_ptr) and np.array_equal(ta.view_id, tb.view_id)
    assert np.array_equal(ta.cost.view(np.uint32), tb.cost.view(np.uint32))
    assert np.array_equal(la, lb)


@pytest.fixture(scope="module")
def pillow_route(jpeg_scene):
    s, files, pixels = jpeg_scene
    c = M.Context(0)
    c.set_mesh(s.verts, s.faces, s.normals); c.set_views(s.cams, pixels)
    r = _table_and_labels(c, s)
    c.set_views(s.cams, s.images)
    r2 = _table_and_labels(c, s)
    c.close()
    return r, r2


def test_set_views_jpeg(jpeg_scene, pillow_route):
    s, files, pixels = jpeg_scene
    c = M.Context(0)
    try:
        c.set_mesh(s.verts, s.faces, s.normals)
        st = c.set_views_jpeg(s.cams, files)
        assert st["files"] == s.n_views and st["batches"] == 1
        _same_result(_table_and_labels(c, s), pillow_route[0])
        # a second scene through set_views works as before
        c.set_views(s.cams, s.images)
        _same_result(_table_and_labels(c, s), pillow_route[1])
        # a size mismatch between a file and its view is refused; the context stays usable
        cams = {k: np.array(v).copy() for k, v in s.cams.items()}
        cams["width"][3] += 1
        with pytest.raises(M.MvsError) as e:
            c.set_views_jpeg(cams, files)
        assert e.value.status == 1 and "view 3" in str(e.value) and "320 x 240" in str(e.value) and "321 x 240" in str(e.value)
        # three batches: the same bytes, so the same table
        cap = _cap_for(_scratch_needs(c, files), 3)
        st = c.set_views_jpeg(s.cams, files, params=M.default_jpegdec_params(max_scratch_bytes=cap))
        assert st["batches"] == 3
        _same_result(_table_and_labels(c, s), pillow_route[0])
        # views that bring pixels beside views that bring files
        mixed = [None if j % 3 == 0 else f for j, f in enumerate(files)]
        c.set_views_jpeg(s.cams, mixed, images=pixels)
        _same_result(_table_and_labels(c, s), pillow_route[0])
        # a corrupt file among the views
        bad = list(files); bad[5] = files[5][:-2]
        with pytest.raises(M.MvsError) as e:
            c.set_views_jpeg(s.cams, bad)
        assert "view 5" in str(e.value) and "no EOI" in str(e.value)
        c.set_views_jpeg(s.cams, files)
        _same_result(_table_and_labels(c, s), pillow_route[0])
    finally:
        c.close()
