"""csrc/jpeg_base.h on the host (DESIGN.md section 4 "Model output" item 9): tests/cpp/test_jpeg.cpp -- a stand-alone program with its own
main -- is compiled against it with the address and undefined-behaviour sanitizers and run on the crafted images of
tests/tools/jpeg_decode.py, both subsamplings, qualities 1, 50, 90 and 100.  Inside it asserts on the tables (prefix codes with the DHT's
counts, the quantiser rule's end points, the colour transform's range, bit placement) and on the refusals.  Every file it writes must pass
the strict parser, carry the coefficients of the numpy statement one for one, and open in Pillow at the true size; the DQT must be the
table Pillow's own encoder writes at every quality 1 .. 100 and the DHT the tables of a Pillow file written with optimize=False.

Fidelity and size are measured against Pillow's file of the same image, quality and subsampling (optimize=False: the same tables, so only
the transform's rounding, the chroma filter and the restart markers differ).  Measured over the crafted set (96 files):
  PSNR of Pillow's decode against the input, Pillow's file minus the twin's: -0.35 .. +1.143 dB (the largest on the 8 x 8 noise image
  `ends_stuffed` at quality 100, 4:4:4: 49.69 against 50.84 dB, where the transform's rounding is all the error there is); asserted with
  twice that, 2.286 dB.
  bytes, twin / Pillow: 0.9901 (photo_256, 4:2:0, quality 100) .. 1.1146 (photo_256, 4:4:4, quality 1: 128 restart segments of 8 flat
  MCUs pay 2 marker bytes and the padding each); asserted with the range widened by a tenth of its width on either side."""
import io
import os
import subprocess

import numpy as np
import pytest
from PIL import Image

from conftest import ROOT
import jpeg_decode as JD

CSRC = os.path.join(ROOT, "mvs-texturing_amd", "csrc")
IMAGES = JD.images()
QUALITIES = (1, 50, 90, 100)
CASES = [(n, s, q) for n in sorted(IMAGES) for s in (0, 1) for q in QUALITIES]
SHORTFALL_DB = 2 * 1.143
RATIO_LO, RATIO_HI = 0.9901 - 0.1 * (1.1146 - 0.9901), 1.1146 + 0.1 * (1.1146 - 0.9901)


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    d = tmp_path_factory.mktemp("jpeg")
    exe = str(d / "test_jpeg")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + CSRC, os.path.join(ROOT, "tests", "cpp", "test_jpeg.cpp"), "-o", exe])
    with open(str(d / "manifest"), "w") as f:
        for k, v in IMAGES.items():
            (d / (k + ".rgb")).write_bytes(v.tobytes())
            f.write("image %s %d %d\n" % (k, v.shape[1], v.shape[0]))
    r = subprocess.run([exe, str(d)], capture_output=True, text=True)
    return d, r


@pytest.fixture(scope="module")
def files(run):
    d, r = run
    assert r.returncode == 0, r.stdout + r.stderr
    return {(n, s, q): (d / ("%s_s%d_q%d.jpg" % (n, s, q))).read_bytes() for n, s, q in CASES}


@pytest.fixture(scope="module")
def parsed(files):
    return {k: JD.parse(v) for k, v in files.items()}


def _pillow_file(img, quality, sub):
    b = io.BytesIO()
    Image.fromarray(img).save(b, "JPEG", quality=quality, subsampling=2 if sub else 0, optimize=False)
    return b.getvalue()


def _pillow_tables(data):
    """the DQT (zig-zag order as in the file) and DHT segments of a JPEG file that Pillow wrote, read marker by marker"""
    dqt, dht, i = {}, {}, 2
    while data[i + 1] != 0xDA:
        assert data[i] == 0xFF
        m, n = data[i + 1], data[i + 2] << 8 | data[i + 3]
        s, j = data[i + 4:i + 2 + n], 0
        while m == 0xDB and j < len(s):
            dqt[s[j] & 15] = list(s[j + 1:j + 65]); j += 65
        while m == 0xC4 and j < len(s):
            bits = list(s[j + 1:j + 17])
            dht[(s[j] >> 4, s[j] & 15)] = (bits, list(s[j + 17:j + 17 + sum(bits)])); j += 17 + sum(bits)
        i += 2 + n
    return dqt, dht


def _decode(data):
    im = Image.open(io.BytesIO(data))
    im.load()
    return im


def test_tables_arithmetic_and_refusals_under_sanitizers(run):
    _, r = run
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


@pytest.mark.parametrize("name", sorted(IMAGES))
def test_files_parse_strictly_and_carry_the_numpy_coefficients(parsed, name):
    img = IMAGES[name]
    for sub in (0, 1):
        for q in QUALITIES:
            P = parsed[(name, sub, q)]
            assert (P["width"], P["height"], P["subsampling"]) == (img.shape[1], img.shape[0], sub)
            for t in (0, 1):
                assert np.array_equal(P["quant"][t], JD.quant_tables(q)[t]), (sub, q, t)
            want = JD.coefficients(img, q, sub)
            assert P["coefficients"].shape == want.shape and np.array_equal(P["coefficients"], want), (sub, q)


@pytest.mark.parametrize("name", sorted(IMAGES))
def test_pillow_decodes_to_the_true_size(files, name):
    for sub in (0, 1):
        for q in QUALITIES:
            im = _decode(files[(name, sub, q)])
            assert im.format == "JPEG" and im.mode == "RGB" and im.size == IMAGES[name].shape[1::-1]


def test_dqt_is_pillows_at_every_quality():
    """mvs_encode_jpeg of the product library where it is built, the numpy rule otherwise: both against Image.quantization of a file
    Pillow's encoder wrote at the same quality (Pillow hands the tables out in natural order; the file holds them in zig-zag order)"""
    img = IMAGES["side_8"]
    for q in range(1, 101):
        data = _pillow_file(img, q, 0)
        quant = Image.open(io.BytesIO(data)).quantization
        dqt, _ = _pillow_tables(data)
        ours = JD.quant_tables(q)
        for t in (0, 1):
            assert list(quant[t]) == ours[t].tolist(), (q, t)
            assert dqt[t] == ours[t][JD.ZIGZAG].tolist(), (q, t)


def test_twin_dqt_at_every_quality():
    import mvs_texturing_amd as M
    if not os.path.exists(M.lib_path()):
        pytest.skip("HIP library not built (run __graft_entry__.build())")
    img = IMAGES["side_8"]
    for q in range(1, 101):
        dqt, _ = _pillow_tables(_pillow_file(img, q, 1))
        z = M.encode_jpeg(img, q, 1)
        assert z[20:25] == b"\xff\xdb\x00\x43\x00" and list(z[25:89]) == dqt[0] and z[89:94] == b"\xff\xdb\x00\x43\x01" and list(z[94:158]) == dqt[1], q
        assert list(Image.open(io.BytesIO(z)).quantization[0]) == list(Image.open(io.BytesIO(_pillow_file(img, q, 1))).quantization[0])


def test_dht_is_pillows_unoptimised_set(parsed):
    _, dht = _pillow_tables(_pillow_file(IMAGES["photo_256"], 90, 1))
    assert sorted(dht) == [(0, 0), (0, 1), (1, 0), (1, 1)]
    for key in CASES[::7]:
        assert parsed[key]["dht"] == dht, key


def test_fidelity_against_pillows_own_file(files):
    worst = -99.0
    for name, sub, q in CASES:
        img = IMAGES[name]
        mine = JD.psnr(np.asarray(_decode(files[(name, sub, q)])), img)
        ref = JD.psnr(np.asarray(_decode(_pillow_file(img, q, sub))), img)
        worst = max(worst, ref - mine)
        print("%s 4:%s q%d: %.3f dB, Pillow's file %.3f dB" % (name, "2:0" if sub else "4:4", q, mine, ref))
        assert ref - mine <= SHORTFALL_DB, (name, sub, q, mine, ref)
    print("largest shortfall %.3f dB" % worst)


def test_sizes_against_pillows_own_file(files):
    lo, hi = 9.0, 0.0
    for name, sub, q in CASES:
        ratio = len(files[(name, sub, q)]) / len(_pillow_file(IMAGES[name], q, sub))
        lo, hi = min(lo, ratio), max(hi, ratio)
        print("%s 4:%s q%d: %d bytes, %.4f of Pillow's" % (name, "2:0" if sub else "4:4", q, len(files[(name, sub, q)]), ratio))
        assert RATIO_LO <= ratio <= RATIO_HI, (name, sub, q, ratio)
    print("ratios %.4f .. %.4f" % (lo, hi))


def test_the_crafted_images_reach_the_cases_they_were_made_for(parsed):
    seg = lambda n, s: parsed[(n, s, 90)]["segments"]
    assert [seg("mcus444_%d" % m, 0) for m in (JD.R - 1, JD.R, JD.R + 1)] == [1, 1, 2]
    assert [seg("mcus420_%d" % m, 1) for m in (JD.R - 1, JD.R, JD.R + 1)] == [1, 1, 2]
    assert seg("straddle_77x43", 1) == 2 and seg("straddle_77x43", 0) == 8          # 5 and 10 MCUs per row: no multiple of R
    assert seg("wrap_203x171", 1) == 18 and seg("wrap_203x171", 0) == 72           # RST0 .. RST7 more than twice over
    for s in (0, 1):
        flat = parsed[("flat_24", s, 90)]
        assert np.count_nonzero(flat["coefficients"][:, 1:]) == 0 and flat["eob"] == len(flat["coefficients"]) and flat["zrl"] == 0
        assert parsed[("zrl_one", s, 50)]["zrl"] == 4 and parsed[("zrl_two", s, 50)]["zrl"] == 8
        c = parsed[("zrl_two", s, 50)]["coefficients"][0]
        assert np.nonzero(c)[0].tolist() == [40]
    assert parsed[("ends_stuffed", 0, 100)]["segments_ending_stuffed"] == 1
    big = parsed[("checker_grey", 0, 100)]["coefficients"]
    assert np.abs(big[:, 1:]).max() >= 512 and np.abs(parsed[("noise_40x24", 0, 100)]["coefficients"][:, 1:]).max() >= 128   # categories 10 and 8
    assert parsed[("checker_colour", 0, 100)]["stuffed_bytes"] >= 50 and parsed[("noise_40x24", 0, 100)]["stuffed_bytes"] >= 1


def test_the_parser_refuses_what_it_should(files):
    good = files[("wrap_203x171", 1, 90)]
    JD.parse(good)
    at = JD.HEADER_BYTES
    rst = good.index(b"\xff\xd0", at)
    bad = [good[:rst + 1] + b"\xd1" + good[rst + 2:],                 # RST1 where RST0 is due
           good[:rst] + good[rst + 2:],                               # a marker missing
           good[:at + 5] + b"\xff\xc4" + good[at + 7:],               # a marker inside the entropy data
           good[:-2],                                                 # no EOI
           good[:20] + good[25:]]                                     # a segment out of place
    ff = good.index(b"\xff\x00", at)
    bad.append(good[:ff + 1] + good[ff + 2:])                         # an unstuffed 0xFF
    for b in bad:
        with pytest.raises(JD.BadJpeg):
            JD.parse(b)


def test_the_product_and_the_program_compile_the_same_definition(files):
    """mvs_encode_jpeg of the product library gives the stand-alone program's bytes on every case, and refuses what it refuses"""
    import mvs_texturing_amd as M
    if not os.path.exists(M.lib_path()):
        pytest.skip("HIP library not built (run __graft_entry__.build())")
    for name, sub, q in CASES:
        assert M.encode_jpeg(IMAGES[name], q, sub) == files[(name, sub, q)], (name, sub, q)
    px = np.zeros((1, 1, 3), np.uint8)
    for img, q, s, status in ((np.zeros((0, 4, 3), np.uint8), 90, 1, 1), (px, 0, 1, 1), (px, 101, 1, 1), (px, 90, 2, 1), (px, 90, -1, 1),
                              (np.zeros((1, 65536, 3), np.uint8), 90, 1, 7), (np.zeros((65536, 1, 3), np.uint8), 90, 0, 7)):
        with pytest.raises(M.MvsError) as e:
            M.encode_jpeg(img, q, s)
        assert e.value.status == status, (img.shape, q, s)
    assert JD.parse(M.encode_jpeg(px, 90, 1))["coefficients"].shape == (6, 64)
