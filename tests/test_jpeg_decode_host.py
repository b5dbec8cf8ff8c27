"""csrc/jpeg_dec.h on the host (DESIGN.md section 4 "View input"): the twin M.decode_jpeg against libjpeg-turbo (Pillow's decode) and
against the numpy statement tests/tools/jpeg_full_decode.py, bit for bit, on Pillow-encoded files -- sizes 1x1, 7x5, 8x8, 9x130, 16x16,
17x33, 35x50 and 64x48, each with subsampling 0 / 1 / 2, quality 30 / 90 / 100, optimize off / on, smooth content and smooth content plus
noise of sigma 40; restart_marker_blocks=3 and restart_marker_rows=1; grayscale -- and on the library's own files (M.encode_jpeg, 4:4:4 and
4:2:0, DRI 8), whose coefficients as the strict parser tests/tools/jpeg_decode.py finds them must be the ones the twin decoded.

Every refusal of the format comes from a file made by Pillow or by byte surgery on a good file, and must carry its reason in the message.

tests/cpp/test_jpeg_dec.cpp -- a stand-alone program with its own main -- runs the parser and the twin under the address and
undefined-behaviour sanitizers on the good files, the refusal files and every prefix of a good file."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import mvs_texturing_amd as M
import jpeg_decode as JD
import jpeg_full_decode as FD

CSRC = os.path.join(ROOT, "mvs-texturing_amd", "csrc")
CASES = FD.pillow_cases()
REFUSALS = FD.refusals()


@pytest.fixture(scope="module")
def decoded():
    return {k: M.decode_jpeg(f, coefficients=True) for k, f in CASES.items()}


@pytest.mark.parametrize("name", sorted(CASES))
def test_twin_equals_libjpeg_and_numpy(decoded, name):
    img, coef = decoded[name]
    ref = FD.pillow_decode(CASES[name])
    assert img.shape == ref.shape and img.dtype == np.uint8
    assert np.array_equal(img, ref), "twin differs from libjpeg-turbo on %d bytes" % int((img != ref).sum())
    st = FD.decode(CASES[name])
    assert np.array_equal(st["coefficients"], coef)
    assert np.array_equal(st["rgb"], img)


def test_case_set_is_the_one_stated():
    names = set(CASES)
    for (h, w) in FD.SIZES:
        for sub in (0, 1, 2):
            for q in (30, 90, 100):
                for opt in (0, 1):
                    for noise in (0, 40):
                        assert "%dx%d_s%d_q%d_o%d_n%d" % (w, h, sub, q, opt, noise) in names
    assert {(w, h) for (h, w) in FD.SIZES} == {(1, 1), (7, 5), (8, 8), (9, 130), (16, 16), (17, 33), (35, 50), (64, 48)}
    samplings = {FD.decode(CASES["64x48_s%d_q90_o0_n0" % s])["sampling"] for s in (0, 1, 2)}
    assert samplings == {(1, 1), (2, 1), (2, 2)}
    assert FD.decode(CASES["rst_blocks3_s2"])["restart_interval"] == 3 and FD.decode(CASES["rst_rows1_s2"])["segments"] == 3
    assert FD.decode(CASES["gray_17x33"])["components"] == 1


@pytest.mark.parametrize("sub", (0, 1))
@pytest.mark.parametrize("name", ("side_1", "side_17", "straddle_77x43", "noise_40x24", "zrl_two", "ends_stuffed"))
def test_own_files(name, sub):
    """the library's own encoder's files: the pixels are libjpeg's, the coefficients the strict parser's"""
    f = M.encode_jpeg(JD.images()[name], 100 if name == "ends_stuffed" else 90, sub)
    img, coef = M.decode_jpeg(f, coefficients=True)
    assert np.array_equal(img, FD.pillow_decode(f))
    p = JD.parse(f)
    assert p["restart_interval"] == 8
    nat = np.zeros_like(p["coefficients"]); nat[:, JD.ZIGZAG] = p["coefficients"]
    assert np.array_equal(nat, coef)
    assert np.array_equal(FD.decode(f)["rgb"], img)


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refusals(name):
    f, why = REFUSALS[name]
    with pytest.raises(M.MvsError) as e:
        M.decode_jpeg(f)
    assert e.value.status == 1 and why in str(e.value), str(e.value)
    assert M.jpeg_probe(f) is None or name in ("second_scan", "dnl", "marker_inside", "rst_swapped", "rst_removed", "rst_one_more", "invalid_code", "run_past_63",
                                               "dc_outside_int16", "segment_incomplete")   # (the probe reads the headers only)


def test_refusal_set_covers_the_format():
    for k in ("progressive", "cmyk", "precision_12", "dht_removed", "cut_tail", "rst_swapped", "adobe_rgb", "invalid_code", "sampling_440", "second_scan", "dnl",
              "dht_overfull", "no_eoi", "run_past_63", "dc_outside_int16", "segment_incomplete"):
        assert k in REFUSALS


def test_probe_and_trailing_bits():
    f = CASES["35x50_s2_q90_o0_n40"]
    assert M.jpeg_probe(f) == (35, 50)
    # bits behind a segment's last block are ignored, as libjpeg ignores them
    longer = f[:-2] + b"\x12\x34" + f[-2:]
    assert np.array_equal(M.decode_jpeg(longer), M.decode_jpeg(f))


def test_idct_32_and_64_bit_paths_agree_with_the_statement():
    """black and white noise at quality 100: blocks above the 32-bit bound (jpeg_dec.h IDCT_FITS32) beside smooth blocks below it"""
    f = FD.pillow_file(FD.idct_paths_image(), quality=100, subsampling=0)
    st = FD.decode(f)
    q = 1   # quality 100: every quantiser is 1
    sums = np.abs(st["coefficients"] * q).sum(axis=1)
    assert (sums > 5400).any() and (sums <= 5400).any()
    assert np.array_equal(M.decode_jpeg(f), st["rgb"]) and np.array_equal(st["rgb"], FD.pillow_decode(f))


def test_sanitized_program(tmp_path):
    exe = str(tmp_path / "test_jpeg_dec")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + CSRC, os.path.join(ROOT, "tests", "cpp", "test_jpeg_dec.cpp"), "-o", exe])
    good = ["35x50_s2_q90_o0_n40", "9x130_s1_q100_o1_n40", "1x1_s2_q30_o0_n0", "64x48_s0_q90_o1_n0", "rst_blocks3_s2", "rst_rows1_s1", "gray_17x33", "gray_rst"]
    with open(str(tmp_path / "manifest"), "w") as m:
        for k in good:
            (tmp_path / (k + ".jpg")).write_bytes(CASES[k]); m.write("good %s\n" % k)
        for k, (f, why) in sorted(REFUSALS.items()):
            (tmp_path / (k + ".jpg")).write_bytes(f); m.write("bad %s %s\n" % (k, why))
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "failures 0" in r.stdout
    for k in good:
        ref = FD.pillow_decode(CASES[k])
        assert (tmp_path / (k + ".rgb")).read_bytes() == ref.tobytes()
