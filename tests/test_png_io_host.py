"""csrc/png_io.h and csrc/fmt6.h are plain host C++: tests/cpp/test_png_fmt.cpp -- a stand-alone program with its own main -- is compiled
against them with the address and undefined-behaviour sanitizers and run.  It checks fmt6.h against snprintf on the float grid (DESIGN.md
section 4 "Model output" item 2) and writes PNGs of 1 x 1, 3 x 5, 256 x 256 and 300 x 100 (rows crossing a 65535-byte stored block) at
level 0 and, where libz.so.1 resolves, level 1; they are decoded here with struct + zlib (every chunk CRC, the Adler-32 sum) and with PIL
where it imports, and must hold the pattern's pixels."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import obj_model as OM

CSRC = os.path.join(ROOT, "mvs-texturing_amd", "csrc")
SIZES = ((1, 1), (3, 5), (256, 256), (300, 100))


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    d = tmp_path_factory.mktemp("png")
    exe = str(d / "test_png_fmt")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + CSRC, os.path.join(ROOT, "tests", "cpp", "test_png_fmt.cpp"), "-o", exe, "-ldl"])
    r = subprocess.run([exe, str(d)], capture_output=True, text=True)
    return d, r


def pattern(w, h):
    y, x, c = np.meshgrid(np.arange(h), np.arange(w), np.arange(3), indexing="ij")
    return ((7 * x + 13 * y + 29 * c + x * y) & 255).astype(np.uint8)


def test_formatting_and_encoder_under_sanitizers(run):
    _, r = run
    assert r.returncode == 0 and r.stdout.strip() in ("ok zlib=0", "ok zlib=1"), r.stdout + r.stderr


def _check_file(path, w, h, level):
    data = open(path, "rb").read()
    img, chunks = OM.decode_png(data)
    assert chunks == [b"IHDR", b"IDAT", b"IEND"]
    assert img.shape == (h, w, 3) and np.array_equal(img, pattern(w, h))
    if level == 0:
        raw = h * (3 * w + 1)
        assert len(data) == 8 + 25 + 12 + 12 + 2 + raw + 5 * ((raw + 65534) // 65535) + 4       # signature, IHDR, IDAT and IEND frames, zlib header, stored blocks, Adler-32
    try:
        from PIL import Image
    except ImportError:
        return
    with Image.open(path) as im:
        assert im.mode == "RGB" and np.array_equal(np.asarray(im), pattern(w, h))


@pytest.mark.parametrize("w,h", SIZES)
def test_stored_pngs_decode_to_the_pattern(run, w, h):
    d, r = run
    assert r.returncode == 0, r.stdout + r.stderr
    _check_file(str(d / ("%dx%d_l0.png" % (w, h))), w, h, 0)


@pytest.mark.parametrize("w,h", SIZES)
def test_compressed_pngs_decode_to_the_pattern(run, w, h):
    d, r = run
    assert r.returncode == 0, r.stdout + r.stderr
    if r.stdout.strip() != "ok zlib=1":
        pytest.skip("libz.so.1 does not resolve on this machine")
    _check_file(str(d / ("%dx%d_l1.png" % (w, h))), w, h, 1)
    if w * h > 100:
        assert os.path.getsize(str(d / ("%dx%d_l1.png" % (w, h)))) < os.path.getsize(str(d / ("%dx%d_l0.png" % (w, h))))


def test_a_stored_block_boundary_falls_inside_a_row():
    """the case the 300 x 100 image is there for"""
    row = 3 * 300 + 1
    assert row * 100 > 65535 and 65535 % row != 0


def test_headers_have_no_device_code():
    """they are included by the stand-alone program above as they are: png_io.h has no HIP in it, fmt6.h only behind its own macro"""
    text = open(os.path.join(CSRC, "png_io.h")).read()
    assert "hip/" not in text and "__global__" not in text and "__device__" not in text
    text = open(os.path.join(CSRC, "fmt6.h")).read()
    assert "hip/" not in text and "__global__" not in text
