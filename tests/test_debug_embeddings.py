"""Row f10 without a GPU: the debug embedding (DESIGN.md section 4 "Debug model").  tests/tools/debug_model.py -- a numpy restatement
of the rule -- equals, byte for byte, the images upstream's own generate_debug_embeddings.cpp produced (tests/golden/
debug_embedding_pins.npz); the host side of csrc/debug_embed.h, compiled with g++, equals the restatement on every pin, for every id
on a 40 x 13 image and for every position on 1 x 1; the colour table has the properties the definition relies on; and
mvs_debug_view_style is that table."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import debug_model as DM
import mvs_texturing_amd as M
from conftest import ROOT

PIN_SHAPES = [(13, 6), (14, 7), (16, 7), (26, 12), (27, 13), (29, 12), (40, 20), (133, 61)]
PIN_IDS = [0, 7, 10, 42, 99, 100, 105, 999]


def pins():
    z = np.load(os.path.join(ROOT, "tests", "golden", "debug_embedding_pins.npz"))
    views = [dict(position=int(z["position"][k]), id=int(z["view_id"][k]), w=int(z["width"][k]), h=int(z["height"][k]), image=z["image_%02d" % k])
             for k in range(len(z["position"]))]
    return z["colors"], views


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("debug_embed") / "libdebug_embed_host.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC",
                           "-I" + os.path.join(ROOT, "mvs-texturing_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "debug_embed_host.cpp"), "-o", so])
    L = C.CDLL(so)
    L.dbg_table.argtypes = [C.c_void_p] * 3; L.dbg_table.restype = None
    L.dbg_image.argtypes = [C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_void_p]; L.dbg_image.restype = None
    L.dbg_pixel.argtypes = [C.c_int] * 4 + [C.c_uint32]
    return L


def _host_image(L, w, h, view_id, position):
    out = np.zeros((h, w, 3), np.uint8)
    L.dbg_image(w, h, view_id, position, out.ctypes.data)
    return out


def test_pins_hold_what_the_issue_asks_for():
    colors, views = pins()
    assert colors.shape == (150, 3) and colors.dtype == np.uint8
    first = views[:8]
    assert [(v["w"], v["h"]) for v in first] == PIN_SHAPES and [v["id"] for v in first] == PIN_IDS
    assert all(v["position"] != v["id"] for v in views)
    assert {d for v in views for d in "%03d" % v["id"]} == set("0123456789")          # every glyph is pinned
    assert any(v["position"] >= 144 for v in views)


def test_restatement_equals_upstreams_images():
    colors, views = pins()
    for i in range(150):                                                              # the 144 colours and the wrap
        assert np.array_equal(DM.image(1, 1, i, i)[0, 0], colors[i]), i
    assert np.array_equal(colors[144:], colors[:6])
    for v in views:
        assert np.array_equal(DM.image(v["w"], v["h"], v["id"], v["position"]), v["image"]), v["position"]
    assert not DM.stamp(13, 6, 888).any() and not DM.stamp(14, 6, 888).any() and not DM.stamp(13, 7, 888).any()   # no cell fits
    assert DM.stamp(14, 7, 888).sum() == 3 * int(DM.GLYPH[8].sum())


def test_header_equals_the_restatement(host):
    colors, views = pins()
    for v in views:
        got = _host_image(host, v["w"], v["h"], v["id"], v["position"])
        assert np.array_equal(got, v["image"]) and np.array_equal(got, DM.image(v["w"], v["h"], v["id"], v["position"])), v["position"]
    for view_id in range(1000):                                                        # every id: 3 x 2 cells, the gaps and the rest right and below
        assert np.array_equal(_host_image(host, 40, 13, view_id, 5), DM.image(40, 13, view_id, 5)), view_id
    for position in range(288):                                                        # every colour, twice
        assert np.array_equal(_host_image(host, 1, 1, 0, position), DM.image(1, 1, 0, position)), position
    on = DM.stamp(40, 13, 427)
    assert all(bool(host.dbg_pixel(x, y, 40, 13, 427)) == bool(on[y, x]) for y in range(13) for x in range(40))


def test_colour_table(host):
    cols, prod, byts = DM.colour_table()
    style = np.zeros(144, np.uint32); lum = np.zeros(144, np.float32); hp = np.zeros((144, 3), np.float32)
    host.dbg_table(style.ctypes.data, lum.ctypes.data, hp.ctypes.data)
    assert np.array_equal(hp.view(np.uint32), prod.view(np.uint32))                    # the same fp32 values, not just the same bytes
    assert np.array_equal(np.stack([(style >> s) & 255 for s in (0, 8, 16)], 1).astype(np.uint8), byts)
    assert np.array_equal(lum.view(np.uint32), DM.luminance(cols).view(np.uint32))
    assert np.array_equal((style >> 24).astype(np.uint8), np.where(lum > 0.5, 0, 255).astype(np.uint8))
    # the stated order: saturation outermost, then value, hue innermost -- as HSV of the float colours
    mx, mn = cols.max(1), cols.min(1)
    want_v = np.repeat(np.tile(np.array([1.0, 0.7, 0.4, 0.1]), 3), 12)
    want_s = np.repeat(np.array([1.0, 0.6, 0.2]), 48)
    assert np.allclose(mx, want_v, atol=1e-6) and np.allclose((mx - mn) / mx, want_s, atol=1e-6)
    assert byts[0].tolist() == [255, 0, 0] and byts[4].tolist() == [0, 255, 0] and byts[8].tolist() == [0, 0, 255]
    hue_order = [tuple(np.argsort(-cols[i], kind="stable")[:1]) for i in (0, 4, 8)]
    assert hue_order == [(0,), (1,), (2,)]
    # luminance decides nothing: no colour is near the threshold
    margin = float(np.abs(DM.luminance(cols).astype(np.float64) - 0.5).min())
    print("smallest |luminance - 0.5| = %.6f" % margin)
    assert margin > 1e-3
    # channels that sit just below an integer before the truncation: what makes the host-built table necessary
    frac = prod.astype(np.float64) - np.floor(prod.astype(np.float64))
    risky = (frac > 1.0 - 1e-3)
    print("channels within 1e-3 below an integer: %d, in %d colours" % (int(risky.sum()), int(risky.any(1).sum())))
    assert risky.sum() > 0
    assert not np.array_equal(np.rint(prod).astype(np.uint8), byts)                    # rounding instead of truncating changes bytes


def test_debug_view_style_is_the_table():
    assert "mvs_debug_view_style" in M.load_library()._declared
    for position in list(range(288)) + [1000, 2 ** 32 - 1]:
        bg, fg = M.debug_view_style(position)
        wbg, wfg = DM.view_style(position)
        assert bg == tuple(int(x) for x in wbg) and fg == tuple(int(x) for x in wfg), position
