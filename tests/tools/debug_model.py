"""numpy restatement of the debug embedding (DESIGN.md section 4 "Debug model"; csrc/debug_embed.h): the 144 colours in fp32 and in
upstream's operation order, the font colour, and the stamp of three-digit ids in cells of 13 x 6 pixels -- written from the
definition, with loops over cells and a glyph table of its own, so that it shares nothing with the header but the rule.  Held to
upstream's recorded images by tests/test_debug_embeddings.py; the GPU tests compare the device against it."""
import numpy as np

F = np.float32
N_COLOURS = 144
MAX_ID = 999
# the ten 3 x 5 glyphs, digit d in columns 4 d .. 4 d + 2
_ART = (".#. .#. ##. ##. #.. ### .#. ### .#. .#.",
        "#.# ##. ..# ..# #.# #.. #.. ..# #.# #.#",
        "#.# .#. .#. .#. ### ##. ##. ..# .#. .##",
        "#.# .#. #.. ..# ..# ..# #.# .#. #.# ..#",
        ".#. ### ### ##. ..# ##. .#. .#. .#. .#.")
GLYPH = np.array([[[_ART[r][4 * d + c] == "#" for c in range(3)] for r in range(5)] for d in range(10)])   # [digit][row][column]


def colour_table():
    """(colours (144, 3) float32, products (144, 3) float32 = colour * 255.0f, bytes (144, 3) uint8 = the truncated products): saturation
    outermost (1, 0.6, 0.2), then value (1, 0.7, 0.4, 0.1), hue innermost (0 .. 330 in steps of 30); the steps are DOUBLE subtractions
    rounded back to float (`s -= 0.4`, `v -= 0.3`), which is where 0.6f - 1 ulp and its kin come from"""
    cols = []
    s = F(1.0)
    while s > F(0.0):
        v = F(1.0)
        while v > F(0.0):
            h = F(0.0)
            while h < F(360.0):
                c = F(v * s)
                x = F(c * F(F(1.0) - np.abs(F(np.fmod(F(h / F(60.0)), F(2.0)) - F(1.0)))))
                m = F(v - c)
                z = F(0.0)
                rgb = [(c, x, z), (x, c, z), (z, c, x), (z, x, c), (x, z, c), (c, z, x)][int(h) // 60]
                cols.append([F(k + m) for k in rgb])
                h = F(h + F(30.0))
            v = F(np.float64(v) - 0.3)
        s = F(np.float64(s) - 0.4)
    cols = np.array(cols, np.float32)
    assert cols.shape == (N_COLOURS, 3)
    prod = cols * F(255.0)
    return cols, prod, np.trunc(prod).astype(np.uint8)


def luminance(cols):
    """(r * 0.30f + g * 0.59f) + b * 0.11f in fp32"""
    return (cols[:, 0] * F(0.30) + cols[:, 1] * F(0.59)) + cols[:, 2] * F(0.11)


_TABLE = None


def view_style(position):
    """(background (3,) uint8, font (3,) uint8) of the view at `position` of the view list"""
    global _TABLE
    if _TABLE is None:
        cols, _, byts = colour_table()
        _TABLE = (byts, np.where(luminance(cols) > F(0.5), 0, 255).astype(np.uint8))
    i = int(position) % N_COLOURS
    return _TABLE[0][i].copy(), np.full(3, _TABLE[1][i], np.uint8)


def stamp(w, h, view_id):
    """(h, w) bool: the pixels of the font colour -- cells at ox = 0, 13, ... while ox < w - 13 and oy = 0, 6, ... while oy < h - 6"""
    assert 0 <= view_id <= MAX_ID
    on = np.zeros((h, w), bool)
    digits = (view_id // 100, (view_id % 100) // 10, view_id % 10)
    for ox in range(0, max(w - 13, 0), 13):
        for oy in range(0, max(h - 6, 0), 6):
            for k, d in enumerate(digits):
                on[oy:oy + 5, ox + 4 * k:ox + 4 * k + 3] = GLYPH[d]
    return on


def image(w, h, view_id, position):
    """the (h, w, 3) uint8 debug image of a view"""
    bg, fg = view_style(position)
    return np.where(stamp(w, h, view_id)[:, :, None], fg, bg).astype(np.uint8)


def images(sizes, view_ids=None, first_position=0):
    """the images of Context.debug_embeddings packed back to back"""
    out = [image(int(w), int(h), int(first_position + i if view_ids is None else view_ids[i]), first_position + i).reshape(-1) for i, (w, h) in enumerate(sizes)]
    return np.concatenate(out) if out else np.zeros(0, np.uint8)


def crop(img, box):
    """the float crop of a view's debug image under frame box = (min_x, min_y, w, h): byte / 255.0f, outside the view (1, 0, 1)"""
    H, W = img.shape[:2]
    mx, my, w, h = [int(v) for v in box]
    out = np.empty((h, w, 3), np.uint8); out[:] = (255, 0, 255)
    xs = np.arange(mx, mx + w); ys = np.arange(my, my + h)
    okx = (xs >= 0) & (xs < W); oky = (ys >= 0) & (ys < H)
    out[np.ix_(oky, okx)] = img[np.ix_(ys[oky], xs[okx])]
    return out.astype(np.float32) / np.float32(255.0)
