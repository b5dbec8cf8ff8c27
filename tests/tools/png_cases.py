"""PNG files for the view input's PNG route (csrc/png_dec.h, csrc/k_pngdec.hip; DESIGN.md section 4 "View input"), made with Python's zlib
and numpy only: a chunk writer, the five filters applied by hand, a small deflate bit writer for the streams zlib never emits, and a
second statement of inflate plus unfilter in plain Python / numpy (decode()), which also counts what the stats count: IDAT chunks, blocks
per kind, rows per filter type, and the Paeth ties it met.

  good_cases()      name -> file: the sizes, colour types, filter choices, contents, zlib settings and IDAT cuts of the issue, and Pillow's own files
  hand_cases()      name -> file: hand-assembled deflate streams (all data bytes are 0 .. 4, so every byte is a valid filter type)
  library_cases(M)  name -> file: the library's own writers' files
  refusals()        name -> (file, words of the reason, True when the host's chunk walk already refuses it)
"""
import io
import struct
import zlib

import numpy as np

BPP = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}
SIG = b"\x89PNG\r\n\x1a\n"
BAND, SEGMENT = 64, 64   # csrc/png_dec.h UNFILTER_BAND / UNFILTER_SEGMENT (the tests assert that the library says the same)
SIZES = [(1, 1), (1, 300), (300, 1), (5, 7), (21, 4), (22, 4), (64, 48), (130, 9), (3, 600), (SEGMENT + 1, BAND + 1)]   # (w, h)


# ---- container ----
def chunk(kind, data=b""):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)


def ihdr(w, h, ctype, depth=8, interlace=0):
    return chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, ctype, 0, 0, interlace))


def png_file(w, h, ctype, z, plte=None, cuts=None, iend=True, before=b"", between=None):
    """cuts: the zlib stream's IDAT lengths -- an int (every IDAT that long), a list of cut positions, None: one IDAT"""
    if cuts is None:
        parts = [z]
    elif isinstance(cuts, int):
        parts = [z[i:i + cuts] for i in range(0, len(z), cuts)]
    else:
        edges = [0] + list(cuts) + [len(z)]
        parts = [z[a:b] for a, b in zip(edges[:-1], edges[1:])]
    out = SIG + ihdr(w, h, ctype) + before
    if plte is not None:
        out += chunk(b"PLTE", bytes(plte))
    for k, p in enumerate(parts):
        out += chunk(b"IDAT", p)
        if between is not None and k == 0:
            out += between
    return out + (chunk(b"IEND") if iend else b"")


# ---- filters ----
def paeth(a, b, c):
    a, b, c = a.astype(np.int32), b.astype(np.int32), c.astype(np.int32)
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c)).astype(np.uint8)


def filter_image(px, bpp, types):
    """px (h, w * bpp) uint8 -> the filtered stream; types[y] in 0 .. 4"""
    h, n = px.shape
    out = bytearray()
    zero = np.zeros(n, np.uint8)
    for y in range(h):
        cur, up = px[y], px[y - 1] if y else zero
        a = np.concatenate([np.zeros(bpp, np.uint8), cur[:-bpp]]) if n > bpp else np.zeros(n, np.uint8)
        c = np.concatenate([np.zeros(bpp, np.uint8), up[:-bpp]]) if n > bpp else np.zeros(n, np.uint8)
        t = types[y]
        pred = [zero, a, up, ((a.astype(np.uint16) + up) >> 1).astype(np.uint8), paeth(a, up, c)][t]
        out.append(t)
        out += (cur - pred).astype(np.uint8).tobytes()
    return bytes(out)


def deflate(raw, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, wbits=15):
    c = zlib.compressobj(level, zlib.DEFLATED, wbits, 9, strategy)
    return c.compress(raw) + c.flush()


def palette(n=256, seed=5):
    return np.random.RandomState(seed).randint(0, 256, (n, 3)).astype(np.uint8)


def pixels(w, h, ctype, seed, content="random"):
    rng = np.random.RandomState(seed)
    n = w * BPP[ctype]
    if content == "ties":      # small values: the three Paeth distances tie all the time
        return rng.randint(0, 4, (h, n)).astype(np.uint8)
    if content == "smooth":
        x = np.cumsum(rng.randint(-2, 3, (h, n)), axis=1) + np.cumsum(rng.randint(-2, 3, (h, 1)), axis=0) + 128
        return np.clip(x, 0, 255).astype(np.uint8)
    return rng.randint(0, 256, (h, n)).astype(np.uint8)


def row_types(h, mode):
    return [mode] * h if mode < 5 else [(y + (mode - 5)) % 5 for y in range(h)]   # 5: cycling from 0; 7, 8, 9: first row of type 2, 3, 4


def make(w, h, ctype, mode, seed=0, content="random", level=6, strategy=zlib.Z_DEFAULT_STRATEGY, wbits=15, cuts=None, iend=True, n_plte=256):
    px = pixels(w, h, ctype, seed, content)
    if ctype == 3 and n_plte < 256:
        px %= n_plte
    raw = filter_image(px, BPP[ctype], row_types(h, mode))
    return png_file(w, h, ctype, deflate(raw, level, strategy, wbits), plte=palette(n_plte).tobytes() if ctype == 3 else None, cuts=cuts, iend=iend)


def pillow_save(img, **kw):
    b = io.BytesIO()
    img.save(b, "PNG", **kw)
    return b.getvalue()


def pillow_rgb(f):
    import warnings
    from PIL import Image
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")   # (a palette with tRNS: Pillow advises RGBA; the route drops alpha as convert("RGB") does)
        return np.asarray(Image.open(io.BytesIO(f)).convert("RGB"))


def good_cases():
    C = {}
    k = 0
    for (w, h) in SIZES:                       # every size with every colour type, the filter choice walking along
        for ctype in (0, 2, 3, 4, 6):
            mode = (0, 1, 2, 3, 4, 5, 7, 8, 9)[k % 9]
            C["%dx%d_c%d_f%d" % (w, h, ctype, mode)] = make(w, h, ctype, mode, seed=k)
            k += 1
    for ctype in (0, 2, 3, 4, 6):              # every colour type with every filter choice
        for mode in (0, 1, 2, 3, 4, 5, 7, 8, 9):
            C.setdefault("22x4_c%d_f%d" % (ctype, mode), make(22, 4, ctype, mode, seed=100 + mode))
            C.setdefault("5x7_c%d_f%d" % (ctype, mode), make(5, 7, ctype, mode, seed=200 + mode, content="smooth"))
    for ctype in (0, 2, 4, 6):
        C["ties_c%d" % ctype] = make(40, 30, ctype, 4, seed=7, content="ties")
    for level in (0, 1, 6, 9):
        C["level%d" % level] = make(64, 48, 2, 5, seed=11, content="smooth", level=level)
    C["level0_blocks"] = make(150, 150, 2, 0, seed=12, level=0)
    for name, s in (("fixed", zlib.Z_FIXED), ("rle", zlib.Z_RLE), ("huffman", zlib.Z_HUFFMAN_ONLY), ("filtered", zlib.Z_FILTERED)):
        C["strategy_" + name] = make(64, 48, 2, 5, seed=13, content="smooth", strategy=s)
    C["wbits9"] = make(130, 9, 6, 5, seed=14, content="smooth", wbits=9)
    C["wbits15"] = make(130, 9, 6, 5, seed=14, content="smooth", wbits=15)
    C["idat_1"] = make(21, 4, 2, 5, seed=15, cuts=1)
    C["idat_7"] = make(64, 48, 0, 5, seed=16, cuts=7)
    z_len = len(deflate(filter_image(pixels(64, 48, 2, 17, "smooth"), 3, row_types(48, 4))))
    C["idat_mid_symbol"] = make(64, 48, 2, 4, seed=17, content="smooth", cuts=[z_len // 2 + 1])
    C["no_iend"] = make(22, 4, 2, 5, seed=18, iend=False)
    C["plte_short"] = make(22, 4, 3, 1, seed=19, n_plte=7)
    C["trns_skipped"] = SIG + ihdr(5, 7, 3) + chunk(b"PLTE", palette().tobytes()) + chunk(b"tRNS", bytes(range(0, 250, 10))) + chunk(b"IDAT", deflate(filter_image(pixels(5, 7, 3, 20), 1, row_types(7, 5)))) + chunk(b"IEND")
    C["ancillary_between_plte"] = png_file(5, 7, 2, deflate(filter_image(pixels(5, 7, 2, 21), 3, row_types(7, 5))), before=chunk(b"tEXt", b"k\0v") + chunk(b"gAMA", struct.pack(">I", 45455)))
    # more inflated bytes than the image needs: ignored
    px = pixels(22, 4, 2, 22)
    C["excess_bytes"] = png_file(22, 4, 2, deflate(filter_image(px, 3, row_types(4, 5)) + b"\x00" * 100))
    from PIL import Image
    rng = np.random.RandomState(23)
    for mode, shape in (("L", (9, 33)), ("RGB", (9, 33, 3)), ("LA", (9, 33, 2)), ("RGBA", (9, 33, 4))):
        img = Image.fromarray(np.clip(np.cumsum(rng.randint(-3, 4, shape), axis=1) + 120, 0, 255).astype(np.uint8))
        assert img.mode == mode
        for opt in (0, 1):
            C["pillow_%s_o%d" % (mode, opt)] = pillow_save(img, optimize=bool(opt))
    pimg = Image.fromarray(rng.randint(0, 256, (33, 70, 3)).astype(np.uint8)).quantize(200)
    for opt in (0, 1):
        C["pillow_P_o%d" % opt] = pillow_save(pimg, optimize=bool(opt), bits=8)
    return C


def library_cases(M, tmp):
    """mvs_write_png at levels 0 and 6 and the device encoder's file (its host twin gives the same bytes)"""
    import os
    C = {}
    rgb = pixels(77, 43, 2, 31, "smooth").reshape(43, 77, 3)
    for level in (0, 6):
        p = os.path.join(str(tmp), "own_%d.png" % level)
        M.write_png(p, rgb, level)
        with open(p, "rb") as f:
            C["own_level%d" % level] = f.read()
    C["own_device_rle"] = bytes(M.encode_png_rle(rgb))
    C["own_device_rle_flat"] = bytes(M.encode_png_rle(np.full((40, 300, 3), 9, np.uint8)))
    return C


# ---- a deflate bit writer ----
def canonical(lengths):
    """lengths -> {symbol: (code, length)}, codes as the stream states them (first bit = most significant)"""
    code, out = 0, {}
    for l in range(1, 16):
        for s, sl in enumerate(lengths):
            if sl == l:
                out[s] = (code, l)
                code += 1
        code <<= 1
    return out


def complete_lengths(k):
    """k >= 2 code lengths of a complete code"""
    m = k.bit_length() - 1
    short = (1 << (m + 1)) - k
    return [m] * short + [m + 1] * (k - short)


FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32
CLEN_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]


class Stream:
    """a zlib stream written bit by bit; `out` is what it inflates to"""

    def __init__(self, cmf=0x78, flg=None):
        self.bytes, self.acc, self.n, self.out = bytearray(), 0, 0, bytearray()
        flg = flg if flg is not None else (31 - (cmf << 8) % 31) % 31
        self.bytes += bytes([cmf, flg])
        self.lit = self.dist = None

    def bits(self, v, n):
        self.acc |= (v & ((1 << n) - 1)) << self.n
        self.n += n
        while self.n >= 8:
            self.bytes.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, table, s):
        c, l = table[s]
        for i in range(l - 1, -1, -1):
            self.bits((c >> i) & 1, 1)

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)

    def stored(self, data, final=0, nlen=None):
        self.bits(final, 1); self.bits(0, 2); self.align()
        n = len(data)
        self.bytes += struct.pack("<HH", n, (~n & 0xFFFF) if nlen is None else nlen) + bytes(data)
        self.out += bytes(data)

    def fixed(self, final=0):
        self.bits(final, 1); self.bits(1, 2)
        self.lit, self.dist = canonical(FIXED_LIT), canonical(FIXED_DIST)

    def dynamic(self, lit_len, dist_len, final=0, clen_syms=None, hlit=None, hdist=None, clen_len=None):
        """clen_syms: the code length symbols as a list of (symbol, extra value); None: every length as itself"""
        if clen_syms is None:
            clen_syms = [(l, 0) for l in list(lit_len) + list(dist_len)]
        if clen_len is None:
            used = sorted({s for s, _ in clen_syms})
            if len(used) == 1:
                used.append(18 if used[0] != 18 else 17)
            clen_len = [0] * 19
            for s, l in zip(used, complete_lengths(len(used))):
                clen_len[s] = l
        self.bits(final, 1); self.bits(2, 2)
        self.bits((len(lit_len) if hlit is None else hlit) - 257, 5); self.bits((len(dist_len) if hdist is None else hdist) - 1, 5)
        last = max(i for i, s in enumerate(CLEN_ORDER) if clen_len[s]) + 1
        last = max(last, 4)
        self.bits(last - 4, 4)
        for s in CLEN_ORDER[:last]:
            self.bits(clen_len[s], 3)
        table = canonical(clen_len)
        for s, extra in clen_syms:
            self.code(table, s)
            if s >= 16:
                self.bits(extra, {16: 2, 17: 3, 18: 7}[s])
        self.lit, self.dist = canonical(lit_len), canonical(dist_len)

    def literal(self, b):
        self.code(self.lit, b); self.out.append(b)

    def literals(self, data):
        for b in data:
            self.literal(b)

    def match(self, length, dist, check=True):
        k = max(i for i in range(29) if LEN_BASE[i] <= length and (i == 28 or length < 258))
        self.code(self.lit, 257 + k); self.bits(length - LEN_BASE[k], LEN_EXTRA[k])
        d = max(i for i in range(30) if DIST_BASE[i] <= dist)
        self.code(self.dist, d); self.bits(dist - DIST_BASE[d], DIST_EXTRA[d])
        if check:
            for _ in range(length):
                self.out.append(self.out[-dist])

    def symbol(self, s):
        self.code(self.lit, s)

    def end(self):
        self.code(self.lit, 256)

    def finish(self, adler=None):
        self.align()
        self.bytes += struct.pack(">I", zlib.adler32(bytes(self.out)) & 0xFFFFFFFF if adler is None else adler)
        return bytes(self.bytes)


def small(n, seed):
    return bytes(np.random.RandomState(seed).randint(0, 5, n).astype(np.uint8))


def grey_file(s, pitch=256, adler=None):
    """the stream's output as a grey image of pitch - 1 pixels a row, padded by a last stored block to whole rows"""
    pad = -len(s.out) % pitch
    s.stored(small(pad, 99), final=1)
    return png_file(pitch - 1, len(s.out) // pitch, 0, s.finish(adler))


def lit_lengths(symbols, n=286):
    """a complete code over `symbols`, the first ones getting the short codes"""
    l = [0] * n
    for s, v in zip(symbols, complete_lengths(len(symbols))):
        l[s] = v
    return l


def hand_cases():
    C = {}
    s = Stream(); s.stored(small(300, 1)); s.stored(b""); s.stored(small(212, 2))
    C["empty_stored_between"] = grey_file(s)
    s = Stream(); s.stored(small(100, 3)); s.dynamic(lit_lengths([256, 0]), [0]); s.end(); s.fixed(); s.literals(small(50, 4)); s.end()
    C["dynamic_only_end_code"] = grey_file(s)
    s = Stream(); s.stored(small(32768, 5)); s.fixed(); s.match(258, 32768); s.literal(3); s.match(258, 1); s.match(258, 32768); s.end()
    C["match_258_far_and_near"] = grey_file(s)
    s = Stream(); s.fixed(); s.literals(small(70, 6)); s.end(); s.fixed(); s.match(40, 70); s.match(100, 64); s.match(130, 63); s.match(7, 3); s.end(); s.stored(small(9, 7)); s.fixed(); s.match(200, 300); s.end()
    C["match_into_previous_block"] = grey_file(s)
    # lengths: literals 0 .. 4 and 256 (and the length symbols 257 .. 264) code 4 bits each: 14 symbols ... made complete with 2 more
    lit = lit_lengths([0, 1, 2, 3, 4, 256, 257, 258, 259, 260, 261, 262, 263, 264, 265, 266])
    dist = [0, 0, 0, 1]
    syms = [(l, 0) for l in lit[:267]] + [(18, 286 - 267 + 3 - 11)] + [(1, 0)]   # one run of zeros over the literal table's end and three distance lengths
    s = Stream(); s.dynamic(lit, dist, clen_syms=syms); s.literals(small(20, 8)); s.match(12, 4); s.literals(small(5, 9)); s.end()
    C["repeat_across_tables"] = grey_file(s)
    lens15 = list(range(1, 16)) + [15]
    order = [2, 3, 4, 256, 257, 258, 259, 260, 261, 262, 263, 264, 265, 266, 0, 1]   # literals 0 and 1 get the two 15-bit codes
    lit = [0] * 286
    for sym, l in zip(order, lens15):
        lit[sym] = l
    s = Stream(); s.dynamic(lit, complete_lengths(4)); s.literals(small(300, 10)); s.match(9, 2); s.end()
    C["code_15_bits"] = grey_file(s)
    s = Stream(); s.dynamic(lit_lengths([0, 1, 2, 3, 4, 256, 257, 258]), [1]); s.literals(small(10, 11)); s.match(4, 1); s.match(3, 1); s.end()
    C["one_bit_distance_code"] = grey_file(s)
    s = Stream(); s.stored(small(255, 12)); s.fixed(final=1); s.literals(small(256, 13)); s.literal(1); s.end()
    assert s.n != 0   # the final block ends inside a byte
    C["final_block_ends_mid_byte"] = png_file(255, 2, 0, s.finish())
    return C


# ---- refusals ----
def refusals():
    R = {}
    good = make(22, 4, 2, 5, seed=40)

    def zfile(z, w=255, h=1, ctype=0, **kw):
        return png_file(w, h, ctype, z, **kw)

    def reason(name, f, words, host=False):
        R[name] = (f, words, host)

    # the container
    for depth, ctype in ((1, 0), (2, 3), (4, 0), (16, 2)):
        f = SIG + ihdr(8, 8, ctype, depth=depth) + (chunk(b"PLTE", palette(4).tobytes()) if ctype == 3 else b"") + chunk(b"IDAT", deflate(b"\0" * 200)) + chunk(b"IEND")
        reason("depth_%d" % depth, f, "bit depth %d" % depth, True)
    reason("adam7", SIG + ihdr(8, 8, 2, interlace=1) + chunk(b"IDAT", deflate(b"\0" * 400)) + chunk(b"IEND"), "interlaced", True)
    reason("plte_missing", png_file(5, 7, 3, deflate(filter_image(pixels(5, 7, 3, 1), 1, [0] * 7))), "without PLTE", True)
    reason("plte_not_triples", png_file(5, 7, 3, deflate(b"\0" * 42), plte=b"\1\2\3\4"), "PLTE of 4 bytes", True)
    reason("idat_not_consecutive", png_file(22, 4, 2, deflate(filter_image(pixels(22, 4, 2, 2), 3, [0] * 4)), cuts=[20], between=chunk(b"tEXt", b"a\0b")), "not consecutive", True)
    reason("chunk_past_file", good[:-20], "running past the file", True)
    reason("chunk_length_huge", good[:33] + struct.pack(">I", 0x7FFFFFFF) + good[37:], "running past the file", True)
    reason("no_idat", SIG + ihdr(4, 4, 2) + chunk(b"IEND"), "no IDAT", True)
    reason("ihdr_crc", good[:29] + bytes([good[29] ^ 1]) + good[30:], "IHDR's CRC", True)
    reason("colour_type_5", SIG + ihdr(4, 4, 5) + chunk(b"IDAT", deflate(b"\0" * 100)) + chunk(b"IEND"), "colour type 5", True)
    reason("empty_frame", SIG + ihdr(0, 4, 2) + chunk(b"IDAT", deflate(b"\0" * 100)) + chunk(b"IEND"), "empty", True)
    reason("critical_unknown", png_file(4, 4, 2, deflate(b"\0" * 52), before=chunk(b"ABCD", b"x")), "unknown critical chunk", True)
    reason("not_a_png", b"\xff\xd8\xff\xe0" + b"\0" * 40, "no PNG signature", True)
    # the zlib header
    body = deflate(small(256, 50))[2:]
    reason("zlib_cm", zfile(bytes([0x77, 0x09]) + body), "compression method is not 8")   # 0x7709 % 31 == 0
    reason("zlib_cinfo", zfile(bytes([0x88, 0x1C]) + body), "CINFO > 7")
    reason("zlib_fcheck", zfile(bytes([0x78, 0x9D]) + body), "FCHECK")
    reason("zlib_fdict", zfile(bytes([0x78, 0xBB]) + body), "FDICT")
    # deflate
    s = Stream(); s.stored(small(100, 51)); s.bits(1, 1); s.bits(3, 2)
    reason("block_type_3", zfile(s.finish()), "block type 3")
    s = Stream(); s.stored(small(256, 52), final=1, nlen=0x1234)
    reason("stored_len", zfile(s.finish()), "LEN is not ~NLEN")
    ok_lit = lit_lengths([0, 1, 2, 3, 4, 256, 257, 258])
    s = Stream(); s.dynamic(ok_lit + [0], complete_lengths(2), final=1, hlit=287); s.literals(small(256, 53)); s.end()
    reason("hlit_287", zfile(s.finish()), "HLIT above 286")
    s = Stream(); s.dynamic(ok_lit, complete_lengths(2) + [0] * 29, final=1, hdist=31); s.literals(small(256, 54)); s.end()
    reason("hdist_31", zfile(s.finish()), "HDIST above 30")
    s = Stream(); s.fixed(final=1); s.literals(small(256, 55)); s.symbol(286); s.bits(0, 5); s.end()
    reason("symbol_286", zfile(s.finish()), "length symbol 286 or 287")
    s = Stream(); s.fixed(final=1); s.literals(small(256, 56)); s.symbol(257); s.bits(0b01111, 5); s.end()   # distance code 30, its bits reversed
    reason("distance_code_30", zfile(s.finish()), "distance code 30 or 31")
    s = Stream(); s.dynamic(ok_lit, complete_lengths(2), final=1, clen_syms=[(16, 0)] + [(l, 0) for l in ok_lit[3:]] + [(1, 0), (1, 0)], clen_len=None)
    reason("repeat_16_first", zfile(s.finish()), "no previous length")
    s = Stream(); s.dynamic(ok_lit, complete_lengths(2), final=1, clen_syms=[(l, 0) for l in ok_lit] + [(1, 0), (18, 20)])
    reason("repeat_past_end", zfile(s.finish()), "runs past HLIT + HDIST")
    over = [0] * 286; over[0] = over[1] = over[256] = 1
    s = Stream(); s.dynamic(over, complete_lengths(2), final=1)
    reason("oversubscribed", zfile(s.finish()), "over-subscribed")
    inc = [0] * 286; inc[0] = inc[1] = inc[256] = 2
    s = Stream(); s.dynamic(inc, complete_lengths(2), final=1)
    reason("incomplete_literal_code", zfile(s.finish()), "incomplete code")
    s = Stream(); s.dynamic(ok_lit, [2, 2, 2], final=1)
    reason("incomplete_distance_code", zfile(s.finish()), "incomplete code")
    one = [0] * 286; one[256] = 1
    s = Stream(); s.dynamic(one, [0], final=1)
    reason("single_literal_code", zfile(s.finish()), "incomplete code")
    s = Stream(); s.dynamic(ok_lit, complete_lengths(2), final=1, clen_len=[2, 2, 0, 2] + [0] * 15)
    reason("incomplete_length_code", zfile(s.finish()), "incomplete code")
    s = Stream(); s.dynamic(lit_lengths([0, 1, 2, 3, 4, 255, 257, 258]), complete_lengths(2), final=1)
    reason("no_end_code", zfile(s.finish()), "no end-of-block code")
    s = Stream(); s.fixed(final=1); s.literal(1); s.match(3, 2, check=False); s.literals(small(252, 57)); s.end()
    reason("distance_too_far", zfile(s.finish()), "further back than the bytes produced")
    s = Stream(); s.dynamic(ok_lit, [0], final=1); s.literals(small(20, 58)); s.symbol(257); s.bits(0, 1)
    reason("distance_code_unused_table", zfile(s.finish()), "no code matches")
    z = deflate(filter_image(pixels(64, 48, 2, 59, "smooth"), 3, [4] * 48))
    reason("cut_inside_symbol", png_file(64, 48, 2, z[:len(z) // 2]), "ends inside a symbol")
    s = Stream(); s.stored(small(256, 60), final=0)
    reason("no_final_block", zfile(bytes(s.bytes)), "before the final block")
    s = Stream(); s.stored(small(256, 61), final=1)
    reason("cut_in_stored_block", zfile(bytes(s.bytes[:-9])), "ends inside a symbol")
    reason("cut_in_adler", zfile(s.finish()[:-2]), "ends inside a symbol")
    z = deflate(filter_image(pixels(22, 4, 2, 62), 3, [1] * 4))
    reason("adler_mismatch", png_file(22, 4, 2, z[:-1] + bytes([z[-1] ^ 0x40])), "Adler-32 does not match")
    reason("too_few_bytes", png_file(22, 5, 2, z), "fewer inflated bytes than the image needs (268 bytes)")
    raw = bytearray(filter_image(pixels(22, 70, 2, 63), 3, [2] * 70)); raw[67 * 66] = 5; raw[67 * 69] = 200
    reason("filter_type_5", png_file(22, 70, 2, deflate(bytes(raw))), "filter type above 4 in row 66")
    px = pixels(21, 4, 3, 64) % 4; px[1, 3] = 4; px[3, 20] = 255
    reason("palette_index", png_file(21, 4, 3, deflate(filter_image(px, 1, [0, 1, 2, 4])), plte=palette(4).tobytes()), "palette indices at or past PLTE's entries (2 pixels)")
    return R


# ---- the second statement: inflate and unfilter in plain Python / numpy ----
class BitReader:
    def __init__(self, data):
        self.d, self.pos = data, 0

    def bit(self):
        if self.pos >= 8 * len(self.d):
            raise ValueError("stream ended")
        b = (self.d[self.pos >> 3] >> (self.pos & 7)) & 1
        self.pos += 1
        return b

    def bits(self, n):
        v = 0
        for i in range(n):
            v |= self.bit() << i
        return v


def decoder(lengths):
    return {(l, c): s for s, (c, l) in canonical(lengths).items()}


def read_symbol(r, table):
    code = 0
    for l in range(1, 16):
        code = code << 1 | r.bit()
        if (l, code) in table:
            return table[(l, code)]
    raise ValueError("no code")


def inflate(z):
    """-> (bytes, [stored, fixed, dynamic blocks])"""
    assert z[0] & 15 == 8 and (z[0] << 8 | z[1]) % 31 == 0 and not z[1] & 32
    r = BitReader(z[2:])
    out, blocks = bytearray(), [0, 0, 0]
    while True:
        final, kind = r.bit(), r.bits(2)
        if kind == 0:
            r.pos = (r.pos + 7) & ~7
            n, nn = r.bits(16), r.bits(16)
            assert n == (~nn & 0xFFFF)
            at = r.pos >> 3
            out += r.d[at:at + n]
            r.pos += 8 * n
        else:
            if kind == 1:
                lit, dist = decoder(FIXED_LIT), decoder(FIXED_DIST)
            else:
                assert kind == 2
                hlit, hdist, hclen = r.bits(5) + 257, r.bits(5) + 1, r.bits(4) + 4
                cl = [0] * 19
                for i in range(hclen):
                    cl[CLEN_ORDER[i]] = r.bits(3)
                ct, lens = decoder(cl), []
                while len(lens) < hlit + hdist:
                    s = read_symbol(r, ct)
                    if s < 16:
                        lens.append(s)
                    elif s == 16:
                        lens += [lens[-1]] * (3 + r.bits(2))
                    elif s == 17:
                        lens += [0] * (3 + r.bits(3))
                    else:
                        lens += [0] * (11 + r.bits(7))
                assert len(lens) == hlit + hdist
                lit, dist = decoder(lens[:hlit]), decoder(lens[hlit:])
            while True:
                s = read_symbol(r, lit)
                if s < 256:
                    out.append(s)
                elif s == 256:
                    break
                else:
                    n = LEN_BASE[s - 257] + r.bits(LEN_EXTRA[s - 257])
                    d = read_symbol(r, dist)
                    d = DIST_BASE[d] + r.bits(DIST_EXTRA[d])
                    assert d <= len(out)
                    for _ in range(n):
                        out.append(out[-d])
        blocks[kind] += 1
        if final:
            break
    r.pos = (r.pos + 7) & ~7
    adler = struct.unpack(">I", r.d[r.pos >> 3:(r.pos >> 3) + 4])[0]
    return bytes(out), blocks, adler


def decode(f):
    """the file by this module's own reading: rgb, raw, blocks, rows (per filter type), idat_chunks, ties (pa == pb, pb == pc, pa == pc met)"""
    assert f[:8] == SIG
    pos, z, plte, n_idat, head = 8, b"", None, 0, None
    while pos < len(f):
        n, kind = struct.unpack(">I", f[pos:pos + 4])[0], f[pos + 4:pos + 8]
        body = f[pos + 8:pos + 8 + n]
        if kind == b"IHDR":
            head = struct.unpack(">IIBBBBB", body)
        elif kind == b"PLTE":
            plte = np.frombuffer(body, np.uint8).reshape(-1, 3)
        elif kind == b"IDAT":
            z += body; n_idat += 1
        elif kind == b"IEND":
            break
        pos += n + 12
    w, h, depth, ctype = head[:4]
    assert depth == 8 and head[6] == 0
    bpp = BPP[ctype]
    data, blocks, adler = inflate(z)
    need = h * (1 + w * bpp)
    assert len(data) >= need
    if len(data) == need:
        assert zlib.adler32(data) & 0xFFFFFFFF == adler
    raw = data[:need]
    rows, ties = [0] * 5, [0, 0, 0]
    img = np.zeros((h, w * bpp), np.int32)
    src = np.frombuffer(raw, np.uint8).reshape(h, 1 + w * bpp)
    for y in range(h):
        t = int(src[y, 0]); rows[t] += 1
        line = src[y, 1:].astype(np.int32)
        up = img[y - 1] if y else np.zeros(w * bpp, np.int32)
        if t == 0:
            img[y] = line
        elif t == 2:
            img[y] = (line + up) & 255
        else:
            cur = img[y]
            for i in range(w * bpp):
                a = cur[i - bpp] if i >= bpp else 0
                b = up[i]
                c = up[i - bpp] if i >= bpp else 0
                if t == 1:
                    p = a
                elif t == 3:
                    p = (a + b) >> 1
                else:
                    q = a + b - c
                    pa, pb, pc = abs(q - a), abs(q - b), abs(q - c)
                    ties[0] += pa == pb; ties[1] += pb == pc; ties[2] += pa == pc
                    p = a if pa <= pb and pa <= pc else b if pb <= pc else c
                cur[i] = (line[i] + p) & 255
    px = img.astype(np.uint8).reshape(h, w, bpp)
    if ctype == 3:
        rgb = plte[px[:, :, 0]]
    elif bpp < 3:
        rgb = np.repeat(px[:, :, :1], 3, axis=2)
    else:
        rgb = px[:, :, :3]
    return {"rgb": np.ascontiguousarray(rgb), "raw": raw, "blocks": blocks, "rows": rows, "idat_chunks": n_idat, "ties": ties, "size": (w, h), "colour_type": ctype,
            "zlib_bytes": len(z), "raw_bytes": need}
