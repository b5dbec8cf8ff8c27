"""A strict reader of the PNGs row f9 writes (DESIGN.md section 4 "Model output" items 5 and 7), an independent restatement of the per-row
filter choice, and the crafted inputs the tests of the compressed route share.  decode() checks the signature, every chunk's CRC and
(through zlib.decompress) the Adler-32 sum, undoes filters 0 .. 4 and returns the pixels, the filter byte of every row and the raw zlib
stream.  Average and Paeth are undone in png_unfilter.cpp, built on first use with g++ -O2.  Test infrastructure only."""
import ctypes as C
import os
import struct
import subprocess
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "png_unfilter.cpp")
LIB = os.path.join(HERE, "libpng_unfilter.so")
CHUNK = 32768          # csrc/png_rle.h CHUNK
_lib = None


def _load():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB) or os.path.getmtime(LIB) < os.path.getmtime(SRC):
            subprocess.check_call(["g++", "-O2", "-fPIC", "-std=c++17", "-shared", "-o", LIB, SRC])
        _lib = C.CDLL(LIB)
        _lib.png_unfilter_rgb8.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
        _lib.png_unfilter_rgb8.restype = C.c_int
    return _lib


def decode(data):
    """(pixels (H, W, 3) uint8, filter bytes (H,) uint8, zlib stream) of an 8-bit RGB, non-interlaced PNG of the chunks IHDR, IDAT, IEND"""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    at, chunks, idat, ihdr = 8, [], b"", None
    while at < len(data):
        n, typ = struct.unpack(">I4s", data[at:at + 8])
        body = data[at + 8:at + 8 + n]
        (crc,) = struct.unpack(">I", data[at + 8 + n:at + 12 + n])
        assert zlib.crc32(typ + body) & 0xFFFFFFFF == crc, typ
        chunks.append(typ)
        if typ == b"IHDR":
            ihdr = struct.unpack(">IIBBBBB", body)
        elif typ == b"IDAT":
            idat += body
        at += 12 + n
    assert at == len(data) and chunks == [b"IHDR", b"IDAT", b"IEND"]
    w, h, depth, colour, comp, filt, interlace = ihdr
    assert (depth, colour, comp, filt, interlace) == (8, 2, 0, 0, 0)
    d = zlib.decompressobj()
    raw = d.decompress(idat)                         # raises on a wrong Adler-32
    assert d.eof and not d.unused_data and len(raw) == h * (3 * w + 1)
    rows = np.frombuffer(raw, np.uint8).reshape(h, 3 * w + 1)
    out = np.empty((h, w, 3), np.uint8)
    rc = _load().png_unfilter_rgb8(rows.ctypes.data, w, h, out.ctypes.data)
    assert rc == 0, "filter byte above 4 in row %d" % (rc - 1)
    return out, rows[:, 0].copy(), idat


def inflate(z):
    """the bytes of one complete zlib stream with nothing behind it"""
    d = zlib.decompressobj()
    raw = d.decompress(z)
    assert d.eof and not d.unused_data
    return raw


def filtered(img):
    """the rule of DESIGN.md restated in numpy: (filter byte of every row, the filtered stream) of an (H, W, 3) uint8 image -- per row the
    filter whose residuals, read as signed bytes, have the smallest sum of absolute values; ties to the smallest type"""
    h, w, _ = img.shape
    x = img.reshape(h, 3 * w).astype(np.int32)
    a = np.zeros_like(x); a[:, 3:] = x[:, :-3]
    b = np.zeros_like(x); b[1:] = x[:-1]
    c = np.zeros_like(x); c[1:, 3:] = x[:-1, :-3]
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    res = np.stack([x, x - a, x - b, x - (a + b) // 2, x - paeth]) & 255          # (5, H, 3W)
    cost = np.where(res < 128, res, 256 - res).sum(axis=2)                          # (5, H)
    t = cost.argmin(axis=0)                                                         # the first minimum = the smallest type
    rows = np.concatenate([t[:, None], res[t, np.arange(h)]], axis=1).astype(np.uint8)
    return t.astype(np.uint8), rows.tobytes()


def bound(n):
    """the longest zlib stream the format gives n >= 1 filtered bytes; the empty stream is 2 + 5 + 4 bytes"""
    return 2 + n + 10 * ((n + CHUNK - 1) // CHUNK) + 4 if n else 11


def yardstick(stream):
    """zlib's own run-length strategy on the same bytes with the same chunking: the size the tests compare against"""
    z = zlib.compressobj(6, zlib.DEFLATED, 15, 8, zlib.Z_RLE)
    n = 0
    for at in range(0, len(stream), CHUNK):
        n += len(z.compress(stream[at:at + CHUNK])) + len(z.flush(zlib.Z_FULL_FLUSH))
    return n + len(z.flush())


# ---- crafted inputs ----

RUNS = (1, 2, 3, 4, 257, 258, 259, 260, 261, 516, 517, 519)
LENGTH_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)


def _text(rng, n):
    """n bytes of a four-letter alphabet: literals, short runs and long ones"""
    return rng.integers(0, 4, n).astype(np.uint8).tobytes()


def _no_repeat(rng, n):
    v = rng.integers(0, 256, n).astype(np.int64)
    for i in range(1, n):
        if v[i] == v[i - 1]:
            v[i] = (v[i] + 1) & 255
    return v.astype(np.uint8).tobytes()


def streams():
    """name -> bytes: the byte streams of the issue's list"""
    rng = np.random.default_rng(20261019)
    C_ = CHUNK
    out = {"len_%s" % k: _text(rng, n) for k, n in (("0", 0), ("1", 1), ("2", 2), ("Cm1", C_ - 1), ("C", C_), ("Cp1", C_ + 1), ("2C", 2 * C_))}
    for L in RUNS:
        out["run_%d" % L] = b"ab" + b"q" * (L + 1) + b"cd"
    out["run_ends_at_chunk_end"] = _no_repeat(rng, C_ - 100) + b"\xEE" * 100 + b"\x01" + _no_repeat(rng, 49)
    out["run_straddles"] = _no_repeat(rng, C_ - 50) + b"\xEE" * 120 + b"\x01" + _no_repeat(rng, 29)
    out["one_value"] = b"\x07" * (2 * C_ + 5)
    out["no_repeat"] = bytes((3 * i) & 255 for i in range(5000))
    every = bytes(range(256))
    for k, base in enumerate(LENGTH_BASE):
        every += bytes([k + 1]) * (base + 1) + bytes([200 + k])
    out["every_symbol"] = every
    out["random_100000"] = rng.integers(0, 256, 100000).astype(np.uint8).tobytes()
    fib, a, b = [], 1, 1
    for i in range(21):
        fib += [3 * i + 1] * a
        a, b = b, a + b
    out["fibonacci"] = rng.permutation(np.array(fib, np.uint8)).tobytes()
    return out


def pattern(w, h):
    y, x, c = np.meshgrid(np.arange(h), np.arange(w), np.arange(3), indexing="ij")
    return ((7 * x + 13 * y + 29 * c + x * y) & 255).astype(np.uint8)


def bands():
    """48 wide, six bands of six rows on which every filter type wins at least one row"""
    rng = np.random.default_rng(5)
    w = 48
    y, x, c = np.meshgrid(np.arange(6), np.arange(w), np.arange(3), indexing="ij")
    b0 = np.where((x + y) % 2 == 0, 1, 255)                                    # alternating 1 / 255
    b1 = np.broadcast_to(np.array([10, 130, 250, 60, 190, 90])[:, None, None], (6, w, 3))   # a constant per row, far from the row above
    b2 = np.broadcast_to(rng.integers(0, 256, (1, w, 3)), (6, w, 3))           # random columns repeated down the rows
    b3 = (5 * x + 5 * y) % 256                                                 # (5x + 5y) mod 256
    b4 = (rng.integers(0, 256, (1, w, 3)) + 2 * y) % 256                       # random column values plus a small per-row offset
    # under the stated rule (5x + 5y) is a plane, which Paeth predicts exactly: a sixth band, every value the floor of the mean of its left
    # and upper neighbours behind a random first column, is what Average wins
    b5 = np.zeros((6, w, 3), np.int64)
    b5[:, 0] = rng.integers(0, 256, (6, 1))
    up = b4[-1].astype(np.int64)
    for r in range(6):
        for px in range(1, w):
            b5[r, px] = (b5[r, px - 1] + up[px]) // 2
        up = b5[r]
    return np.concatenate([b0, b1, b2, b3, b4, b5]).astype(np.uint8)


def images():
    """name -> (H, W, 3) uint8"""
    out = {"pattern_%dx%d" % (w, h): pattern(w, h) for w, h in ((1, 1), (3, 5), (256, 256), (300, 100))}
    out["zero_128x128"] = np.zeros((128, 128, 3), np.uint8)
    out["bands"] = bands()
    return out


ALIGN_SIZES = [(1 + k, 1 + (7 * k) % 23) for k in range(40)] + [(2, 1)] + [(1, 1)] * 8


def alignment_images():
    """49 small images (ALIGN_SIZES: width, height) of two, sixteen and 256 values in turn: encoded in one call, their packed units start at
    15 or 16 of the 16 residues modulo 16, and the tiny ones at the end are shorter than the bytes up to their first 16-byte boundary"""
    rng = np.random.default_rng(11)
    return [rng.integers(0, (2, 16, 256)[k % 3], (h, w, 3)).astype(np.uint8) for k, (w, h) in enumerate(ALIGN_SIZES)]


def tiny_model():
    """(verts, faces, atlas set) of the smallest model save_model writes: one face, one 16 x 16 atlas of four colours"""
    verts = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    faces = np.array([[0, 1, 2]], np.uint32)
    rng = np.random.default_rng(3)
    atlases = dict(face_ptr=np.array([0, 1], np.uint32), faces=np.array([0], np.uint32), tc_ptr=np.array([0, 3], np.uint32),
                   texcoords_merged=rng.uniform(0, 1, (3, 2)).astype(np.float32), texcoord_ids=np.array([[0, 1, 2]], np.uint32),
                   atlas_size=np.array([16], np.uint32), atlas_pix_ptr=np.array([0, 256], np.uint64), image=rng.integers(0, 4, (256, 3)).astype(np.uint8))
    return verts, faces, atlases
