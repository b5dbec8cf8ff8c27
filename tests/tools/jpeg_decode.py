"""The JPEG route of the model output (DESIGN.md section 4 "Model output" item 9; csrc/jpeg_base.h) stated a second time, in numpy:

  parse(data)            a strict parser of the container and a Huffman decoder down to the quantised coefficients of every block.  It
                         insists on the fixed segment order SOI, APP0 (JFIF 1.01, density 1:1 without unit), DQT 0, DQT 1, SOF0, DHT x4
                         (DC 0, DC 1, AC 0, AC 1), DRI, SOS, data, EOI with their exact lengths and table ids; on one RST marker behind every
                         DRI MCUs but the last group, numbered mod 8; on no other marker inside the entropy data; on a 0x00 behind every 0xFF
                         of it; and on padding bits that are all 1 and fewer than 8 at the end of every segment.
  coefficients(img, quality, subsampling)
                         the forward path in numpy integers: colour, edge extension, subsampling, the two DCT passes with their rounding
                         shifts, the quantiser -- the blocks in coding order, coefficients in zig-zag order.
  images()               the crafted inputs: the smallest shapes at which the indexing can go wrong.

R below is the format's restart interval; everything else is derived here, not imported from the product."""
import numpy as np

R = 8
HEADER_BYTES = 629

QUANT_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                       18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99], np.int64)
QUANT_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66] + [99] * 38, np.int64)


def zigzag():
    """position in the scan -> v * 8 + u: the anti-diagonals of the block, alternately upwards and downwards"""
    order = []
    for s in range(15):
        cells = [(v, s - v) for v in range(8) if 0 <= s - v < 8]
        order += [v * 8 + u for v, u in (cells[::-1] if s % 2 == 0 else cells)]
    return np.array(order)


ZIGZAG = zigzag()


def quant_tables(quality):
    """the two tables in natural order (v * 8 + u) at `quality`"""
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return [np.clip((t * s + 50) // 100, 1, 255) for t in (QUANT_LUMA, QUANT_CHROMA)]


def cosines():
    u, x = np.mgrid[0:8, 0:8]
    c = np.where(u == 0, np.sqrt(0.5), 1.0)
    return np.rint(8192.0 * c * np.cos((2 * x + 1) * u * np.pi / 16.0) / 2.0).astype(np.int64)


def coefficients(img, quality, subsampling):
    """[blocks, 64] int64: the quantised coefficients of every block in coding order (MCUs in raster order; Y Cb Cr, or Y00 Y01 Y10 Y11 Cb Cr),
    zig-zag order inside a block"""
    img = np.asarray(img, np.uint8)
    h, w = img.shape[:2]
    m = 16 if subsampling else 8
    H, W = -(-h // m) * m, -(-w // m) * m
    p = np.pad(img, ((0, H - h), (0, W - w), (0, 0)), mode="edge").astype(np.int64)
    r, g, b = p[..., 0], p[..., 1], p[..., 2]
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    if subsampling:
        cb, cr = [(c.reshape(H // 2, 2, W // 2, 2).sum(axis=(1, 3)) + 2) >> 2 for c in (cb, cr)]
    blocks = lambda c: (c - 128).reshape(c.shape[0] // 8, 8, c.shape[1] // 8, 8).transpose(0, 2, 1, 3)   # [by, bx, y, x]
    yb, cbb, crb = blocks(y), blocks(cb), blocks(cr)
    mh, mw = H // m, W // m
    if subsampling:
        yb = yb.reshape(mh, 2, mw, 2, 8, 8).transpose(0, 2, 1, 3, 4, 5).reshape(mh, mw, 4, 8, 8)
        mcu = np.concatenate([yb, cbb[:, :, None], crb[:, :, None]], axis=2)
        table = [0, 0, 0, 0, 1, 1]
    else:
        mcu = np.stack([yb, cbb, crb], axis=2)
        table = [0, 1, 1]
    s = mcu.reshape(-1, 8, 8)
    C = cosines()
    t = (np.einsum("ux,byx->byu", C, s) + 512) >> 10
    f = (np.einsum("vy,byu->bvu", C, t) + 32768) >> 16
    q = np.stack([quant_tables(quality)[k] for k in table] * (mh * mw)).reshape(-1, 8, 8)
    a = (np.abs(f) + (q >> 1)) // q
    a[:, 0, 1:] = np.minimum(a[:, 0, 1:], 1023); a[:, 1:, :] = np.minimum(a[:, 1:, :], 1023)
    return (np.sign(f) * a).reshape(-1, 64)[:, ZIGZAG]


class BadJpeg(AssertionError):
    pass


def _need(cond, what):
    if not cond:
        raise BadJpeg(what)


def _lookup(bits, vals):
    """a DHT as a table over 16-bit prefixes: (symbol, length), length 0 where no code matches"""
    sym = np.zeros(65536, np.int32); length = np.zeros(65536, np.int32)
    code, at = 0, 0
    for n in range(1, 17):
        for _ in range(bits[n - 1]):
            _need(code < (1 << n), "DHT: more codes than its lengths allow")
            lo = code << (16 - n)
            sym[lo:lo + (1 << (16 - n))] = vals[at]; length[lo:lo + (1 << (16 - n))] = n
            code += 1; at += 1
        code <<= 1
    return sym.tolist(), length.tolist()


def parse(data):
    """dict(width, height, subsampling, quant [2][64] natural order, quant_zigzag, dht {(class, id): (bits, vals)}, restart_interval,
    coefficients [blocks, 64] zig-zag order in coding order, segments, rst_markers, stuffed_bytes, marker_bytes, entropy_bytes, zrl,
    eob, segments_ending_stuffed)"""
    d = bytes(data)
    at = [0]

    def take(n):
        _need(at[0] + n <= len(d), "truncated")
        v = d[at[0]:at[0] + n]; at[0] += n
        return v

    def segment(marker, length):
        h = take(4)
        _need(h[0] == 0xFF and h[1] == marker, "expected marker %02X at %d, found %02X%02X" % (marker, at[0] - 4, h[0], h[1]))
        _need((h[2] << 8 | h[3]) == length, "marker %02X: length %d, expected %d" % (marker, h[2] << 8 | h[3], length))
        return take(length - 2)

    _need(take(2) == b"\xff\xd8", "no SOI")
    _need(segment(0xE0, 16) == b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00", "APP0 is not JFIF 1.01 with density 1:1 without unit")
    out = {"quant_zigzag": [], "quant": [], "dht": {}}
    for t in (0, 1):
        s = segment(0xDB, 67)
        _need(s[0] == t, "DQT: table id / precision")
        zz = np.frombuffer(s[1:], np.uint8).astype(np.int64)
        _need(zz.min() >= 1, "DQT: zero quantiser")
        nat = np.zeros(64, np.int64); nat[ZIGZAG] = zz
        out["quant_zigzag"].append(zz); out["quant"].append(nat)
    s = segment(0xC0, 17)
    _need(s[0] == 8 and s[5] == 3, "SOF0: 8 bit, 3 components")
    out["height"], out["width"] = s[1] << 8 | s[2], s[3] << 8 | s[4]
    _need(out["height"] >= 1 and out["width"] >= 1, "SOF0: empty frame")
    _need(s[7] in (0x11, 0x22), "SOF0: luma sampling")
    sub = out["subsampling"] = 1 if s[7] == 0x22 else 0
    _need(bytes(s[6:]) == bytes([1, s[7], 0, 2, 0x11, 1, 3, 0x11, 1]), "SOF0: component ids, sampling factors or table ids")
    for cls_id, count in ((0x00, 12), (0x01, 12), (0x10, 162), (0x11, 162)):
        s = segment(0xC4, 19 + count)
        _need(s[0] == cls_id, "DHT: class / id order")
        bits, vals = list(s[1:17]), list(s[17:])
        _need(sum(bits) == count and len(set(vals)) == count, "DHT: counts")
        out["dht"][(cls_id >> 4, cls_id & 15)] = (bits, vals)
    s = segment(0xDD, 4)
    ri = out["restart_interval"] = s[0] << 8 | s[1]
    _need(ri == R, "DRI is not the format's R")
    _need(segment(0xDA, 12) == bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]), "SOS: components, tables or spectral selection")
    _need(at[0] == HEADER_BYTES, "header length")
    # ---- the entropy data: split at the RST markers, unstuffed ----
    body = d[at[0]:]
    _need(len(body) >= 2 and body[-2:] == b"\xff\xd9", "no EOI at the end")
    body = body[:-2]
    segs, cur, stuffed, ends_stuffed, i = [], bytearray(), 0, 0, 0
    while i < len(body):
        v = body[i]
        if v != 0xFF:
            cur.append(v); i += 1
            continue
        _need(i + 1 < len(body), "a lone 0xFF ends the entropy data")
        nxt = body[i + 1]
        if nxt == 0x00:
            cur.append(0xFF); stuffed += 1; i += 2
            if i == len(body) or (body[i] == 0xFF and i + 1 < len(body) and 0xD0 <= body[i + 1] <= 0xD7):
                ends_stuffed += 1
        else:
            _need(0xD0 <= nxt <= 0xD7, "marker %02X inside the entropy data at %d" % (nxt, at[0] + i))
            _need(nxt == 0xD0 + (len(segs) & 7), "RST%d where RST%d is due" % (nxt - 0xD0, len(segs) & 7))
            segs.append(bytes(cur)); cur = bytearray(); i += 2
    segs.append(bytes(cur))
    m = 16 if sub else 8
    mcus = -(-out["width"] // m) * -(-out["height"] // m)
    _need(len(segs) == -(-mcus // ri), "%d segments for %d MCUs" % (len(segs), mcus))
    out.update(segments=len(segs), rst_markers=len(segs) - 1, stuffed_bytes=stuffed, segments_ending_stuffed=ends_stuffed,
               marker_bytes=HEADER_BYTES + 2 * (len(segs) - 1) + 2, entropy_bytes=len(body) - 2 * (len(segs) - 1))
    # ---- Huffman decoding ----
    look = {k: _lookup(*v) for k, v in out["dht"].items()}
    table = [0, 0, 0, 0, 1, 1] if sub else [0, 1, 1]
    comp = [0, 0, 0, 0, 1, 2] if sub else [0, 1, 2]
    blocks, zrl, eob = [], 0, 0
    for k, seg in enumerate(segs):
        nbits = 8 * len(seg)
        val = int.from_bytes(seg + b"\xff\xff\xff\xff", "big")
        total = nbits + 32
        pos = 0
        pred = [0, 0, 0]

        def symbol(tab):
            nonlocal pos
            sym, length = tab
            p = (val >> (total - pos - 16)) & 0xFFFF
            _need(length[p] > 0, "segment %d: no code matches at bit %d" % (k, pos))
            pos += length[p]
            return sym[p]

        def value(n):
            nonlocal pos
            if not n:
                return 0
            v = (val >> (total - pos - n)) & ((1 << n) - 1)
            pos += n
            return v if v >> (n - 1) else v - (1 << n) + 1

        for _ in range(min(ri, mcus - k * ri)):
            for bi in range(len(table)):
                c = [0] * 64
                n = symbol(look[(0, table[bi])])
                _need(n <= 11, "DC category")
                pred[comp[bi]] += value(n)
                c[0] = pred[comp[bi]]
                j = 1
                while j < 64:
                    rs = symbol(look[(1, table[bi])])
                    run, n = rs >> 4, rs & 15
                    if n == 0:
                        if run == 15:
                            j += 16; zrl += 1
                            _need(j < 64, "ZRL runs past the block")
                            continue
                        _need(run == 0, "AC symbol %02X" % rs)
                        eob += 1
                        break
                    j += run
                    _need(j < 64 and n <= 10, "AC run past the block or size above 10")
                    c[j] = value(n)
                    _need(c[j] != 0, "zero coded as a value")
                    j += 1
                blocks.append(c)
                _need(pos <= nbits, "segment %d: its MCUs need more bits than it has" % k)
        rest = nbits - pos
        _need(rest < 8, "segment %d: %d bits behind its last MCU" % (k, rest))
        _need(rest == 0 or (val >> 32) & ((1 << rest) - 1) == (1 << rest) - 1, "segment %d: padding bits are not all 1" % k)
    out.update(coefficients=np.array(blocks, np.int64).reshape(-1, 64), zrl=zrl, eob=eob)
    return out


def psnr(a, b):
    e = np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2)
    return 99.0 if e == 0 else 10.0 * np.log10(255.0 ** 2 / e)


def _basis(zz_pos, amplitude):
    """a grey 8 x 8 block: 128 + amplitude x the DCT basis function at zig-zag position zz_pos"""
    v, u = divmod(int(ZIGZAG[zz_pos]), 8)
    y, x = np.mgrid[0:8, 0:8]
    g = 128.0 + amplitude * np.cos((2 * x + 1) * u * np.pi / 16.0) * np.cos((2 * y + 1) * v * np.pi / 16.0)
    return np.repeat(np.clip(np.rint(g), 0, 255).astype(np.uint8)[:, :, None], 3, axis=2)


def images():
    """name -> (H, W, 3) uint8"""
    rs = np.random.RandomState(20240917)
    out = {}

    def smooth(h, w, noise=6.0):
        y, x = np.mgrid[0:h, 0:w].astype(np.float64)
        g = np.stack([128 + 100 * np.sin(x / 9.0 + y / 23.0), 128 + 90 * np.cos(y / 7.0 - x / 31.0), 40 + 170 * (x + y) / max(h + w - 2, 1)], -1)
        return np.clip(np.rint(g + noise * rs.randn(h, w, 3)), 0, 255).astype(np.uint8)

    for n in (1, 7, 8, 9, 15, 16, 17):
        out["side_%d" % n] = smooth(n, n, 20.0)
    out["rect_17x9"] = smooth(9, 17, 20.0)
    for mcus in (R - 1, R, R + 1):                     # one MCU row of R - 1, R, R + 1 MCUs in either sampling mode
        out["mcus444_%d" % mcus] = smooth(8, 8 * mcus)
        out["mcus420_%d" % mcus] = smooth(16, 16 * mcus)
    out["straddle_77x43"] = smooth(43, 77)             # 4:2:0: 5 x 3 MCUs, 4:4:4: 10 x 6 -- segments run across the ends of MCU rows
    out["wrap_203x171"] = smooth(171, 203)             # 4:2:0: 13 x 11 = 143 MCUs, 18 segments; 4:4:4: 26 x 22 = 572 MCUs, 72 segments
    out["flat_24"] = np.tile(np.array([200, 30, 90], np.uint8), (24, 24, 1))
    out["zrl_one"] = np.tile(_basis(20, 110.0), (2, 2, 1))      # one coefficient behind 19 zeros: one ZRL
    out["zrl_two"] = np.tile(_basis(40, 110.0), (2, 2, 1))      # ... behind 39 zeros: two
    y, x = np.mgrid[0:32, 0:32]
    out["checker_grey"] = np.repeat((((x + y) & 1) * 255).astype(np.uint8)[:, :, None], 3, axis=2)
    out["checker_colour"] = np.stack([((x & 1) * 255), ((y & 1) * 255), (((x + y) & 1) * 255)], -1).astype(np.uint8)
    out["noise_40x24"] = rs.randint(0, 256, (24, 40, 3)).astype(np.uint8)
    out["ends_stuffed"] = np.random.RandomState(ENDS_STUFFED_SEED).randint(0, 256, (8, 8, 3)).astype(np.uint8)
    out["photo_256"] = smooth(256, 256, 4.0)
    return out


# an 8 x 8 noise image whose one segment ends on a stuffed byte at quality 100 in 4:4:4 (found by searching the seeds with the host twin)
ENDS_STUFFED_SEED = 3
