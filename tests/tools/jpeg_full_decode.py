"""The view input route (DESIGN.md section 4 "View input"; csrc/jpeg_dec.h) stated a second time, in numpy, independent of the product:

  decode(data)           a general baseline parser (any order of DQT / DHT / DRI / APPn / COM in front of SOS, several tables per segment,
                         tables redefined, any restart interval), a Huffman decoder down to the quantised coefficients, libjpeg's
                         jpeg_idct_islow in int64, the "fancy" triangle upsampling on the components' own sizes and the YCbCr -> RGB
                         conversion with libjpeg's constants.  Returns dict(rgb (H, W, 3) uint8, coefficients int64 [blocks, 64] in coding
                         order and natural order (v * 8 + u), width, height, sampling (h, v), components, restart_interval, segments,
                         stuffed_bytes, entropy (the raw entropy bytes, stuffing and markers included)).
  entropy_range(data)    (begin, end) of the entropy data in the file: behind SOS, in front of EOI.

It refuses (BadJpeg) what it does not read; the product's refusals are tested against the product's own messages, not against this."""
import numpy as np


class BadJpeg(AssertionError):
    pass


def _need(cond, what):
    if not cond:
        raise BadJpeg(what)


def zigzag():
    order = []
    for s in range(15):
        cells = [(v, s - v) for v in range(8) if 0 <= s - v < 8]
        order += [v * 8 + u for v, u in (cells[::-1] if s % 2 == 0 else cells)]
    return np.array(order)


ZIGZAG = zigzag()


def _codes(bits, vals):
    """{(length, code): symbol} of a DHT"""
    out, code, at = {}, 0, 0
    for n in range(1, 17):
        for _ in range(bits[n - 1]):
            _need(code < (1 << n), "DHT: more codes than its lengths allow")
            out[(n, code)] = vals[at]
            code += 1; at += 1
        code <<= 1
    return out


def _headers(d):
    _need(d[:2] == b"\xff\xd8", "no SOI")
    at = 2
    q, h, frame, dri = {}, {}, None, 0
    while True:
        _need(at + 4 <= len(d) and d[at] == 0xFF, "no marker at %d" % at)
        m = d[at + 1]
        if m == 0xFF:
            at += 1
            continue
        n = d[at + 2] << 8 | d[at + 3]
        _need(at + 2 + n <= len(d), "truncated")
        s = d[at + 4:at + 2 + n]
        at += 2 + n
        if m == 0xDB:
            while s:
                _need(s[0] >> 4 == 0, "16-bit DQT")
                t = np.zeros(64, np.int64); t[ZIGZAG] = np.frombuffer(s[1:65], np.uint8)
                q[s[0] & 15] = t; s = s[65:]
        elif m == 0xC4:
            while s:
                bits = list(s[1:17]); cnt = sum(bits)
                h[(s[0] >> 4, s[0] & 15)] = _codes(bits, list(s[17:17 + cnt])); s = s[17 + cnt:]
        elif m == 0xC0:
            _need(s[0] == 8, "precision")
            frame = dict(height=s[1] << 8 | s[2], width=s[3] << 8 | s[4], comps=[(s[6 + 3 * c], s[7 + 3 * c] >> 4, s[7 + 3 * c] & 15, s[8 + 3 * c]) for c in range(s[5])])
        elif m == 0xDD:
            dri = s[0] << 8 | s[1]
        elif m == 0xDA:
            _need(frame is not None and s[0] == len(frame["comps"]), "scan components")
            tabs = [(s[2 + 2 * c] >> 4, s[2 + 2 * c] & 15) for c in range(s[0])]
            _need(bytes(s[1 + 2 * s[0]:]) == b"\x00\x3f\x00", "not a sequential scan")
            return frame, q, h, dri, tabs, at
        else:
            _need(m in (0xFE,) or 0xE0 <= m <= 0xEF, "marker %02X" % m)


def entropy_range(data):
    d = bytes(data)
    at = _headers(d)[5]
    _need(d[-2:] == b"\xff\xd9", "no EOI")
    return at, len(d) - 2


class _Bits:
    def __init__(self, seg):
        self.v = int.from_bytes(seg + b"\x00" * 8, "big"); self.total = 8 * len(seg) + 64; self.pos = 0; self.n = 8 * len(seg)

    def take(self, n):
        if not n:
            return 0
        r = (self.v >> (self.total - self.pos - n)) & ((1 << n) - 1)
        self.pos += n
        return r

    def symbol(self, codes):
        code = 0
        for n in range(1, 17):
            code = code << 1 | self.take(1)
            if (n, code) in codes:
                return codes[(n, code)]
        raise BadJpeg("no code matches")

    def value(self, n):
        v = self.take(n)
        return v if n == 0 or v >> (n - 1) else v - (1 << n) + 1


def _idct(blocks):
    """jpeg_idct_islow on dequantised blocks [n, 8, 8] (rows v, columns u) -> samples 0 .. 255"""
    def pass1d(x, shift):   # along axis 1
        i = [x[:, k] for k in range(8)]
        z1 = (i[2] + i[6]) * 4433
        t2 = z1 - i[6] * 15137; t3 = z1 + i[2] * 6270
        t0 = (i[0] + i[4]) << 13; t1 = (i[0] - i[4]) << 13
        t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
        a0, a1, a2, a3 = i[7], i[5], i[3], i[1]
        z1 = a0 + a3; z2 = a1 + a2; z3 = a0 + a2; z4 = a1 + a3
        z5 = (z3 + z4) * 9633
        a0 = a0 * 2446; a1 = a1 * 16819; a2 = a2 * 25172; a3 = a3 * 12299
        z1 = z1 * -7373; z2 = z2 * -20995; z3 = z3 * -16069 + z5; z4 = z4 * -3196 + z5
        a0 = a0 + z1 + z3; a1 = a1 + z2 + z4; a2 = a2 + z2 + z3; a3 = a3 + z1 + z4
        o = [t10 + a3, t11 + a2, t12 + a1, t13 + a0, t13 - a0, t12 - a1, t11 - a2, t10 - a3]
        return (np.stack(o, axis=1) + (1 << (shift - 1))) >> shift
    w = pass1d(blocks.astype(np.int64), 11)                                # columns: axis 1 is v
    s = pass1d(w.transpose(0, 2, 1), 18).transpose(0, 2, 1)                # rows: axis 1 is u after the transpose
    return np.clip(s + 128, 0, 255)


def _upsample(p, hs, vs, W, H):
    """a component's own-size plane -> W x H by libjpeg's fancy filters"""
    p = p.astype(np.int64)
    if hs == 1 and vs == 1:
        return p[:H, :W]
    if vs == 2:
        up = np.concatenate([p[:1], p[:-1]]); dn = np.concatenate([p[1:], p[-1:]])
        c = np.empty((2 * p.shape[0], p.shape[1]), np.int64)
        c[0::2] = 3 * p + up; c[1::2] = 3 * p + dn
        lf = np.concatenate([c[:, :1], c[:, :-1]], axis=1); rt = np.concatenate([c[:, 1:], c[:, -1:]], axis=1)
        o = np.empty((c.shape[0], 2 * c.shape[1]), np.int64)
        o[:, 0::2] = (3 * c + lf + 8) >> 4; o[:, 1::2] = (3 * c + rt + 7) >> 4
        return o[:H, :W]
    lf = np.concatenate([p[:, :1], p[:, :-1]], axis=1); rt = np.concatenate([p[:, 1:], p[:, -1:]], axis=1)
    o = np.empty((p.shape[0], 2 * p.shape[1]), np.int64)
    o[:, 0::2] = (3 * p + lf + 1) >> 2; o[:, 1::2] = (3 * p + rt + 2) >> 2
    return o[:H, :W]


def decode(data):
    d = bytes(data)
    frame, q, h, dri, tabs, at = _headers(d)
    _need(d[-2:] == b"\xff\xd9", "no EOI")
    W, H, comps = frame["width"], frame["height"], frame["comps"]
    _need(len(comps) in (1, 3), "components")
    hs, vs = (comps[0][1], comps[0][2]) if len(comps) == 3 else (1, 1)
    if len(comps) == 3:
        _need((hs, vs) in ((1, 1), (2, 1), (2, 2)) and comps[1][1:3] == (1, 1) and comps[2][1:3] == (1, 1), "sampling")
    body = d[at:-2]
    segs, cur, i, stuffed = [], bytearray(), 0, 0
    while i < len(body):
        if body[i] != 0xFF:
            cur.append(body[i]); i += 1
        elif i + 1 < len(body) and body[i + 1] == 0:
            cur.append(0xFF); stuffed += 1; i += 2
        else:
            _need(i + 1 < len(body) and body[i + 1] == 0xD0 + (len(segs) & 7), "marker in the entropy data at %d" % i)
            segs.append(bytes(cur)); cur = bytearray(); i += 2
    segs.append(bytes(cur))
    mw, mh = -(-W // (8 * hs)), -(-H // (8 * vs))
    slots = [0] * (hs * vs) + [1, 2] if len(comps) == 3 else [0]
    interval = dri or mw * mh
    _need(len(segs) == -(-(mw * mh) // interval), "segment count")
    blocks = []
    for k, seg in enumerate(segs):
        b = _Bits(seg); pred = [0, 0, 0]
        for _ in range(min(interval, mw * mh - k * interval)):
            for c in slots:
                co = [0] * 64
                pred[c] += b.value(b.symbol(h[(0, tabs[c][0])])); co[0] = pred[c]
                j = 1
                while j < 64:
                    rs = b.symbol(h[(1, tabs[c][1])]); r, n = rs >> 4, rs & 15
                    if n == 0:
                        if r != 15:
                            break
                        j += 16
                        continue
                    j += r
                    _need(j < 64, "run past the block")
                    co[ZIGZAG[j]] = b.value(n); j += 1
                blocks.append(co)
            _need(b.pos <= b.n, "segment too short")
    coef = np.array(blocks, np.int64).reshape(-1, 64)
    qc = np.stack([q[comps[c][3]] for c in slots] * (mw * mh))
    samples = _idct((coef * qc).reshape(-1, 8, 8)).reshape(mh, mw, len(slots), 8, 8)
    luma = samples[:, :, :hs * vs].reshape(mh, mw, vs, hs, 8, 8).transpose(0, 2, 4, 1, 3, 5).reshape(mh * vs * 8, mw * hs * 8)
    out = dict(coefficients=coef, width=W, height=H, sampling=(hs, vs), components=len(comps), restart_interval=dri, segments=len(segs), stuffed_bytes=stuffed, entropy=body)
    if len(comps) == 1:
        out["rgb"] = np.repeat(luma[:H, :W, None], 3, axis=2).astype(np.uint8)
        return out
    cw, ch = -(-W // hs), -(-H // vs)
    cb, cr = [_upsample(samples[:, :, hs * vs + k].transpose(0, 2, 1, 3).reshape(mh * 8, mw * 8)[:ch, :cw], hs, vs, W, H) - 128 for k in (0, 1)]
    y = luma[:H, :W]
    rgb = np.stack([y + ((91881 * cr + 32768) >> 16), y + ((-22554 * cb - 46802 * cr + 32768) >> 16), y + ((116130 * cb + 32768) >> 16)], axis=2)
    out["rgb"] = np.clip(rgb, 0, 255).astype(np.uint8)
    return out


# ---- the files the tests share ----
def picture(h, w, noise=0.0, seed=7):
    """smooth content, plus gaussian noise of sigma `noise`"""
    rs = np.random.RandomState(seed + 1000 * h + w)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    g = np.stack([128 + 100 * np.sin(x / 9.0 + y / 23.0), 128 + 90 * np.cos(y / 7.0 - x / 31.0), 40 + 170 * (x + y) / max(h + w - 2, 1)], -1)
    return np.clip(np.rint(g + noise * rs.randn(h, w, 3)), 0, 255).astype(np.uint8)


def idct_paths_image():
    """black and white noise under a smooth strip: at quality 100 its blocks' dequantised magnitudes sum to more than 5400 (the 64-bit IDCT
    of jpeg_dec.h) and to less (the 32-bit one)"""
    img = np.repeat((np.random.RandomState(5).randint(0, 2, (24, 40)) * 255).astype(np.uint8)[:, :, None], 3, axis=2)
    img[:8] = picture(8, 40)
    return img


def pillow_file(img, **kw):
    import io
    from PIL import Image
    f = io.BytesIO()
    Image.fromarray(img).save(f, "JPEG", **kw)
    return f.getvalue()


def pillow_decode(data):
    import io
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


SIZES = ((1, 1), (5, 7), (8, 8), (130, 9), (16, 16), (33, 17), (50, 35), (48, 64))   # (H, W): 1x1, 7x5, 8x8, 9x130, 16x16, 17x33, 35x50, 64x48


def pillow_cases():
    """name -> file: every size x subsampling x quality x optimize x content; then restart markers and grayscale"""
    out = {}
    for (h, w) in SIZES:
        for sub in (0, 1, 2):
            for q in (30, 90, 100):
                for opt in (False, True):
                    for noise in (0.0, 40.0):
                        out["%dx%d_s%d_q%d_o%d_n%d" % (w, h, sub, q, int(opt), int(noise))] = pillow_file(picture(h, w, noise), quality=q, subsampling=sub, optimize=opt)
    for sub in (0, 1, 2):
        out["rst_blocks3_s%d" % sub] = pillow_file(picture(50, 35, 40.0), quality=90, subsampling=sub, restart_marker_blocks=3)
        out["rst_rows1_s%d" % sub] = pillow_file(picture(48, 64, 40.0), quality=90, subsampling=sub, restart_marker_rows=1)
    for (h, w) in ((1, 1), (33, 17), (48, 64)):
        out["gray_%dx%d" % (w, h)] = pillow_file(picture(h, w, 20.0)[:, :, 1], quality=90)
    out["gray_rst"] = pillow_file(picture(50, 35, 40.0)[:, :, 0], quality=100, restart_marker_blocks=3)
    return out


# ---- files that must be refused: (file, the reason the message must contain) ----
def _segments(d):
    """[(marker, offset of its FF, total length with the marker)] of the markers in front of the entropy data"""
    out, at = [], 2
    while True:
        m, n = d[at + 1], d[at + 2] << 8 | d[at + 3]
        out.append((m, at, n + 2))
        at += n + 2
        if m == 0xDA:
            return out


def _pack(bits):
    """a string of '0' / '1' as entropy data: padded with 1 bits, stuffed"""
    bits += "1" * (-len(bits) % 8)
    raw = int(bits, 2).to_bytes(len(bits) // 8, "big") if bits else b""
    return raw.replace(b"\xff", b"\xff\x00")


def _crafted(width, symbols_per_block, blocks):
    """a grayscale file of `width` x 8 with Annex K's tables (a Pillow file, optimize off) whose entropy data is `blocks` times the
    (class, symbol, value bits) triples of symbols_per_block"""
    base = pillow_file(picture(8, width)[:, :, 0], quality=90)
    _, _, h, _, tabs, at = _headers(base)
    enc = {cls: {sym: format(code, "0%db" % n) for (n, code), sym in h[(cls, tabs[0][cls])].items()} for cls in (0, 1)}
    bits = "".join(enc[cls][sym] + val for cls, sym, val in symbols_per_block) * blocks
    return base[:at] + _pack(bits) + b"\xff\xd9"


def refusals():
    """name -> (file, reason)"""
    import io
    from PIL import Image
    img = picture(48, 64, 20.0)
    good = pillow_file(img, quality=90, subsampling=2)
    segs = _segments(good)
    at = segs[-1][1] + segs[-1][2]                                   # the entropy data's first byte
    out = {}
    out["progressive"] = (pillow_file(img, quality=90, progressive=True), "SOF2")
    f = io.BytesIO(); Image.fromarray(img).convert("CMYK").save(f, "JPEG"); out["cmyk"] = (f.getvalue(), "4 components")
    sof = [s for s in segs if s[0] == 0xC0][0][1]
    b = bytearray(good); b[sof + 4] = 12; out["precision_12"] = (bytes(b), "precision")
    b = bytearray(good); b[sof + 11] = 0x12; out["sampling_440"] = (bytes(b), "luma sampling 1x2")
    dht = [s for s in segs if s[0] == 0xC4]
    out["dht_removed"] = (good[:dht[-1][1]] + good[dht[-1][1] + dht[-1][2]:], "no DHT defined")
    b = bytearray(good); o = dht[0][1] + 5                            # the first table's counts: three codes of one bit, three fewer further on
    k = max(range(16), key=lambda i: b[o + i]); b[o] += 3; b[o + k] -= 3
    out["dht_overfull"] = (bytes(b), "more codes than its lengths allow")
    out["cut_tail"] = (good[:len(good) * 2 // 3], "truncated")
    out["no_eoi"] = (good[:-2], "no EOI")
    out["cut_in_headers"] = (good[:sof + 6], "truncated")
    b = bytearray(good); b[at + 40:at + 42] = b"\xff\xda"; out["second_scan"] = (bytes(b), "a second scan")
    b = bytearray(good); b[at + 40:at + 42] = b"\xff\xdc"; out["dnl"] = (bytes(b), "DNL")
    b = bytearray(good); b[at + 40:at + 42] = b"\xff\xc4"; out["marker_inside"] = (bytes(b), "marker other than RSTn")
    rst = pillow_file(img, quality=90, subsampling=2, restart_marker_blocks=2)
    marks = [i for i in range(len(rst) - 1) if rst[i] == 0xFF and 0xD0 <= rst[i + 1] <= 0xD7]
    b = bytearray(rst); b[marks[1] + 1], b[marks[2] + 1] = b[marks[2] + 1], b[marks[1] + 1]
    out["rst_swapped"] = (bytes(b), "restart marker out of sequence")
    out["rst_removed"] = (rst[:marks[3]] + rst[marks[3] + 2:], "restart marker out of sequence")   # (the ones behind it no longer count up)
    out["rst_one_more"] = (pillow_file(img[:16, :32], quality=90, subsampling=2, restart_marker_blocks=1)[:-2] + b"\xff\xd1\xff\xd9", "number of restart segments")
    app14 = b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00\x00"
    out["adobe_rgb"] = (good[:2] + app14 + good[2:], "transform 0")
    # an entropy byte changed so that a code becomes invalid: all ones is no code of Annex K's tables (optimize off)
    plain = pillow_file(img, quality=90, subsampling=0)
    ps = _segments(plain); pa = ps[-1][1] + ps[-1][2]
    b = bytearray(plain); b[pa + 30:pa + 36] = b"\xff\x00\xff\x00\xff\x00"
    out["invalid_code"] = (bytes(b), "prefix that no code matches")
    out["run_past_63"] = (_crafted(8, [(0, 0, "")] + [(1, 0xF1, "1")] * 5, 1), "run past coefficient 63")
    out["dc_outside_int16"] = (_crafted(8 * 17, [(0, 11, "1" * 11), (1, 0x00, "")], 17), "DC value outside int16")
    out["segment_incomplete"] = (_crafted(8 * 4, [(0, 3, "101"), (1, 0x00, "")], 2), "before its blocks are complete")
    return out
