"""ctypes driver of the CPU model of row f8 (atlas_model.cpp; DESIGN.md section 4 "Texture atlases"), plus numpy statements of the
order-free rules the device uses: the packing loop as "the first remaining patch after the cursor that fits" (item 4) and the edge
padding as levels of chessboard distance (item 7).  Built on first use with g++ -O2 -mfma -ffp-contract=off -fno-fast-math.  Test
infrastructure only."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "atlas_model.cpp")
LIB = os.path.join(HERE, "libatlas_model.so")
PATCH_ARRAYS = {"box": np.int32, "face_ptr": np.uint32, "faces": np.uint32, "texcoords": np.float32, "pix_ptr": np.uint64, "image": np.float32,
                "validity": np.uint8}
ARRAYS = {"atlas_size": np.uint32, "atlas_pix_ptr": np.uint64, "image": np.uint8, "patch_atlas": np.uint32, "patch_pos": np.int32, "patch_order": np.uint32,
          "face_ptr": np.uint32, "faces": np.uint32, "texcoords": np.float32, "tc_ptr": np.uint32, "texcoords_merged": np.float32, "texcoord_ids": np.uint32}
PACK_ARRAYS = ("atlas_size", "atlas_pix_ptr", "patch_atlas", "patch_pos", "patch_order")
# mvs_atlas_stats' counters in order (viewsel.ATLAS_COUNTS)
STATS = ("atlases", "atlases_256", "atlases_512", "atlases_1024", "atlases_2048", "atlases_4096", "atlases_8192", "pixels", "valid_pixels", "padded_pixels",
         "free_rects_peak", "merged_texcoords")
COUNTERS = ("pref_jumps", "halvings", "breaks", "break_is_widest", "waits_too_wide", "ties", "refused_inserts", "foreign_fill", "outer_ring", "wrapped_area")
SIZES = (256, 512, 1024, 2048, 4096, 8192)
UNSUPPORTED = 7
_lib = None


def build(force=False):
    if force or not os.path.exists(LIB) or os.path.getmtime(LIB) < os.path.getmtime(SRC):
        subprocess.check_call(["g++", "-O2", "-mfma", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-std=c++17", "-shared", "-o", LIB, SRC])
    return LIB


def load():
    global _lib
    if _lib is None:
        L = C.CDLL(build())
        vp = C.c_void_p
        L.atlas_model_run.restype = vp
        L.atlas_model_run.argtypes = [C.c_uint32] + [vp] * 7 + [C.c_int]
        L.atlas_model_status.argtypes = [vp]; L.atlas_model_status.restype = C.c_int
        L.atlas_model_stats.argtypes = [vp, vp, vp, vp]
        L.atlas_model_array.argtypes = [vp, C.c_char_p, C.POINTER(C.c_uint64)]; L.atlas_model_array.restype = vp
        L.atlas_model_free.argtypes = [vp]
        L.atlas_model_bin.argtypes = [C.c_uint32, C.c_uint32, vp, vp]; L.atlas_model_bin.restype = None
        _lib = L
    return _lib


def flat(patches):
    """a patch set (the library's or a crafted dict) as flat contiguous arrays of the right types"""
    return {k: np.ascontiguousarray(patches[k], dt).reshape(-1) for k, dt in PATCH_ARRAYS.items()}


def set_from_sizes(wh):
    """a patch set of the given (w, h) list: one face per patch (its id) whose corners are (0, 0), (w, 0), (0, h); black, all valid"""
    wh = np.asarray(wh, np.int64).reshape(-1, 2)
    n = len(wh)
    box = np.zeros((n, 4), np.int32); box[:, 2:] = wh
    pix_ptr = np.zeros(n + 1, np.uint64); pix_ptr[1:] = np.cumsum(wh[:, 0] * wh[:, 1])
    tc = np.zeros((n, 3, 2), np.float32); tc[:, 1, 0] = wh[:, 0]; tc[:, 2, 1] = wh[:, 1]
    return dict(box=box, face_ptr=np.arange(n + 1, dtype=np.uint32), faces=np.arange(n, dtype=np.uint32), texcoords=tc, pix_ptr=pix_ptr,
                image=np.zeros(0, np.float32), validity=np.zeros(0, np.uint8))


def run(patches, pack_only=False):
    """(status, arrays, stats, counters, (ms_pack, ms_total)): status 7 = MVS_ERR_UNSUPPORTED (the rest None).  pack_only: items 1 - 4 alone
    (image / validity are not read)."""
    L = load()
    a = flat(patches)
    NP = a["box"].size // 4
    if NP == 0:
        a["pix_ptr"] = np.zeros(1, np.uint64); a["face_ptr"] = np.zeros(1, np.uint32)
    ptr = lambda x: x.ctypes.data if x.size else None
    h = L.atlas_model_run(NP, *[ptr(a[k]) for k in PATCH_ARRAYS], 1 if pack_only else 0)
    try:
        st = L.atlas_model_status(h)
        if st:
            return st, None, None, None, None
        out = {}
        for name, dt in ARRAYS.items():
            n = C.c_uint64()
            p = L.atlas_model_array(h, name.encode(), C.byref(n))
            out[name] = np.frombuffer(C.string_at(p, n.value * np.dtype(dt).itemsize), dt).copy() if n.value else np.zeros(0, dt)
        s = (C.c_uint64 * len(STATS))(); c = (C.c_uint64 * len(COUNTERS))(); ms = (C.c_double * 2)()
        L.atlas_model_stats(h, s, c, ms)
        return 0, out, dict(zip(STATS, [int(x) for x in s])), dict(zip(COUNTERS, [int(x) for x in c])), (float(ms[0]), float(ms[1]))
    finally:
        L.atlas_model_free(h)


def bin_insert(size, wh):
    """item 3 alone: the (w, h) list offered in order to one bin -> (n, 3) placed, min_x, min_y"""
    wh = np.ascontiguousarray(wh, np.int32).reshape(-1, 2)
    out = np.zeros((len(wh), 3), np.int32)
    load().atlas_model_bin(int(size), len(wh), wh.ctypes.data, out.ctypes.data)
    return out


def atlas_view(arrays, a):
    s = int(arrays["atlas_size"][a]); o = int(arrays["atlas_pix_ptr"][a])
    return np.asarray(arrays["image"]).reshape(-1, 3)[o:o + s * s].reshape(s, s, 3)


def craft(rng, sizes, hole=0.15, edge_valid=True, faces_per_patch=3):
    """a crafted patch set: random colours (some outside [0, 1], a NaN), validity with holes (and, with edge_valid, valid pixels on the
    frame's edges), `faces_per_patch` faces each (one number, or one per patch) whose corners repeat within the patch"""
    sizes = np.asarray(sizes, np.int64).reshape(-1, 2)
    n = len(sizes)
    per_patch = np.broadcast_to(np.asarray(faces_per_patch, np.int64), (n,))
    box = np.zeros((n, 4), np.int32); box[:, 2:] = sizes
    pix_ptr = np.zeros(n + 1, np.uint64); pix_ptr[1:] = np.cumsum(sizes[:, 0] * sizes[:, 1])
    N = int(pix_ptr[-1])
    image = rng.uniform(-0.1, 1.1, (N, 3)).astype(np.float32)
    image[rng.integers(0, N, max(1, N // 50))] = rng.integers(0, 256, (max(1, N // 50), 3)).astype(np.float32) / np.float32(255.0)
    image[rng.integers(0, N)] = np.nan
    validity = np.where(rng.random(N) < hole, 0, 255).astype(np.uint8)
    if not edge_valid:
        for p in range(n):
            w, h = sizes[p]; v = validity[int(pix_ptr[p]):int(pix_ptr[p + 1])].reshape(h, w)
            v[0, :] = 0; v[-1, :] = 0; v[:, 0] = 0; v[:, -1] = 0
    image[validity == 0] = 0
    faces, tcs, fptr = [], [], [0]
    for p in range(n):
        w, h = sizes[p]
        corners = np.stack([rng.integers(0, w + 1, 4), rng.integers(0, h + 1, 4)], 1).astype(np.float32) + rng.choice([0.0, 0.5, 0.25], (4, 2)).astype(np.float32)
        for k in range(int(per_patch[p])):
            faces.append(len(faces))
            tcs.append(corners[[k % 4, (k + 1) % 4, (k + 2) % 4]])
        fptr.append(len(faces))
    return dict(box=box, face_ptr=np.asarray(fptr, np.uint32), faces=np.asarray(faces, np.uint32)[::-1].copy(), texcoords=np.asarray(tcs, np.float32).reshape(-1),
                pix_ptr=pix_ptr, image=image.reshape(-1), validity=validity)


# ---- the order-free rules in numpy ----

def rule_texture_size(w, h):
    """item 2 on the remaining patches in order, 32-bit unsigned arithmetic by masks"""
    w = np.asarray(w, np.int64); h = np.asarray(h, np.int64)
    M = 0xFFFFFFFF
    size = 8192
    while True:
        pad = size >> 7
        W = w + 2 * pad; H = h + 2 * pad
        area = (W * H) & M
        waste = (area - w * h) & M
        brk = waste > w * h                                      # waste / size > 1.0 in double: both are integers below 2^32
        b = int(np.argmax(brk)) if brk.any() else len(w)
        upto = min(b + 1, len(w))
        max_w = int(W[:upto].max()); max_h = int(H[:upto].max())
        total = int(area[:b].sum()) & M
        assert max_w < 8192 and max_h < 8192
        if size > 4096 and max_w < 4096 and max_h < 4096 and total // (4096 * 4096) < 8:
            size = 4096; continue
        if size <= 256:
            return 256
        if max_h < size // 2 and max_w < size // 2 and total / float(size * size) < 0.2:
            size //= 2; continue
        return size


def rule_pack(wh):
    """items 1 - 4 in their order-free form -> atlas_size, patch_atlas, patch_pos (n, 2), patch_order"""
    wh = np.asarray(wh, np.int64).reshape(-1, 2)
    n = len(wh)
    ids = np.arange(n)[::-1]
    order = ids[np.argsort(-(wh[ids, 0] * wh[ids, 1]), kind="stable")]
    remaining = list(order)
    atlas_size, patch_atlas, patch_pos, patch_order = [], np.zeros(n, np.uint32), np.zeros((n, 2), np.int32), []
    f32 = np.float32
    while remaining:
        rem = np.asarray(remaining)
        size = rule_texture_size(wh[rem, 0], wh[rem, 1]); pad = size >> 7
        W = wh[rem, 0] + 2 * pad; H = wh[rem, 1] + 2 * pad
        free = [(0, 0, size, size)]
        placed = np.zeros(len(rem), bool)
        cursor = 0
        while True:
            fr = np.asarray(free, np.int64).reshape(-1, 4)
            fw = fr[:, 2] - fr[:, 0]; fh = fr[:, 3] - fr[:, 1]
            j = -1
            for base in range(cursor, len(rem), 512):            # the first patch after the cursor that fits any free rectangle
                sl = slice(base, min(base + 512, len(rem)))
                fits = ((W[sl, None] <= fw[None, :]) & (H[sl, None] <= fh[None, :])).any(1)
                if fits.any():
                    j = base + int(np.argmax(fits)); break
            if j < 0:
                break
            ok = (W[j] <= fw) & (H[j] <= fh)
            score = np.where(ok, (fw * fh - W[j] * H[j]) & 0xFFFFFFFF, 1 << 40)
            r = int(np.argmin(score))                             # the first minimum in list order
            bx0, by0, bx1, by1 = free.pop(r)
            x1, y1 = bx0 + int(W[j]), by0 + int(H[j])
            area = lambda q: (q[2] - q[0]) * (q[3] - q[1])
            h_top, h_bottom = (bx0, y1, bx1, by1), (x1, by0, bx1, y1)
            v_left, v_right = (bx0, y1, x1, by1), (x1, by0, bx1, by1)
            hr = f32(area(h_top)) / f32(area(h_bottom)) if area(h_top) and area(h_bottom) else f32(1)
            vr = f32(area(v_left)) / f32(area(v_right)) if area(v_left) and area(v_right) else f32(1)
            for q in ((v_left, v_right) if abs(f32(1) - hr) < abs(f32(1) - vr) else (h_top, h_bottom)):
                if area(q):
                    free.append(q)
            p = int(rem[j])
            patch_atlas[p] = len(atlas_size); patch_pos[p] = (bx0, by0); patch_order.append(p); placed[j] = True
            cursor = j + 1
        assert placed.any()
        atlas_size.append(size)
        remaining = [int(p) for p, d in zip(rem, placed) if not d]
    return np.asarray(atlas_size, np.uint32), patch_atlas, patch_pos, np.asarray(patch_order, np.uint32)


def _shift(a, i, j, fill):
    """b[y, x] = a[y + j, x + i], `fill` outside"""
    h, w = a.shape[:2]
    b = np.full_like(a, fill)
    ys = slice(max(0, -j), min(h, h - j)); xs = slice(max(0, -i), min(w, w - i))
    yd = slice(max(0, j), min(h, h + j)); xd = slice(max(0, i), min(w, w + i))
    b[ys, xs] = a[yd, xd]
    return b


def rule_pad(image, mask, padding):
    """item 7 in its level form: image (s, s, 3) uint8 and mask (s, s) after composition -> (padded image, levels); level 0 = valid at the
    start, d = filled in iteration d - 1 from the neighbours of lower level, 255 = never.  Level d is looked for among the neighbours of
    level d - 1 only (index lists, not whole-image passes: an atlas of 8192 has 65 levels)."""
    mask = np.asarray(mask, np.uint8)
    h, w = mask.shape
    img = np.zeros((h + 2, w + 2, 3), np.uint8); img[1:-1, 1:-1] = np.asarray(image, np.uint8)    # a border of level 255: never read
    lev = np.full((h + 2, w + 2), 255, np.int64); lev[1:-1, 1:-1] = np.where(mask == 255, 0, 255)
    open_ = np.zeros((h + 2, w + 2), bool)
    f32 = np.float32
    nbrs = [(i, j) for j in (-1, 0, 1) for i in (-1, 0, 1)]                                       # j outer, i inner
    gauss = {(i, j): f32((2 - abs(i)) * (2 - abs(j))) / f32(16) for i, j in nbrs}
    ys, xs = np.nonzero(lev == 0)
    for d in range(1, padding + 2):
        open_[1:-1, 1:-1] = (lev[1:-1, 1:-1] == 255) & ((mask != 255) if d == 1 else (mask == 0))
        cy = np.concatenate([ys + j for i, j in nbrs]); cx = np.concatenate([xs + i for i, j in nbrs])
        keep = open_[cy, cx]
        flat = np.unique(cy[keep] * (w + 2) + cx[keep])
        if not len(flat):
            break
        ys, xs = flat // (w + 2), flat % (w + 2)
        norm = np.zeros(len(flat), f32); value = np.zeros((len(flat), 3), f32)
        for i, j in nbrs:
            ok = lev[ys + j, xs + i] < d
            wgt = gauss[(i, j)]
            norm = np.where(ok, norm + wgt, norm)
            px = img[ys + j, xs + i].astype(f32) / f32(255.0)
            value = np.where(ok[:, None], value + px * wgt, value)
        img[ys, xs] = ((value / norm[:, None]) * f32(255.0)).astype(np.uint8)
        lev[ys, xs] = d
    return img[1:-1, 1:-1], lev[1:-1, 1:-1]


def compose(patches, arrays, a):
    """items 5 alone for atlas a: (image (s, s, 3) uint8, mask (s, s)) before the padding, from the placement in `arrays`"""
    P = flat(patches)
    s = int(arrays["atlas_size"][a]); pad = s >> 7
    img = np.zeros((s, s, 3), np.uint8); mask = np.zeros((s, s), np.uint8)
    box = P["box"].reshape(-1, 4); pos = np.asarray(arrays["patch_pos"]).reshape(-1, 2)
    f32 = np.float32
    for p in np.flatnonzero(np.asarray(arrays["patch_atlas"]) == a):
        w, h = int(box[p, 2]), int(box[p, 3]); o = int(P["pix_ptr"][p])
        src = P["image"].reshape(-1, 3)[o:o + w * h].reshape(h, w, 3)
        with np.errstate(invalid="ignore"):
            v = np.where(src > f32(0), src, f32(0)); v = np.where(v < f32(1), v, f32(1))      # std::max(0, x) then std::min(1, .): a NaN becomes 0
            q = ((f32(255.0) * v) / f32(1.0) + f32(0.5)).astype(np.uint8)
        x0, y0 = int(pos[p, 0]) + pad, int(pos[p, 1]) + pad
        img[y0:y0 + h, x0:x0 + w] = q
        mask[y0:y0 + h, x0:x0 + w] = P["validity"][o:o + w * h].reshape(h, w)
    return img, mask
