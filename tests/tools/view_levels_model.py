"""Pyramid levels of the view input (DESIGN.md section 4 "View input" item 14), restated in numpy for the tests -- independently of
csrc/level.h: the clamp x1 = min(2x + 1, w - 1) is an edge-replicating pad to an even size, the 2 x 2 mean four strided slices."""
import numpy as np


def level_size(w, h, level):
    for _ in range(level):
        w, h = (w + 1) >> 1, (h + 1) >> 1
    return w, h


def half(img):
    """one level: (H, W[, C]) uint8 -> ((H + 1) // 2, (W + 1) // 2[, C]), (sum of the clamped 2 x 2 block + 2) >> 2"""
    h, w = img.shape[:2]
    pad = ((0, h & 1), (0, w & 1)) + ((0, 0),) * (img.ndim - 2)
    p = np.pad(img, pad, mode="edge").astype(np.uint32)
    return ((p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + 2) >> 2).astype(np.uint8)


def halve(img, level):
    """level k: half applied k times, the bytes rounded at every level"""
    for _ in range(level):
        img = half(img)
    return np.ascontiguousarray(img)


def one_shot(img, level):
    """what level k is NOT: the clamped 2^k x 2^k block summed once and divided once"""
    n = 1 << level
    h, w = img.shape[:2]
    wl, hl = level_size(w, h, level)
    ys = np.minimum(np.arange(hl * n), h - 1); xs = np.minimum(np.arange(wl * n), w - 1)
    p = img[ys][:, xs].astype(np.uint32).reshape((hl, n, wl, n) + img.shape[2:])
    return ((p.sum(axis=(1, 3)) + (n * n) // 2) // (n * n)).astype(np.uint8)


def keep_level(mask, level):
    """the keep rule: an (H, W) mask (0 = leave out) -> bool at the level; a level pixel is kept iff every source pixel of its clamped
    2^k x 2^k block is kept, level by level"""
    m = np.asarray(mask) != 0
    for _ in range(level):
        h, w = m.shape
        p = np.pad(m, ((0, h & 1), (0, w & 1)), mode="edge")
        m = p[0::2, 0::2] & p[0::2, 1::2] & p[1::2, 0::2] & p[1::2, 1::2]
    return m
