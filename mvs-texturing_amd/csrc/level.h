// level.h -- view input: pyramid levels (DESIGN.md section 4 "View input" item 14), the arithmetic stated ONCE for the host and the
// device: level_kernel and keep_level_kernel (k_level.hip) and the sequential host twin below.
//   DEFINED HERE from recollection of mve/image_tools.h rescale_half_size<uint8_t> (MVE is absent): the destination of a w x h image is
//   (w + 1) / 2 x (h + 1) / 2, a pixel the mean of its 2 x 2 source block, the second column / row CLAMPED to the image (x1 = min(2x + 1,
//   w - 1)), rounded as (sum + 2) >> 2 -- MVE's (unsigned char)(0.25f * sum + 0.5f) gives the same integer for every sum 0 .. 1020.  A box
//   filter: this is not rescale_half_size_gaussian.  Level k is `half` applied k times, the bytes ROUNDED AT EVERY LEVEL (one sum over
//   the 4^k block divided once is another function).  Plain integer arithmetic: the GPU and the CPU agree by construction.
//   tests/cpp/test_level.cpp runs the host side under the sanitizers.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <vector>

#include "dmath.h"

namespace mvs {

constexpr uint32_t LEVEL_MAX = 4;

MVS_HD int level_dim(int v, uint32_t level) { for (uint32_t k = 0; k < level; ++k) v = (v + 1) >> 1; return v; }
MVS_HD uint32_t half_round(uint32_t a, uint32_t b, uint32_t c, uint32_t d) { return (a + b + c + d + 2u) >> 2; }

// One `half` on a window of nw columns and nh rows whose right / lower edge is the clamp: destination row y reads the source rows
// half_row0(y) and half_row1(y, nh); r0 / r1 point at their first sample (`ch` samples per pixel); sample (x, c) of the destination row.
// The host twin calls it on whole images, the kernel on the window of one work item, whose right / lower edge is either the image's (the
// clamp is the definition's) or even (the clamp is never taken).
MVS_HD int half_row0(int y) { return 2 * y; }
MVS_HD int half_row1(int y, int nh) { return 2 * y + 1 < nh ? 2 * y + 1 : nh - 1; }
MVS_HD uint8_t half_sample(const uint8_t* r0, const uint8_t* r1, int nw, int ch, int x, int c) {
    const int x0 = 2 * x, x1 = 2 * x + 1 < nw ? 2 * x + 1 : nw - 1;
    return (uint8_t)half_round(r0[x0 * ch + c], r0[x1 * ch + c], r1[x0 * ch + c], r1[x1 * ch + c]);
}

// The keep rule of a level (a level pixel is kept iff everything that went into it is kept) in the bit domain: one step on the n words
// v[0, n) (n even or 1) of one row that is already the AND of its two source rows, bit b of word i = pixel 32 i + b, bits beyond the
// width ONE (neutral: the clamped column is x1 = x0).  ANDs neighbouring bits and compacts the even ones: v[0, max(n / 2, 1)).
MVS_HD uint32_t even_bits(uint32_t t) {   // bits 0, 2, 4 .. 30 of t -> bits 0 .. 15
    t &= 0x55555555u;
    t = (t | (t >> 1)) & 0x33333333u; t = (t | (t >> 2)) & 0x0F0F0F0Fu; t = (t | (t >> 4)) & 0x00FF00FFu; t = (t | (t >> 8)) & 0x0000FFFFu;
    return t;
}
MVS_HD uint32_t keep_half_pair(uint32_t lo, uint32_t hi) { return even_bits(lo & (lo >> 1)) | (even_bits(hi & (hi >> 1)) << 16); }

// ---- the sequential host twin ----
inline void halve_once_host(const uint8_t* in, int w, int h, int ch, uint8_t* out) {
    const int wl = (w + 1) >> 1, hl = (h + 1) >> 1;
    for (int y = 0; y < hl; ++y)
        for (int x = 0; x < wl; ++x)
            for (int c = 0; c < ch; ++c)
                out[((size_t)y * wl + x) * ch + c] = half_sample(in + (size_t)half_row0(y) * w * ch, in + (size_t)half_row1(y, h) * w * ch, w, ch, x, c);
}
// rgb [h][w][ch] -> out [level_dim(h)][level_dim(w)][ch], exactly sized
inline void halve_image_host(const uint8_t* rgb, int w, int h, int ch, uint32_t level, uint8_t* out) {
    if (level == 0) { memcpy(out, rgb, (size_t)w * h * ch); return; }
    std::vector<uint8_t> a, b;
    const uint8_t* in = rgb;
    for (uint32_t k = 1; k <= level; ++k) {
        const int wl = (w + 1) >> 1, hl = (h + 1) >> 1;
        uint8_t* to = out;
        if (k < level) { b.resize((size_t)wl * hl * ch); to = b.data(); }
        halve_once_host(in, w, h, ch, to);
        if (k < level) { a.swap(b); in = a.data(); }
        w = wl; h = hl;
    }
}

}  // namespace mvs
