// debug_embed.h -- row f10: the images of the view-selection debug model (generate_debug_embeddings.cpp), written once for host and
//   device (DESIGN.md section 4 "Debug model").  A view's image is a flat colour of its own -- colour (position % 144) of an HSV
//   sweep -- stamped all over with its three-digit id in cells of 13 x 6 pixels.  The colour table is built ON THE HOST, in fp32 and in
//   upstream's operation order (debug_style_table), and handed to the kernels as data: 60 of its 144 colours have a channel one ulp
//   below an integer before the truncation to a byte, so any other order of the same arithmetic changes bytes.  debug_pixel is the
//   stamp: glyph or background for one pixel, from divisions by the two cell sizes alone.  Plain header, no dependency: the tests
//   compile the host side with g++ (tests/test_debug_embeddings.py).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define DBG_HD __host__ __device__ inline
#else
#define DBG_HD inline
#endif

namespace mvs {

constexpr int DEBUG_COLOURS = 144;        // 3 saturations x 4 values x 12 hues
constexpr int DEBUG_CELL_W = 13, DEBUG_CELL_H = 6;
constexpr uint32_t DEBUG_MAX_ID = 999;    // three digits (upstream asserts digit <= 9 and would read past its font)

// background bytes r, g, b in bits 0 - 23, the font byte (0 or 255, all three channels) in bits 24 - 31
DBG_HD uint32_t debug_style_pack(uint8_t r, uint8_t g, uint8_t b, uint8_t font) { return (uint32_t)r | (uint32_t)g << 8 | (uint32_t)b << 16 | (uint32_t)font << 24; }

// generate_debug_colors (generate_debug_embeddings.cpp:41-69) and the font colour (:82-83), host only.  `s -= 0.4` and `v -= 0.3`
// are double subtractions rounded back to float, as upstream writes them; luminance = (r*0.30f + g*0.59f) + b*0.11f is DEFINED HERE
// (math::interpolate is MVE's) and decides nothing: no colour is closer than 0.01 to 0.5.  lum (may be null): the 144 luminances.
inline void debug_style_table(uint32_t style[DEBUG_COLOURS], float* lum = nullptr, float* prod = nullptr /* [3 * 144]: channel * 255.0f before the truncation */) {
    int n = 0;
    for (float s = 1.0f; s > 0.0f; s -= 0.4) {
        for (float v = 1.0f; v > 0.0f; v -= 0.3) {
            for (float h = 0.0f; h < 360.0f; h += 30.0f) {
                const float c = v * s;
                const float x = c * (1.0f - fabsf(fmodf(h / 60.0f, 2.0f) - 1.0f));
                const float m = v - c;
                float r = 0.0f, g = 0.0f, b = 0.0f;
                if (h < 60.0f) { r = c; g = x; }
                else if (h < 120.0f) { r = x; g = c; }
                else if (h < 180.0f) { g = c; b = x; }
                else if (h < 240.0f) { g = x; b = c; }
                else if (h < 300.0f) { r = x; b = c; }
                else { r = c; b = x; }
                r = r + m; g = g + m; b = b + m;
                const float l = (r * 0.30f + g * 0.59f) + b * 0.11f;
                const float pr = r * 255.0f, pg = g * 255.0f, pb = b * 255.0f;
                if (n < DEBUG_COLOURS) {
                    style[n] = debug_style_pack((uint8_t)pr, (uint8_t)pg, (uint8_t)pb, l > 0.5f ? 0 : 255);
                    if (lum) lum[n] = l;
                    if (prod) { prod[3 * n] = pr; prod[3 * n + 1] = pg; prod[3 * n + 2] = pb; }
                }
                ++n;
            }
        }
    }
}

// the ten 3 x 5 glyphs, one 15-bit word per digit: bit 3 * row + column (row 0 on top, column 0 on the left)
DBG_HD uint32_t debug_glyph(uint32_t digit) {
    switch (digit) {
        case 0: return 0x2b6au; case 1: return 0x749au; case 2: return 0x72a3u; case 3: return 0x38a3u; case 4: return 0x49e9u;
        case 5: return 0x38cfu; case 6: return 0x2acau; case 7: return 0x2527u; case 8: return 0x2aaau; default: return 0x29aau;
    }
}
// the three glyph words of an id (<= DEBUG_MAX_ID), hundreds in bits 0 - 14, tens in 15 - 29, ones in 30 - 44
DBG_HD uint64_t debug_id_glyphs(uint32_t id) {
    return (uint64_t)debug_glyph(id / 100u) | (uint64_t)debug_glyph((id % 100u) / 10u) << 15 | (uint64_t)debug_glyph(id % 10u) << 30;
}
// pixel (x, y) of a w x h image stamped with the glyphs `g` of its id: true = font colour, false = background.  Cells start at
// ox = 13 i while ox < w - 13 and oy = 6 j while oy < h - 6; digit k occupies columns 4 k .. 4 k + 2 and rows 0 .. 4 of a cell.
DBG_HD bool debug_pixel_glyphs(int x, int y, int w, int h, uint64_t g) {
    const int cx = x / DEBUG_CELL_W, rx = x % DEBUG_CELL_W, cy = y / DEBUG_CELL_H, ry = y % DEBUG_CELL_H;
    if (cx * DEBUG_CELL_W >= w - DEBUG_CELL_W || cy * DEBUG_CELL_H >= h - DEBUG_CELL_H) return false;   // no cell starts here
    if (ry == 5 || rx >= 11 || (rx & 3) == 3) return false;                                              // the gaps of a cell
    return (g >> (15 * (rx >> 2) + 3 * ry + (rx & 3))) & 1u;
}
DBG_HD bool debug_pixel(int x, int y, int w, int h, uint32_t id) { return debug_pixel_glyphs(x, y, w, h, debug_id_glyphs(id)); }

// what the kernels read per image: its size, its id and its colour (position % 144)
struct DebugView { int32_t width, height; uint32_t id, colour; };

// the whole image on the host (the tests' handle on this header; the library's images come from k_debug.hip)
inline void debug_image_host(int w, int h, uint32_t id, uint32_t position, uint8_t* rgb) {
    uint32_t style[DEBUG_COLOURS];
    debug_style_table(style);
    const uint32_t st = style[position % DEBUG_COLOURS];
    const uint8_t font = (uint8_t)(st >> 24);
    const uint64_t g = debug_id_glyphs(id);
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            const bool on = debug_pixel_glyphs(x, y, w, h, g);
            for (int c = 0; c < 3; ++c) rgb[((size_t)y * w + x) * 3 + c] = on ? font : (uint8_t)(st >> (8 * c));
        }
}

}  // namespace mvs
