// jpeg_base.h -- the JPEG route of the model output (rows f9 and f11; DESIGN.md section 4 "Model output" item 9), defined ONCE for the host
// and the device: a baseline sequential JPEG (SOF0, 8 bit, JFIF APP0, YCbCr, 4:4:4 or 4:2:0) whose every step is integer arithmetic, cut
// into restart segments of R MCUs that are coded independently of each other.
//   Shared pieces (JPEG_HD; k_jpeg.hip calls them from its kernels, the host twin below with one thread): luma() / chroma_b() / chroma_r(),
//     mcu_sample(), dct_sum() with dct_round1() / dct_round2(), quantise(), category(), dc_symbol() / ac_symbol(), put_words() / image_byte(); the tables of a
//     call (cosines, quantisers, zig-zag positions, Huffman codes) travel as one `Tables` that build_tables() fills on the host.
//   Host twin (plain sequential C++, no HIP, no library): encode_jpeg() of an RGB image -- the same bytes as the device route.  header() and
//     the constants are what the device route's framing uses.  tests/cpp/test_jpeg.cpp runs this file under the sanitizers.
//
// The format, step by step (all values int32; >> is the arithmetic shift, i.e. floor):
//   colour     Y  = ( 19595 R + 38470 G +  7471 B           + 32768) >> 16
//              Cb = (-11059 R - 21709 G + 32768 B + 8388608 + 32767) >> 16        (8388608 = 128 << 16: the chroma offset; 32767 keeps 255)
//              Cr = ( 32768 R - 27439 G -  5329 B + 8388608 + 32767) >> 16
//   sampling   4:4:4: MCU 8 x 8, blocks Y Cb Cr.  4:2:0: MCU 16 x 16, blocks Y00 Y01 Y10 Y11 Cb Cr, a chroma sample = (sum of its 2 x 2 + 2) >> 2.
//              Pixels right of / below the image repeat its last column / row.  Every sample is level-shifted by -128.
//   DCT        C[u][x] = round(8192 c(u) cos((2 x + 1) u pi / 16) / 2), c(0) = 1 / sqrt 2, c(u > 0) = 1: the table COSINE below.
//              pass 1 (rows)     t[y][u] = (sum_x C[u][x] s[y][x] +   512) >> 10        (3 fraction bits stay)
//              pass 2 (columns)  F[v][u] = (sum_y C[v][y] t[y][u] + 32768) >> 16
//              |s| <= 128 and sum |C[u][.]| <= 32136, so |sum| <= 4.2e6 in pass 1, |t| <= 4017, and |sum| <= 1.3e8 in pass 2.
//   quantiser  Annex K's two tables T, s = q < 50 ? 5000 / q : 200 - 2 q, Q = clamp((T s + 50) / 100, 1, 255);
//              coefficient = sign(F) ((|F| + Q / 2) / Q)  (nearest, ties away from zero); an AC coefficient is clamped to +-1023.
//   entropy    Annex K's four Huffman tables; DC difference by category, (run, size) symbols, ZRL per 16 zeros, EOB.
//   restarts   DRI = R MCUs in raster order.  A segment starts with DC predictions 0, ends padded with 1 bits to a whole byte, every 0xFF
//              byte of it is followed by 0x00, and every segment but the last is followed by RST(k mod 8).
//   file       SOI, APP0 (JFIF 1.01, density 1:1 without unit), DQT x2 (zig-zag order), SOF0 (the true size), DHT x4, DRI, SOS, data, EOI.
//
// R: a coefficient costs at most 16 bits of code + 10 bits of value = 26 bits (a DC difference 11 + 11 = 22), a block at most 64 x 26 =
// 1664 bits = 208 bytes, 416 when every byte is stuffed.  A 4:2:0 MCU has 6 blocks and 768 bytes of pixels.  A workgroup keeps, per MCU,
// 768 B of pixels + 384 B of samples + 768 B of pass-1 values + 792 B of coefficients (2712 B, reused for the 2496 B of stuffed output) and
// 1248 B of unstuffed output: 3960 B.  R = 8 gives 30.9 KiB + 2.7 KiB of tables + 1.6 KiB of scans = 35.2 KiB: four workgroups in a CU's
// 160 KiB, and at most 48 blocks per segment, which one wave scans.  A segment's slot is its worst case: 48 x 416 + 2 bytes (4:4:4: 24 x 416 + 2).
#pragma once
#include <stdint.h>
#include <stddef.h>
#include <string.h>
#include <string>
#include <vector>

#include "../../include/mvs_viewsel.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define JPEG_M __host__ __device__
#else
#define JPEG_M
#endif
#define JPEG_HD JPEG_M inline

namespace mvs {
namespace jpeg_base {

constexpr uint32_t R = 8;                       // MCUs per restart segment
constexpr uint32_t MAX_SIDE = 65535;            // SOF0 holds 16 bits per side
constexpr uint32_t MAX_MCU_BLOCKS = 6;
constexpr uint32_t MAX_BLOCKS = R * MAX_MCU_BLOCKS;             // blocks of a segment
constexpr uint32_t COEF_BITS = 26;                              // the longest code with its value bits
constexpr uint32_t BLOCK_BYTES = 64 * COEF_BITS / 8;            // 208: a block's worst case before stuffing
constexpr uint32_t COS_PITCH = 9;                               // row distance of the cosine table as the kernels hold it (LDS banks)
constexpr uint32_t HEADER_BYTES = 629;                          // SOI .. SOS
static_assert(MAX_BLOCKS <= 64, "one wave scans the blocks of a segment");

JPEG_HD uint32_t mcu_blocks(uint32_t sub) { return sub ? 6u : 3u; }
JPEG_HD uint32_t mcu_shift(uint32_t sub) { return sub ? 4u : 3u; }                                  // log2 of the MCU's side
JPEG_HD uint32_t segment_worst_bytes(uint32_t sub) { return R * mcu_blocks(sub) * BLOCK_BYTES * 2u + 2u; }   // stuffed, with its RST marker
JPEG_HD uint32_t block_table(uint32_t sub, uint32_t bi) { return bi >= (sub ? 4u : 1u) ? 1u : 0u; }   // block bi of an MCU: 0 luma, 1 chroma tables
// the block of the same component in front of block b of a segment (b = MCU * blocks + bi); -1: the segment's first
JPEG_HD int prev_block(uint32_t sub, uint32_t b) {
    const uint32_t B = mcu_blocks(sub), bi = b % B;
    if (sub && bi >= 1u && bi <= 3u) return (int)b - 1;
    if (b < B) return -1;
    return (int)(b - B) + (sub && bi == 0u ? 3 : 0);
}

// ---- constants of the format (host side; the kernels read them through Tables) ----
constexpr int32_t COSINE[8][8] = {
    {2896, 2896, 2896, 2896, 2896, 2896, 2896, 2896},
    {4017, 3406, 2276, 799, -799, -2276, -3406, -4017},
    {3784, 1567, -1567, -3784, -3784, -1567, 1567, 3784},
    {3406, -799, -4017, -2276, 2276, 4017, 799, -3406},
    {2896, -2896, -2896, 2896, 2896, -2896, -2896, 2896},
    {2276, -4017, 799, 3406, -3406, -799, 4017, -2276},
    {1567, -3784, 3784, -1567, -1567, 3784, -3784, 1567},
    {799, -2276, 3406, -4017, 4017, -3406, 2276, -799}};
constexpr uint8_t ZIGZAG[64] = {   // position in the zig-zag scan -> index v * 8 + u
    0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
constexpr uint8_t QUANT_BASE[2][64] = {   // Annex K tables K.1 and K.2, index v * 8 + u
    {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};
// Annex K tables K.3 - K.6: codes per length 1 .. 16, then the symbols in code order.  Order here and in the file: DC luma, DC chroma, AC luma, AC chroma.
constexpr uint8_t HUFF_CLASS_ID[4] = {0x00, 0x01, 0x10, 0x11};
constexpr uint8_t HUFF_BITS[4][16] = {
    {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0},
    {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0},
    {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125},
    {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119}};
constexpr uint32_t HUFF_COUNT[4] = {12, 12, 162, 162};
constexpr uint8_t HUFF_DC_VALS[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
constexpr uint8_t HUFF_AC_VALS[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1,
     0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
     0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a,
     0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
     0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3,
     0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1,
     0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36,
     0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
     0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a,
     0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca,
     0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};
inline const uint8_t* huff_vals(uint32_t t) { return t < 2u ? HUFF_DC_VALS : HUFF_AC_VALS[t - 2u]; }

// ---- the tables of one call: plain words, copied into LDS by every workgroup ----
struct Tables {
    int32_t cosine[8 * COS_PITCH];   // C[u][x] at u * COS_PITCH + x
    uint32_t dc[2][16];              // by category: length << 16 | code;  [0] luma, [1] chroma
    uint32_t ac[2][256];             // by run << 4 | size
    uint16_t quant[2][64];           // index v * 8 + u
    uint8_t zz_pos[64];              // index v * 8 + u -> position in the zig-zag scan
};
static_assert(sizeof(Tables) % 4 == 0, "copied word by word");

inline uint32_t quant_scaled(uint32_t base, int quality) {
    const uint32_t s = quality < 50 ? 5000u / (uint32_t)quality : 200u - 2u * (uint32_t)quality, v = (base * s + 50u) / 100u;
    return v < 1u ? 1u : v > 255u ? 255u : v;
}
inline void build_tables(int quality, Tables& T) {
    memset(&T, 0, sizeof(T));
    for (uint32_t u = 0; u < 8u; ++u) for (uint32_t x = 0; x < 8u; ++x) T.cosine[u * COS_PITCH + x] = COSINE[u][x];
    for (uint32_t t = 0; t < 2u; ++t) for (uint32_t i = 0; i < 64u; ++i) T.quant[t][i] = (uint16_t)quant_scaled(QUANT_BASE[t][i], quality);
    for (uint32_t k = 0; k < 64u; ++k) T.zz_pos[ZIGZAG[k]] = (uint8_t)k;
    for (uint32_t t = 0; t < 4u; ++t) {   // canonical codes: ascending within a length, doubled from one length to the next
        uint32_t code = 0, at = 0;
        for (uint32_t len = 1; len <= 16u; ++len, code <<= 1)
            for (uint32_t i = 0; i < HUFF_BITS[t][len - 1u]; ++i, ++at, ++code) (t < 2u ? T.dc[t] : T.ac[t - 2u])[huff_vals(t)[at]] = len << 16 | code;
    }
}

// ---- arithmetic ----
JPEG_HD int32_t luma(int32_t r, int32_t g, int32_t b) { return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16; }
JPEG_HD int32_t chroma_b(int32_t r, int32_t g, int32_t b) { return (-11059 * r - 21709 * g + 32768 * b + 8388608 + 32767) >> 16; }
JPEG_HD int32_t chroma_r(int32_t r, int32_t g, int32_t b) { return (32768 * r - 27439 * g - 5329 * b + 8388608 + 32767) >> 16; }
// sample (x, y) of block bi of an MCU, level-shifted; px(x, y, c): channel c of the MCU's pixel (x, y), the edge already repeated
template <class Px>
JPEG_HD int32_t mcu_sample(const Px& px, uint32_t sub, uint32_t bi, uint32_t x, uint32_t y) {
    if (!sub || bi < 4u) {
        const uint32_t X = sub ? 8u * (bi & 1u) + x : x, Y = sub ? 8u * (bi >> 1) + y : y;
        const int32_t r = px(X, Y, 0u), g = px(X, Y, 1u), b = px(X, Y, 2u);
        return (!sub && bi == 1u ? chroma_b(r, g, b) : !sub && bi == 2u ? chroma_r(r, g, b) : luma(r, g, b)) - 128;
    }
    int32_t sum = 0;
    for (uint32_t j = 0; j < 2u; ++j)
        for (uint32_t i = 0; i < 2u; ++i) {
            const int32_t r = px(2u * x + i, 2u * y + j, 0u), g = px(2u * x + i, 2u * y + j, 1u), b = px(2u * x + i, 2u * y + j, 2u);
            sum += bi == 4u ? chroma_b(r, g, b) : chroma_r(r, g, b);
        }
    return ((sum + 2) >> 2) - 128;
}
// one output of a pass: c = the table's row, get(i) = the i-th value along the transformed direction
template <class Get>
JPEG_HD int32_t dct_sum(const int32_t* c, const Get& get) {
    int32_t s = 0;
    for (uint32_t i = 0; i < 8u; ++i) s += c[i] * get(i);
    return s;
}
JPEG_HD int32_t dct_round1(int32_t s) { return (s + 512) >> 10; }
JPEG_HD int32_t dct_round2(int32_t s) { return (s + 32768) >> 16; }
JPEG_HD int32_t quantise(int32_t f, uint32_t q, bool ac) {
    const uint32_t a = (uint32_t)(f < 0 ? -f : f);
    uint32_t v = (a + (q >> 1)) / q;
    if (ac && v > 1023u) v = 1023u;
    return f < 0 ? -(int32_t)v : (int32_t)v;
}
JPEG_HD uint32_t category(int32_t v) {   // the bits of |v|
    uint32_t a = (uint32_t)(v < 0 ? -v : v), n = 0;
    while (a) { ++n; a >>= 1; }
    return n;
}
// a symbol with its value bits behind it: `bits` of `n` bits.  dc_symbol: a DC difference; ac_symbol: a non-zero coefficient behind run < 16 zeros.
JPEG_HD void coded(uint32_t entry, int32_t v, uint32_t cat, uint32_t& bits, uint32_t& n) {
    const uint32_t value = (uint32_t)(v < 0 ? v + (int32_t)(1u << cat) - 1 : v);
    bits = (entry & 0xFFFFu) << cat | value; n = (entry >> 16) + cat;
}
JPEG_HD void dc_symbol(const Tables& T, uint32_t t, int32_t diff, uint32_t& bits, uint32_t& n) { const uint32_t c = category(diff); coded(T.dc[t][c], diff, c, bits, n); }
JPEG_HD void ac_symbol(const Tables& T, uint32_t t, uint32_t run, int32_t v, uint32_t& bits, uint32_t& n) { const uint32_t c = category(v); coded(T.ac[t][run << 4 | c], v, c, bits, n); }
constexpr uint32_t ZRL = 0xF0, EOB = 0x00;

// ---- the bit image of a segment: words whose most significant bit comes first ----
// the words that `n` <= 32 bits `bits` at bit `pos` set: hi into word pos / 32, lo into the next
JPEG_HD void put_words(uint32_t pos, uint32_t bits, uint32_t n, uint32_t& hi, uint32_t& lo) {
    const uint64_t x = n ? (uint64_t)bits << (64u - n - (pos & 31u)) : 0ull;   // n + (pos & 31) <= 63
    hi = (uint32_t)(x >> 32); lo = (uint32_t)x;
}
JPEG_HD uint32_t image_byte(const uint32_t* w, uint32_t i) { return (w[i >> 2] >> (24u - 8u * (i & 3u))) & 0xFFu; }

// ---- the file's head: SOI .. SOS (HEADER_BYTES) ----
inline void header(uint32_t width, uint32_t height, uint32_t sub, const Tables& T, std::vector<uint8_t>& o) {
    auto u8 = [&o](uint32_t v) { o.push_back((uint8_t)v); };
    auto u16 = [&o](uint32_t v) { o.push_back((uint8_t)(v >> 8)); o.push_back((uint8_t)v); };
    u16(0xFFD8);
    u16(0xFFE0); u16(16); for (char c : {'J', 'F', 'I', 'F', '\0'}) u8((uint8_t)c);
    u8(1); u8(1); u8(0); u16(1); u16(1); u8(0); u8(0);
    for (uint32_t t = 0; t < 2u; ++t) { u16(0xFFDB); u16(67); u8(t); for (uint32_t k = 0; k < 64u; ++k) u8(T.quant[t][ZIGZAG[k]]); }
    u16(0xFFC0); u16(17); u8(8); u16(height); u16(width); u8(3);
    u8(1); u8(sub ? 0x22 : 0x11); u8(0); u8(2); u8(0x11); u8(1); u8(3); u8(0x11); u8(1);
    for (uint32_t t = 0; t < 4u; ++t) {
        u16(0xFFC4); u16(19u + HUFF_COUNT[t]); u8(HUFF_CLASS_ID[t]);
        for (uint32_t i = 0; i < 16u; ++i) u8(HUFF_BITS[t][i]);
        for (uint32_t i = 0; i < HUFF_COUNT[t]; ++i) u8(huff_vals(t)[i]);
    }
    u16(0xFFDD); u16(4); u16(R);
    u16(0xFFDA); u16(12); u8(3); u8(1); u8(0x00); u8(2); u8(0x11); u8(3); u8(0x11); u8(0); u8(63); u8(0);
}

inline mvs_status fail(std::string& msg, mvs_status st, const char* what) { msg = what; return st; }
// what the twin and the device route refuse alike
inline mvs_status check_params(int quality, int sub, std::string& msg) {
    if (quality < 1 || quality > 100) return fail(msg, MVS_ERR_INVALID, "jpeg: quality 1 .. 100");
    if (sub != 0 && sub != 1) return fail(msg, MVS_ERR_INVALID, "jpeg: subsampling 0 (4:4:4) or 1 (4:2:0)");
    return MVS_OK;
}
inline mvs_status check_frame(uint32_t width, uint32_t height, std::string& msg) {
    if (!width || !height) return fail(msg, MVS_ERR_INVALID, "jpeg: empty frame");
    if (width > MAX_SIDE || height > MAX_SIDE) return fail(msg, MVS_ERR_UNSUPPORTED, "jpeg: a side above 65535");
    return MVS_OK;
}

// ---- the host twin ----
/* the JPEG file of rgb [height][width][3] in `out` */
inline mvs_status encode_jpeg(const uint8_t* rgb, uint32_t width, uint32_t height, int quality, int subsampling, std::vector<uint8_t>& out, std::string& msg) {
    out.clear();
    if (!rgb) return fail(msg, MVS_ERR_INVALID, "jpeg: null image");
    mvs_status st = check_params(quality, subsampling, msg);
    if (st == MVS_OK) st = check_frame(width, height, msg);
    if (st != MVS_OK) return st;
    const uint32_t sub = (uint32_t)subsampling, B = mcu_blocks(sub), lg = mcu_shift(sub), M = 1u << lg;
    const uint32_t mw = (width + M - 1u) >> lg, mh = (height + M - 1u) >> lg;
    const uint64_t total = (uint64_t)mw * mh;
    Tables T;
    build_tables(quality, T);
    header(width, height, sub, T, out);
    std::vector<int32_t> coef((size_t)MAX_BLOCKS * 64u);
    std::vector<uint32_t> image;
    for (uint64_t m0 = 0, seg = 0; m0 < total; m0 += R, ++seg) {
        const uint32_t nm = (uint32_t)(total - m0 < R ? total - m0 : R), nb = nm * B;
        // ---- the coefficients of the segment's blocks, in zig-zag order ----
        for (uint32_t b = 0; b < nb; ++b) {
            const uint64_t m = m0 + b / B;
            const uint32_t bi = b % B, x0 = (uint32_t)(m % mw) << lg, y0 = (uint32_t)(m / mw) << lg;
            auto px = [&](uint32_t x, uint32_t y, uint32_t c) -> int32_t {
                const uint32_t X = x0 + x < width ? x0 + x : width - 1u, Y = y0 + y < height ? y0 + y : height - 1u;
                return rgb[3u * ((size_t)Y * width + X) + c];
            };
            int32_t s[64], t[64];
            for (uint32_t p = 0; p < 64u; ++p) s[p] = mcu_sample(px, sub, bi, p & 7u, p >> 3);
            for (uint32_t p = 0; p < 64u; ++p) t[p] = dct_round1(dct_sum(&T.cosine[(p & 7u) * COS_PITCH], [&](uint32_t i) { return s[(p & ~7u) + i]; }));
            for (uint32_t p = 0; p < 64u; ++p) {
                const int32_t f = dct_round2(dct_sum(&T.cosine[(p >> 3) * COS_PITCH], [&](uint32_t i) { return t[8u * i + (p & 7u)]; }));
                coef[(size_t)b * 64u + T.zz_pos[p]] = quantise(f, T.quant[block_table(sub, bi)][p], p != 0u);
            }
        }
        // ---- the codes into a zeroed image ----
        image.assign((size_t)nb * BLOCK_BYTES / 4u + 2u, 0u);
        uint32_t pos = 0;
        auto put = [&](uint32_t bits, uint32_t n) {
            uint32_t hi, lo;
            put_words(pos, bits, n, hi, lo);
            image[pos >> 5] |= hi; image[(pos >> 5) + 1u] |= lo;
            pos += n;
        };
        for (uint32_t b = 0; b < nb; ++b) {
            const uint32_t t = block_table(sub, b % B);
            const int32_t* c = &coef[(size_t)b * 64u];
            const int pb = prev_block(sub, b);
            uint32_t bits, n, run = 0;
            dc_symbol(T, t, c[0] - (pb < 0 ? 0 : coef[(size_t)pb * 64u]), bits, n);
            put(bits, n);
            for (uint32_t k = 1; k < 64u; ++k) {
                if (!c[k]) { ++run; continue; }
                for (; run >= 16u; run -= 16u) put(T.ac[t][ZRL] & 0xFFFFu, T.ac[t][ZRL] >> 16);
                ac_symbol(T, t, run, c[k], bits, n);
                put(bits, n);
                run = 0;
            }
            if (run) put(T.ac[t][EOB] & 0xFFFFu, T.ac[t][EOB] >> 16);
        }
        const uint32_t pad = (8u - (pos & 7u)) & 7u;
        put((1u << pad) - 1u, pad);
        for (uint32_t i = 0; i < pos / 8u; ++i) {
            const uint32_t v = image_byte(image.data(), i);
            out.push_back((uint8_t)v);
            if (v == 0xFFu) out.push_back(0);
        }
        if (m0 + R < total) { out.push_back(0xFF); out.push_back((uint8_t)(0xD0u + (uint32_t)(seg & 7u))); }
    }
    out.push_back(0xFF); out.push_back(0xD9);
    return MVS_OK;
}

}  // namespace jpeg_base
}  // namespace mvs
