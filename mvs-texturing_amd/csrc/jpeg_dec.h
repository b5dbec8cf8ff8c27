// jpeg_dec.h -- the view input route (DESIGN.md section 4 "View input"), defined ONCE for the host and the device: a baseline JPEG (one SOF0
// frame, 8 bit, grayscale or YCbCr in 4:4:4 / 4:2:2 / 4:2:0, one interleaved scan, any restart interval) decoded to 8-bit RGB with the
// arithmetic of libjpeg's default decoder, so that the pixels are the ones libjpeg-turbo (Pillow) gives, bit for bit.
//   Shared pieces (JPEGD_HD; k_jpegdec.hip calls them from its kernels, the host twin below with one thread): peek16() / symbol() / step()
//     -- ONE decoder step on a state (bit position, block slot of the MCU, zig-zag index) --, block_place(), idct_column() / idct_row(),
//     idct_fits32(), upsampled(), colour().
//   Host side (plain sequential C++, no HIP, no library): parse_headers() -- the markers up to SOS, which is all the device route reads on
//     the host --, err_text(), and the twin decode_jpeg(), the sequential statement the kernels equal byte for byte.
//     tests/cpp/test_jpeg_dec.cpp runs this file under the sanitizers.
//
// The arithmetic (all values integers; >> is the arithmetic shift, i.e. floor):
//   entropy    DC: a category symbol n <= 15 and n value bits, a difference to the previous block of the component (0 at a segment's start);
//              AC: (run, size) symbols; size 0 with run 15 skips 16 coefficients, size 0 with any other run ends the block (as libjpeg).
//              A value of n bits v stands for v when its first bit is 1 and for v - 2^n + 1 otherwise.
//   dequantise coef * q (int32: |coef| < 2^15, q < 2^8).
//   IDCT       libjpeg's jpeg_idct_islow, CONST_BITS 13, PASS1_BITS 2: columns first, (x + 1024) >> 11, then rows, (x + 131072) >> 18, + 128,
//              clamped to 0 .. 255.  DEFINED HERE: libjpeg masks the sum into its range table, which wraps on absurd values where this clamps.
//              Every intermediate of a pass is sum_k c_k in_k with sum-free |c_k| < 65536, and a pass-1 output is at most 6 S + 1 for a column
//              of absolute sum S (the true gain is 11363 / 2048 = 5.55).  So with T = the block's sum of |dequantised|: pass 1 stays below
//              65536 T + 2^10 and pass 2 below 65536 (6 T + 8) + 2^17, which is < 2^31 for T <= 5400 (idct_fits32): those blocks take
//              32-bit arithmetic, all others 64-bit.  Both give the same exact integers.
//   planes     component c has ceil(width h_c / hmax) x ceil(height v_c / vmax) samples of its own; the blocks beyond are decoded and dropped.
//   upsampling libjpeg's "fancy" triangle filters on the component's own size, edge samples replicated:
//              2x1: out[2i] = (3 s[i] + s[i-1] + 1) >> 2, out[2i+1] = (3 s[i] + s[i+1] + 2) >> 2
//              2x2: per column c = 3 near + far (far: the row above for the upper output row, the row below for the lower one), then
//                   out[2i] = (3 c[i] + c[i-1] + 8) >> 4, out[2i+1] = (3 c[i] + c[i+1] + 7) >> 4
//   colour     cb, cr minus 128: R = y + ((91881 cr + 32768) >> 16), G = y + ((-22554 cb - 46802 cr + 32768) >> 16),
//              B = y + ((116130 cb + 32768) >> 16), clamped.  Grayscale: R = G = B = y.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include <string.h>
#include <string>
#include <vector>

#include "../../include/mvs_viewsel.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define JPEGD_M __host__ __device__
#else
#define JPEGD_M
#endif
#define JPEGD_HD JPEGD_M inline

namespace mvs {
namespace jpeg_dec {

constexpr uint32_t MAX_FILE_BYTES = 1u << 28;   // bit positions inside a file stay below 2^31
constexpr int32_t IDCT_FITS32 = 5400;
constexpr uint8_t ZIGZAG[64] = {   // position in the zig-zag scan -> index v * 8 + u
    0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// what the entropy data can be refused for: bits of a per-image word on the device, the lowest one set names the reason
enum : uint32_t {
    E_SECOND_SCAN = 1u << 0, E_DNL = 1u << 1, E_MARKER = 1u << 2, E_RST_ORDER = 1u << 3, E_SEGMENTS = 1u << 4,
    E_CODE = 1u << 5, E_RUN = 1u << 6, E_DC = 1u << 7, E_INCOMPLETE = 1u << 8
};
inline const char* err_text(uint32_t bits) {
    if (bits & E_SECOND_SCAN) return "a second scan";
    if (bits & E_DNL) return "a DNL marker";
    if (bits & E_MARKER) return "a marker other than RSTn inside the entropy data";
    if (bits & E_RST_ORDER) return "a restart marker out of sequence";
    if (bits & E_SEGMENTS) return "the number of restart segments is not the frame's";
    if (bits & E_CODE) return "a Huffman prefix that no code matches";
    if (bits & E_RUN) return "a run past coefficient 63";
    if (bits & E_DC) return "a DC value outside int16";
    if (bits & E_INCOMPLETE) return "a segment ends before its blocks are complete";
    return "";
}

// one DHT as the decoder reads it: codes up to 8 bits in one lookup, longer ones by the canonical walk
struct HuffDec {
    int32_t maxcode[17];   // [l]: the largest code of l bits, -1 without one
    int32_t valoff[17];    // [l]: index into vals of the first code of l bits, minus that code
    uint16_t look[256];    // by the next 8 bits: length << 8 | symbol, 0 where the code is longer (or none matches)
    uint8_t vals[256];
};
// a file's frame and tables: plain words, uploaded as they are
struct Frame {
    uint32_t width, height, ncomp;      // ncomp 1 or 3
    uint32_t hs, vs;                    // luma sampling (1 x 1 for a single component)
    uint32_t mw, mh, bpm;               // MCUs across and down, blocks per MCU
    uint32_t interval;                  // MCUs per restart segment (the whole scan without DRI)
    uint32_t nseg;                      // restart segments due
    uint32_t cw, ch;                    // the chroma planes' own size
    uint32_t td[3], ta[3];              // per component: DC and AC table
    uint16_t quant[3][64];              // per component, index v * 8 + u
    uint8_t zz[64];                     // ZIGZAG, where the kernels can index it
    HuffDec dc[2], ac[2];
};
static_assert(sizeof(Frame) % 4 == 0, "copied word by word");

JPEGD_HD uint32_t slot_comp(const Frame& F, uint32_t slot) { const uint32_t ny = F.hs * F.vs; return slot < ny ? 0u : slot - ny + 1u; }
JPEGD_HD uint32_t plane_pitch(const Frame& F, uint32_t c) { return 8u * F.mw * (c ? 1u : F.hs); }   // planes hold whole MCUs
JPEGD_HD uint32_t plane_rows(const Frame& F, uint32_t c) { return 8u * F.mh * (c ? 1u : F.vs); }
// block b of the image in coding order: its component and the sample (x0, y0) of its corner in that component's plane
JPEGD_HD void block_place(const Frame& F, uint32_t b, uint32_t& c, uint32_t& x0, uint32_t& y0) {
    const uint32_t mcu = b / F.bpm, slot = b % F.bpm, mx = mcu % F.mw, my = mcu / F.mw;
    c = slot_comp(F, slot);
    if (c) { x0 = 8u * mx; y0 = 8u * my; }
    else { x0 = 8u * (mx * F.hs + slot % F.hs); y0 = 8u * (my * F.vs + slot / F.hs); }
}

// ---- entropy decoding ----
// 16 bits from bit `pos` of a byte string; by(i) = byte i (0 behind the string's end)
template <class Bytes>
JPEGD_HD uint32_t peek16(const Bytes& by, uint32_t pos) {
    const uint32_t i = pos >> 3, w = by(i) << 16 | by(i + 1u) << 8 | by(i + 2u);
    return (w >> (8u - (pos & 7u))) & 0xFFFFu;
}
// the code at the head of w16: its length (0: none matches) and symbol
JPEGD_HD uint32_t symbol(const HuffDec& T, uint32_t w16, uint32_t& sym) {
    const uint32_t e = T.look[w16 >> 8];
    if (e) { sym = e & 255u; return e >> 8; }
    for (uint32_t l = 9; l <= 16u; ++l) {
        const int32_t code = (int32_t)(w16 >> (16u - l));
        if (code <= T.maxcode[l]) { sym = T.vals[(code + T.valoff[l]) & 255]; return l; }
    }
    return 0;
}
JPEGD_HD int32_t extend(uint32_t v, uint32_t n) { return n && !(v >> (n - 1u)) ? (int32_t)v - (int32_t)(1u << n) + 1 : (int32_t)v; }

struct State { uint32_t pos, slot, k; };   // bit position in the segment, block slot inside the MCU, zig-zag index of the next coefficient
struct Step { uint32_t err; int32_t zz; int32_t value; bool block_done; };   // zz: the coefficient this step gave (-1: none)
// ONE symbol with its value bits from state s.  An invalid prefix advances one bit, an overlong run ends the block: that keeps a
// speculative decoder going; an exact one stops at Step::err.
template <class Bytes>
JPEGD_HD Step step(const Frame& F, const Bytes& by, State& s) {
    Step r{0u, -1, 0, false};
    const uint32_t c = slot_comp(F, s.slot);
    uint32_t sym = 0;
    const uint32_t len = symbol(s.k ? F.ac[F.ta[c]] : F.dc[F.td[c]], peek16(by, s.pos), sym);
    if (!len) { r.err = E_CODE; s.pos += 1u; return r; }
    s.pos += len;
    if (!s.k) {
        if (sym > 15u) { r.err = E_DC; sym = 0; }
        r.zz = 0; r.value = extend(sym ? peek16(by, s.pos) >> (16u - sym) : 0u, sym);
        s.pos += sym; s.k = 1;
    } else {
        const uint32_t run = sym >> 4, n = sym & 15u;
        if (n) {
            s.k += run;
            if (s.k > 63u) { r.err = E_RUN; s.k = 64; }
            else { r.zz = (int32_t)s.k; r.value = extend(peek16(by, s.pos) >> (16u - n), n); s.pos += n; s.k += 1u; }
        } else if (run == 15u) {
            s.k += 16u;
            if (s.k > 64u) { r.err = E_RUN; s.k = 64; }
        } else s.k = 64;
    }
    if (s.k >= 64u) { s.k = 0; s.slot = s.slot + 1u == F.bpm ? 0u : s.slot + 1u; r.block_done = true; }
    return r;
}

// ---- IDCT: one pass over eight values; I = int32_t where idct_fits32, int64_t otherwise ----
template <class I>
JPEGD_HD void idct_pass(const I in[8], I out[8]) {
    I z1 = (in[2] + in[6]) * (I)4433;
    const I tmp2 = z1 - in[6] * (I)15137, tmp3 = z1 + in[2] * (I)6270;
    const I tmp0 = (in[0] + in[4]) * (I)8192, tmp1 = (in[0] - in[4]) * (I)8192;
    const I tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    I t0 = in[7], t1 = in[5], t2 = in[3], t3 = in[1];
    z1 = t0 + t3;
    I z2 = t1 + t2, z3 = t0 + t2, z4 = t1 + t3;
    const I z5 = (z3 + z4) * (I)9633;
    t0 *= (I)2446; t1 *= (I)16819; t2 *= (I)25172; t3 *= (I)12299;
    z1 *= (I)-7373; z2 *= (I)-20995; z3 *= (I)-16069; z4 *= (I)-3196;
    z3 += z5; z4 += z5;
    t0 += z1 + z3; t1 += z2 + z4; t2 += z2 + z3; t3 += z1 + z4;
    out[0] = tmp10 + t3; out[7] = tmp10 - t3; out[1] = tmp11 + t2; out[6] = tmp11 - t2;
    out[2] = tmp12 + t1; out[5] = tmp12 - t1; out[3] = tmp13 + t0; out[4] = tmp13 - t0;
}
JPEGD_HD bool idct_fits32(int32_t abs_sum) { return abs_sum <= IDCT_FITS32; }
// a column of dequantised coefficients -> pass-1 values; a row of those -> samples 0 .. 255
JPEGD_HD void idct_column(const int32_t in[8], int32_t out[8], bool fits32) {
    if (fits32) { int32_t o[8]; idct_pass<int32_t>(in, o); for (int i = 0; i < 8; ++i) out[i] = (o[i] + 1024) >> 11; }
    else { int64_t a[8], o[8]; for (int i = 0; i < 8; ++i) a[i] = in[i]; idct_pass<int64_t>(a, o); for (int i = 0; i < 8; ++i) out[i] = (int32_t)((o[i] + 1024) >> 11); }
}
JPEGD_HD void idct_row(const int32_t in[8], uint8_t out[8], bool fits32) {
    if (fits32) { int32_t o[8]; idct_pass<int32_t>(in, o); for (int i = 0; i < 8; ++i) { const int32_t v = ((o[i] + 131072) >> 18) + 128; out[i] = (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v); } }
    else { int64_t a[8], o[8]; for (int i = 0; i < 8; ++i) a[i] = in[i]; idct_pass<int64_t>(a, o); for (int i = 0; i < 8; ++i) { const int64_t v = ((o[i] + 131072) >> 18) + 128; out[i] = (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v); } }
}

// ---- upsampling and colour ----
// the chroma sample at pixel (x, y); s(i, j) = sample (i, j) of the component's own cw x ch plane
template <class S>
JPEGD_HD int32_t upsampled(const S& s, uint32_t cw, uint32_t ch, uint32_t hs, uint32_t vs, uint32_t x, uint32_t y) {
    if (hs == 1u) return s(x, y);
    const uint32_t i = x >> 1, io = (x & 1u) ? (i + 1u < cw ? i + 1u : i) : (i ? i - 1u : 0u);
    if (vs == 1u) return (3 * s(i, y) + s(io, y) + ((x & 1u) ? 2 : 1)) >> 2;
    const uint32_t j = y >> 1, jf = (y & 1u) ? (j + 1u < ch ? j + 1u : j) : (j ? j - 1u : 0u);
    const int32_t c = 3 * s(i, j) + s(i, jf), co = 3 * s(io, j) + s(io, jf);
    return (3 * c + co + ((x & 1u) ? 7 : 8)) >> 4;
}
JPEGD_HD uint8_t clamp8(int32_t v) { return (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v); }
JPEGD_HD void colour(int32_t y, int32_t cb, int32_t cr, uint8_t rgb[3]) {
    cb -= 128; cr -= 128;
    rgb[0] = clamp8(y + ((91881 * cr + 32768) >> 16));
    rgb[1] = clamp8(y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
    rgb[2] = clamp8(y + ((116130 * cb + 32768) >> 16));
}

// ---- the host side ----
inline mvs_status fail(std::string& msg, const std::string& what) { msg = "jpeg: " + what; return MVS_ERR_INVALID; }

inline bool build_huff(const uint8_t bits[16], const uint8_t* vals, uint32_t count, HuffDec& T) {
    memset(&T, 0, sizeof(T));
    memcpy(T.vals, vals, count);
    uint32_t code = 0, at = 0;
    for (uint32_t l = 1; l <= 16u; ++l, code <<= 1) {
        T.maxcode[l] = -1; T.valoff[l] = 0;
        if (!bits[l - 1u]) continue;
        T.valoff[l] = (int32_t)at - (int32_t)code;
        for (uint32_t i = 0; i < bits[l - 1u]; ++i, ++at, ++code) {
            if (code >= (1u << l)) return false;   // more codes than the length holds
            if (l <= 8u) for (uint32_t p = code << (8u - l), e = p + (1u << (8u - l)); p < e; ++p) T.look[p] = (uint16_t)(l << 8 | vals[at]);
        }
        T.maxcode[l] = (int32_t)code - 1;
    }
    return true;
}

// The markers from SOI to SOS.  F: the frame and the tables the scan uses; scan_begin: the first byte of the entropy data, which runs to
// the file's last two bytes, an EOI.  Everything item by item of DESIGN.md "View input" that is not accepted is refused here.
inline mvs_status parse_headers(const uint8_t* d, size_t n, Frame& F, size_t& scan_begin, std::string& msg) {
    memset(&F, 0, sizeof(F));
    scan_begin = 0;
    if (!d || n < 4 || d[0] != 0xFF || d[1] != 0xD8) return fail(msg, "no SOI: not a JPEG file");
    if (n >= MAX_FILE_BYTES) return fail(msg, "a file of 256 MB or more");
    uint16_t quant[4][64]; bool have_q[4] = {};
    HuffDec huff[2][2]; bool have_h[2][2] = {};
    uint8_t comp_id[3] = {}, comp_tq[3] = {}, comp_hv[3] = {};
    bool have_sof = false, jfif = false, adobe = false; uint32_t adobe_transform = 0, dri = 0;
    size_t at = 2;
    for (;;) {
        if (at + 2 > n) return fail(msg, "truncated file: it ends before SOS");
        if (d[at] != 0xFF) return fail(msg, "no marker where one is due (byte " + std::to_string(at) + ")");
        while (at + 1 < n && d[at + 1] == 0xFF) ++at;   // fill bytes
        if (at + 2 > n) return fail(msg, "truncated file: it ends before SOS");
        const uint32_t m = d[at + 1];
        at += 2;
        if (m == 0xD9) return fail(msg, "EOI before any scan");
        if (m == 0xD8 || (m >= 0xD0 && m <= 0xD7) || m == 0x01) return fail(msg, "marker " + std::to_string(m) + " in front of SOS");
        if (at + 2 > n) return fail(msg, "truncated file: a marker without its length");
        const size_t len = (size_t)d[at] << 8 | d[at + 1];
        if (len < 2 || at + len > n) return fail(msg, "truncated file: a marker segment runs past its end");
        const uint8_t* s = d + at + 2; const size_t sl = len - 2;
        at += len;
        if (m == 0xC0) {
            if (have_sof) return fail(msg, "a second frame");
            if (sl < 6) return fail(msg, "SOF0 too short");
            if (s[0] != 8) return fail(msg, "sample precision " + std::to_string(s[0]) + ": 8-bit samples only");
            F.height = (uint32_t)s[1] << 8 | s[2]; F.width = (uint32_t)s[3] << 8 | s[4]; F.ncomp = s[5];
            if (!F.height) return fail(msg, "frame height 0: DNL is not supported");
            if (!F.width) return fail(msg, "empty frame");
            if (F.ncomp != 1u && F.ncomp != 3u) return fail(msg, std::to_string(F.ncomp) + " components: 1 (grayscale) or 3 (YCbCr) only");
            if (sl != 6 + 3 * (size_t)F.ncomp) return fail(msg, "SOF0 length");
            for (uint32_t c = 0; c < F.ncomp; ++c) { comp_id[c] = s[6 + 3 * c]; comp_hv[c] = s[7 + 3 * c]; comp_tq[c] = s[8 + 3 * c]; if (comp_tq[c] > 3) return fail(msg, "quantiser id above 3"); }
            have_sof = true;
        } else if (m >= 0xC1 && m <= 0xCF && m != 0xC4 && m != 0xC8 && m != 0xCC) {
            return fail(msg, std::string("frame marker SOF") + std::to_string(m - 0xC0) + (m == 0xC2 ? " (progressive)" : m == 0xC1 ? " (extended sequential)" : m >= 0xC9 ? " (arithmetic)" : "") + ": baseline SOF0 only");
        } else if (m == 0xCC) {
            return fail(msg, "DAC: arithmetic coding is not supported");
        } else if (m == 0xDC) {
            return fail(msg, "a DNL marker");
        } else if (m == 0xDB) {
            for (size_t o = 0; o < sl;) {
                const uint32_t pq = s[o] >> 4, tq = s[o] & 15u;
                if (pq) return fail(msg, "DQT of 16-bit precision");
                if (tq > 3) return fail(msg, "DQT id above 3");
                if (o + 65 > sl) return fail(msg, "truncated file: a DQT shorter than its table");
                for (uint32_t k = 0; k < 64u; ++k) quant[tq][ZIGZAG[k]] = s[o + 1 + k];
                have_q[tq] = true; o += 65;
            }
        } else if (m == 0xC4) {
            for (size_t o = 0; o < sl;) {
                const uint32_t tc = s[o] >> 4, th = s[o] & 15u;
                if (tc > 1 || th > 1) return fail(msg, "DHT class or id above 1");
                if (o + 17 > sl) return fail(msg, "truncated file: a DHT shorter than its lengths");
                uint32_t count = 0;
                for (uint32_t i = 0; i < 16u; ++i) count += s[o + 1 + i];
                if (count > 256 || o + 17 + count > sl) return fail(msg, "a DHT with more symbols than it holds");
                if (!build_huff(s + o + 1, s + o + 17, count, huff[tc][th])) return fail(msg, "a DHT with more codes than its lengths allow");
                have_h[tc][th] = true; o += 17 + count;
            }
        } else if (m == 0xDD) {
            if (sl != 2) return fail(msg, "DRI length");
            dri = (uint32_t)s[0] << 8 | s[1];
        } else if (m == 0xE0) {
            if (sl >= 5 && !memcmp(s, "JFIF", 5)) jfif = true;
        } else if (m == 0xEE) {
            if (sl >= 12 && !memcmp(s, "Adobe", 5)) { adobe = true; adobe_transform = s[11]; }
        } else if (m == 0xDA) {
            if (!have_sof) return fail(msg, "SOS in front of the frame");
            if (sl != 4 + 2 * (size_t)F.ncomp || s[0] != F.ncomp) return fail(msg, "the scan does not hold all components of the frame: one interleaved scan only");
            for (uint32_t c = 0; c < F.ncomp; ++c) {
                if (s[1 + 2 * c] != comp_id[c]) return fail(msg, "the scan's components are not the frame's in order");
                F.td[c] = s[2 + 2 * c] >> 4; F.ta[c] = s[2 + 2 * c] & 15u;
                if (F.td[c] > 1 || F.ta[c] > 1) return fail(msg, "the scan names a Huffman table id above 1");
                if (!have_h[0][F.td[c]] || !have_h[1][F.ta[c]]) return fail(msg, "the scan uses a Huffman table that no DHT defined");
                if (!have_q[comp_tq[c]]) return fail(msg, "the frame uses a quantiser that no DQT defined");
                memcpy(F.quant[c], quant[comp_tq[c]], sizeof(F.quant[c]));
            }
            const uint8_t* t = s + 1 + 2 * F.ncomp;
            if (t[0] != 0 || t[1] != 63 || t[2] != 0) return fail(msg, "spectral selection or successive approximation in the scan: sequential only");
            break;
        }
        // APPn, COM and anything else with a length: skipped
    }
    if (F.ncomp == 3u) {
        if (adobe && adobe_transform == 0) return fail(msg, "Adobe APP14 with transform 0: the file stores RGB, not YCbCr");
        if (!jfif && !adobe && comp_id[0] == 'R' && comp_id[1] == 'G' && comp_id[2] == 'B') return fail(msg, "component ids R, G, B: the file stores RGB, not YCbCr");
        if (comp_hv[1] != 0x11 || comp_hv[2] != 0x11) return fail(msg, "chroma sampling other than 1x1");
        if (comp_hv[0] != 0x11 && comp_hv[0] != 0x21 && comp_hv[0] != 0x22) return fail(msg, "luma sampling " + std::to_string(comp_hv[0] >> 4) + "x" + std::to_string(comp_hv[0] & 15) + ": 4:4:4, 4:2:2 and 4:2:0 only");
        F.hs = comp_hv[0] >> 4; F.vs = comp_hv[0] & 15u;
    } else F.hs = F.vs = 1;
    for (int k = 0; k < 2; ++k) { F.dc[k] = huff[0][k]; F.ac[k] = huff[1][k]; }
    memcpy(F.zz, ZIGZAG, sizeof(F.zz));
    F.bpm = F.ncomp == 1u ? 1u : F.hs * F.vs + 2u;
    F.mw = (F.width + 8u * F.hs - 1u) / (8u * F.hs); F.mh = (F.height + 8u * F.vs - 1u) / (8u * F.vs);
    F.cw = (F.width + F.hs - 1u) / F.hs; F.ch = (F.height + F.vs - 1u) / F.vs;
    const uint32_t mcus = F.mw * F.mh;
    F.interval = dri ? dri : mcus;
    F.nseg = (mcus + F.interval - 1u) / F.interval;
    scan_begin = at;
    if (n < at + 2 || d[n - 2] != 0xFF || d[n - 1] != 0xD9) return fail(msg, "truncated file: no EOI at its end");
    return MVS_OK;
}
// blocks due in segment k
inline uint32_t segment_blocks(const Frame& F, uint32_t k) {
    const uint32_t mcus = F.mw * F.mh, first = k * F.interval;
    return (mcus - first < F.interval ? mcus - first : F.interval) * F.bpm;
}

// ---- the host twin ----
// rgb [height][width][3] of the file d[0, n); coefs (optional): the quantised coefficients int16 [blocks][64] in coding order, index v * 8 + u
inline mvs_status decode_jpeg(const uint8_t* d, size_t n, std::vector<uint8_t>& rgb, uint32_t& width, uint32_t& height, std::vector<int16_t>* coefs, std::string& msg) {
    rgb.clear(); width = height = 0;
    Frame F; size_t begin = 0;
    const mvs_status st = parse_headers(d, n, F, begin, msg);
    if (st != MVS_OK) return st;
    // ---- unstuff and split ----
    std::vector<uint8_t> clean; std::vector<size_t> seg_start{0};
    for (size_t i = begin, end = n - 2; i < end; ++i) {
        if (d[i] != 0xFF) { clean.push_back(d[i]); continue; }
        const uint32_t nx = i + 1 < end ? d[i + 1] : 0xFFu;
        if (nx == 0x00) { clean.push_back(0xFF); ++i; continue; }
        if (nx >= 0xD0 && nx <= 0xD7) {
            if (nx != 0xD0 + ((seg_start.size() - 1) & 7u)) return fail(msg, err_text(E_RST_ORDER));
            seg_start.push_back(clean.size()); ++i; continue;
        }
        return fail(msg, err_text(nx == 0xDA ? E_SECOND_SCAN : nx == 0xDC ? E_DNL : E_MARKER));
    }
    if (seg_start.size() != F.nseg) return fail(msg, err_text(E_SEGMENTS));
    seg_start.push_back(clean.size());
    // ---- entropy decode: coefficients in natural order, DC differences made values ----
    const size_t nblocks = (size_t)F.mw * F.mh * F.bpm;
    std::vector<int16_t> coef(nblocks * 64, 0);
    size_t b0 = 0;
    for (uint32_t k = 0; k < F.nseg; ++k) {
        const uint8_t* seg = clean.data() + seg_start[k];
        const uint32_t len = (uint32_t)(seg_start[k + 1] - seg_start[k]), due = segment_blocks(F, k);
        auto by = [&](uint32_t i) -> uint32_t { return i < len ? seg[i] : 0u; };
        State s{0, 0, 0};
        int32_t pred[3] = {0, 0, 0};
        for (uint32_t b = 0; b < due;) {
            if (s.pos >= 8u * len) return fail(msg, err_text(E_INCOMPLETE));
            const uint32_t c = slot_comp(F, s.slot);
            const Step r = step(F, by, s);
            if (r.err) return fail(msg, err_text(r.err));
            if (s.pos > 8u * len) return fail(msg, err_text(E_INCOMPLETE));
            if (r.zz == 0) {
                pred[c] += r.value;
                if (pred[c] < -32768 || pred[c] > 32767) return fail(msg, err_text(E_DC));
                coef[(b0 + b) * 64] = (int16_t)pred[c];
            } else if (r.zz > 0) coef[(b0 + b) * 64 + F.zz[r.zz]] = (int16_t)r.value;
            if (r.block_done) ++b;
        }
        b0 += due;
    }
    // ---- IDCT into the planes ----
    std::vector<uint8_t> plane[3];
    for (uint32_t c = 0; c < F.ncomp; ++c) plane[c].assign((size_t)plane_pitch(F, c) * plane_rows(F, c), 0);
    for (size_t b = 0; b < nblocks; ++b) {
        uint32_t c, x0, y0;
        block_place(F, (uint32_t)b, c, x0, y0);
        int32_t v[64], w[64], sum = 0;
        for (uint32_t i = 0; i < 64u; ++i) { v[i] = coef[b * 64 + i] * (int32_t)F.quant[c][i]; sum = sum > IDCT_FITS32 ? sum : sum + (v[i] < 0 ? -v[i] : v[i]); }
        const bool f32 = idct_fits32(sum);
        for (uint32_t x = 0; x < 8u; ++x) {
            int32_t in[8], out[8];
            for (uint32_t y = 0; y < 8u; ++y) in[y] = v[8 * y + x];
            idct_column(in, out, f32);
            for (uint32_t y = 0; y < 8u; ++y) w[8 * y + x] = out[y];
        }
        for (uint32_t y = 0; y < 8u; ++y) idct_row(&w[8 * y], &plane[c][(size_t)(y0 + y) * plane_pitch(F, c) + x0], f32);
    }
    // ---- upsampling and colour ----
    width = F.width; height = F.height;
    rgb.resize((size_t)width * height * 3);
    const uint32_t py = plane_pitch(F, 0), pc = plane_pitch(F, 1);
    for (uint32_t y = 0; y < height; ++y)
        for (uint32_t x = 0; x < width; ++x) {
            uint8_t* o = &rgb[3 * ((size_t)y * width + x)];
            const int32_t Y = plane[0][(size_t)y * py + x];
            if (F.ncomp == 1u) { o[0] = o[1] = o[2] = (uint8_t)Y; continue; }
            auto cb = [&](uint32_t i, uint32_t j) -> int32_t { return plane[1][(size_t)j * pc + i]; };
            auto cr = [&](uint32_t i, uint32_t j) -> int32_t { return plane[2][(size_t)j * pc + i]; };
            colour(Y, upsampled(cb, F.cw, F.ch, F.hs, F.vs, x, y), upsampled(cr, F.cw, F.ch, F.hs, F.vs, x, y), o);
        }
    if (coefs) coefs->swap(coef);
    return MVS_OK;
}

}  // namespace jpeg_dec
}  // namespace mvs
