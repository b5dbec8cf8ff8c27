// png_dec.h -- the view input route for PNG files (DESIGN.md section 4 "View input"), defined ONCE for the host and the device: an 8-bit,
// non-interlaced PNG of colour type 0, 2, 3, 4 or 6 inflated (RFC 1950 / 1951), unfiltered (libpng's arithmetic) and converted to 8-bit RGB,
// so that the pixels are the ones Pillow's convert("RGB") gives, bit for bit.
//   Shared pieces (PNGD_HD; k_pngdec.hip runs them in its kernels, the host twin below with one thread): Bits -- the bit reader over the
//     stream's 32-bit words --, Huff and decode() -- one Huffman symbol --, length_of() / distance_of(), code_refusal(), inflate() -- the
//     whole zlib stream on an environment that supplies the words, the tables' storage and the output --, unfilter_byte(), adler_join().
//   Host side (plain sequential C++, no HIP, no library): parse_container() -- every chunk walked by its length, which is all the device
//     route reads on the host --, err_text() / refusal(), and the twin decode_png(), the sequential statement the kernels equal byte for byte.
//     tests/cpp/test_png_dec.cpp runs this file under the sanitizers.
//
// The format:
//   container  signature, IHDR first (CRC checked), optional PLTE in front of the IDATs (CRC checked; a multiple of 3 bytes, at most 768;
//              required for colour type 3), one or more CONSECUTIVE IDAT chunks, whose payloads back to back are the zlib stream.  IEND
//              is not required: the file may end behind the last IDAT's CRC.  Ancillary chunks are skipped, tRNS included; an unknown
//              critical chunk is refused.  DEFINED HERE: IDAT CRCs are not checked -- the stream's Adler-32 is, and it covers every
//              byte that becomes a pixel.
//   zlib       CM 8, CINFO <= 7, FCHECK, no FDICT; stored, fixed and dynamic blocks.  A code may be incomplete in two cases only, both
//              distance codes: no distance code at all (a block of literals), and zlib's single code of one bit.
//              More inflated bytes than height * (1 + width * bpp) are counted and ignored.  DEFINED HERE: the stream is still read to
//              its end and refused for what it does wrong there, and with such excess bytes the Adler-32, which covers them, is not checked.
//   filters    per row its type 0 .. 4 and width * bpp bytes, arithmetic mod 256; a = the byte bpp to the left, b = the byte above,
//              c = the byte above a; the row above the first and the bytes left of a row's first pixel are zero.  1: x + a, 2: x + b,
//              3: x + ((a + b) >> 1), 4: x + paeth(a, b, c), where paeth takes a, b or c by the smallest of |b - c|, |a - c|, |a + b - 2c|,
//              ties in the order a, b, c.
//   colour     grey: R = G = B; grey + alpha and RGBA lose their alpha; palette: PLTE[index].  DEFINED HERE: an index at or past PLTE's
//              entries is refused with the count of such pixels.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include <string.h>
#include <string>
#include <vector>

#include "png_io.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PNGD_M __host__ __device__
#else
#define PNGD_M
#endif
#define PNGD_HD PNGD_M inline

namespace mvs {
namespace png_dec {

constexpr uint32_t MAX_FILE_BYTES = 1u << 28;      // bit positions inside a stream stay below 2^31
constexpr uint64_t MAX_RAW_BYTES = 0x7FF00000ull;  // positions in the filtered stream stay in 32 bits
constexpr uint32_t FAST_BITS = 10;                 // codes up to this length take one lookup
constexpr uint32_t UNFILTER_BAND = 64;             // rows of one band of the unfilter kernel: one lane each
constexpr uint32_t UNFILTER_SEGMENT = 64;          // pixels of a row staged in LDS at a time

// what a stream can be refused for: a per-file word on the device, the first one met
enum : uint32_t {
    E_NONE = 0, E_CM, E_CINFO, E_FCHECK, E_FDICT, E_BTYPE, E_STORED_LEN, E_HLIT, E_HDIST, E_REPEAT_FIRST, E_REPEAT_PAST, E_OVERSUBSCRIBED,
    E_INCOMPLETE, E_NO_EOB, E_SYMBOL, E_DISTCODE, E_CODE, E_DISTANCE, E_TRUNCATED, E_ADLER, E_SHORT, E_FILTER, E_PALETTE
};
inline const char* err_text(uint32_t e) {
    switch (e) {
    case E_CM: return "zlib: the compression method is not 8";
    case E_CINFO: return "zlib: a window above 32 KiB (CINFO > 7)";
    case E_FCHECK: return "zlib: FCHECK does not match";
    case E_FDICT: return "zlib: a preset dictionary (FDICT)";
    case E_BTYPE: return "deflate: block type 3";
    case E_STORED_LEN: return "deflate: a stored block whose LEN is not ~NLEN";
    case E_HLIT: return "deflate: HLIT above 286";
    case E_HDIST: return "deflate: HDIST above 30";
    case E_REPEAT_FIRST: return "deflate: a repeat code 16 with no previous length";
    case E_REPEAT_PAST: return "deflate: a repeat that runs past HLIT + HDIST";
    case E_OVERSUBSCRIBED: return "deflate: an over-subscribed code";
    case E_INCOMPLETE: return "deflate: an incomplete code";
    case E_NO_EOB: return "deflate: no end-of-block code";
    case E_SYMBOL: return "deflate: length symbol 286 or 287";
    case E_DISTCODE: return "deflate: distance code 30 or 31";
    case E_CODE: return "deflate: a prefix that no code matches";
    case E_DISTANCE: return "deflate: a distance further back than the bytes produced";
    case E_TRUNCATED: return "deflate: the stream ends inside a symbol or before the final block's end";
    case E_ADLER: return "zlib: the Adler-32 does not match";
    case E_SHORT: return "fewer inflated bytes than the image needs";
    case E_FILTER: return "a filter type above 4";
    case E_PALETTE: return "palette indices at or past PLTE's entries";
    }
    return "";
}
// the message behind "png: ": `at` is the stream's byte (inflate), the row (filter), the count (inflated bytes, palette pixels)
inline std::string refusal(uint32_t e, uint64_t at) {
    const std::string t = err_text(e);
    if (e == E_ADLER) return t;
    if (e == E_SHORT) return t + " (" + std::to_string(at) + " bytes)";
    if (e == E_FILTER) return t + " in row " + std::to_string(at);
    if (e == E_PALETTE) return t + " (" + std::to_string(at) + " pixels)";
    return t + " (byte " + std::to_string(at) + " of the zlib stream)";
}

// ---- deflate's tables as arithmetic ----
struct Extra { uint32_t base, bits; };
PNGD_HD Extra length_of(uint32_t sym) {   // sym 257 .. 285
    if (sym < 265u) return Extra{sym - 254u, 0u};
    if (sym == 285u) return Extra{258u, 0u};
    const uint32_t e = (sym - 261u) >> 2;
    return Extra{3u + ((4u + ((sym - 261u) & 3u)) << e), e};
}
PNGD_HD Extra distance_of(uint32_t code) {   // code 0 .. 29
    if (code < 4u) return Extra{code + 1u, 0u};
    const uint32_t e = (code >> 1) - 1u;
    return Extra{1u + ((2u + (code & 1u)) << e), e};
}
// the order of the code length code's lengths in a dynamic header, 3 bits each: 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
PNGD_HD uint32_t clen_order(uint32_t i) { return i < 3u ? 16u + i : (uint32_t)((0xF1E2D3C4B5A69780ull >> (4u * (i - 3u))) & 15u); }   // (a nibble each, i = 3 lowest)

// one Huffman code as the decoder reads it: codes up to FAST_BITS in one lookup by the next bits, longer ones by the canonical walk
struct Huff {
    uint16_t look[1u << FAST_BITS];   // length << 9 | symbol, 0: the code is longer, or none matches
    uint16_t count[16];               // codes of every length
    uint16_t sym[288];                // the symbols by (length, symbol)
};
enum CodeKind : uint32_t { KIND_CLEN = 0, KIND_LITLEN = 1, KIND_DIST = 2 };
// count [16] -> what the code is refused for, or E_NONE
PNGD_HD uint32_t code_refusal(const uint32_t* count, uint32_t kind) {
    int32_t left = 1; uint32_t total = 0;
    for (uint32_t l = 1; l < 16u; ++l) {
        left = left * 2 - (int32_t)count[l]; total += count[l];
        if (left < 0) return E_OVERSUBSCRIBED;
    }
    if (left > 0 && !(kind == KIND_DIST && (total == 0u || (total == 1u && count[1] == 1u)))) return E_INCOMPLETE;
    return E_NONE;
}
PNGD_HD uint32_t bit_reverse(uint32_t v, uint32_t n) { uint32_t r = 0; for (uint32_t i = 0; i < n; ++i) r |= ((v >> i) & 1u) << (n - 1u - i); return r; }

// ---- the bit reader: 64 bits ahead, refilled by whole words; words behind the stream's end are zero ----
template <class Env>
struct Bits {
    uint64_t buf = 0; uint32_t cnt = 0, next = 0;
    PNGD_M void fill(Env& E) { if (cnt < 32u) { buf |= (uint64_t)E.word(next) << cnt; ++next; cnt += 32u; } }   // then at least 32 bits
    PNGD_M uint32_t get(uint32_t n) { const uint32_t v = (uint32_t)buf & ((1u << n) - 1u); buf >>= n; cnt -= n; return v; }   // n <= 16
    PNGD_M void drop(uint32_t n) { buf >>= n; cnt -= n; }
    PNGD_M uint32_t consumed() const { return next * 32u - cnt; }   // bits
    PNGD_M void seek(Env& E, uint32_t byte) { buf = 0; cnt = 0; next = byte >> 2; fill(E); drop(8u * (byte & 3u)); }
};
// one symbol of H from a reader with at least 15 bits (fill() first); -1: no code matches the prefix
template <class Env>
PNGD_M inline int32_t decode(Env& E, const Huff& H, Bits<Env>& B) {
    const uint32_t e = E.uni(H.look[(uint32_t)B.buf & ((1u << FAST_BITS) - 1u)]);
    if (e) { B.drop(e >> 9); return (int32_t)(e & 511u); }
    uint32_t code = 0, first = 0, index = 0;
    for (uint32_t l = 1; l < 16u; ++l) {
        code |= (uint32_t)(B.buf >> (l - 1u)) & 1u;
        const uint32_t c = E.uni(H.count[l]);
        if (code < first + c) { B.drop(l); return (int32_t)E.uni(H.sym[index + (code - first)]); }
        index += c; first = (first + c) << 1; code <<= 1;
    }
    return -1;
}

struct Inflated {
    uint32_t err = 0, pos = 0;        // the refusal and the stream's byte it was met at
    uint32_t blocks[3] = {0, 0, 0};   // stored, fixed, dynamic
    uint32_t adler = 0;               // as the stream states it
    uint64_t produced = 0;            // bytes inflated, the excess included
};

// The whole zlib stream.  Env supplies: n (the stream's bytes), word(i), uni(v) (a value all lanes share), lens() (352 bytes), lit() / dist()
// (the two Huff), build(H, lens, n, kind) -> refusal (fills H from n lengths), put(byte), copy_stored(byte position, count),
// copy_match(distance, length), produced().  Every iteration of every loop consumes at least one bit or ends the loop.
template <class Env>
PNGD_M inline void inflate(Env& E, Inflated& R) {
    Bits<Env> B;
    const uint32_t n_bits = 8u * E.n;
#define PNGD_FAIL(code) { R.err = (code); R.pos = B.consumed() / 8u; R.produced = E.produced(); return; }
    B.fill(E);
    const uint32_t cmf = B.get(8), flg = B.get(8);
    if ((cmf & 15u) != 8u) PNGD_FAIL(E_CM)
    if ((cmf >> 4) > 7u) PNGD_FAIL(E_CINFO)
    if (((cmf << 8) | flg) % 31u) PNGD_FAIL(E_FCHECK)
    if (flg & 0x20u) PNGD_FAIL(E_FDICT)
    bool fixed_built = false;
    for (;;) {
        B.fill(E);
        const uint32_t final = B.get(1), type = B.get(2);
        if (B.consumed() > n_bits) PNGD_FAIL(E_TRUNCATED)
        if (type == 3u) PNGD_FAIL(E_BTYPE)
        if (type == 0u) {
            B.drop(B.cnt & 7u);
            B.fill(E);
            const uint32_t len = B.get(16), nlen = B.get(16);
            if (B.consumed() > n_bits) PNGD_FAIL(E_TRUNCATED)
            if (len != (~nlen & 0xFFFFu)) PNGD_FAIL(E_STORED_LEN)
            const uint32_t p = B.consumed() / 8u;
            if (len > E.n - p) PNGD_FAIL(E_TRUNCATED)
            E.copy_stored(p, len);
            B.seek(E, p + len);
            R.blocks[0] += 1u;
        } else {
            uint8_t* lens = E.lens();
            if (type == 1u) {
                if (!fixed_built) {
                    for (uint32_t s = 0; s < 288u; ++s) lens[s] = (uint8_t)(s < 144u ? 8u : s < 256u ? 9u : s < 280u ? 7u : 8u);
                    (void)E.build(E.lit(), lens, 288u, KIND_LITLEN);
                    for (uint32_t s = 0; s < 32u; ++s) lens[s] = 5u;
                    (void)E.build(E.dist(), lens, 32u, KIND_DIST);
                    fixed_built = true;
                }
                R.blocks[1] += 1u;
            } else {
                fixed_built = false;
                const uint32_t hlit = B.get(5) + 257u, hdist = B.get(5) + 1u, hclen = B.get(4) + 4u;
                if (B.consumed() > n_bits) PNGD_FAIL(E_TRUNCATED)
                if (hlit > 286u) PNGD_FAIL(E_HLIT)
                if (hdist > 30u) PNGD_FAIL(E_HDIST)
                for (uint32_t i = 0; i < 19u; ++i) lens[i] = 0;
                for (uint32_t i = 0; i < hclen; ++i) { B.fill(E); lens[clen_order(i)] = (uint8_t)B.get(3); }
                if (B.consumed() > n_bits) PNGD_FAIL(E_TRUNCATED)
                uint32_t why = E.build(E.lit(), lens, 19u, KIND_CLEN);   // (the code length code borrows the literal table)
                if (why) PNGD_FAIL(why)
                uint32_t i = 0, prev = 0;
                while (i < hlit + hdist) {
                    B.fill(E);
                    const int32_t s = decode(E, E.lit(), B);
                    if (s < 0) PNGD_FAIL(E_CODE)
                    uint32_t rep = 1, val = (uint32_t)s;
                    if (s == 16) { if (i == 0u) PNGD_FAIL(E_REPEAT_FIRST) rep = 3u + B.get(2); val = prev; }
                    else if (s == 17) { rep = 3u + B.get(3); val = 0; }
                    else if (s == 18) { rep = 11u + B.get(7); val = 0; }
                    if (B.consumed() > n_bits) PNGD_FAIL(E_TRUNCATED)
                    if (i + rep > hlit + hdist) PNGD_FAIL(E_REPEAT_PAST)
                    for (uint32_t k = 0; k < rep; ++k) lens[32u + i + k] = (uint8_t)val;   // (behind the 19 lengths the table was built from)
                    i += rep; prev = val;
                }
                if (E.uni(lens[32u + 256u]) == 0u) PNGD_FAIL(E_NO_EOB)
                why = E.build(E.lit(), lens + 32u, hlit, KIND_LITLEN);
                if (why) PNGD_FAIL(why)
                why = E.build(E.dist(), lens + 32u + hlit, hdist, KIND_DIST);
                if (why) PNGD_FAIL(why)
                R.blocks[2] += 1u;
            }
            for (;;) {
                B.fill(E);
                const int32_t s = decode(E, E.lit(), B);
                if (s < 0) PNGD_FAIL(E_CODE)
                if (s < 256) { if (B.consumed() > n_bits) PNGD_FAIL(E_TRUNCATED) E.put((uint32_t)s); continue; }
                if (s == 256) { if (B.consumed() > n_bits) PNGD_FAIL(E_TRUNCATED) break; }
                if (s >= 286) PNGD_FAIL(E_SYMBOL)
                const Extra L = length_of((uint32_t)s);
                const uint32_t len = L.base + B.get(L.bits);
                B.fill(E);
                const int32_t d = decode(E, E.dist(), B);
                if (d < 0) PNGD_FAIL(E_CODE)
                if (d >= 30) PNGD_FAIL(E_DISTCODE)
                const Extra D = distance_of((uint32_t)d);
                const uint32_t dist = D.base + B.get(D.bits);
                if (B.consumed() > n_bits) PNGD_FAIL(E_TRUNCATED)
                if ((uint64_t)dist > E.produced()) PNGD_FAIL(E_DISTANCE)
                E.copy_match(dist, len);
            }
        }
        if (final) break;
    }
    B.drop(B.cnt & 7u);
    B.fill(E);
    uint32_t a = 0;
    for (int k = 0; k < 4; ++k) a = a << 8 | B.get(8);
    if (B.consumed() > n_bits) PNGD_FAIL(E_TRUNCATED)
    R.adler = a; R.pos = B.consumed() / 8u; R.produced = E.produced();
#undef PNGD_FAIL
}

// ---- filters ----
PNGD_HD uint32_t paeth(uint32_t a, uint32_t b, uint32_t c) {
    const int32_t p = (int32_t)(a + b) - (int32_t)c;
    const int32_t pa = p > (int32_t)a ? p - (int32_t)a : (int32_t)a - p, pb = p > (int32_t)b ? p - (int32_t)b : (int32_t)b - p, pc = p > (int32_t)c ? p - (int32_t)c : (int32_t)c - p;
    return pa <= pb && pa <= pc ? a : pb <= pc ? b : c;
}
PNGD_HD uint32_t unfilter_byte(uint32_t type, uint32_t x, uint32_t a, uint32_t b, uint32_t c) {
    const uint32_t add = type == 1u ? a : type == 2u ? b : type == 3u ? (a + b) >> 1 : type == 4u ? paeth(a, b, c) : 0u;
    return (x + add) & 0xFFu;
}
PNGD_HD uint32_t bytes_per_pixel(uint32_t colour_type) { return colour_type == 0u || colour_type == 3u ? 1u : colour_type == 4u ? 2u : colour_type == 2u ? 3u : 4u; }

// ---- Adler-32 of two pieces joined: (a1, b1) in front of (a2, b2) of len2 bytes, each computed from (1, 0) ----
constexpr uint32_t ADLER_MOD = 65521u, ADLER_PIECE = 4096u;   // (a piece stays below png_io.h's 5552-byte run bound: its sums fit 32 bits)
PNGD_HD void adler_join(uint32_t& a1, uint32_t& b1, uint32_t a2, uint32_t b2, uint64_t len2) {
    const uint64_t b = (uint64_t)b1 + b2 + (len2 % ADLER_MOD) * ((a1 + ADLER_MOD - 1u) % ADLER_MOD);
    a1 = (a1 + a2 + ADLER_MOD - 1u) % ADLER_MOD; b1 = (uint32_t)(b % ADLER_MOD);
}

// ---- the container ----
struct Piece { size_t off, len; };
struct File {
    uint32_t width = 0, height = 0, colour_type = 0, bpp = 0, n_plte = 0;
    uint8_t plte[768] = {};
    std::vector<Piece> idat;   // the IDAT payloads in the file, the empty ones left out
    uint64_t idat_chunks = 0, zlib_bytes = 0, raw_bytes = 0;
};
inline uint32_t be32(const uint8_t* p) { return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3]; }
inline bool has_signature(const uint8_t* data, size_t size) {
    static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
    return data && size >= 8 && !memcmp(data, sig, 8);
}
inline mvs_status parse_container(const uint8_t* data, size_t size, File& F, std::string& msg) {
    using png_detail::fail; using png_detail::crc32_update;
    F = File{};
    if (!has_signature(data, size)) return fail(msg, MVS_ERR_INVALID, "png: no PNG signature");
    if (size > MAX_FILE_BYTES) return fail(msg, MVS_ERR_INVALID, "png: a file above 256 MiB");
    size_t pos = 8; int idat_state = 0; bool first = true, plte = false;
    while (pos < size) {
        if (size - pos < 12 || be32(data + pos) > size - pos - 12) return fail(msg, MVS_ERR_INVALID, "png: a chunk running past the file");
        const size_t len = be32(data + pos);
        const uint8_t* type = data + pos + 4; const uint8_t* body = type + 4;
        const bool crc_ok = (~crc32_update(0xFFFFFFFFu, type, len + 4)) == be32(body + len);
        const bool is_idat = !memcmp(type, "IDAT", 4);
        if (first != !memcmp(type, "IHDR", 4)) return fail(msg, MVS_ERR_INVALID, first ? "png: IHDR is not the first chunk" : "png: a second IHDR");
        if (first) {
            if (len != 13) return fail(msg, MVS_ERR_INVALID, "png: IHDR is not 13 bytes");
            if (!crc_ok) return fail(msg, MVS_ERR_INVALID, "png: IHDR's CRC does not match");
            F.width = be32(body); F.height = be32(body + 4); F.colour_type = body[9];
            if (!F.width || !F.height || F.width > 0x7FFFFFFFu || F.height > 0x7FFFFFFFu) return fail(msg, MVS_ERR_INVALID, "png: an empty or oversized frame");
            if (body[9] != 0 && body[9] != 2 && body[9] != 3 && body[9] != 4 && body[9] != 6) return fail(msg, MVS_ERR_INVALID, "png: colour type " + std::to_string(body[9]));
            if (body[8] != 8) return fail(msg, MVS_ERR_INVALID, "png: bit depth " + std::to_string(body[8]) + " (8 is accepted)");
            if (body[10] != 0) return fail(msg, MVS_ERR_INVALID, "png: compression method " + std::to_string(body[10]));
            if (body[11] != 0) return fail(msg, MVS_ERR_INVALID, "png: filter method " + std::to_string(body[11]));
            if (body[12] != 0) return fail(msg, MVS_ERR_INVALID, "png: interlaced (Adam7)");
            F.bpp = bytes_per_pixel(F.colour_type);
            F.raw_bytes = (uint64_t)F.height * (1ull + (uint64_t)F.width * F.bpp);
            if (F.raw_bytes > MAX_RAW_BYTES) return fail(msg, MVS_ERR_INVALID, "png: an image above 2 GiB of filtered bytes");
            first = false;
        } else if (is_idat) {
            if (idat_state == 2) return fail(msg, MVS_ERR_INVALID, "png: IDAT chunks that are not consecutive");
            idat_state = 1; F.idat_chunks += 1; F.zlib_bytes += len;
            if (len) F.idat.push_back(Piece{(size_t)(body - data), len});
        } else {
            if (idat_state == 1) idat_state = 2;
            if (!memcmp(type, "IEND", 4)) break;
            if (!memcmp(type, "PLTE", 4)) {
                if (plte) return fail(msg, MVS_ERR_INVALID, "png: a second PLTE");
                if (idat_state) return fail(msg, MVS_ERR_INVALID, "png: PLTE behind IDAT");
                if (!crc_ok) return fail(msg, MVS_ERR_INVALID, "png: PLTE's CRC does not match");
                if (len % 3 || len > 768 || !len) return fail(msg, MVS_ERR_INVALID, "png: PLTE of " + std::to_string(len) + " bytes");
                memcpy(F.plte, body, len); F.n_plte = (uint32_t)(len / 3); plte = true;
            } else if (!(type[0] & 0x20)) return fail(msg, MVS_ERR_INVALID, "png: an unknown critical chunk " + std::string((const char*)type, 4));
        }
        pos += len + 12;
    }
    if (first) return fail(msg, MVS_ERR_INVALID, "png: no IHDR");
    if (!idat_state) return fail(msg, MVS_ERR_INVALID, "png: no IDAT chunk");
    if (F.colour_type == 3 && !plte) return fail(msg, MVS_ERR_INVALID, "png: colour type 3 without PLTE");
    return MVS_OK;
}

// ---- the host twin ----
inline void build_huff(Huff& H, const uint8_t* lens, uint32_t n, uint32_t* count) {
    memset(&H, 0, sizeof(H));
    uint32_t offs[17] = {0, 0};
    for (uint32_t l = 0; l < 16u; ++l) count[l] = 0;
    for (uint32_t s = 0; s < n; ++s) count[lens[s]] += 1u;
    count[0] = 0;
    for (uint32_t l = 1; l < 16u; ++l) { offs[l + 1] = offs[l] + count[l]; H.count[l] = (uint16_t)count[l]; }
    for (uint32_t s = 0; s < n; ++s) if (lens[s]) H.sym[offs[lens[s]]++] = (uint16_t)s;
}
inline void fill_look(Huff& H) {   // (a code that code_refusal accepts)
    uint32_t code = 0, idx = 0;
    for (uint32_t l = 1; l <= FAST_BITS; ++l) {
        for (uint32_t k = 0; k < H.count[l]; ++k, ++code, ++idx)
            for (uint32_t i = bit_reverse(code, l); i < (1u << FAST_BITS); i += 1u << l) H.look[i] = (uint16_t)(l << 9 | H.sym[idx]);
        code <<= 1;
    }
}
struct HostEnv {
    const uint8_t* z; uint32_t n; std::vector<uint8_t>& out; uint64_t need, made = 0;
    Huff L, D; uint8_t lens_[352];
    HostEnv(const uint8_t* z_, uint32_t n_, std::vector<uint8_t>& out_, uint64_t need_) : z(z_), n(n_), out(out_), need(need_) {}
    uint32_t word(uint32_t i) const { uint32_t v = 0; for (uint32_t k = 0; k < 4u; ++k) if ((uint64_t)4u * i + k < n) v |= (uint32_t)z[(size_t)4u * i + k] << (8u * k); return v; }
    template <class T> T uni(T v) const { return v; }
    uint8_t* lens() { return lens_; }
    Huff& lit() { return L; }
    Huff& dist() { return D; }
    uint64_t produced() const { return made; }
    uint32_t build(Huff& H, const uint8_t* lens, uint32_t count_n, uint32_t kind) {
        uint32_t count[16];
        build_huff(H, lens, count_n, count);
        const uint32_t why = code_refusal(count, kind);
        if (!why) fill_look(H);
        return why;
    }
    void put(uint32_t b) { if (made < need) out[(size_t)made] = (uint8_t)b; ++made; }
    void copy_stored(uint32_t p, uint32_t len) { for (uint32_t i = 0; i < len; ++i) put(z[p + i]); }
    void copy_match(uint32_t dist, uint32_t len) { for (uint32_t i = 0; i < len; ++i) put(made - dist < need ? out[(size_t)(made - dist)] : 0u); }
};
struct Counts { uint64_t idat_chunks = 0, zlib_bytes = 0, raw_bytes = 0, blocks[3] = {0, 0, 0}, rows[5] = {0, 0, 0, 0, 0}; };

// the file -> rgb [height][width][3]; raw (may be null): the inflated, still filtered stream; counts (may be null)
inline mvs_status decode_png(const uint8_t* data, size_t size, std::vector<uint8_t>& rgb, uint32_t& width, uint32_t& height, std::vector<uint8_t>* raw_out, std::string& msg, Counts* counts = nullptr) {
    using png_detail::fail;
    rgb.clear(); width = height = 0;
    File F;
    const mvs_status st = parse_container(data, size, F, msg);
    if (st != MVS_OK) return st;
    std::vector<uint8_t> z; z.reserve((size_t)F.zlib_bytes);
    for (const Piece& p : F.idat) z.insert(z.end(), data + p.off, data + p.off + p.len);
    std::vector<uint8_t> raw((size_t)F.raw_bytes);
    HostEnv E(z.data(), (uint32_t)z.size(), raw, F.raw_bytes);
    Inflated R;
    inflate(E, R);
    if (counts) { counts->idat_chunks = F.idat_chunks; counts->zlib_bytes = F.zlib_bytes; counts->raw_bytes = F.raw_bytes; for (int k = 0; k < 3; ++k) counts->blocks[k] = R.blocks[k]; }
    if (R.err) return fail(msg, MVS_ERR_INVALID, "png: " + refusal(R.err, R.pos));
    if (R.produced < F.raw_bytes) return fail(msg, MVS_ERR_INVALID, "png: " + refusal(E_SHORT, R.produced));
    if (R.produced == F.raw_bytes && png_detail::adler32_update(1u, raw.data(), raw.size()) != R.adler) return fail(msg, MVS_ERR_INVALID, "png: " + refusal(E_ADLER, 0));
    if (raw_out) *raw_out = raw;
    const size_t pitch = 1 + (size_t)F.width * F.bpp, bpp = F.bpp;
    rgb.resize((size_t)F.width * F.height * 3);
    std::vector<uint8_t> rows(2 * pitch, 0);   // the row above and the current one, unfiltered
    uint64_t bad = 0;
    for (uint32_t y = 0; y < F.height; ++y) {
        uint8_t* cur = rows.data() + (y & 1u) * pitch; const uint8_t* up = rows.data() + ((y + 1u) & 1u) * pitch;
        const uint8_t* in = raw.data() + (size_t)y * pitch;
        const uint32_t type = in[0];
        if (type > 4u) { rgb.clear(); return fail(msg, MVS_ERR_INVALID, "png: " + refusal(E_FILTER, y)); }
        if (counts) counts->rows[type] += 1;
        for (size_t i = 1; i < pitch; ++i) cur[i] = (uint8_t)unfilter_byte(type, in[i], i > bpp ? cur[i - bpp] : 0u, up[i], i > bpp ? up[i - bpp] : 0u);
        uint8_t* o = rgb.data() + (size_t)y * F.width * 3;
        for (uint32_t x = 0; x < F.width; ++x) {
            const uint8_t* p = cur + 1 + (size_t)x * bpp;
            if (F.colour_type == 3u) { if (p[0] >= F.n_plte) { ++bad; o[3 * x] = o[3 * x + 1] = o[3 * x + 2] = 0; } else memcpy(o + 3 * x, F.plte + 3u * p[0], 3); }
            else if (bpp < 3) o[3 * x] = o[3 * x + 1] = o[3 * x + 2] = p[0];
            else memcpy(o + 3 * x, p, 3);
        }
    }
    if (bad) { rgb.clear(); return fail(msg, MVS_ERR_INVALID, "png: " + refusal(E_PALETTE, bad)); }
    width = F.width; height = F.height;
    return MVS_OK;
}

}  // namespace png_dec
}  // namespace mvs
