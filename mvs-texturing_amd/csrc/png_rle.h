// png_rle.h -- the compressed PNG route of the model output (row f9; DESIGN.md section 4 "Model output" item 7), defined ONCE for the host
// and the device: per-row PNG filters chosen by the smallest sum of absolute residuals, the filtered stream cut into independent chunks of
// CHUNK bytes, every chunk coded with distance-1 run matches and a dynamic Huffman block of its own behind an empty stored block.
//   Shared pieces (PNGRLE_HD; k_png.hip calls them from its kernels with a workgroup, the host twin below with one thread):
//     residual / row costs, token(), walk_tokens(), huff_lengths() with its length limit, huff_codes(), build_header() / emit_header(),
//     token bits and emission through a bit sink, the trailer, adler_span() / adler_append().
//   Host twin (plain sequential C++, no HIP, no zlib): deflate_rle() of a byte stream, encode_png_rle() of an RGB image -- the same bytes
//     as the device route.  The PNG framing is png_io.h's; tests/cpp/test_png_rle.cpp runs this file under the sanitizers.
// A step that runs over the symbols of an alphabet takes a `Par`: each(n, f) runs f(0 .. n - 1), sync() separates steps, lead() is true
// for the one caller that does the sequential steps, add() counts.  SeqPar is one thread; k_png.hip's BlockPar a workgroup, all of whose
// threads make the call.
#pragma once
#include <stdint.h>
#include <stddef.h>

#include "png_io.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PNGRLE_M __host__ __device__
#else
#define PNGRLE_M
#endif
#define PNGRLE_HD PNGRLE_M inline

namespace mvs {
namespace png_rle {

constexpr uint32_t CHUNK = 32768;       // C: bytes of the filtered stream per chunk (the host and the device share it)
constexpr uint32_t NLIT = 286;          // literal / length alphabet
constexpr uint32_t NCL = 19;            // code-length alphabet
constexpr uint32_t LIT_BITS = 15, CL_BITS = 7;
constexpr uint32_t EOB = 256;
constexpr uint32_t MAX_MATCH = 258, MIN_MATCH = 3;
constexpr uint32_t ADLER_MOD = 65521;
constexpr uint64_t MAX_STREAM = 0x7FF00000ull;   // a raw or compressed stream of this many bytes is refused (one IDAT chunk; png_io.h)

// ---- filters (PNG specification, 3 bytes per pixel; a = left, b = up, c = upper left, absent neighbours are 0) ----
PNGRLE_HD uint32_t paeth(uint32_t a, uint32_t b, uint32_t c) {
    const int p = (int)a + (int)b - (int)c;
    const int pa = p > (int)a ? p - (int)a : (int)a - p, pb = p > (int)b ? p - (int)b : (int)b - p, pc = p > (int)c ? p - (int)c : (int)c - p;
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);   // ties: left, up, upper left
}
PNGRLE_HD uint32_t residual(uint32_t t, uint32_t x, uint32_t a, uint32_t b, uint32_t c) {
    const uint32_t pred = t == 0u ? 0u : t == 1u ? a : t == 2u ? b : t == 3u ? ((a + b) >> 1) : paeth(a, b, c);
    return (x - pred) & 0xFFu;
}
PNGRLE_HD uint32_t residual_cost(uint32_t r) { return r < 128u ? r : 256u - r; }   // |r read as a signed 8-bit integer|
template <class T>
PNGRLE_HD uint32_t best_filter(const T cost[5]) {
    uint32_t t = 0;
    for (uint32_t k = 1; k < 5u; ++k) if (cost[k] < cost[t]) t = k;   // a tie goes to the smallest t
    return t;
}

// ---- tokens ----
// the position of offset o in a maximal range of L repeating positions: 0 = covered by a match, 1 = literal, otherwise the match's length
PNGRLE_HD uint32_t token(uint32_t o, uint32_t L) {
    const uint32_t o2 = o - o % MAX_MATCH, r = L - o2;
    if (r < MIN_MATCH) return 1u;
    return o == o2 ? (r < MAX_MATCH ? r : MAX_MATCH) : 0u;
}
// f(position, token) for every position of [begin, end) that emits one.  b(i) = byte i of the chunk; `before` = repeating positions
// directly in front of `begin`, `after` = repeating positions from `end` on (both 0 when [begin, end) is the whole chunk).
template <class Bytes, class F>
PNGRLE_HD void walk_tokens(const Bytes& b, uint32_t begin, uint32_t end, uint32_t before, uint32_t after, F&& f) {
    uint32_t i = begin;
    while (i < end) {
        if (i == 0u || b(i) != b(i - 1u)) { f(i, 1u); ++i; continue; }
        const uint32_t o0 = i == begin ? before : 0u;
        uint32_t j = i + 1u;
        while (j < end && b(j) == b(j - 1u)) ++j;
        const uint32_t L = o0 + (j - i) + (j == end ? after : 0u);
        for (uint32_t q = i; q < j; ++q) { const uint32_t t = token(o0 + (q - i), L); if (t) f(q, t); }
        i = j;
    }
}
// length 3 .. 258 -> symbol 257 .. 285, the number of its extra bits and their value
PNGRLE_HD uint32_t length_symbol(uint32_t len, uint32_t& extra_bits, uint32_t& extra) {
    extra_bits = 0u; extra = 0u;
    if (len == MAX_MATCH) return 285u;
    const uint32_t l = len - MIN_MATCH;
    if (l < 8u) return 257u + l;
    uint32_t lg = 3u;
    while ((l >> (lg + 1u)) != 0u) ++lg;
    extra_bits = lg - 2u; extra = l & ((1u << extra_bits) - 1u);
    return 257u + 4u * extra_bits + (l >> extra_bits);
}

// ---- one thread as a Par ----
struct SeqPar {
    template <class F> PNGRLE_M void each(uint32_t n, F&& f) const { for (uint32_t i = 0; i < n; ++i) f(i); }
    PNGRLE_M void sync() const {}
    PNGRLE_M bool lead() const { return true; }
    PNGRLE_M void add(uint32_t* p, uint32_t v) const { *p += v; }
};

// ---- Huffman code lengths ----
// scratch of one build (LDS on the device).  The tree: leaves [0, m) = the used symbols by (frequency, symbol), internal nodes [m, 2m - 1)
// in the order they are made.
struct HuffWork {
    uint16_t sorted[NLIT + 2];
    uint16_t parent[2 * NLIT + 4];
    uint32_t weight[NLIT + 2];
    uint32_t count[LIT_BITS + 2], next[LIT_BITS + 2];
    uint32_t m, deep;
};
// len[s] of the n symbols with frequencies freq (0: unused, length 0): the Huffman code of the two-queue construction (of two equal
// weights a leaf goes before an internal node, leaves in (frequency, symbol) order) where it is at most `limit` deep; otherwise the
// counts per length are folded to `limit` and repaired until the Kraft sum is 1, and the rarest symbols take the longest codes.  One
// used symbol gets length 1 beside an unused one of length 1: every result with a used symbol is a complete prefix code.
template <class Par>
PNGRLE_HD void huff_lengths(const Par& par, const uint32_t* freq, uint32_t n, uint32_t limit, uint8_t* len, HuffWork& W) {
    if (par.lead()) { W.m = 0u; W.deep = 0u; }
    par.each(n, [&](uint32_t s) { len[s] = 0; });
    par.sync();
    par.each(n, [&](uint32_t s) {
        const uint32_t fs = freq[s];
        if (!fs) return;
        uint32_t rank = 0, used = 0;
        for (uint32_t q = 0; q < n; ++q) {
            const uint32_t fq = freq[q];
            if (fq) { ++used; if (fq < fs || (fq == fs && q < s)) ++rank; }
        }
        W.sorted[rank] = (uint16_t)s;
        if (rank == 0u) W.m = used;
    });
    par.sync();
    const uint32_t m = W.m;
    if (m < 2u) {
        if (m == 1u && par.lead()) { const uint32_t s = W.sorted[0], other = s ? 0u : 1u; len[s] = 1; if (other < n) len[other] = 1; }
        par.sync();
        return;
    }
    if (par.lead()) {
        uint32_t li = 0, ii = 0;
        for (uint32_t k = 0; k + 1u < m; ++k) {
            uint32_t w = 0;
            for (int pick = 0; pick < 2; ++pick) {
                uint32_t node;
                if (li < m && (ii >= k || freq[W.sorted[li]] <= W.weight[ii])) { node = li; w += freq[W.sorted[li]]; ++li; }
                else { node = m + ii; w += W.weight[ii]; ++ii; }
                W.parent[node] = (uint16_t)(m + k);
            }
            W.weight[k] = w;
        }
    }
    par.sync();
    const uint32_t root = 2u * m - 2u;
    par.each(m, [&](uint32_t i) {
        uint32_t d = 0, node = i;
        while (node != root) { node = W.parent[node]; ++d; }
        len[W.sorted[i]] = (uint8_t)(d > 255u ? 255u : d);
        if (d > limit) W.deep = 1u;
    });
    par.sync();
    if (W.deep) {
        if (par.lead()) {
            for (uint32_t d = 0; d <= limit; ++d) W.count[d] = 0u;
            for (uint32_t i = 0; i < m; ++i) { const uint32_t d = len[W.sorted[i]]; W.count[d < limit ? d : limit] += 1u; }
            uint32_t total = 0;
            for (uint32_t d = 1; d <= limit; ++d) total += W.count[d] << (limit - d);
            while (total > (1u << limit)) {
                W.count[limit] -= 1u;
                for (uint32_t d = limit - 1u; d >= 1u; --d)
                    if (W.count[d]) { W.count[d] -= 1u; W.count[d + 1u] += 2u; break; }
                total -= 1u;
            }
            uint32_t i = 0;
            for (uint32_t d = limit; d >= 1u; --d)
                for (uint32_t c = 0; c < W.count[d]; ++c) len[W.sorted[i++]] = (uint8_t)d;
        }
        par.sync();
    }
}
// canonical codes of the lengths, bit-reversed: ready to be sent from the least significant bit on
template <class Par>
PNGRLE_HD void huff_codes(const Par& par, const uint8_t* len, uint32_t n, uint32_t limit, uint16_t* code, HuffWork& W) {
    if (par.lead()) for (uint32_t d = 0; d <= limit; ++d) W.count[d] = 0u;
    par.sync();
    par.each(n, [&](uint32_t s) { if (len[s]) par.add(&W.count[len[s]], 1u); });
    par.sync();
    if (par.lead()) {
        uint32_t c = 0;
        W.count[0] = 0u;
        for (uint32_t d = 1; d <= limit; ++d) { c = (c + W.count[d - 1u]) << 1; W.next[d] = c; }
    }
    par.sync();
    par.each(n, [&](uint32_t s) {
        const uint32_t l = len[s];
        if (!l) { code[s] = 0; return; }
        uint32_t v = W.next[l];
        for (uint32_t q = 0; q < s; ++q) v += len[q] == l ? 1u : 0u;
        uint32_t r = 0;
        for (uint32_t k = 0; k < l; ++k) r |= ((v >> k) & 1u) << (l - 1u - k);
        code[s] = (uint16_t)r;
    });
    par.sync();
}
// sum over the used symbols of 2^(limit - len), 2^limit for a complete code (the tested property)
PNGRLE_HD uint32_t kraft_sum(const uint8_t* len, uint32_t n, uint32_t limit) {
    uint32_t k = 0;
    for (uint32_t s = 0; s < n; ++s) if (len[s]) k += 1u << (limit - len[s]);
    return k;
}

// ---- the header of a dynamic block ----
struct Header {
    uint8_t sym[NLIT + 2], extra[NLIT + 2];   // the code lengths as symbols of the code-length alphabet, and the values of their extra bits
    uint8_t cl_len[NCL + 1]; uint16_t cl_code[NCL + 1]; uint32_t cl_freq[NCL + 1];
    uint32_t n_tok, hlit, hclen, bits;
};
PNGRLE_HD uint32_t cl_order(uint32_t i) {
    const uint8_t order[NCL] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    return order[i];
}
PNGRLE_HD uint32_t cl_extra_bits(uint32_t sym) { return sym == 16u ? 2u : sym == 17u ? 3u : sym == 18u ? 7u : 0u; }
// one thread: HLIT lengths of `len` and ONE distance length (1 with a match in the block, else 0), run-length coded greedily -- zeros by
// 18 (11 .. 138), 17 (3 .. 10) and singles; other values once, then 16 (3 .. 6) and singles -- and the code of those symbols; H.bits =
// the header's bits, the block's 3 included
PNGRLE_HD void build_header(const uint8_t* len, bool has_match, Header& H, HuffWork& W) {
    uint32_t hlit = 257u;
    for (uint32_t s = NLIT - 1u; s >= 257u; --s) if (len[s]) { hlit = s + 1u; break; }
    const uint32_t T = hlit + 1u;
    for (uint32_t k = 0; k <= NCL; ++k) H.cl_freq[k] = 0u;
    uint32_t n_tok = 0;
    auto value = [&](uint32_t i) -> uint32_t { return i < hlit ? len[i] : (has_match ? 1u : 0u); };
    auto tok = [&](uint32_t sym, uint32_t extra) { H.sym[n_tok] = (uint8_t)sym; H.extra[n_tok] = (uint8_t)extra; ++n_tok; H.cl_freq[sym] += 1u; };
    uint32_t i = 0;
    while (i < T) {
        const uint32_t v = value(i);
        uint32_t run = 1u;
        while (i + run < T && value(i + run) == v) ++run;
        i += run;
        if (v == 0u) {
            while (run >= 3u) {
                if (run >= 11u) { const uint32_t k = run < 138u ? run : 138u; tok(18u, k - 11u); run -= k; }
                else { tok(17u, run - 3u); run = 0u; }
            }
        } else {
            tok(v, 0u); run -= 1u;
            while (run >= 3u) { const uint32_t k = run < 6u ? run : 6u; tok(16u, k - 3u); run -= k; }
        }
        for (; run; --run) tok(v, 0u);
    }
    H.n_tok = n_tok; H.hlit = hlit;
    const SeqPar one;
    huff_lengths(one, H.cl_freq, NCL, CL_BITS, H.cl_len, W);
    huff_codes(one, H.cl_len, NCL, CL_BITS, H.cl_code, W);
    uint32_t hclen = 4u;
    for (uint32_t k = NCL - 1u; k >= 4u; --k) if (H.cl_len[cl_order(k)]) { hclen = k + 1u; break; }
    H.hclen = hclen;
    uint32_t bits = 3u + 5u + 5u + 4u + 3u * hclen;
    for (uint32_t k = 0; k < n_tok; ++k) bits += H.cl_len[H.sym[k]] + cl_extra_bits(H.sym[k]);
    H.bits = bits;
}
// a bit sink: put(bit position, value, number of bits <= 32) ORs the value in, least significant bit first
template <class Sink>
PNGRLE_HD uint32_t emit_header(Sink& k, const Header& H) {   // one thread; returns H.bits
    uint32_t pos = 0;
    k.put(pos, 4u, 3u); pos += 3u;                        // BFINAL 0, BTYPE 10
    k.put(pos, H.hlit - 257u, 5u); pos += 5u;
    k.put(pos, 0u, 5u); pos += 5u;                        // one distance code
    k.put(pos, H.hclen - 4u, 4u); pos += 4u;
    for (uint32_t i = 0; i < H.hclen; ++i) { k.put(pos, H.cl_len[cl_order(i)], 3u); pos += 3u; }
    for (uint32_t i = 0; i < H.n_tok; ++i) {
        const uint32_t s = H.sym[i], l = H.cl_len[s], e = cl_extra_bits(s);
        k.put(pos, (uint32_t)H.cl_code[s] | ((uint32_t)H.extra[i] << l), l + e); pos += l + e;
    }
    return pos;
}
PNGRLE_HD uint32_t token_bits(const uint8_t* len, uint32_t tok, uint32_t byte) {
    if (tok == 1u) return len[byte];
    uint32_t eb, ev;
    const uint32_t s = length_symbol(tok, eb, ev);
    return len[s] + eb + 1u;   // the distance code of symbol 0 is one bit
}
template <class Sink>
PNGRLE_HD uint32_t token_put(Sink& k, uint32_t pos, const uint8_t* len, const uint16_t* code, uint32_t tok, uint32_t byte) {
    if (tok == 1u) { k.put(pos, code[byte], len[byte]); return len[byte]; }
    uint32_t eb, ev;
    const uint32_t s = length_symbol(tok, eb, ev), l = len[s];
    k.put(pos, (uint32_t)code[s] | (ev << l), l + eb + 1u);   // ... and that bit is 0
    return l + eb + 1u;
}
// the empty stored block behind a chunk whose bits end at `pos`; returns the chunk's bytes
template <class Sink>
PNGRLE_HD uint32_t trailer_put(Sink& k, uint32_t pos, bool last) {
    k.put(pos, last ? 1u : 0u, 3u);
    const uint32_t byte = (pos + 3u + 7u) / 8u;
    k.put(8u * byte, 0xFFFF0000u, 32u);   // LEN 0, NLEN 0xFFFF
    return byte + 4u;
}
// a dynamic block of D bits (its 3 header bits included) is used for a chunk of n bytes iff this holds; otherwise one stored block
PNGRLE_HD bool use_dynamic(uint32_t D, uint32_t n) { return D < 40u + 8u * n; }

// ---- Adler-32 in pieces ----
// A = the sum of the bytes of [begin, end), B = the sum of (end - i) * byte i
template <class Bytes>
PNGRLE_HD void adler_span(const Bytes& b, uint32_t begin, uint32_t end, uint32_t& A, uint64_t& B) {
    uint32_t a = 0; uint64_t bb = 0;
    for (uint32_t i = begin; i < end; ++i) { a += b(i); bb += a; }
    A = a; B = bb;
}
// the checksum `adler` of a stream, continued by n bytes whose sums are A and B (adler_span, any residues modulo 65521)
PNGRLE_HD uint32_t adler_append(uint32_t adler, uint64_t A, uint64_t B, uint64_t n) {
    const uint64_t a0 = adler & 0xFFFFu, b0 = adler >> 16;
    const uint64_t b = (b0 + (n % ADLER_MOD) * a0 + B % ADLER_MOD) % ADLER_MOD, a = (a0 + A % ADLER_MOD) % ADLER_MOD;
    return (uint32_t)(b << 16 | a);
}

// ---- the host twin ----
struct ByteSink {
    uint8_t* p;
    void put(uint32_t bit, uint32_t v, uint32_t) { uint64_t x = (uint64_t)v << (bit & 7u); for (size_t at = bit >> 3; x; ++at, x >>= 8) p[at] |= (uint8_t)x; }
};
// one chunk b[0, n), 1 <= n <= CHUNK, appended to z with its trailer; *stored += 1 for a stored block
inline void encode_chunk(const uint8_t* b, uint32_t n, bool last, std::vector<uint8_t>& z, uint64_t* stored) {
    uint32_t freq[NLIT + 2] = {0};
    bool has_match = false;
    auto bytes = [&](uint32_t i) -> uint32_t { return b[i]; };
    walk_tokens(bytes, 0u, n, 0u, 0u, [&](uint32_t q, uint32_t t) {
        if (t == 1u) { freq[b[q]] += 1u; return; }
        uint32_t eb, ev;
        freq[length_symbol(t, eb, ev)] += 1u; has_match = true;
    });
    freq[EOB] = 1u;
    uint8_t len[NLIT + 2]; uint16_t code[NLIT + 2];
    HuffWork W; Header H;
    const SeqPar one;
    huff_lengths(one, freq, NLIT, LIT_BITS, len, W);
    huff_codes(one, len, NLIT, LIT_BITS, code, W);
    build_header(len, has_match, H, W);
    uint64_t body = 0;
    walk_tokens(bytes, 0u, n, 0u, 0u, [&](uint32_t q, uint32_t t) { body += token_bits(len, t, b[q]); });
    const uint64_t D = H.bits + body + len[EOB];
    std::vector<uint8_t> out((size_t)n + 16, 0);
    ByteSink k{out.data()};
    uint32_t total;
    if (D < 0xFFFFFFFFull && use_dynamic((uint32_t)D, n)) {
        uint32_t pos = emit_header(k, H);
        walk_tokens(bytes, 0u, n, 0u, 0u, [&](uint32_t q, uint32_t t) { pos += token_put(k, pos, len, code, t, b[q]); });
        k.put(pos, code[EOB], len[EOB]); pos += len[EOB];
        total = trailer_put(k, pos, last);
    } else {
        out[0] = 0; out[1] = (uint8_t)n; out[2] = (uint8_t)(n >> 8); out[3] = (uint8_t)~n; out[4] = (uint8_t)(~n >> 8);
        memcpy(out.data() + 5, b, n);
        total = trailer_put(k, 8u * (5u + n), last);
        if (stored) *stored += 1u;
    }
    z.insert(z.end(), out.begin(), out.begin() + total);
}
// the zlib stream of bytes[0, n): 78 01, the chunks, the big-endian Adler-32
inline mvs_status deflate_rle(const uint8_t* bytes, uint64_t n, std::vector<uint8_t>& z, std::string& msg, uint64_t* chunks = nullptr, uint64_t* stored = nullptr) {
    z.clear();
    if (n && !bytes) return png_detail::fail(msg, MVS_ERR_INVALID, "deflate_rle: null argument");
    const uint64_t nc = (n + CHUNK - 1) / CHUNK;
    if (n >= MAX_STREAM || 2 + n + 10 * nc + 4 >= MAX_STREAM) return png_detail::fail(msg, MVS_ERR_UNSUPPORTED, "deflate_rle: stream too large for one IDAT chunk");
    z.reserve((size_t)(n / 4 + 64));
    z.push_back(0x78); z.push_back(0x01);
    uint32_t adler = 1u;
    for (uint64_t at = 0; at < n; at += CHUNK) {
        const uint32_t k = (uint32_t)(n - at < CHUNK ? n - at : CHUNK);
        const uint8_t* b = bytes + at;
        encode_chunk(b, k, at + k == n, z, stored);
        uint32_t A; uint64_t B;
        adler_span([&](uint32_t i) -> uint32_t { return b[i]; }, 0u, k, A, B);
        adler = adler_append(adler, A, B, k);
    }
    if (!n) { const uint8_t fin[5] = {1, 0, 0, 0xFF, 0xFF}; z.insert(z.end(), fin, fin + 5); }
    png_detail::put_be32(z, adler);
    if (chunks) *chunks = nc;
    return MVS_OK;
}
// the filtered stream of rgb [height][width][3]: per row the filter byte and 3 * width residuals; rows[t] += 1 per row of filter t
inline void filter_image(const uint8_t* rgb, uint32_t width, uint32_t height, std::vector<uint8_t>& raw, uint64_t rows[5]) {
    const size_t rb = 3 * (size_t)width;
    raw.resize((size_t)height * (rb + 1));
    for (uint32_t y = 0; y < height; ++y) {
        const uint8_t* cur = rgb + (size_t)y * rb; const uint8_t* up = y ? cur - rb : nullptr;
        auto nb = [&](size_t x, uint32_t& a, uint32_t& b, uint32_t& c) { a = x >= 3 ? cur[x - 3] : 0u; b = up ? up[x] : 0u; c = (up && x >= 3) ? up[x - 3] : 0u; };
        uint64_t cost[5] = {0, 0, 0, 0, 0};
        for (size_t x = 0; x < rb; ++x) {
            uint32_t a, b, c; nb(x, a, b, c);
            for (uint32_t t = 0; t < 5u; ++t) cost[t] += residual_cost(residual(t, cur[x], a, b, c));
        }
        const uint32_t t = best_filter(cost);
        uint8_t* o = &raw[(size_t)y * (rb + 1)];
        o[0] = (uint8_t)t;
        for (size_t x = 0; x < rb; ++x) { uint32_t a, b, c; nb(x, a, b, c); o[1 + x] = (uint8_t)residual(t, cur[x], a, b, c); }
        if (rows) rows[t] += 1u;
    }
}
constexpr size_t PNG_FRAME = 8 + 25 + 12 + 12;   // signature, IHDR, the IDAT chunk's frame, IEND: the bytes of a PNG beside its zlib stream
// the PNG of a zlib stream into dst [zn + PNG_FRAME]: the signature, the IHDR encode_png writes, one IDAT, IEND
inline void frame_png(uint8_t* dst, uint32_t width, uint32_t height, const uint8_t* z, size_t zn) {
    using namespace png_detail;
    std::vector<uint8_t> head;
    static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
    head.insert(head.end(), sig, sig + 8);
    std::vector<uint8_t> ihdr;
    put_be32(ihdr, width); put_be32(ihdr, height);
    const uint8_t tail[5] = {8, 2, 0, 0, 0};
    ihdr.insert(ihdr.end(), tail, tail + 5);
    put_chunk(head, "IHDR", ihdr.data(), ihdr.size());
    put_be32(head, (uint32_t)zn);
    head.insert(head.end(), {'I', 'D', 'A', 'T'});
    memcpy(dst, head.data(), head.size());
    uint8_t* p = dst + head.size();
    if (z != p) memmove(p, z, zn);
    const uint32_t crc = ~crc32_update(crc32_update(0xFFFFFFFFu, (const uint8_t*)"IDAT", 4), p, zn);
    std::vector<uint8_t> end;
    put_be32(end, crc);
    put_chunk(end, "IEND", nullptr, 0);
    memcpy(p + zn, end.data(), end.size());
}
inline mvs_status check_frame(uint32_t width, uint32_t height, std::string& msg) {
    if (!width || !height) return png_detail::fail(msg, MVS_ERR_INVALID, "encode_png_rle: empty frame");
    if (width > 0x7FFFFFFFu || height > 0x7FFFFFFFu || (3ull * width + 1ull) * height >= MAX_STREAM) return png_detail::fail(msg, MVS_ERR_UNSUPPORTED, "encode_png_rle: image too large for one IDAT chunk");
    return MVS_OK;
}
/* the PNG file of rgb [height][width][3] in `out` */
inline mvs_status encode_png_rle(const uint8_t* rgb, uint32_t width, uint32_t height, std::vector<uint8_t>& out, std::string& msg, uint64_t rows[5] = nullptr) {
    out.clear();
    if (!rgb) return png_detail::fail(msg, MVS_ERR_INVALID, "encode_png_rle: null image");
    mvs_status st = check_frame(width, height, msg);
    if (st != MVS_OK) return st;
    std::vector<uint8_t> raw, z;
    filter_image(rgb, width, height, raw, rows);
    st = deflate_rle(raw.data(), raw.size(), z, msg);
    if (st != MVS_OK) return st;
    out.resize(z.size() + PNG_FRAME);
    frame_png(out.data(), width, height, z.data(), z.size());
    return MVS_OK;
}

}  // namespace png_rle
}  // namespace mvs
