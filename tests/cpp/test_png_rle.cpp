// Stand-alone host program for csrc/png_rle.h (and csrc/png_io.h, whose framing it uses); tests/test_png_rle_host.py compiles it with the
// address and undefined-behaviour sanitizers.  argv[1]: a directory with a file `manifest`, one case per line:
//   stream <name>            <name>.bin holds a byte stream;       its zlib stream is written to <name>.z
//   image <name> <w> <h>     <name>.rgb holds h * w * 3 bytes;     its PNG is written to <name>.png
// Before the cases the Huffman builder is checked on its own: the Fibonacci histogram (1, 1, 2, 3, ... 10946: 21 symbols whose unlimited
// code is 20 deep) must come out at most 15 deep with a Kraft sum of exactly 1, a histogram that fits must keep its Huffman depths, and
// a one-symbol and a two-symbol histogram must give complete prefix codes; token() is compared with greedy splitting.  Prints "ok".
#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>

#include "png_rle.h"

using namespace mvs::png_rle;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { if (failures++ < 20) printf("%s:%d: %s\n", __FILE__, __LINE__, #c); } } while (0)

static std::vector<uint8_t> slurp(const std::string& path) {
    std::vector<uint8_t> v;
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) { printf("cannot open %s\n", path.c_str()); ++failures; return v; }
    uint8_t buf[65536]; size_t k;
    while ((k = fread(buf, 1, sizeof(buf), f)) > 0) v.insert(v.end(), buf, buf + k);
    fclose(f);
    return v;
}

// the codes must be prefix-free: canonical codes of a complete set of lengths are, so check lengths and distinctness
static void check_code(const uint32_t* freq, uint32_t n, uint32_t limit, bool expect_complete) {
    std::vector<uint8_t> len(n + 2); std::vector<uint16_t> code(n + 2);
    HuffWork W;
    const SeqPar one;
    huff_lengths(one, freq, n, limit, len.data(), W);
    huff_codes(one, len.data(), n, limit, code.data(), W);
    for (uint32_t s = 0; s < n; ++s) { CHECK(len[s] <= limit); if (freq[s]) CHECK(len[s] >= 1); }
    if (expect_complete) CHECK(kraft_sum(len.data(), n, limit) == (1u << limit));
    for (uint32_t a = 0; a < n; ++a)
        for (uint32_t b = a + 1; b < n; ++b) {
            if (!len[a] || !len[b]) continue;
            const uint32_t k = len[a] < len[b] ? len[a] : len[b], mask = (1u << k) - 1u;   // reversed codes: a prefix is the low bits
            CHECK((code[a] & mask) != (code[b] & mask));
        }
}

static void builder_checks() {
    {   // Fibonacci: 21 symbols, 28 656 bytes
        uint32_t freq[NLIT + 2] = {0};
        uint32_t a = 1, b = 1, total = 0;
        for (int i = 0; i < 21; ++i) { freq[3 * i + 1] = a; total += a; const uint32_t c = a + b; a = b; b = c; }
        CHECK(total == 28656u && freq[61] == 10946u);
        check_code(freq, NLIT, LIT_BITS, true);
        std::vector<uint8_t> len(NLIT + 2); HuffWork W;
        huff_lengths(SeqPar(), freq, NLIT, 32u, len.data(), W);
        uint32_t deepest = 0; for (uint32_t s = 0; s < NLIT; ++s) deepest = len[s] > deepest ? len[s] : deepest;
        CHECK(deepest == 20u);
        huff_lengths(SeqPar(), freq, NLIT, LIT_BITS, len.data(), W);
        deepest = 0; for (uint32_t s = 0; s < NLIT; ++s) deepest = len[s] > deepest ? len[s] : deepest;
        CHECK(deepest == 15u && kraft_sum(len.data(), NLIT, LIT_BITS) == 1u << 15);
    }
    {   // a histogram that fits keeps the Huffman cost: 1, 1, 2, 4, 8 -> depths 4, 4, 3, 2, 1
        uint32_t freq[NLIT + 2] = {0};
        freq[10] = 1; freq[20] = 1; freq[30] = 2; freq[40] = 4; freq[50] = 8;
        std::vector<uint8_t> len(NLIT + 2); HuffWork W;
        huff_lengths(SeqPar(), freq, NLIT, LIT_BITS, len.data(), W);
        CHECK(len[10] == 4 && len[20] == 4 && len[30] == 3 && len[40] == 2 && len[50] == 1);
        check_code(freq, NLIT, LIT_BITS, true);
    }
    { uint32_t freq[NCL + 1] = {0}; freq[7] = 5; check_code(freq, NCL, CL_BITS, true); }
    { uint32_t freq[NCL + 1] = {0}; freq[0] = 9; check_code(freq, NCL, CL_BITS, true); }
    { uint32_t freq[NCL + 1] = {0}; freq[3] = 1; freq[18] = 1000; check_code(freq, NCL, CL_BITS, true); }
    { uint32_t freq[NCL + 1]; for (uint32_t i = 0; i <= NCL; ++i) freq[i] = 1u << i; check_code(freq, NCL, CL_BITS, true); }   // 18 deep without the limit
    // token(): greedy pieces of at most 258, leftovers of 1 or 2 as literals
    for (uint32_t L = 1; L <= 1100; ++L) {
        std::vector<uint32_t> want(L, 0u);
        uint32_t at = 0;
        while (L - at >= 3) { const uint32_t k = L - at < 258 ? L - at : 258; want[at] = k; at += k; }
        for (; at < L; ++at) want[at] = 1;
        for (uint32_t o = 0; o < L; ++o) CHECK(token(o, L) == want[o]);
    }
    for (uint32_t len = 3; len <= 258; ++len) {   // RFC 1951's table of length codes
        static const uint32_t base[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
        static const uint32_t bits[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
        uint32_t s = 28; while (base[s] > len) --s;
        uint32_t eb, ev;
        CHECK(length_symbol(len, eb, ev) == 257 + s && eb == bits[s] && ev == len - base[s]);
    }
}

int main(int argc, char** argv) {
    if (argc < 2) { printf("usage: test_png_rle <dir>\n"); return 2; }
    builder_checks();
    const std::string dir(argv[1]);
    FILE* mf = fopen((dir + "/manifest").c_str(), "r");
    if (!mf) { printf("no manifest\n"); return 2; }
    char kind[32], name[256]; unsigned w, h;
    std::string msg;
    while (fscanf(mf, "%31s %255s", kind, name) == 2) {
        std::vector<uint8_t> out;
        std::string path = dir + "/" + name;
        if (!strcmp(kind, "stream")) {
            const std::vector<uint8_t> in = slurp(path + ".bin");
            CHECK(deflate_rle(in.data(), in.size(), out, msg) == MVS_OK);
            CHECK(out.size() <= 2 + in.size() + 10 * ((in.size() + CHUNK - 1) / CHUNK) + 4 + (in.empty() ? 5 : 0));
            path += ".z";
        } else {
            if (fscanf(mf, "%u %u", &w, &h) != 2) { ++failures; break; }
            const std::vector<uint8_t> in = slurp(path + ".rgb");
            CHECK(in.size() == (size_t)3 * w * h);
            CHECK(encode_png_rle(in.data(), w, h, out, msg) == MVS_OK);
            path += ".png";
        }
        CHECK(mvs::write_file(path.c_str(), out.data(), out.size(), msg) == MVS_OK);
    }
    fclose(mf);
    std::vector<uint8_t> out;
    CHECK(deflate_rle(nullptr, 5, out, msg) == MVS_ERR_INVALID);
    CHECK(encode_png_rle(nullptr, 1, 1, out, msg) == MVS_ERR_INVALID);
    const uint8_t px[3] = {1, 2, 3};
    CHECK(encode_png_rle(px, 0, 1, out, msg) == MVS_ERR_INVALID);
    CHECK(encode_png_rle(px, 0x7FFFFFFFu, 2, out, msg) == MVS_ERR_UNSUPPORTED);
    if (failures) { printf("%d failures\n", failures); return 1; }
    printf("ok\n");
    return 0;
}
