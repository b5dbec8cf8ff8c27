// Stand-alone host program for csrc/jpeg_base.h; tests/test_jpeg_host.py compiles it with the address and undefined-behaviour sanitizers.
// argv[1]: a directory with a file `manifest`, one case per line:
//   image <name> <w> <h>     <name>.rgb holds h * w * 3 bytes;  its JPEGs are written to <name>_s<subsampling>_q<quality>.jpg for
//                            subsampling 0, 1 and quality 1, 50, 90, 100
// Before the cases the tables are checked on their own: every Huffman table is a prefix code with the counts of its DHT, the zig-zag
// positions are a permutation, the quantiser rule gives the base tables at quality 50 and ones at quality 100, the colour transform keeps
// 0 .. 255, and a bit put at every position of two words reads back.  Then the refusals.  Prints "ok".
#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>

#include "jpeg_base.h"

using namespace mvs::jpeg_base;

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

static bool spill(const std::string& path, const std::vector<uint8_t>& v) {
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) return false;
    const bool ok = fwrite(v.data(), 1, v.size(), f) == v.size();
    return fclose(f) == 0 && ok;
}

static void table_checks() {
    Tables T;
    build_tables(50, T);
    for (uint32_t t = 0; t < 2u; ++t) for (uint32_t i = 0; i < 64u; ++i) CHECK(T.quant[t][i] == QUANT_BASE[t][i]);
    build_tables(100, T);
    for (uint32_t t = 0; t < 2u; ++t) for (uint32_t i = 0; i < 64u; ++i) CHECK(T.quant[t][i] == 1u);
    build_tables(1, T);
    for (uint32_t t = 0; t < 2u; ++t) for (uint32_t i = 0; i < 64u; ++i) CHECK(T.quant[t][i] == 255u);
    CHECK(quant_scaled(16, 25) == 32u && quant_scaled(16, 75) == 8u && quant_scaled(99, 90) == 20u);
    bool seen[64] = {false};
    for (uint32_t i = 0; i < 64u; ++i) { CHECK(T.zz_pos[i] < 64u && !seen[T.zz_pos[i]]); seen[T.zz_pos[i] & 63u] = true; CHECK(ZIGZAG[T.zz_pos[i] & 63u] == i); }
    for (uint32_t t = 0; t < 4u; ++t) {   // counts, lengths and prefix freedom
        const uint32_t n = t < 2u ? 16u : 256u, *e = t < 2u ? T.dc[t] : T.ac[t - 2u];
        uint32_t count[17] = {0}, used = 0;
        for (uint32_t s = 0; s < n; ++s) if (e[s]) { CHECK((e[s] >> 16) >= 1u && (e[s] >> 16) <= 16u); ++count[(e[s] >> 16) & 15u ? (e[s] >> 16) : 16u]; ++used; }
        CHECK(used == HUFF_COUNT[t]);
        for (uint32_t l = 1; l <= 16u; ++l) CHECK(count[l] == HUFF_BITS[t][l - 1u]);
        for (uint32_t a = 0; a < n; ++a)
            for (uint32_t b = a + 1; b < n; ++b) {
                if (!e[a] || !e[b]) continue;
                const uint32_t la = e[a] >> 16, lb = e[b] >> 16, k = la < lb ? la : lb;
                CHECK(((e[a] & 0xFFFFu) >> (la - k)) != ((e[b] & 0xFFFFu) >> (lb - k)));
                CHECK((e[a] & 0xFFFFu) != (1u << la) - 1u);   // no code of all ones
            }
    }
    CHECK((T.ac[0][ZRL] >> 16) == 11u && (T.ac[1][ZRL] >> 16) == 10u && (T.ac[0][EOB] >> 16) == 4u && (T.ac[1][EOB] >> 16) == 2u);
    for (uint32_t s = 0; s < 256u; ++s) if (T.ac[0][s]) CHECK((T.ac[0][s] >> 16) + (s & 15u) <= COEF_BITS && (T.ac[1][s] >> 16) + (s & 15u) <= COEF_BITS);
    for (int r = 0; r < 256; r += 5) for (int g = 0; g < 256; g += 3) for (int b = 0; b < 256; b += 5) {
        const int32_t y = luma(r, g, b), cb = chroma_b(r, g, b), cr = chroma_r(r, g, b);
        CHECK(y >= 0 && y <= 255 && cb >= 0 && cb <= 255 && cr >= 0 && cr <= 255);
        if (r == g && g == b) CHECK(y == r && cb == 128 && cr == 128);
    }
    CHECK(chroma_b(0, 0, 255) == 255 && chroma_r(255, 0, 0) == 255 && chroma_b(255, 255, 0) == 0 && chroma_r(0, 255, 255) == 0);
    CHECK(quantise(5, 10, true) == 1 && quantise(-5, 10, true) == -1 && quantise(4, 10, true) == 0 && quantise(-14, 10, true) == -1 && quantise(7, 5, true) == 1 && quantise(8, 5, true) == 2);
    CHECK(quantise(5000, 1, true) == 1023 && quantise(-5000, 1, false) == -5000);
    CHECK(category(0) == 0u && category(1) == 1u && category(-1) == 1u && category(-1023) == 10u && category(1024) == 11u && category(-2040) == 11u);
    for (uint32_t pos = 0; pos < 33u; ++pos)
        for (uint32_t n = 1; n <= COEF_BITS; ++n) {
            uint32_t w[3] = {0, 0, 0}, hi, lo;
            put_words(pos, (1u << n) - 1u, n, hi, lo);
            w[pos >> 5] |= hi; w[(pos >> 5) + 1u] |= lo;
            for (uint32_t bit = 0; bit < 96u; ++bit) CHECK(((image_byte(w, bit >> 3) >> (7u - (bit & 7u))) & 1u) == (bit >= pos && bit < pos + n ? 1u : 0u));
        }
    // the flat block: DC only; pass 1 and pass 2 on a constant
    {
        int32_t t8[8];
        for (uint32_t u = 0; u < 8u; ++u) t8[u] = dct_round1(dct_sum(&T.cosine[u * COS_PITCH], [](uint32_t) { return 127; }));
        CHECK(t8[0] == (2896 * 8 * 127 + 512) >> 10);
        for (uint32_t u = 1; u < 8u; ++u) CHECK(t8[u] == 0);
        CHECK(dct_round2(dct_sum(&T.cosine[0], [&](uint32_t) { return t8[0]; })) == 1016);
    }
    for (uint32_t b = 0; b < 12u; ++b) {
        const int want1[12] = {-1, 0, 1, 2, -1, -1, 3, 6, 7, 8, 4, 5}, want0[12] = {-1, -1, -1, 0, 1, 2, 3, 4, 5, 6, 7, 8};
        CHECK(prev_block(1, b) == want1[b] && prev_block(0, b) == want0[b]);
    }
}

int main(int argc, char** argv) {
    if (argc < 2) { printf("usage: test_jpeg <dir>\n"); return 2; }
    table_checks();
    const std::string dir(argv[1]);
    FILE* mf = fopen((dir + "/manifest").c_str(), "r");
    if (!mf) { printf("no manifest\n"); return 2; }
    char kind[32], name[256]; unsigned w, h;
    std::string msg;
    std::vector<uint8_t> out;
    while (fscanf(mf, "%31s %255s %u %u", kind, name, &w, &h) == 4) {
        const std::vector<uint8_t> in = slurp(dir + "/" + name + ".rgb");
        CHECK(in.size() == (size_t)3 * w * h);
        if (in.size() != (size_t)3 * w * h) continue;
        for (int sub = 0; sub < 2; ++sub)
            for (int q : {1, 50, 90, 100}) {
                CHECK(encode_jpeg(in.data(), w, h, q, sub, out, msg) == MVS_OK);
                CHECK(out.size() >= HEADER_BYTES + 2u && out[HEADER_BYTES - 1] == 0 && out[HEADER_BYTES - 14] == 0xFF && out[HEADER_BYTES - 13] == 0xDA);
                CHECK(spill(dir + "/" + name + "_s" + std::to_string(sub) + "_q" + std::to_string(q) + ".jpg", out));
            }
    }
    fclose(mf);
    const uint8_t px[3] = {1, 2, 3};
    CHECK(encode_jpeg(nullptr, 1, 1, 90, 1, out, msg) == MVS_ERR_INVALID);
    CHECK(encode_jpeg(px, 0, 1, 90, 1, out, msg) == MVS_ERR_INVALID);
    CHECK(encode_jpeg(px, 1, 1, 0, 1, out, msg) == MVS_ERR_INVALID);
    CHECK(encode_jpeg(px, 1, 1, 101, 1, out, msg) == MVS_ERR_INVALID);
    CHECK(encode_jpeg(px, 1, 1, 90, 2, out, msg) == MVS_ERR_INVALID);
    CHECK(encode_jpeg(px, 1, 1, 90, -1, out, msg) == MVS_ERR_INVALID);
    CHECK(encode_jpeg(px, 65536, 1, 90, 1, out, msg) == MVS_ERR_UNSUPPORTED);
    CHECK(encode_jpeg(px, 1, 65536, 90, 0, out, msg) == MVS_ERR_UNSUPPORTED);
    CHECK(encode_jpeg(px, 1, 1, 90, 1, out, msg) == MVS_OK && out.size() > HEADER_BYTES + 2u);
    if (failures) { printf("%d failures\n", failures); return 1; }
    printf("ok\n");
    return 0;
}
