// Stand-alone host program for csrc/fmt6.h and csrc/png_io.h (tests/test_png_io_host.py compiles it with the address and
// undefined-behaviour sanitizers).  argv[1]: a directory.
//   fmt6: every exponent 0 .. 255 with mantissas 0, 1, 0x7FFFFF and 64 random ones, both signs; every k / 2^n with n <= 12, k < 4096 (the
//   ties), both signs; 2^20 random bit patterns; unsigned integers around every power of ten -- against snprintf.
//   png_io: PNGs of 1 x 1, 3 x 5, 256 x 256 and 300 x 100 (its rows cross the 65535-byte stored block) of the pattern
//   pixel(x, y, c) = (7 x + 13 y + 29 c + x y) & 255, at level 0 as <w>x<h>_l0.png and, where libz.so.1 resolves, level 1 as <w>x<h>_l1.png.
// Prints "ok zlib=<0|1>".
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <random>
#include <string>
#include <vector>

#include "fmt6.h"
#include "png_io.h"

static int failures = 0;

static void check_float(uint32_t bits) {
    float x; memcpy(&x, &bits, 4);
    char want[96]; snprintf(want, sizeof(want), "%.6f", (double)x);
    if (isnan(x)) snprintf(want, sizeof(want), "%s", (bits >> 31) ? "-nan" : "nan");   // by sign bit, whatever the conversion to double did
    char got[96]; memset(got, '#', sizeof(got));
    const uint32_t n = fmt6::float_len(bits);
    if (n > fmt6::MAX_FLOAT_LEN) { if (failures++ < 10) printf("0x%08x: length %u\n", bits, n); return; }
    fmt6::float_put(got + 1, bits, n);
    const bool wide = isfinite(x) && fabsf(x) >= 18446744073709551616.0f;
    if (n != strlen(want) || memcmp(got + 1, want, n) != 0 || got[0] != '#' || got[n + 1] != '#' || wide != fmt6::is_wide(bits) || fmt6::is_nonfinite(bits) != !isfinite(x)) {
        got[n + 1] = 0;
        if (failures++ < 10) printf("0x%08x: got %s want %s\n", bits, got + 1, want);
    }
}

static void check_u32(uint32_t v) {
    char want[16]; snprintf(want, sizeof(want), "%u", v);
    char got[16]; memset(got, '#', sizeof(got));
    const uint32_t n = fmt6::u32_put(got + 1, v);
    if (n != strlen(want) || n != fmt6::u32_len(v) || memcmp(got + 1, want, n) != 0 || got[0] != '#' || got[n + 1] != '#') { if (failures++ < 10) printf("%u: wrong digits\n", v); }
}

int main(int argc, char** argv) {
    if (argc < 2) { printf("usage: test_png_fmt <directory>\n"); return 2; }
    std::mt19937 rng(20240611u);
    for (uint32_t ex = 0; ex < 256; ++ex)
        for (uint32_t sign = 0; sign < 2; ++sign) {
            for (uint32_t man : {0u, 1u, 0x7FFFFFu}) check_float(sign << 31 | ex << 23 | man);
            for (int k = 0; k < 64; ++k) check_float(sign << 31 | ex << 23 | (rng() & 0x7FFFFFu));
        }
    for (int n = 0; n <= 12; ++n)
        for (int k = 0; k < 4096; ++k)
            for (float s : {1.0f, -1.0f}) {
                const float x = s * ldexpf((float)k, -n);
                uint32_t bits; memcpy(&bits, &x, 4);
                check_float(bits);
            }
    for (int k = 0; k < (1 << 20); ++k) check_float((uint32_t)rng());
    for (const float x : {0.0078125f, 0.0234375f, -1e-7f, 3.402823466e38f, -3.402823466e38f, 18446744073709551616.0f, 18446742974197923840.0f, 999999.9375f, 0.9999995f})
        { uint32_t bits; memcpy(&bits, &x, 4); check_float(bits); }
    for (uint64_t p = 1; p <= 10000000000ull; p *= 10)
        for (int d = -2; d <= 2; ++d) { const uint64_t v = p + (uint64_t)(int64_t)d; if (v <= 0xFFFFFFFFull) check_u32((uint32_t)v); }
    check_u32(0u); check_u32(0xFFFFFFFFu);

    const bool have_z = mvs::png_zlib_available();
    const unsigned sizes[4][2] = {{1, 1}, {3, 5}, {256, 256}, {300, 100}};
    for (const auto& wh : sizes) {
        const unsigned w = wh[0], h = wh[1];
        std::vector<uint8_t> rgb((size_t)3 * w * h);
        for (unsigned y = 0; y < h; ++y)
            for (unsigned x = 0; x < w; ++x)
                for (unsigned c = 0; c < 3; ++c) rgb[((size_t)y * w + x) * 3 + c] = (uint8_t)((7 * x + 13 * y + 29 * c + x * y) & 255u);
        for (int level = 0; level <= (have_z ? 1 : 0); ++level) {
            std::string msg;
            const std::string path = std::string(argv[1]) + "/" + std::to_string(w) + "x" + std::to_string(h) + "_l" + std::to_string(level) + ".png";
            if (mvs::write_png(path.c_str(), rgb.data(), w, h, level, msg) != MVS_OK) { if (failures++ < 10) printf("%s: %s\n", path.c_str(), msg.c_str()); }
        }
    }
    std::string msg; std::vector<uint8_t> png; const uint8_t px[3] = {1, 2, 3};
    if (mvs::encode_png(px, 0, 1, 0, png, msg) != MVS_ERR_INVALID || mvs::encode_png(nullptr, 1, 1, 0, png, msg) != MVS_ERR_INVALID || mvs::encode_png(px, 1, 1, 10, png, msg) != MVS_ERR_INVALID)
        { failures++; printf("encode_png accepted a bad argument\n"); }
    if (mvs::write_png((std::string(argv[1]) + "/no/such/dir/x.png").c_str(), px, 1, 1, 0, msg) != MVS_ERR_INVALID) { failures++; printf("write_png: no error for a missing directory\n"); }
    if (failures) { printf("%d failures\n", failures); return 1; }
    printf("ok zlib=%d\n", have_z ? 1 : 0);
    return 0;
}
