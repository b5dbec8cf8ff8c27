// test_tone.cpp -- csrc/tone.h on the host, as a program of its own (tests/test_tone_mapping_host.py builds it with the address and
// undefined-behaviour sanitizers and runs it): the special values, the texel table, the round trip through the byte, and -- for the
// comparison with the product library, which compiles the same header -- gamma_pow of every float of <dir>/inputs.f32 under both
// exponents, written to <dir>/pow_2.2.f32 and <dir>/pow_inv.f32, and the two tables to <dir>/table_none.f32 / table_gamma.f32.
#include "tone.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

using namespace mvs;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

static uint32_t bits(float x) { uint32_t u; memcpy(&u, &x, sizeof(u)); return u; }
static float from_bits(uint32_t u) { float x; memcpy(&x, &u, sizeof(x)); return x; }

// mve::image::float_to_byte_image(img, 0.0f, 1.0f) on one value, as row f8 states it (k_atlas.hip, tests/tools/atlas_model.cpp)
static uint8_t float_to_byte(float x) {
    float v = (0.0f < x) ? x : 0.0f;
    v = (v < 1.0f) ? v : 1.0f;
    v = (255.0f * (v - 0.0f)) / (1.0f - 0.0f);
    return (uint8_t)(v + 0.5f);
}

static std::vector<float> read_floats(const std::string& path) {
    std::vector<float> v;
    if (FILE* f = std::fopen(path.c_str(), "rb")) {
        float buf[4096];
        size_t n;
        while ((n = std::fread(buf, sizeof(float), 4096, f)) > 0) v.insert(v.end(), buf, buf + n);
        std::fclose(f);
    }
    return v;
}
static void write_floats(const std::string& path, const std::vector<float>& v) {
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) { std::printf("cannot write %s\n", path.c_str()); std::exit(2); }
    if (!v.empty()) std::fwrite(v.data(), sizeof(float), v.size(), f);
    std::fclose(f);
}

int main(int argc, char** argv) {
    const float powers[2] = {TONE_POWER, TONE_INV_POWER};
    CHECK(bits(TONE_POWER) == 0x400CCCCDu);
    CHECK(bits(TONE_INV_POWER) == bits(1.0f / 2.2f));
    for (float p : powers) {
        CHECK(std::isnan(gamma_pow(from_bits(0x7FC00000u), p)));          // quiet NaN
        CHECK(std::isnan(gamma_pow(from_bits(0x7F800001u), p)));          // signalling NaN
        CHECK(std::isnan(gamma_pow(from_bits(0xFFC12345u), p)));          // NaN with the sign set
        CHECK(std::isnan(gamma_pow(-1.0f, p)));
        CHECK(std::isnan(gamma_pow(from_bits(0x80000001u), p)));          // the smallest negative subnormal
        CHECK(std::isnan(gamma_pow(from_bits(0xFF800000u), p)));          // -inf
        CHECK(bits(gamma_pow(0.0f, p)) == 0u);
        CHECK(bits(gamma_pow(-0.0f, p)) == 0u);                           // +0, not -0
        CHECK(bits(gamma_pow(from_bits(0x7F800000u), p)) == 0x7F800000u); // +inf
        CHECK(bits(gamma_pow(1.0f, p)) == 0x3F800000u);
        CHECK(gamma_pow(from_bits(0x00000001u), p) >= 0.0f);              // subnormal inputs take the same path
        CHECK(gamma_pow(from_bits(0x007FFFFFu), p) >= 0.0f);
        CHECK(gamma_pow(from_bits(0x7F7FFFFFu), p) > 1.0f);               // the largest finite float
    }
    CHECK(bits(gamma_pow(from_bits(0x7F7FFFFFu), TONE_POWER)) == 0x7F800000u);   // overflows to +inf
    CHECK(gamma_pow(from_bits(0x00000001u), TONE_POWER) == 0.0f);                // underflows to +0
    CHECK(std::isfinite(gamma_pow(from_bits(0x7F7FFFFFu), TONE_INV_POWER)));
    CHECK(gamma_pow(from_bits(0x00000001u), TONE_INV_POWER) > 0.0f);
    // a subnormal RESULT: x^2.2 = 2^-140 at x = 2^(-140 / 2.2)
    { const float r = gamma_pow(std::ldexp(1.0f, -64), TONE_POWER); CHECK(r > 0.0f && r < from_bits(0x00800000u)); }
    // the tables
    std::vector<float> none(256), gamma(256);
    for (int b = 0; b < 256; ++b) { none[b] = tone_table_entry(TONE_NONE, b); gamma[b] = tone_table_entry(TONE_GAMMA, b); }
    CHECK(bits(gamma[0]) == 0u && bits(gamma[255]) == 0x3F800000u);
    for (int b = 0; b < 256; ++b) {
        CHECK(bits(none[b]) == bits((float)b / 255.0f));
        CHECK(bits(gamma[b]) == bits(gamma_pow((float)b / 255.0f, TONE_POWER)));
        if (b) CHECK(gamma[b] > gamma[b - 1]);
        CHECK(float_to_byte(gamma_pow(gamma[b], TONE_INV_POWER)) == b);   // row f10's round trip
        CHECK(float_to_byte(none[b]) == b);
    }
    if (argc > 1) {
        const std::string dir(argv[1]);
        const std::vector<float> in = read_floats(dir + "/inputs.f32");
        for (int k = 0; k < 2; ++k) {
            std::vector<float> out(in.size());
            for (size_t i = 0; i < in.size(); ++i) out[i] = gamma_pow(in[i], powers[k]);
            write_floats(dir + (k ? "/pow_inv.f32" : "/pow_2.2.f32"), out);
        }
        write_floats(dir + "/table_none.f32", none);
        write_floats(dir + "/table_gamma.f32", gamma);
    }
    if (failures) return 1;
    std::printf("ok\n");
    return 0;
}
