// tone.h -- tone mapping `gamma` of rows f5 - f10 (generate_texture_patches.cpp:126-132, generate_texture_atlases.cpp:102-104): ONE text
//   of pow for the host and the device.  Host-and-device header (MVS_HD), compiled by hipcc into the kernels and the product library's
//   host twin and by g++ into tests/cpp/test_tone.cpp; -ffp-contract=off as for dmath.h.  DESIGN.md section 4 "Tone mapping".
//
//   DEFINED HERE (MVE is absent): mve::image::gamma_correct(image, power) on a float image is, from recollection, std::pow(value, power)
//   on every value of every channel.  std::pow is not the same bits in glibc and in the device library, so gamma_pow below takes its
//   place on both sides: no libm call, only IEEE fp64 + - * /, fma, conversions and integer operations on the bits -- every step is
//   correctly rounded by definition, so host and device agree bit for bit.
//
//   gamma_pow(x, power), power finite and > 0 (the two exponents in use are (double)2.2f and (double)(1.0f / 2.2f)):
//     NaN -> NaN;  x < 0 (-inf included) -> NaN (both exponents are non-integers);  +-0 -> +0;  +inf -> +inf;  otherwise
//     1. x = m 2^e with m in [1/sqrt 2, sqrt 2), taken from the bits (a subnormal is normalised first with a count of leading zeros);
//     2. s = (m - 1) / (m + 1), log m = 2 s (1 + s^2/3 + s^4/5 + ... + s^22/23), Horner in s^2 with fma  (|s| <= 0.1716: the first
//        term left out is below 2^-64 of the sum);
//     3. log x = e LN2_HI + (log m + e LN2_LO)  (LN2_HI has 21 trailing zero bits: the first product is exact);
//     4. y = (double)power * log x, clamped to [-120, 100] (beyond: the fp32 result is 0 or +inf either way);
//     5. k = round-half-away(y / ln 2) by conversion, r = fma(-k, LN2_LO, fma(-k, LN2_HI, y)), |r| <= 0.3466;
//        exp r = Taylor polynomial of degree 13, Horner with fma (remainder below 2^-57);
//     6. the product with 2^k, which is put together from the exponent bits (k in [-174, 145]: a normal double, the product exact);
//     7. one conversion to float, which rounds, overflows to +inf and produces subnormal results.
//   Error: the fp64 value is within a relative 2^-43 of x^power at |y| <= 230, so the fp32 result is within 0.5 ulp + 2^-19 ulp.
#pragma once
#include <stdint.h>
#include <string.h>

#ifndef MVS_HD
#if defined(__HIPCC__)
#define MVS_HD __host__ __device__ __forceinline__
#else
#define MVS_HD inline
#endif
#endif

namespace mvs {

enum { TONE_NONE = 0, TONE_GAMMA = 1 };                     // mvs_*_params.tone_mapping (tex::ToneMapping, settings.h)
constexpr float TONE_POWER = 2.2f;                          // generate_texture_patches.cpp:131
constexpr float TONE_INV_POWER = 1.0f / 2.2f;               // generate_texture_atlases.cpp:103

MVS_HD double tone_from_bits(uint64_t u) { double d; memcpy(&d, &u, sizeof(d)); return d; }
MVS_HD double tone_fma(double a, double b, double c) { return __builtin_fma(a, b, c); }

MVS_HD float gamma_pow(float x, float power) {
    uint32_t u;
    memcpy(&u, &x, sizeof(u));
    const uint32_t qnan = 0x7FC00000u, pinf = 0x7F800000u;
    float special;
    if ((u & 0x7FFFFFFFu) > pinf) { memcpy(&special, &qnan, sizeof(special)); return special; }   // NaN
    if ((u & 0x7FFFFFFFu) == 0u) return 0.0f;                                                     // +-0
    if (u >> 31) { memcpy(&special, &qnan, sizeof(special)); return special; }                    // x < 0
    if (u == pinf) return x;                                                                      // +inf
    // 1. mantissa and exponent
    int e = (int)(u >> 23);
    uint32_t m = u & 0x007FFFFFu;
    if (e == 0) {                                    // subnormal: m != 0
        const int shift = __builtin_clz(m) - 8;      // brings the leading one to bit 23
        m = (m << shift) & 0x007FFFFFu;
        e = 1 - shift;
    }
    e -= 127;
    uint64_t mbits = 0x3FF0000000000000ull | ((uint64_t)m << 29);      // [1, 2)
    if (m > 0x003504F3u) { mbits -= 0x0010000000000000ull; e += 1; }   // above float(sqrt 2): halve
    const double md = tone_from_bits(mbits);
    // 2. log m
    const double s = (md - 1.0) / (md + 1.0);
    const double s2 = s * s;
    double q = 1.0 / 23.0;
    q = tone_fma(q, s2, 1.0 / 21.0);
    q = tone_fma(q, s2, 1.0 / 19.0);
    q = tone_fma(q, s2, 1.0 / 17.0);
    q = tone_fma(q, s2, 1.0 / 15.0);
    q = tone_fma(q, s2, 1.0 / 13.0);
    q = tone_fma(q, s2, 1.0 / 11.0);
    q = tone_fma(q, s2, 1.0 / 9.0);
    q = tone_fma(q, s2, 1.0 / 7.0);
    q = tone_fma(q, s2, 1.0 / 5.0);
    q = tone_fma(q, s2, 1.0 / 3.0);
    q = tone_fma(q, s2, 1.0);
    const double logm = (2.0 * s) * q;
    // 3. log x
    const double LN2_HI = tone_from_bits(0x3FE62E42FEE00000ull);   // 6.93147180369123816490e-01
    const double LN2_LO = tone_from_bits(0x3DEA39EF35793C76ull);   // 1.90821492927058770002e-10
    const double INV_LN2 = tone_from_bits(0x3FF71547652B82FEull);  // 1.44269504088896338700e+00
    const double ed = (double)e;
    const double logx = ed * LN2_HI + (logm + ed * LN2_LO);
    // 4. y
    double y = (double)power * logx;
    if (y > 100.0) y = 100.0;
    if (y < -120.0) y = -120.0;
    // 5. exp y
    const double t = y * INV_LN2;
    const int k = (int)(t < 0.0 ? t - 0.5 : t + 0.5);
    const double kd = (double)k;
    const double r = tone_fma(-kd, LN2_LO, tone_fma(-kd, LN2_HI, y));
    double p = 1.0 / 6227020800.0;
    p = tone_fma(p, r, 1.0 / 479001600.0);
    p = tone_fma(p, r, 1.0 / 39916800.0);
    p = tone_fma(p, r, 1.0 / 3628800.0);
    p = tone_fma(p, r, 1.0 / 362880.0);
    p = tone_fma(p, r, 1.0 / 40320.0);
    p = tone_fma(p, r, 1.0 / 5040.0);
    p = tone_fma(p, r, 1.0 / 720.0);
    p = tone_fma(p, r, 1.0 / 120.0);
    p = tone_fma(p, r, 1.0 / 24.0);
    p = tone_fma(p, r, 1.0 / 6.0);
    p = tone_fma(p, r, 0.5);
    p = tone_fma(p, r, 1.0);
    p = tone_fma(p, r, 1.0);
    // 6.-7.
    const double scale = tone_from_bits((uint64_t)(k + 1023) << 52);
    return (float)(p * scale);
}

// the texel table of a mode: table[b] = the value of byte b of a view's image (rows f5, f6, f10)
MVS_HD float tone_table_entry(int mode, int b) {
    const float v = (float)b / 255.0f;               // byte_to_float_image
    return mode == TONE_GAMMA ? gamma_pow(v, TONE_POWER) : v;
}

}  // namespace mvs
