// fmt6.h -- the numbers of the model output (row f9; DESIGN.md section 4 "Model output" item 2): a float as glibc prints it through
// `std::fixed << std::setprecision(6)` / printf("%.6f") -- the EXACT value rounded to six decimals, ties to even, '-' whenever the sign
// bit is set, the integer part exact at every magnitude, inf / -inf / nan / -nan by sign bit -- and unsigned integers in plain decimal.
// Integer arithmetic only, the same on host and device: k_model.hip formats with it into LDS, tests/cpp/test_png_fmt.cpp runs it on the
// CPU against snprintf.  No arrays, no recursion: a caller that asks for the length first and then lets *_put write that many bytes
// keeps every digit loop in registers.
//
//   |x| < 2^64 ("narrow"):  x = m 2^e with m < 2^24.  e >= 0: the integer m << e, fraction 000000.  e < 0: N = m 10^6 < 2^44,
//                           q = N >> -e rounded by the remainder against the half (ties to even), printed as q / 10^6 '.' q % 10^6.
//   |x| >= 2^64 ("wide"):   e in [41, 104]: m << e in four 32-bit limbs, divided by 10^9 limb by limb (64 / 32-bit divisions by a
//                           constant) into at most five groups of nine digits; the fraction is 000000.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FMT6_HD __host__ __device__ inline
#else
#define FMT6_HD inline
#endif

namespace fmt6 {

constexpr uint32_t MAX_FLOAT_LEN = 47;   // '-' + 39 digits + '.' + 6 digits (FLT_MAX)

FMT6_HD uint32_t digits_u64(uint64_t v) {   // decimal digits of v (1 for 0)
    uint32_t n = 1;
    while (v >= 10000ull) { v /= 10000ull; n += 4; }
    const uint32_t w = (uint32_t)v;
    return n + (w >= 10u) + (w >= 100u) + (w >= 1000u);
}
FMT6_HD uint32_t u32_len(uint32_t v) { return 1u + (v >= 10u) + (v >= 100u) + (v >= 1000u) + (v >= 10000u) + (v >= 100000u) + (v >= 1000000u) + (v >= 10000000u) + (v >= 100000000u) + (v >= 1000000000u); }
// the `n` low decimal digits of v, most significant first, at dst[0 .. n)
FMT6_HD void put_digits(char* dst, uint64_t v, uint32_t n) {
    for (uint32_t i = n; i-- > 0;) { dst[i] = (char)('0' + (uint32_t)(v % 10ull)); v /= 10ull; }
}
FMT6_HD void put_digits32(char* dst, uint32_t v, uint32_t n) {
    for (uint32_t i = n; i-- > 0;) { dst[i] = (char)('0' + v % 10u); v /= 10u; }
}
FMT6_HD uint32_t u32_put(char* dst, uint32_t v) { const uint32_t n = u32_len(v); put_digits32(dst, v, n); return n; }

FMT6_HD bool is_nonfinite(uint32_t bits) { return ((bits >> 23) & 0xFFu) == 0xFFu; }
FMT6_HD bool is_wide(uint32_t bits) { const uint32_t ex = (bits >> 23) & 0xFFu; return ex >= 191u && ex != 0xFFu; }   // 2^64 <= |x| < inf

// |x| < 2^64: integer part and the six decimals as one number below 10^6
FMT6_HD void narrow(uint32_t bits, uint64_t& ip, uint32_t& frac) {
    const uint32_t ex = (bits >> 23) & 0xFFu, man = bits & 0x7FFFFFu;
    const uint64_t m = ex ? (uint64_t)(man | 0x800000u) : (uint64_t)man;
    const int e = (int)(ex ? ex : 1u) - 150;
    if (e >= 0) { ip = m << e; frac = 0; return; }   // e <= 40: below 2^64
    const uint32_t s = (uint32_t)(-e);
    const uint64_t N = m * 1000000ull;               // < 2^44
    if (s >= 46u) { ip = 0; frac = 0; return; }      // N < 2^44 <= half: rounds to zero
    uint64_t q = N >> s;
    const uint64_t r = N & ((1ull << s) - 1ull), half = 1ull << (s - 1u);
    q += (r > half || (r == half && (q & 1ull))) ? 1ull : 0ull;
    ip = q / 1000000ull; frac = (uint32_t)(q % 1000000ull);
}

// |x| >= 2^64: m << e as limbs, least significant first
struct Limbs { uint32_t l0, l1, l2, l3; };
FMT6_HD Limbs wide_limbs(uint32_t bits) {
    const uint32_t ex = (bits >> 23) & 0xFFu;
    const uint64_t m = (uint64_t)((bits & 0x7FFFFFu) | 0x800000u);
    const uint32_t e = ex - 150u;   // 41 .. 104
    uint64_t lo, hi;
    if (e < 64u) { lo = m << e; hi = m >> (64u - e); } else { lo = 0; hi = m << (e - 64u); }
    return Limbs{(uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32)};
}
FMT6_HD uint32_t div1e9(Limbs& v) {   // v /= 10^9, returns the remainder
    uint64_t t = (uint64_t)v.l3;
    v.l3 = (uint32_t)(t / 1000000000ull); t = ((t % 1000000000ull) << 32) | v.l2;
    v.l2 = (uint32_t)(t / 1000000000ull); t = ((t % 1000000000ull) << 32) | v.l1;
    v.l1 = (uint32_t)(t / 1000000000ull); t = ((t % 1000000000ull) << 32) | v.l0;
    v.l0 = (uint32_t)(t / 1000000000ull);
    return (uint32_t)(t % 1000000000ull);
}
FMT6_HD bool limbs_zero(const Limbs& v) { return (v.l0 | v.l1 | v.l2 | v.l3) == 0u; }
FMT6_HD uint32_t wide_int_digits(uint32_t bits) {
    Limbs v = wide_limbs(bits);
    uint32_t n = 0, top = 0;
    while (!limbs_zero(v)) { top = div1e9(v); n += 9; }
    return n - 9u + u32_len(top);   // at least 2^64: three groups or more
}

FMT6_HD uint32_t float_len(uint32_t bits) {
    const uint32_t sign = bits >> 31;
    if (is_nonfinite(bits)) return sign + 3u;
    if (is_wide(bits)) return sign + wide_int_digits(bits) + 7u;
    uint64_t ip; uint32_t fr;
    narrow(bits, ip, fr);
    return sign + digits_u64(ip) + 7u;
}

// writes float_len(bits) bytes at dst (`len` = that length, which the caller has: the digits are laid down from the end)
FMT6_HD void float_put(char* dst, uint32_t bits, uint32_t len) {
    const uint32_t sign = bits >> 31;
    if (sign) dst[0] = '-';
    if (is_nonfinite(bits)) {
        const bool inf = (bits & 0x7FFFFFu) == 0u;
        dst[sign] = inf ? 'i' : 'n'; dst[sign + 1u] = inf ? 'n' : 'a'; dst[sign + 2u] = inf ? 'f' : 'n';
        return;
    }
    dst[len - 7u] = '.';
    if (is_wide(bits)) {
        put_digits32(dst + len - 6u, 0u, 6u);
        Limbs v = wide_limbs(bits);
        uint32_t end = len - 7u;   // one past the last integer digit not written yet
        while (true) {
            const uint32_t g = div1e9(v);
            if (limbs_zero(v)) { put_digits32(dst + sign, g, end - sign); break; }
            put_digits32(dst + end - 9u, g, 9u); end -= 9u;
        }
        return;
    }
    uint64_t ip; uint32_t fr;
    narrow(bits, ip, fr);
    put_digits32(dst + len - 6u, fr, 6u);
    put_digits(dst + sign, ip, len - 7u - sign);
}

}  // namespace fmt6
