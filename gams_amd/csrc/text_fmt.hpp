// text_fmt.hpp -- the two float formats of the text entries in integer arithmetic, shared by the device formatters
// (text.hip) and the host layer (gams_host_c.cpp exposes them to the tests): `{:.4}` of an anno proportion and the
// shortest round-trip `{}` of a peak amplitude.  Plain C++: no HIP header needed.
#pragma once

#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define GAMS_HD __host__ __device__
#else
#define GAMS_HD
#endif

// anno.rs:140 prints the f32 prop as `{:.4}`: the exact binary value rounded half to even at the fourth decimal
// (what "%.4f" of the widened double prints).  For p in [0, 1] that is q / 10^4 with the integer q below, 0 .. 10000.
// p = m * 2^e with m < 2^24: below 2^-15 (< 5e-5) the answer is 0; otherwise e >= -38, so m * 10^4 < 2^38 and the
// quotient and remainder by 2^-e are exact in 64 bits.  p must be a finite value in [0, 1] (the callers check).
// Shared by the text (gams_fmt_prop4) and the sw summary's Prop sums, as sw_f4_units / sw_put_f4 are.
GAMS_HD inline uint32_t gams_prop4_units(float p) {
    uint32_t b;
    memcpy(&b, &p, 4);
    const uint32_t ex = (b >> 23) & 0xffu;
    if (ex < 112u) return 0u;                       // p < 2^-15; ex <= 127 since p <= 1
    const uint64_t m = (uint64_t)((b & 0x7fffffu) | 0x800000u);
    const uint32_t s = 150u - ex;                   // p = m / 2^s, 23 <= s <= 38
    const uint64_t num = m * 10000u;
    uint64_t qq = num >> s;
    const uint64_t r = num & ((1ull << s) - 1u), half = 1ull << (s - 1u);
    if (r > half || (r == half && (qq & 1u))) ++qq;
    return (uint32_t)qq;
}

// ... as text: always six bytes "d.dddd", written to out[0..6).  Returns false (nothing written) when p is not a finite
// value in [0, 1].
GAMS_HD inline bool gams_fmt_prop4(float p, char *out) {
    if (!(p >= 0.0f && p <= 1.0f)) return false;   // NaN fails both
    const uint32_t q = gams_prop4_units(p);
    out[0] = (char)('0' + q / 10000u);
    out[1] = '.';
    out[2] = (char)('0' + q / 1000u % 10u);
    out[3] = (char)('0' + q / 100u % 10u);
    out[4] = (char)('0' + q / 10u % 10u);
    out[5] = (char)('0' + q % 10u);
    return true;
}

// peak.rs prints the f32 amplitudes |gc - gc'| with `{}`: the shortest decimal that parses back to the same f32, the
// closest to v where several are equally short, in positional notation ("0", "0.0268", "0.026800007", "1") -- what
// gams::fmt_f32 makes of std::to_chars.  For a finite v in [0, 1] the text goes to out[0..len) and len is returned;
// out == nullptr: the length only.  Returns 0 (nothing written) for NaN, -0, anything outside [0, 1] and a nonzero v
// below 2^-64, which the 128-bit arithmetic below does not cover: the caller flags such a value.  len <= 31.
//
// v = m * 2^-s with m < 2^24 (23 <= s <= 87).  With q decimals the two candidates are D = floor(v * 10^q) and D + 1;
// in units of 2^-s * 10^-q they lie rl = m * 10^q - D * 2^s below and rh = 2^s - rl above v, and one of them parses
// back to v when it is within half the gap to v's neighbour on that side: 2 * r <= 10^q (the bound itself only for an
// even m: ties parse to even).  Below a power of two the gap is half as wide (4 * rl <= 10^q), so there the closer
// candidate may fail where the other one passes: both are tried, the closer of those that pass is taken.  The first q
// with a passing candidate gives the shortest text; nine significant digits always pass, so q <= 28 and every product
// stays below 2^124.  No division wider than 64 bits (there is no 128-bit divide on the device).
GAMS_HD inline uint32_t gams_fmt_f32_short(float v, char *out) {
    __extension__ typedef unsigned __int128 u128;
    if (!(v >= 0.0f && v <= 1.0f)) return 0;        // NaN fails both
    uint32_t b;
    memcpy(&b, &v, 4);
    if (b == 0u) {
        if (out) out[0] = '0';
        return 1;
    }
    const uint32_t ex = b >> 23;
    if ((b >> 31) || ex < 63u) return 0;            // -0; below 2^-64
    const uint64_t m = (uint64_t)((b & 0x7fffffu) | 0x800000u);
    const uint32_t s = 150u - ex;                   // v = m / 2^s
    const bool even = !(m & 1u), pow2 = (b & 0x7fffffu) == 0u;
    const u128 one = (u128)1 << s;
    u128 p10 = 1;
    for (uint32_t q = 0; q <= 28u; ++q, p10 *= 10u) {
        const u128 num = (u128)m * p10;
        const u128 d = num >> s;
        const u128 rl = num - (d << s), rh = one - rl;
        const u128 wl = pow2 ? 4u * rl : 2u * rl, wh = 2u * rh;
        const bool okl = d != 0u && (even ? wl <= p10 : wl < p10);
        const bool okh = even ? wh <= p10 : wh < p10;
        if (!okl && !okh) continue;
        if ((d >> 40) != 0u) return 0;              // (more than nine digits: cannot happen)
        uint64_t r = (uint64_t)d;
        if (!okl || (okh && (rh < rl || (rh == rl && (r & 1u))))) ++r;
        if (q == 0u) {                              // r == 1: v is 1
            if (out) out[0] = '1';
            return 1;
        }
        if (out) {                                  // "0." and r as q decimals
            out[0] = '0';
            out[1] = '.';
            for (uint32_t k = q; k > 0u; --k) {
                out[1u + k] = (char)('0' + r % 10u);
                r /= 10u;
            }
        }
        return 2u + q;
    }
    return 0;
}

// The ΔG column prints its f32 as `{:.4}`: the exact binary value rounded half to even at the fourth
// decimal, the sign kept even where every digit is zero ("-0.0000") -- what "%.4f" of the widened double prints.
// |v| = m * 2^-s with m < 2^24; below 2^20 s is at least 4, m * 10^4 stays under 2^38 and quotient and remainder by 2^s
// are exact in 64 bits; from s = 39 on the value is below half a unit and q is 0.  The text goes to out[0..len), len <= 13
// is returned; out == nullptr: the length only.  Returns 0 (nothing written) for NaN, an infinity and |v| >= 2^20: the
// caller flags such a value.
constexpr uint32_t kGamsDg4MaxLen = 13;
GAMS_HD inline uint32_t gams_fmt_dg4(float v, char *out) {
    uint32_t b;
    memcpy(&b, &v, 4);
    const uint32_t ex = (b >> 23) & 0xffu;
    if (ex >= 147u) return 0;                       // 2^20 and beyond, infinities, NaN
    const uint32_t s = 150u - ex;                   // >= 4
    uint64_t q = 0;
    if (s < 39u) {
        const uint64_t num = (uint64_t)((b & 0x7fffffu) | 0x800000u) * 10000u;
        q = num >> s;
        const uint64_t r = num & ((1ull << s) - 1u), half = 1ull << (s - 1u);
        if (r > half || (r == half && (q & 1u))) ++q;
    }
    const uint32_t neg = b >> 31;
    uint32_t ip = (uint32_t)(q / 10000u), fr = (uint32_t)(q % 10000u), digits = 1;
    for (uint32_t t = ip; t >= 10u; t /= 10u) ++digits;
    const uint32_t len = neg + digits + 5u;
    if (out) {
        if (neg) out[0] = '-';
        for (uint32_t k = digits; k > 0u; --k) {
            out[neg + k - 1u] = (char)('0' + ip % 10u);
            ip /= 10u;
        }
        char *const f = out + neg + digits;
        f[0] = '.';
        f[1] = (char)('0' + fr / 1000u);
        f[2] = (char)('0' + fr / 100u % 10u);
        f[3] = (char)('0' + fr / 10u % 10u);
        f[4] = (char)('0' + fr % 10u);
    }
    return len;
}
