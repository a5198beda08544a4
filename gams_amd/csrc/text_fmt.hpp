// text_fmt.hpp -- `{:.4}` of an anno proportion in integer arithmetic, shared by the device formatter
// (text.hip) and the host layer (gams_host_c.cpp exposes it to the tests).  Plain C++: no HIP header needed.
#pragma once

#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define GAMS_HD __host__ __device__
#else
#define GAMS_HD
#endif

// anno.rs:140 prints the f32 prop as `{:.4}`: the exact binary value rounded half to even at the fourth decimal
// (what "%.4f" of the widened double prints).  For p in [0, 1] the text is always six bytes "d.dddd", written to
// out[0..6).  p = m * 2^e with m < 2^24: below 2^-15 (< 5e-5) the answer is 0.0000; otherwise e >= -38, so
// m * 10^4 < 2^38 and the quotient and remainder by 2^-e are exact in 64 bits.  Returns false (nothing written)
// when p is not a finite value in [0, 1].
GAMS_HD inline bool gams_fmt_prop4(float p, char *out) {
    if (!(p >= 0.0f && p <= 1.0f)) return false;   // NaN fails both
    uint32_t b;
    memcpy(&b, &p, 4);
    const uint32_t ex = (b >> 23) & 0xffu;
    uint32_t q = 0;
    if (ex >= 112u) {                               // p >= 2^-15; ex <= 127 since p <= 1
        const uint64_t m = (uint64_t)((b & 0x7fffffu) | 0x800000u);
        const uint32_t s = 150u - ex;               // p = m / 2^s, 23 <= s <= 38
        const uint64_t num = m * 10000u;
        uint64_t qq = num >> s;
        const uint64_t r = num & ((1ull << s) - 1u), half = 1ull << (s - 1u);
        if (r > half || (r == half && (qq & 1u))) ++qq;
        q = (uint32_t)qq;
    }
    out[0] = (char)('0' + q / 10000u);
    out[1] = '.';
    out[2] = (char)('0' + q / 1000u % 10u);
    out[3] = (char)('0' + q / 100u % 10u);
    out[4] = (char)('0' + q / 10u % 10u);
    out[5] = (char)('0' + q % 10u);
    return true;
}
