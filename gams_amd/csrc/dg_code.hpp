// dg_code.hpp -- what the ΔG kernel (dg.hip) and its host twin (dg_code.cpp) share: the byte -> code map of the
// nearest-neighbour free energy (src/libs/delta_g.rs:78-115), four bases at once.  Plain C++17; compiles for the host
// and for the device.
#pragma once

#include <cstdint>

#if defined(__HIP__) || defined(__HIPCC__)
#define GAMS_DG_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define GAMS_DG_HD inline
#endif

// Four bases in a little-endian word -> their 2-bit codes, A C G T = 0 1 2 3 in either case, base k of the word at bits
// [2k, 2k + 2) of *codes8; bit k of the result says that base k is none of ACGTacgt (its code then means nothing).
// With bit 5 cleared the four letters are 0x41 0x43 0x47 0x54: bits [2:1] tell them apart (0 1 3 2) and the other six
// bits are 0x41, or 0x50 where bits [2:1] say T.
GAMS_DG_HD uint32_t dg_code4(uint32_t w, uint32_t *codes8) {
    const uint32_t u = w & 0xDFDFDFDFu;
    const uint32_t t = (u >> 1) & 0x03030303u;                    // A C G T -> 0 1 3 2
    const uint32_t hi = (t >> 1) & 0x01010101u;
    const uint32_t c = t ^ hi;                                    // -> 0 1 2 3
    const uint32_t is_t = hi & ~t;                                // bit 0 of a byte: t == 2
    const uint32_t y = (u & 0xF9F9F9F9u) ^ (0x41414141u ^ (is_t | (is_t << 4)));
    const uint32_t nz = (((y & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | y) & 0x80808080u;   // bit 7 of a byte: it is not zero
    uint32_t g = nz >> 7;
    g |= g >> 7;
    g |= g >> 14;
    uint32_t p = c | (c >> 6);
    p |= p >> 12;
    *codes8 = p & 0xFFu;
    return g & 0xFu;
}

// one byte: its code, or 4 for a byte that is no base
GAMS_DG_HD uint32_t dg_code1(uint8_t b) {
    uint32_t c;
    return (dg_code4(0x41414100u | b, &c) & 1u) ? 4u : (c & 3u);
}

// The range the entries of a device call carry: a window or an oligo, and the serial chain of its sum
constexpr uint32_t kDgMaxBases = 65535;
