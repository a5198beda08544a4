// seq_gz_crc.hpp -- the raw CRC-32 of a block of at most 64 KiB, folded by the 256 threads of a workgroup from 16-byte
// pieces that lie 4096 bytes apart (device code; gz_hist_kernel of seq_gz.hip and gunzip_decode_kernel of
// seq_gunzip.hip).  A lane folds its pieces by Horner's rule -- multiply by x^(8 * 4080), then four table slices over
// the piece --, the lanes' terms are shifted to the block's end by a table of x^(128 j) and joined by XOR.
#pragma once

#include <hip/hip_runtime.h>

#include "seq_gz_code.hpp"

namespace gams_gz {

constexpr uint32_t kShift16 = 512;   // entries of the x^(128 j) table: a lane's last piece ends < 8192 bytes before its block does

// the table the host uploads for CrcPieces::finish
inline void crc_shift16_fill(uint32_t *shift16) {
    for (uint32_t j = 0; j < kShift16; ++j) shift16[j] = gf2_xpow8(16u * j);
}
// x^(8 * 4080): the gap between the end of a lane's piece and the start of its next
inline uint32_t crc_x_gap() { return gf2_xpow8(kTile - 16u); }

// the four table slices in LDS, by the 256 threads of the workgroup (two barriers)
__device__ __forceinline__ void crc_slices_build(uint32_t (*T)[256], uint32_t tid) {
    uint32_t t = crc_table0(tid);
    T[0][tid] = t;
    __syncthreads();
    for (uint32_t k = 1; k < 4; ++k) {
        t = (t >> 8) ^ T[0][t & 0xffu];
        T[k][tid] = t;
    }
    __syncthreads();
}

// One lane's pieces, in ascending order: piece(v, m, base) takes the m <= 16 bytes at `base` of the block (only the
// block's last piece is short).
struct CrcPieces {
    uint32_t acc = 0, end = 0;
    bool whole = true;   // the lane's last piece had all 16 bytes
    __device__ __forceinline__ void piece(const uint32_t (*T)[256], uint32_t x_gap, const uint4 &v, uint32_t m, uint32_t base) {
        acc = gf2_mul(acc, x_gap);
        if (m == 16u) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t w = j == 0 ? v.x : j == 1 ? v.y : j == 2 ? v.z : v.w;
                acc ^= w;
                acc = T[3][acc & 0xffu] ^ T[2][(acc >> 8) & 0xffu] ^ T[1][(acc >> 16) & 0xffu] ^ T[0][acc >> 24];
            }
        } else {
            const uint64_t lo = ((uint64_t)v.y << 32) | v.x, hi = ((uint64_t)v.w << 32) | v.z;
            for (uint32_t k = 0; k < m; ++k) {
                const uint32_t c = (uint32_t)((k < 8u ? lo >> (8u * k) : hi >> (8u * (k - 8u))) & 0xffu);
                acc = T[0][(acc ^ c) & 0xffu] ^ (acc >> 8);
            }
            whole = false;
        }
        end = base + m;
    }
    // The raw CRC of the block's n bytes, on thread 0 (one barrier; every thread of the workgroup calls it).  red: four
    // words of LDS; tail_crc: one, zeroed in front of an earlier barrier.
    __device__ __forceinline__ uint32_t finish(uint32_t n, const uint32_t *shift16, uint32_t *red, uint32_t *tail_crc) const {
        // every whole piece ends 16 q + (n & 15) bytes before the block does; the one short piece ends with it
        uint32_t term = 0;
        if (end != 0 && whole) term = gf2_mul(acc, shift16[(n - end) >> 4]);
        if (end != 0 && !whole) *tail_crc = acc;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) term ^= __shfl_xor(term, d, 64);
        if ((threadIdx.x & 63u) == 0) red[threadIdx.x >> 6] = term;
        __syncthreads();
        return threadIdx.x == 0 ? gf2_mul(red[0] ^ red[1] ^ red[2] ^ red[3], gf2_xpow8(n & 15u)) ^ *tail_crc : 0u;
    }
};

}  // namespace gams_gz
