// gc_plane.cpp -- host side of the 1-bit G/C plane (plain C++, no device code): bit i & 7 of plane byte
// i >> 3 says whether base i is one of C, G, c, g, i.e. (seq[i] & 0xDB) == 0x43 (0xDB drops the case bit 0x20
// and the C/G bit 0x04).  The upload paths of api.hip run it over bytes a CPU core has in its cache anyway;
// the wave tile kernels then stream the plane instead of classifying the bytes.
#include <cstdint>
#include <cstring>

#include "../../include/gams_gpu.h"
#include "../../include/gams_gpu_diag.h"
#include "gc_plane.hpp"

#if defined(__x86_64__)
#include <immintrin.h>
#endif

namespace {

// eight bases -> eight bits.  t sets bit 7 of every byte whose low seven bits differ from 0x43 under the mask
// (no carry leaves a byte: <= 0x5B + 0x7F), so ~(t | x) has bit 7 set exactly on the G/C bytes; the multiply
// gathers the eight bit-7s into the top byte (bit 8i + 7 lands on bit 56 + i, no two terms meet).
inline uint8_t gc_bits8(uint64_t x) {
    const uint64_t t = ((x & 0x5B5B5B5B5B5B5B5Bull) ^ 0x4343434343434343ull) + 0x7F7F7F7F7F7F7F7Full;
    const uint64_t f = (~(t | x) & 0x8080808080808080ull) >> 7;
    return (uint8_t)((f * 0x0102040810204080ull) >> 56);
}

// the last n < 8 bases of a run: bits past n stay zero
inline uint8_t gc_bits_tail(const uint8_t *seq, size_t n) {
    uint64_t x = 0;
    std::memcpy(&x, seq, n);   // missing bytes read as 0, which is no G/C
    return gc_bits8(x);
}

void classify_swar(const uint8_t *seq, size_t n, uint8_t *plane) {
    size_t i = 0;
    for (; i + 8 <= n; i += 8) {
        uint64_t x;
        std::memcpy(&x, seq + i, 8);
        plane[i >> 3] = gc_bits8(x);
    }
    if (i < n) plane[i >> 3] = gc_bits_tail(seq + i, n - i);
}

#if defined(__x86_64__)
__attribute__((target("avx2"))) void classify_avx2(const uint8_t *seq, size_t n, uint8_t *plane) {
    const __m256i keep = _mm256_set1_epi8((char)0xDB), want = _mm256_set1_epi8(0x43);
    size_t i = 0;
    for (; i + 32 <= n; i += 32) {
        const __m256i x = _mm256_loadu_si256(reinterpret_cast<const __m256i *>(seq + i));
        const uint32_t m = (uint32_t)_mm256_movemask_epi8(_mm256_cmpeq_epi8(_mm256_and_si256(x, keep), want));
        std::memcpy(plane + (i >> 3), &m, 4);
    }
    if (i < n) classify_swar(seq + i, n - i, plane + (i >> 3));
}

// the same, leaving a copy of the bases in dst (the staging slot of an upload)
__attribute__((target("avx2"))) void copy_classify_avx2(uint8_t *dst, const uint8_t *seq, size_t n, uint8_t *plane) {
    const __m256i keep = _mm256_set1_epi8((char)0xDB), want = _mm256_set1_epi8(0x43);
    size_t i = 0;
    for (; i + 32 <= n; i += 32) {
        const __m256i x = _mm256_loadu_si256(reinterpret_cast<const __m256i *>(seq + i));
        _mm256_storeu_si256(reinterpret_cast<__m256i *>(dst + i), x);
        const uint32_t m = (uint32_t)_mm256_movemask_epi8(_mm256_cmpeq_epi8(_mm256_and_si256(x, keep), want));
        std::memcpy(plane + (i >> 3), &m, 4);
    }
    if (i < n) {
        std::memcpy(dst + i, seq + i, n - i);
        classify_swar(seq + i, n - i, plane + (i >> 3));
    }
}
#endif

bool have_avx2() {
#if defined(__x86_64__)
    static const bool yes = __builtin_cpu_supports("avx2");   // asked once
    return yes;
#else
    return false;
#endif
}

}  // namespace

void gams_gc_copy_classify(uint8_t *dst, const uint8_t *seq, size_t n, uint8_t *plane) {
#if defined(__x86_64__)
    if (have_avx2()) {
        copy_classify_avx2(dst, seq, n, plane);
        return;
    }
#endif
    // portable: blocks small enough that the classifier finds the copy's bytes in the L1
    for (size_t o = 0; o < n; o += 16384) {
        const size_t m = n - o < 16384 ? n - o : 16384;
        std::memcpy(dst + o, seq + o, m);
        classify_swar(dst + o, m, plane + (o >> 3));
    }
}

extern "C" {

int gams_gc_plane(const uint8_t *seq, uint64_t n, uint8_t *plane) { return gams_gc_plane_with(seq, n, plane, GAMS_GC_BODY_AUTO); }

int gams_gc_plane_with(const uint8_t *seq, uint64_t n, uint8_t *plane, int body) {
    if (n && (!seq || !plane)) return GAMS_EINVAL;
    if (body != GAMS_GC_BODY_AUTO && body != GAMS_GC_BODY_PORTABLE && body != GAMS_GC_BODY_AVX2) return GAMS_EINVAL;
    if (body == GAMS_GC_BODY_AVX2 && !have_avx2()) return GAMS_EUNSUPPORTED;
#if defined(__x86_64__)
    if (body != GAMS_GC_BODY_PORTABLE && have_avx2()) {
        classify_avx2(seq, (size_t)n, plane);
        return GAMS_OK;
    }
#endif
    classify_swar(seq, (size_t)n, plane);
    return GAMS_OK;
}

}  // extern "C"
