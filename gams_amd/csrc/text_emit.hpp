// text_emit.hpp -- what the device paths that write finished TSV text share (device only): the wave rows and
// `--signal` rows (wave_rows.hpp), the `sw` rows (sw.hip), the `locate` / `locate --count` / `anno` / `peak` rows (text.hip).
// Decimal output, the round4 float format of the `sw` and `peak` rows (sw_put_f4), RowOut -- the field sequence of a row
// written once, for the pass that counts its bytes and the pass that writes them --, the workgroup sum behind a block's
// byte count, the one-workgroup prefix over those counts, the copy of a block's text from its LDS stage to the global
// text, and BlockWriter -- the prefix inside a block, the choice between the stage and the text, and that copy, written
// once for the four kernels that stage a block (`locate` / `anno` rows are never staged: text_row_write_kernel keeps its
// own few lines).  The row composers and the gctab lookup stay with their owners; the other two float formats
// (gams_fmt_prop4 and gams_fmt_f32_short) are text_fmt.hpp's, which the host layer shares.  In front of them, the two
// helpers the units that READ text share (text.hip, runlist.hip): the exact zero-byte mask and the run of digits.
#pragma once

#include "common.hpp"
#include "text_fmt.hpp"

namespace {

// ---- what the kernels that read text share (text.hip, runlist.hip)
// 0x80 in exactly the zero bytes of y
__device__ __forceinline__ uint32_t zero_bytes(uint32_t y) {
    return ~(((y & 0x7f7f7f7fu) + 0x7f7f7f7fu) | y | 0x7f7f7f7fu);
}
__device__ __forceinline__ bool is_digit_c(char c) { return c >= '0' && c <= '9'; }

// The run of digits at s[p..e), looked at up to its eleventh digit (a run of more than ten is invalid anyway): p moves
// past what was looked at; the value is that of the first ten digits, or 0x80000000 for any value above INT32_MAX.
// Branch-free over a fixed trip count in 32-bit arithmetic (the input buffer carries 16 bytes of padding, so the
// eleven loads stay inside it): the branchy 64-bit form of this loop came out of the compiler returning a wrong
// value for one of the two runs of a range.
__device__ __forceinline__ uint32_t digits(const char *s, uint64_t &p, uint64_t e) {
    uint32_t v = 0, nd = 0;
    bool run = true, over = false;
#pragma unroll
    for (uint32_t u = 0; u < 11u; ++u) {
        const uint32_t d = (uint32_t)(uint8_t)s[p + u] - (uint32_t)'0';
        run = run && (p + u < e) && d < 10u;
        const bool take = run && u < 10u;
        over = over || (take && (v > 214748364u || v * 10u + d > 0x7fffffffu));
        v = take && !over ? v * 10u + d : v;
        nd += run ? 1u : 0u;
    }
    p += nd;
    return over ? 0x80000000u : v;
}

__device__ __forceinline__ uint32_t dec_digits(uint32_t v) {
    return v < 10u ? 1u : v < 100u ? 2u : v < 1000u ? 3u : v < 10000u ? 4u : v < 100000u ? 5u : v < 1000000u ? 6u
         : v < 10000000u ? 7u : v < 100000000u ? 8u : v < 1000000000u ? 9u : 10u;
}
// the decimal digits of v at p; returns their end
__device__ __forceinline__ char *put_dec(char *p, uint32_t v) {
    const uint32_t n = dec_digits(v);
    char *e = p + n;
    do {
        *--e = (char)('0' + v % 10u);
        v /= 10u;
    } while (v);
    return p + n;
}
// an i32 as Rust's `{}` prints it
__device__ __forceinline__ uint32_t i32_len(int32_t v) {
    return v < 0 ? 1u + dec_digits(0u - (uint32_t)v) : dec_digits((uint32_t)v);
}
__device__ __forceinline__ char *put_i32(char *p, int32_t v) {
    if (v < 0) {
        *p++ = '-';
        return put_dec(p, 0u - (uint32_t)v);
    }
    return put_dec(p, (uint32_t)v);
}
__device__ __forceinline__ char *put_bytes(char *q, const char *src, uint64_t n) {
    for (uint64_t k = 0; k < n; ++k) q[k] = src[k];
    return q + n;
}

// the integer m of a round4 value v in [0, 1000), the f32 nearest to m / 10^4: exact in double.  What sw_put_f4 prints
// and what the sw summary adds up (sw.hip), so that the table and the text cannot disagree
__device__ __forceinline__ uint32_t sw_f4_units(float v) { return (uint32_t)((double)v * 10000.0 + 0.5); }

// a round4 value (the f32 nearest to m / 10^4) as Rust prints it; returns the length (p == nullptr: length only);
// *bad set for values not covered
__device__ __forceinline__ uint32_t sw_put_f4(char *p, float v, bool *bad) {
    if (v != v) {
        if (p) { p[0] = 'N'; p[1] = 'a'; p[2] = 'N'; }
        return 3u;
    }
    if (!(v >= 0.0f) || !(v < 1000.0f)) {
        *bad = true;
        return 1u;
    }
    if (v == 0.0f && (__float_as_uint(v) >> 31)) {        // round(x, 4) of a tiny negative: Rust prints "-0"
        if (p) { p[0] = '-'; p[1] = '0'; }
        return 2u;
    }
    const uint32_t m = sw_f4_units(v);
    const uint32_t ip = m / 10000u;
    uint32_t fr = m % 10000u, nd = 4u;
    while (nd && fr % 10u == 0u) {
        fr /= 10u;
        --nd;
    }
    const uint32_t n = dec_digits(ip) + (nd ? 1u + nd : 0u);
    if (p) {
        p = put_dec(p, ip);
        if (nd) {
            *p++ = '.';
            char *e = p + nd;
            for (uint32_t q = 0; q < nd; ++q) {
                *--e = (char)('0' + fr % 10u);
                fr /= 10u;
            }
        }
    }
    return n;
}

// serde_json prints an f32 through ryu: the shortest round-trip digits, always with a decimal point, positional for a
// value that is 0 or lies in [1e-5, 1] -- there it is the text sw_put_f4 / gams_fmt_f32_short make, with ".0" behind a
// text without a point ("0", "1": the only ones of one byte).  Nothing else is covered (-0, NaN, ryu's exponent form).
__device__ __forceinline__ bool json_f32_covered(float v) { return __float_as_uint(v) == 0u || (v >= 1e-5f && v <= 1.0f); }

// The bytes of one row.  A row is described once, as a sequence of fields put to a RowOut: RowOut<false> only adds up
// their lengths in n, RowOut<true> writes them at q.  Len is the type of a length (a line echoed by the text entries
// may pass 4 GB).  `bad` is set for a value that has no text of the reference's.
template <bool kWrite, typename Len = uint32_t>
struct RowOut;
template <typename Len>
struct RowOut<false, Len> {
    Len n = 0;
    __device__ __forceinline__ void bytes(const char *, Len len) { n += len; }
    __device__ __forceinline__ void esc(const char *src, Len len) {   // inside a JSON string: '"' and '\\' get a backslash
        Len x = 0;
        for (Len k = 0; k < len; ++k) x += (src[k] == '"' || src[k] == '\\') ? 1u : 0u;
        n += len + x;
    }
    __device__ __forceinline__ void ch(char) { ++n; }
    __device__ __forceinline__ void dec(uint32_t v) { n += dec_digits(v); }
    __device__ __forceinline__ void i32(int32_t v) { n += i32_len(v); }
    __device__ __forceinline__ void f4(float v, bool &bad) { n += sw_put_f4(nullptr, v, &bad); }   // a round4 value
    __device__ __forceinline__ void prop4(float) { n += 6u; }                                      // `{:.4}` of a prop in [0, 1]
    __device__ __forceinline__ void f32s(float v, bool &bad) {                                     // `{}` of an amplitude
        const uint32_t l = gams_fmt_f32_short(v, nullptr);
        if (l == 0u) bad = true;
        n += l ? l : 1u;
    }
    // the same two values as JSON numbers (json_f32_covered)
    __device__ __forceinline__ void f4j(float v, bool &bad) {
        const uint32_t l = json_f32_covered(v) ? sw_put_f4(nullptr, v, &bad) : 0u;
        if (l == 0u) bad = true;
        n += l > 1u ? l : 3u;
    }
    __device__ __forceinline__ void f32j(float v, bool &bad) {
        const uint32_t l = json_f32_covered(v) ? gams_fmt_f32_short(v, nullptr) : 0u;
        if (l == 0u) bad = true;
        n += l > 1u ? l : 3u;
    }
    // `{:.4}` of a ΔG (gams_fmt_dg4); NaN -- None -- is an empty field, a value it does not cover is flagged and empty
    __device__ __forceinline__ void dg4(float v, bool &bad) {
        if (v != v) return;
        const uint32_t l = gams_fmt_dg4(v, nullptr);
        if (l == 0u) bad = true;
        n += l;
    }
};
template <typename Len>
struct RowOut<true, Len> {
    char *q;
    __device__ __forceinline__ void bytes(const char *src, Len len) { q = put_bytes(q, src, len); }
    __device__ __forceinline__ void esc(const char *src, Len len) {
        for (Len k = 0; k < len; ++k) {
            const char c = src[k];
            if (c == '"' || c == '\\') *q++ = '\\';
            *q++ = c;
        }
    }
    __device__ __forceinline__ void ch(char c) { *q++ = c; }
    __device__ __forceinline__ void dec(uint32_t v) { q = put_dec(q, v); }
    __device__ __forceinline__ void i32(int32_t v) { q = put_i32(q, v); }
    __device__ __forceinline__ void f4(float v, bool &bad) { q += sw_put_f4(q, v, &bad); }
    __device__ __forceinline__ void prop4(float v) {       // (the counting pass flags a prop outside [0, 1]: nothing is written)
        (void)gams_fmt_prop4(v, q);
        q += 6;
    }
    __device__ __forceinline__ void f32s(float v, bool &bad) {
        const uint32_t l = gams_fmt_f32_short(v, q);
        if (l == 0u) bad = true;
        q += l ? l : 1u;
    }
    __device__ __forceinline__ void f4j(float v, bool &bad) {      // (a value not covered: flagged by the counting pass)
        const uint32_t l = json_f32_covered(v) ? sw_put_f4(q, v, &bad) : 0u;
        if (l == 1u) { q[1] = '.'; q[2] = '0'; }
        q += l > 1u ? l : 3u;
    }
    __device__ __forceinline__ void f32j(float v, bool &bad) {
        const uint32_t l = json_f32_covered(v) ? gams_fmt_f32_short(v, q) : 0u;
        if (l == 1u) { q[1] = '.'; q[2] = '0'; }
        q += l > 1u ? l : 3u;
    }
    __device__ __forceinline__ void dg4(float v, bool &) {         // (a value not covered: flagged by the counting pass)
        if (v != v) return;
        q += gams_fmt_dg4(v, q);
    }
};

// Sum of v over a 256-thread workgroup (4 waves); `ws` is LDS scratch of 4 elements, the call holds one barrier.
__device__ __forceinline__ uint32_t block_sum_256(uint32_t v, uint32_t *ws) {
    const uint32_t tid = threadIdx.x;
    for (int d = 32; d; d >>= 1) v += (uint32_t)__shfl_xor((int)v, d, 64);
    if ((tid & 63u) == 0u) ws[tid >> 6] = v;
    __syncthreads();
    return ws[0] + ws[1] + ws[2] + ws[3];
}

// stage[mis, mis + tot) -> dst[0, tot) by a workgroup of 256, after the barrier that completes the stage.  `stage`
// is 16-B aligned LDS and mis = dst's offset inside a 16-B unit of the text, so the middle leaves as 16-B stores on
// 16-B boundaries and only the ragged ends go byte by byte.
__device__ __forceinline__ void stage_flush_256(const char *stage, uint32_t mis, uint32_t tot, char *dst) {
    const uint32_t tid = threadIdx.x;
    const uint32_t head = min(tot, (16u - mis) & 15u);          // bytes in front of the first 16-B boundary
    if (tid < head) dst[tid] = stage[mis + tid];
    const uint32_t units = (tot - head) >> 4;
    const uint4 *const su = reinterpret_cast<const uint4 *>(stage + mis + head);   // 16-B aligned: mis + head is 0 mod 16
    uint4 *const du = reinterpret_cast<uint4 *>(dst + head);
    for (uint32_t q = tid; q < units; q += 256u) du[q] = su[q];
    const uint32_t done = head + (units << 4);
    if (tid < tot - done) dst[done + tid] = stage[mis + done + tid];
}

// The writer of a block's rows, one contiguous stretch of the text.  Every thread of a workgroup of 256 gives the bytes
// of its own rows (`mine`): `rel` is where they begin inside the block, `tot` the block's bytes, blk0 = blk_off[block]
// its first byte in the text.  A block that fits the kernel's stage -- stage_if(tot <= its bound, stage): 16-B aligned
// LDS of that bound + 16 bytes, begun at the offset blk0 has inside a 16-B unit, where a row's single-byte stores cost
// nothing -- is put together there and leaves through flush() as 16-B stores; a longer one is written to the text
// directly, and one that would end beyond text_cap is not written at all.  T is the type of the scan, `scr` its 4
// elements of LDS.
template <typename T>
struct BlockWriter {
    char *stage = nullptr, *dst;     // dst: the block's first byte
    T rel, tot;
    uint64_t blk0;
    uint32_t mis;
    bool staged = false, fits;       // (the same for every thread of the block)
    __device__ __forceinline__ BlockWriter(T mine, T *scr, const unsigned long long *blk_off, char *text, uint64_t text_cap) {
        rel = block_excl_scan_256<T>(mine, scr, tot);
        blk0 = blk_off[blockIdx.x];
        dst = text + blk0;
        mis = (uint32_t)(blk0 & 15u);
        fits = blk0 + tot <= text_cap;
    }
    __device__ __forceinline__ void stage_if(bool small, char *stage_) {
        stage = stage_;
        staged = small && fits;
    }
    // row(p) writes the row that begins `off` bytes into the block at p, where it goes
    template <typename F>
    __device__ __forceinline__ void put(T off, F row) const {
        if (staged)
            row(stage + mis + (uint32_t)off);
        else if (fits)
            row(dst + off);
    }
    // behind the block's last put()
    __device__ __forceinline__ void flush() const {
        if (!staged) return;
        __syncthreads();
        stage_flush_256(stage, mis, (uint32_t)tot, dst);
    }
};

// exclusive prefix of nb block counts (one workgroup of 1024): blk_off[b] = bytes in front of block b, the total
// into blk_off[nb] and words[slot]
template <typename T>
__global__ __launch_bounds__(1024) void blk_offsets_scan_kernel(const T *blk, uint32_t nb, unsigned long long *blk_off,
                                                                unsigned long long *words, uint32_t slot) {
    __shared__ unsigned long long wsum[16];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    const uint32_t per = (nb + 1023u) / 1024u;
    const uint32_t b0 = min(nb, tid * per), b1 = min(nb, b0 + per);
    unsigned long long mine = 0;
    for (uint32_t b = b0; b < b1; ++b) mine += blk[b];
    const unsigned long long inc = wave_incl_scan_u64(mine);
    if (lane == 63u) wsum[wv] = inc;
    __syncthreads();
    unsigned long long base = 0, all = 0;
    for (uint32_t w = 0; w < 16u; ++w) {
        if (w < wv) base += wsum[w];
        all += wsum[w];
    }
    unsigned long long off = base + inc - mine;
    for (uint32_t b = b0; b < b1; ++b) {
        blk_off[b] = off;
        off += blk[b];
    }
    if (tid == 0u) {
        blk_off[nb] = all;
        words[slot] = all;
    }
}

}  // namespace
