// seq_gz_code.cpp -- host twin of gams_gpu_seq_gz (plain C++, no device code): the member the kernels of seq_gz.hip
// write for the same bases, byte for byte, from the builder both share (seq_gz_code.hpp).  One pass per block for the
// histogram, one for the bits; the CRC-32 runs over the whole input with four table slices.
#include <cstdint>
#include <cstring>

#include "../../include/gams_gpu.h"
#include "../../include/gams_gpu_diag.h"
#include "seq_gz_code.hpp"
#include "seq_gunzip_code.hpp"

namespace {

using namespace gams_gz;

struct CrcTables {
    uint32_t t[4][256];
    CrcTables() {
        for (uint32_t i = 0; i < 256; ++i) t[0][i] = crc_table0(i);
        for (int k = 1; k < 4; ++k)
            for (uint32_t i = 0; i < 256; ++i) t[k][i] = (t[k - 1][i] >> 8) ^ t[0][t[k - 1][i] & 0xffu];
    }
};

uint32_t crc32_of(const uint8_t *p, uint64_t n) {
    static const CrcTables T;
    uint32_t c = 0xFFFFFFFFu;
    for (; n >= 4; n -= 4, p += 4) {
        c ^= (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
        c = T.t[3][c & 0xffu] ^ T.t[2][(c >> 8) & 0xffu] ^ T.t[1][(c >> 16) & 0xffu] ^ T.t[0][c >> 24];
    }
    for (; n; --n) c = T.t[0][(c ^ *p++) & 0xffu] ^ (c >> 8);
    return ~c;
}

void put_le32(uint8_t *p, uint32_t v) {
    for (int k = 0; k < 4; ++k) p[k] = (uint8_t)(v >> (8 * k));
}

}  // namespace

int gams_seq_gz_host_with(const uint8_t *seq, uint64_t n, uint32_t block, uint32_t chunk, uint8_t *out, uint64_t cap,
                          uint64_t *n_out) {
    if (!n_out || (n && !seq) || (cap && !out) || !block_ok(block) || (chunk && !chunk_ok(chunk))) return GAMS_EINVAL;
    const uint32_t extra = idx_extra(n, chunk);
    const uint64_t nb = n_blocks(n, block);
    uint32_t hist[256], tab[kLit], hdr[kHdrWords], hdr_bits = 0;
    // sizes first: the call either fits or writes nothing
    uint64_t bits = 0;
    for (uint64_t b = 0; b < nb; ++b) {
        const uint64_t lo = b * block, m = n - lo < block ? n - lo : block;
        std::memset(hist, 0, sizeof hist);
        for (uint64_t i = 0; i < m; ++i) ++hist[seq[lo + i]];
        uint64_t bb = 0;
        build_block(hist, b + 1 == nb, tab, hdr, &hdr_bits, &bb);
        bits += bb;
    }
    const uint64_t total = kHead + extra + (bits + 7) / 8 + kTail;
    *n_out = total;
    if (cap == 0) return GAMS_OK;
    if (cap < total) return GAMS_EINVAL;
    const uint8_t head[kHead] = {0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 0, 0xff};
    std::memcpy(out, head, kHead);
    uint8_t *q = out + kHead, *entry = nullptr;
    if (extra) {
        out[3] = 4;   // FLG: FEXTRA
        const uint32_t xlen = extra - 2u;
        q[0] = (uint8_t)xlen, q[1] = (uint8_t)(xlen >> 8);
        q[2] = 'G', q[3] = 'I';
        q[4] = (uint8_t)(xlen - 4u), q[5] = (uint8_t)((xlen - 4u) >> 8);
        put_le32(q + 6, block);
        put_le32(q + 10, chunk);
        entry = q + kIdxFixed;
        q += extra;
    }
    uint64_t acc = 0, at = 0;   // the bits not yet written, from bit 0; the bits of the body so far
    uint32_t na = 0;
    auto put = [&](uint32_t v, uint32_t nbits) {
        acc |= (uint64_t)v << na;
        at += nbits;
        for (na += nbits; na >= 8; na -= 8, acc >>= 8) *q++ = (uint8_t)acc;
    };
    for (uint64_t b = 0; b < nb; ++b) {
        const uint64_t lo = b * block, m = n - lo < block ? n - lo : block;
        std::memset(hist, 0, sizeof hist);
        for (uint64_t i = 0; i < m; ++i) ++hist[seq[lo + i]];
        uint64_t bb = 0;
        build_block(hist, b + 1 == nb, tab, hdr, &hdr_bits, &bb);
        if (entry && m) put_le32(entry + 4 * (lo / chunk), (uint32_t)at);   // (a block begins a chunk: chunk divides kTile)
        for (uint32_t k = 0; k < hdr_bits; k += 32) put(hdr[k >> 5], hdr_bits - k < 32 ? hdr_bits - k : 32);
        for (uint64_t i = 0; i < m; ++i) {
            if (entry && i && (i & (chunk - 1u)) == 0) put_le32(entry + 4 * ((lo + i) / chunk), (uint32_t)at);
            const uint32_t e = tab[seq[lo + i]];
            put(e & 0xffffu, e >> 16);
        }
        put(tab[256] & 0xffffu, tab[256] >> 16);
    }
    if (na) *q++ = (uint8_t)acc;
    put_le32(q, crc32_of(seq, n));
    put_le32(q + 4, (uint32_t)n);
    return GAMS_OK;
}

extern "C" {

int gams_deflate_lengths(const uint32_t *freq, uint32_t n_sym, uint32_t limit, uint8_t *len) {
    if (!freq || !len) return GAMS_EINVAL;
    return code_lengths(ArrFreq{freq}, n_sym, limit, len) ? GAMS_OK : GAMS_EINVAL;
}

int gams_seq_gz_host(const uint8_t *seq, uint64_t n, uint8_t *out, uint64_t cap, uint64_t *n_out) {
    return gams_seq_gz_host_with(seq, n, GAMS_SEQ_GZ_BLOCK, 0, out, cap, n_out);
}

int gams_seq_gz_host_block(const uint8_t *seq, uint64_t n, uint32_t block, uint8_t *out, uint64_t cap, uint64_t *n_out) {
    return gams_seq_gz_host_with(seq, n, block, 0, out, cap, n_out);
}

int gams_seq_gz_host_indexed(const uint8_t *seq, uint64_t n, uint8_t *out, uint64_t cap, uint64_t *n_out) {
    return gams_seq_gz_host_with(seq, n, GAMS_SEQ_GZ_BLOCK, GAMS_SEQ_GZ_CHUNK, out, cap, n_out);
}

int gams_seq_gz_host_indexed_block(const uint8_t *seq, uint64_t n, uint32_t block, uint8_t *out, uint64_t cap, uint64_t *n_out) {
    return gams_seq_gz_host_with(seq, n, block, GAMS_SEQ_GZ_CHUNK, out, cap, n_out);
}

int gams_seq_gz_host_indexed_chunk(const uint8_t *seq, uint64_t n, uint32_t block, uint32_t chunk, uint8_t *out, uint64_t cap,
                                   uint64_t *n_out) {
    if (!chunk) return GAMS_EINVAL;
    return gams_seq_gz_host_with(seq, n, block, chunk, out, cap, n_out);
}

int gams_seq_gunzip_host(const uint8_t *member, uint64_t n_bytes, uint8_t *out, uint64_t cap, uint64_t *n_out, int *status) {
    if (!member || !n_out || !status || (cap && !out)) return GAMS_EINVAL;
    return gams_gunzip::gunzip_member(member, n_bytes, out, cap, n_out, status) ? GAMS_OK : GAMS_EINVAL;
}

}  // extern "C"
