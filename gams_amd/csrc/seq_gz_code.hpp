// seq_gz_code.hpp -- the gzip members of the `seq:` values (gams_gpu_seq_gz, gams_seq_gz_host): what the host twin
// (seq_gz_code.cpp) and the kernels (seq_gz.hip) share, so that both write the same bytes.  Integer-only plain C++,
// no tie is broken by anything but (frequency, symbol): two builds of one histogram are one code.
//
// A member (RFC 1952) is
//   1f 8b 08 00  00 00 00 00  00 ff     ID1 ID2, CM = 8 (deflate), FLG = 0 (no name, no comment, no header CRC),
//                                       MTIME = 0 (none: two encodings of the same bases are the same bytes),
//                                       XFL = 0 (neither "slowest" 2 nor "fastest" 4: no matcher ran at any level),
//                                       OS = 255 (unknown: the bytes do not depend on where they were made)
//   the deflate body, then CRC-32 of the bases and ISIZE = their number mod 2^32, both little-endian.
// The body (RFC 1951) is a run of dynamic-Huffman blocks, BTYPE = 2, one per `block` input bytes, the last one taking
// the remainder and carrying BFINAL; an input of no bytes is one final block.  A block is its literals, then
// end-of-block: HLIT = 257 always, HDIST = 0 with the one distance code given length 0 (no distance code is ever read),
// the 258 lengths run-length coded with 16 / 17 / 18 the way zlib's scan_tree cuts the runs.  The literal code is
// limited to 15 bits and the code-length code to 7; both are complete, but for a code with one used symbol, which gets
// length 1 (the literal code of the empty block: only end-of-block).
#pragma once

#include <cstdint>

#if defined(__HIP__) || defined(__HIPCC__)
#define GAMS_GZ_HD __host__ __device__
#else
#define GAMS_GZ_HD
#endif

namespace gams_gz {

constexpr uint32_t kLit = 257;        // literals and end-of-block
constexpr uint32_t kSeq = 258;        // the lengths the header lists: kLit, then the one distance code
constexpr uint32_t kMaxSym = 288;     // the largest alphabet gams_deflate_lengths takes
constexpr uint32_t kHdrWords = 128;   // a block header is at most 14 + 3 * 19 + 258 * (7 + 7) = 3683 bits
constexpr uint32_t kTile = 4096;      // bytes a pack workgroup encodes between two flushes; a block is a multiple
constexpr uint32_t kMinBlock = kTile, kMaxBlock = 1u << 24;
constexpr uint32_t kHead = 10, kTail = 8;

GAMS_GZ_HD inline bool block_ok(uint32_t block) { return block >= kMinBlock && block <= kMaxBlock && block % kTile == 0; }
GAMS_GZ_HD inline uint64_t n_blocks(uint64_t n, uint32_t block) { return n ? (n + block - 1) / block : 1; }

// ---- the indexed member (GAMS_SEQ_GZ_INDEXED): FLG = 4 (FEXTRA, RFC 1952 2.3.1.1), and between the ten header bytes
// and the body
//   XLEN (u16)   'G' 'I' LEN (u16)   block (u32)   chunk (u32)   ceil(n / chunk) bit offsets (u32)      all little-endian
// LEN = XLEN - 4 = 8 + 4 * entries.  Entry j is relative to the first bit of the body: where j * chunk is a multiple of
// `block` it is the BFINAL bit of the block that begins with base j * chunk, everywhere else the first bit of the
// literal code of base j * chunk.  Body and trailer are those of the plain member, bit for bit; every gzip reader skips
// the field.  `chunk` divides kTile and is a multiple of 16: a chunk begins with a lane of the pack kernel.  An index
// that would not fit XLEN <= 65535 (more than kIdxMaxEntries chunks: 67,092,480 bases at chunk 4096) is not written:
// that ctg gets the plain member.
constexpr uint32_t kIdxFixed = 2 + 4 + 8;                      // XLEN, the subfield's head, block and chunk
constexpr uint32_t kIdxMaxEntries = (65535u - 12u) / 4u;       // 16,380
GAMS_GZ_HD inline bool chunk_ok(uint32_t c) { return c == 512u || c == 1024u || c == 2048u || c == 4096u; }
GAMS_GZ_HD inline uint64_t idx_entries(uint64_t n, uint32_t chunk) { return (n + chunk - 1) / chunk; }
// the bytes between header and body of the member of n bases: 0 without an index (chunk 0, or one that does not fit)
GAMS_GZ_HD inline uint32_t idx_extra(uint64_t n, uint32_t chunk) {
    if (chunk == 0 || idx_entries(n, chunk) > kIdxMaxEntries) return 0;
    return kIdxFixed + 4u * (uint32_t)idx_entries(n, chunk);
}

// ---- CRC-32 (the reflected polynomial 0xEDB88320): bit 31 of a word is the coefficient of x^0
constexpr uint32_t kPoly = 0xEDB88320u;
// a * b mod P
GAMS_GZ_HD inline uint32_t gf2_mul(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (int i = 31; i >= 0; --i) {
        p ^= b & (0u - ((a >> i) & 1u));
        b = (b >> 1) ^ (kPoly & (0u - (b & 1u)));
    }
    return p;
}
// x^(8 n) mod P: what n bytes behind a message do to its raw CRC
GAMS_GZ_HD inline uint32_t gf2_xpow8(uint64_t n) {
    uint32_t r = 0x80000000u, b = 0x00800000u;   // x^0, x^8
    for (; n; n >>= 1) {
        if (n & 1u) r = gf2_mul(r, b);
        b = gf2_mul(b, b);
    }
    return r;
}
// entry i of the byte table (slice 0): i * x^32 mod P over eight steps
GAMS_GZ_HD inline uint32_t crc_table0(uint32_t i) {
    for (int k = 0; k < 8; ++k) i = (i >> 1) ^ (kPoly & (0u - (i & 1u)));
    return i;
}
// the CRC-32 of a message from its raw CRC (register 0 at the start, nothing inverted): the two inversions are one
// more term, ~0 * x^(8 n), and ~0
GAMS_GZ_HD inline uint32_t crc_finish(uint32_t raw, uint64_t n) { return raw ^ gf2_mul(0xFFFFFFFFu, gf2_xpow8(n)) ^ 0xFFFFFFFFu; }

// ---- code lengths
// Length-limited prefix code of the symbols with freq(s) != 0 among n_sym <= kMaxSym: len[s] in 1..limit, 0 for an
// unused symbol; complete (Kraft sum 1) for two or more used symbols, length 1 for one.  The Huffman tree over the
// symbols sorted by (frequency, symbol) by the two-queue merge, a leaf before an internal node of equal weight; depths
// beyond `limit` are folded into it and the overfull code is thinned by moving one code of the longest shorter length
// a level down per excess unit (each step takes 2^-limit off the Kraft sum and keeps the number of codes); the
// lengths, longest first, then go to the symbols in sorted order.  false: n_sym or limit out of range, or more used
// symbols than 2^limit codes.
template <typename Freq>
GAMS_GZ_HD inline bool code_lengths(Freq freq, uint32_t n_sym, uint32_t limit, uint8_t *len) {
    if (n_sym == 0 || n_sym > kMaxSym || limit == 0 || limit > 15) return false;
    uint16_t sym[kMaxSym];
    uint32_t n = 0;
    for (uint32_t s = 0; s < n_sym; ++s) {
        len[s] = 0;
        if (freq(s)) sym[n++] = (uint16_t)s;
    }
    if (n == 0) return true;
    if (n == 1) {
        len[sym[0]] = 1;
        return true;
    }
    if (n > (1u << limit)) return false;
    for (uint32_t i = 1; i < n; ++i) {   // insertion sort: ascending frequency, the symbols of one frequency stay ascending
        const uint16_t s = sym[i];
        const uint32_t f = freq(s);
        uint32_t j = i;
        for (; j > 0 && freq(sym[j - 1]) > f; --j) sym[j] = sym[j - 1];
        sym[j] = s;
    }
    // nodes 0 .. n-1 are the leaves in sorted order, n .. 2n-2 the internal nodes in the order they are made (their
    // weights never decrease); up[] holds a node's parent, then its depth
    uint64_t iw[kMaxSym - 1];
    uint16_t up[2 * kMaxSym - 1];
    uint32_t li = 0, ii = 0, ni = 0;
    for (uint32_t k = 0; k + 1 < n; ++k) {
        uint64_t w = 0;
        for (int side = 0; side < 2; ++side) {
            if (li < n && (ii >= ni || (uint64_t)freq(sym[li]) <= iw[ii])) {
                w += freq(sym[li]);
                up[li++] = (uint16_t)(n + ni);
            } else {
                w += iw[ii];
                up[n + ii++] = (uint16_t)(n + ni);
            }
        }
        iw[ni++] = w;
    }
    uint32_t cnt[16];
    for (uint32_t l = 0; l < 16; ++l) cnt[l] = 0;
    up[2 * n - 2] = 0;
    for (uint32_t v = 2 * n - 2; v-- > 0;) {
        up[v] = (uint16_t)(up[up[v]] + 1u);
        if (v < n) ++cnt[up[v] < limit ? up[v] : limit];
    }
    uint32_t total = 0;
    for (uint32_t l = 1; l <= limit; ++l) total += cnt[l] << (limit - l);
    for (; total > (1u << limit); --total) {
        --cnt[limit];
        for (uint32_t l = limit - 1; l >= 1; --l)
            if (cnt[l]) {
                --cnt[l];
                cnt[l + 1] += 2;
                break;
            }
    }
    uint32_t i = 0;
    for (uint32_t l = limit; l >= 1; --l)
        for (uint32_t c = 0; c < cnt[l]; ++c) len[sym[i++]] = (uint8_t)l;
    return true;
}

// the canonical code of symbol s among len[0 .. n_sym), its bits reversed (deflate packs a code from its first bit)
struct Canon {
    uint16_t next[16];
    GAMS_GZ_HD Canon(const uint8_t *len, uint32_t n_sym) {
        uint16_t cnt[16];
        for (uint32_t l = 0; l < 16; ++l) cnt[l] = 0;
        for (uint32_t s = 0; s < n_sym; ++s) ++cnt[len[s]];
        cnt[0] = 0;
        uint32_t code = 0;
        next[0] = 0;
        for (uint32_t l = 1; l < 16; ++l) {
            code = (code + cnt[l - 1]) << 1;
            next[l] = (uint16_t)code;
        }
    }
    // the symbols are asked in ascending order, each used one once
    GAMS_GZ_HD uint32_t take(uint32_t l) {
        uint32_t c = next[l]++, r = 0;
        for (uint32_t k = 0; k < l; ++k) r |= ((c >> k) & 1u) << (l - 1 - k);
        return r;
    }
};

// bits appended to zeroed words, first bit in bit 0 of word 0
struct BitSink {
    uint32_t *w;
    uint32_t pos = 0;
    GAMS_GZ_HD explicit BitSink(uint32_t *words) : w(words) {}
    GAMS_GZ_HD void put(uint32_t v, uint32_t n) {
        if (n == 0) return;
        const uint32_t sh = pos & 31u;
        w[pos >> 5] |= v << sh;
        if (sh + n > 32u) w[(pos >> 5) + 1] |= v >> (32u - sh);
        pos += n;
    }
};

struct LitFreq {   // the literal alphabet of a block: its byte histogram and one end-of-block
    const uint32_t *hist;
    GAMS_GZ_HD uint32_t operator()(uint32_t s) const { return s < 256u ? hist[s] : 1u; }
};
struct ArrFreq {
    const uint32_t *f;
    GAMS_GZ_HD uint32_t operator()(uint32_t s) const { return f[s]; }
};

// One block from its histogram: tab[s] = (length << 16) | reversed code for the 257 literal symbols, the header's bits
// in hdr[0 .. kHdrWords) (zero behind *hdr_bits), and the bits of the whole block, end-of-block included.
GAMS_GZ_HD inline void build_block(const uint32_t *hist, bool final, uint32_t *tab, uint32_t *hdr, uint32_t *hdr_bits,
                                   uint64_t *block_bits) {
    uint8_t len[kSeq];
    code_lengths(LitFreq{hist}, kLit, 15, len);
    len[kLit] = 0;   // the distance code: never used
    uint64_t bits = 0;
    {
        Canon lit(len, kLit);
        for (uint32_t s = 0; s < kLit; ++s) {
            tab[s] = len[s] ? ((uint32_t)len[s] << 16) | lit.take(len[s]) : 0u;
            bits += (uint64_t)LitFreq{hist}(s) * len[s];
        }
    }
    // the run-length form of the 258 lengths (zlib's cuts: a run of zeros is 18 for 11..138, 17 for 3..10; a run of
    // another length is the length once, then 16 for 3..6 repeats)
    uint8_t cs[kSeq], cx[kSeq];
    uint32_t m = 0, cf[19];
    for (uint32_t k = 0; k < 19; ++k) cf[k] = 0;
    for (uint32_t i = 0; i < kSeq;) {
        const uint8_t v = len[i];
        uint32_t run = 1;
        while (i + run < kSeq && len[i + run] == v) ++run;
        i += run;
        if (v == 0) {
            while (run >= 11) {
                const uint32_t r = run < 138 ? run : 138;
                cs[m] = 18, cx[m++] = (uint8_t)(r - 11);
                run -= r;
            }
            if (run >= 3) {
                cs[m] = 17, cx[m++] = (uint8_t)(run - 3);
                run = 0;
            }
        } else {
            cs[m] = v, cx[m++] = 0;
            --run;
            while (run >= 3) {
                const uint32_t r = run < 6 ? run : 6;
                cs[m] = 16, cx[m++] = (uint8_t)(r - 3);
                run -= r;
            }
        }
        for (; run; --run) cs[m] = v, cx[m++] = 0;
    }
    for (uint32_t k = 0; k < m; ++k) ++cf[cs[k]];
    uint8_t cl[19];
    code_lengths(ArrFreq{cf}, 19, 7, cl);
    uint32_t cc[19];
    {
        Canon c(cl, 19);
        for (uint32_t s = 0; s < 19; ++s) cc[s] = cl[s] ? c.take(cl[s]) : 0u;
    }
    const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    uint32_t hclen = 19;
    while (hclen > 4 && cl[order[hclen - 1]] == 0) --hclen;
    for (uint32_t k = 0; k < kHdrWords; ++k) hdr[k] = 0;
    BitSink out(hdr);
    out.put(final ? 1u : 0u, 1);
    out.put(2u, 2);              // BTYPE: dynamic
    out.put(kLit - 257u, 5);     // HLIT
    out.put(0u, 5);              // HDIST: one distance code
    out.put(hclen - 4u, 4);
    for (uint32_t k = 0; k < hclen; ++k) out.put(cl[order[k]], 3);
    for (uint32_t k = 0; k < m; ++k) {
        out.put(cc[cs[k]], cl[cs[k]]);
        if (cs[k] == 16) out.put(cx[k], 2);
        if (cs[k] == 17) out.put(cx[k], 3);
        if (cs[k] == 18) out.put(cx[k], 7);
    }
    *hdr_bits = out.pos;
    *block_bits = out.pos + bits;
}

// the RESP frame in front of a member (GAMS_LOADER_RESP): "*3\r\n$3\r\nSET\r\n${4 + id}\r\nseq:{id}\r\n${member}\r\n"
GAMS_GZ_HD inline uint32_t dec_len(uint64_t v) {
    uint32_t n = 1;
    for (; v >= 10; v /= 10) ++n;
    return n;
}
GAMS_GZ_HD inline uint64_t resp_front(uint64_t id_bytes, uint64_t member_bytes) {
    return 14u + dec_len(4u + id_bytes) + 2u + 4u + id_bytes + 3u + dec_len(member_bytes) + 2u;
}

}  // namespace gams_gz

// the host twin with the block size and the index's chunk (0: the plain member) as arguments (gams_seq_gz_host_block,
// gams_seq_gz_host_indexed_chunk of gams_gpu_diag.h)
int gams_seq_gz_host_with(const uint8_t *seq, uint64_t n, uint32_t block, uint32_t chunk, uint8_t *out, uint64_t cap,
                          uint64_t *n_out);
