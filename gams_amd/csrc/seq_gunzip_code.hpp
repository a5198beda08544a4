// seq_gunzip_code.hpp -- the decoder of the indexed `seq:` members (seq_gz_code.hpp has the format): what the host twin
// (gams_seq_gunzip_host, seq_gz_code.cpp) and the kernels (seq_gunzip.hip) share.  Integer-only plain C++, no intrinsics.
//
// Nothing in a member is trusted.  The input is touched through BitReader alone, which never loads outside
// [member, member + n_bytes) and reads zeros behind the end; every loop is bounded by construction (a chunk decodes at
// most `chunk` symbols of at least one bit, a header lists at most 19 + 258 lengths, a code has at most 15 bits).  A
// member is taken only if the pieces chain: block k's header is parsed from its entry, its first chunk starts where the
// header ends, every chunk decodes exactly its number of literals and lands on the next entry, the block's last chunk
// then reads end-of-block and lands on the next block's entry, the last block carries BFINAL (and no earlier one) and
// ends inside the last byte in front of the trailer with zero padding.  Entry 0 is 0, so the parses cover every bit of
// the body once, in order: what they yield is what a sequential inflater yields.  Anything else -- entries out of
// order or beyond the body, BTYPE != 2, HLIT != 257 or HDIST != 1 codes, an over-subscribed or incomplete code (but the
// one-symbol literal code of the empty block), a repeat with nothing before it or past the 258 lengths, no end-of-block
// code, a distance code, a symbol above 256, end-of-block inside a block -- makes the member FOREIGN, never a fault.
#pragma once

#include <cstdint>

#include "seq_gz_code.hpp"

namespace gams_gunzip {

using gams_gz::kLit;
using gams_gz::kSeq;

constexpr uint32_t kLutBits = 10;              // the primary table covers codes of up to 10 bits; longer ones walk
constexpr uint32_t kMaxBlock = 65536;          // the decoder stages a block in LDS: larger blocks are refused
constexpr int kDone = 0, kForeign = 1;         // GAMS_SEQ_GZ_DONE, GAMS_SEQ_GZ_FOREIGN

// the bytes of a member; a load behind the end reads zero
struct BitReader {
    const uint8_t *p;
    uint64_t n_bytes;
    GAMS_GZ_HD uint32_t byte(uint64_t i) const { return i < n_bytes ? p[i] : 0u; }
    GAMS_GZ_HD uint32_t le16(uint64_t i) const { return byte(i) | (byte(i + 1) << 8); }
    GAMS_GZ_HD uint32_t le32(uint64_t i) const { return le16(i) | (le16(i + 2) << 16); }
};

// a position in the member, in bits from its first byte, with at least 32 bits in hand
struct BitCursor {
    BitReader r;
    uint64_t buf, next, pos;
    uint32_t have;
    GAMS_GZ_HD BitCursor(const BitReader &r_, uint64_t bit) : r(r_), pos(bit) {
        const uint64_t b = bit >> 3;
        buf = ((uint64_t)r.le32(b) | ((uint64_t)r.le32(b + 4) << 32)) >> (bit & 7u);
        have = 64u - (uint32_t)(bit & 7u);
        next = b + 8;
    }
    GAMS_GZ_HD uint32_t peek(uint32_t n) const { return (uint32_t)buf & ((1u << n) - 1u); }   // n <= 16
    GAMS_GZ_HD void skip(uint32_t n) {                                                        // n <= 16
        buf >>= n;
        have -= n;
        pos += n;
        if (have < 32u) {
            buf |= (uint64_t)r.le32(next) << have;
            have += 32u;
            next += 4;
        }
    }
    GAMS_GZ_HD uint32_t take(uint32_t n) {
        const uint32_t v = peek(n);
        skip(n);
        return v;
    }
};

// the literal code of one block, ready to decode, and where its literals begin
struct DecodeTab {
    uint16_t lut[1u << kLutBits];   // by the next lut_bits bits of the stream: (length << 9) | symbol, 0: not a code of <= lut_bits bits
    uint16_t sorted[kSeq];          // the used symbols by (length, symbol)
    uint16_t count[16];             // codes per length
    uint32_t lut_bits;              // min(longest code, kLutBits)
    uint32_t hdr_bits;              // from the block's BFINAL bit to its first literal
    uint32_t final;                 // BFINAL
    uint32_t ok;                    // 0: the header was refused, nothing else here means anything
};
constexpr uint32_t kTabWords = (uint32_t)(sizeof(DecodeTab) / 4);
static_assert(sizeof(DecodeTab) % 4 == 0, "copied by words");

GAMS_GZ_HD inline uint32_t rev_bits(uint32_t c, uint32_t l) {
    uint32_t r = 0;
    for (uint32_t k = 0; k < l; ++k) r |= ((c >> k) & 1u) << (l - 1 - k);
    return r;
}

// one symbol through a canonical code given by count[] and sorted[], bit by bit (zlib's puff walks the same way):
// its length, 0 if the next 15 bits begin no code
GAMS_GZ_HD inline uint32_t walk(uint32_t bits, const uint16_t *count, const uint16_t *sorted, uint32_t max_len, uint32_t *sym) {
    uint32_t code = 0, first = 0, index = 0;
    for (uint32_t l = 1; l <= max_len; ++l) {
        code |= (bits >> (l - 1)) & 1u;
        const uint32_t c = count[l];
        if (code < first + c) {
            *sym = sorted[index + (code - first)];
            return l;
        }
        index += c;
        first = (first + c) << 1;
        code <<= 1;
    }
    return 0;
}

// The dynamic-Huffman block header at bit `at` of the member into t.  false: refused.
GAMS_GZ_HD inline bool parse_header(const BitReader &r, uint64_t at, DecodeTab &t) {
    t.ok = 0;
    BitCursor c(r, at);
    t.final = c.take(1);
    if (c.take(2) != 2u) return false;                        // BTYPE
    if (c.take(5) != kLit - 257u) return false;               // HLIT: 257 literal / length codes
    if (c.take(5) != 0u) return false;                        // HDIST: one distance code
    const uint32_t hclen = c.take(4) + 4u;
    const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    uint8_t cl[19];
    for (uint32_t k = 0; k < 19; ++k) cl[k] = 0;
    for (uint32_t k = 0; k < hclen; ++k) cl[order[k]] = (uint8_t)c.take(3);
    // the code-length code: complete, by its 7-bit table: (length << 5) | symbol
    uint32_t kraft = 0;
    for (uint32_t s = 0; s < 19; ++s)
        if (cl[s]) kraft += 1u << (7u - cl[s]);
    if (kraft != 128u) return false;
    uint8_t clut[128];
    {
        gams_gz::Canon canon(cl, 19);
        for (uint32_t s = 0; s < 19; ++s)
            if (cl[s]) {
                const uint32_t code = canon.take(cl[s]);      // reversed: as the stream holds it
                for (uint32_t k = code; k < 128u; k += 1u << cl[s]) clut[k] = (uint8_t)((cl[s] << 5) | s);
            }
    }
    // the 258 lengths, run-length coded across both alphabets
    uint8_t len[kSeq];
    uint32_t n = 0;
    while (n < kSeq) {                                        // every turn adds at least one length
        const uint32_t e = clut[c.peek(7)];
        c.skip(e >> 5);
        const uint32_t s = e & 31u;
        if (s < 16u) {
            len[n++] = (uint8_t)s;
            continue;
        }
        uint32_t rep, v = 0;
        if (s == 16u) {
            if (n == 0) return false;                         // nothing to repeat
            v = len[n - 1];
            rep = 3u + c.take(2);
        } else if (s == 17u) {
            rep = 3u + c.take(3);
        } else {
            rep = 11u + c.take(7);
        }
        if (n + rep > kSeq) return false;
        for (; rep; --rep) len[n++] = (uint8_t)v;
    }
    if (len[kLit] != 0 || len[256] == 0) return false;        // a distance code; no end-of-block
    uint32_t used = 0, longest = 0;
    for (uint32_t l = 0; l < 16; ++l) t.count[l] = 0;
    for (uint32_t s = 0; s < kLit; ++s)
        if (len[s]) {
            ++t.count[len[s]];
            ++used;
            if (len[s] > longest) longest = len[s];
        }
    kraft = 0;
    for (uint32_t l = 1; l < 16; ++l) kraft += (uint32_t)t.count[l] << (15u - l);
    if (kraft != 32768u && !(used == 1u && longest == 1u)) return false;   // over-subscribed or incomplete
    uint16_t slot[16];
    slot[0] = slot[1] = 0;
    for (uint32_t l = 1; l < 15; ++l) slot[l + 1] = (uint16_t)(slot[l] + t.count[l]);
    for (uint32_t s = 0; s < kLit; ++s)
        if (len[s]) t.sorted[slot[len[s]]++] = (uint16_t)s;
    for (uint32_t k = used; k < kSeq; ++k) t.sorted[k] = 0;
    t.lut_bits = longest < kLutBits ? longest : kLutBits;
    const uint32_t size = 1u << t.lut_bits;
    for (uint32_t k = 0; k < (1u << kLutBits); ++k) t.lut[k] = 0;
    {
        gams_gz::Canon canon(len, kLit);
        for (uint32_t s = 0; s < kLit; ++s)
            if (len[s]) {
                const uint32_t code = canon.take(len[s]);
                if (len[s] <= t.lut_bits)
                    for (uint32_t k = code; k < size; k += 1u << len[s]) t.lut[k] = (uint16_t)(((uint32_t)len[s] << 9) | s);
            }
    }
    t.hdr_bits = (uint32_t)(c.pos - at);
    t.ok = 1;
    return true;
}

// n_sym literals from bit `start` on through t: put(k, byte) for k = 0 .. n_sym - 1; with `eob` the end-of-block code
// has to follow them.  *end is the bit behind the last code read.  false: a symbol that is no literal (or no code at
// all), or no end-of-block where one was due.
template <typename Put>
GAMS_GZ_HD inline bool decode_chunk(const BitReader &r, const DecodeTab &t, uint64_t start, uint32_t n_sym, bool eob, Put put,
                                    uint64_t *end) {
    BitCursor c(r, start);
    const uint32_t mask = (1u << t.lut_bits) - 1u;
    for (uint32_t k = 0; k < n_sym + (eob ? 1u : 0u); ++k) {
        const uint32_t bits = c.peek(15);
        const uint32_t e = t.lut[bits & mask];
        uint32_t sym = e & 511u, l = e >> 9;
        if (l == 0) l = walk(bits, t.count, t.sorted, 15, &sym);
        if (l == 0) return false;
        c.skip(l);
        if (k < n_sym) {
            if (sym > 255u) return false;
            put(k, (uint8_t)sym);
        } else if (sym != 256u) {
            return false;
        }
    }
    *end = c.pos;
    return true;
}

// what the ten header bytes, the subfield and the trailer say, checked against one another in O(1): false: FOREIGN
struct Member {
    uint32_t block, chunk, n_entries, isize, crc;
    uint64_t idx;         // byte of entry 0
    uint64_t body;        // first byte of the deflate body
    uint64_t body_bits;   // from there to the trailer
};
GAMS_GZ_HD inline bool parse_member(const BitReader &r, Member &m) {
    const uint8_t head[gams_gz::kHead] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff};
    if (r.n_bytes < gams_gz::kHead + gams_gz::kIdxFixed + 1u + gams_gz::kTail) return false;
    for (uint32_t k = 0; k < gams_gz::kHead; ++k)
        if (r.byte(k) != head[k]) return false;
    const uint32_t xlen = r.le16(10), len = r.le16(14);
    if (r.byte(12) != 'G' || r.byte(13) != 'I' || xlen < 12u || len != xlen - 4u) return false;
    m.block = r.le32(16);
    m.chunk = r.le32(20);
    if (!gams_gz::chunk_ok(m.chunk) || m.block < gams_gz::kTile || m.block > kMaxBlock || m.block % gams_gz::kTile) return false;
    m.idx = 24;
    m.body = 12u + (uint64_t)xlen;
    if (m.body + 1u + gams_gz::kTail > r.n_bytes) return false;
    m.body_bits = 8u * (r.n_bytes - gams_gz::kTail - m.body);
    m.crc = r.le32(r.n_bytes - 8u);
    m.isize = r.le32(r.n_bytes - 4u);
    m.n_entries = (len - 8u) / 4u;
    if (len != 8u + 4u * m.n_entries || m.n_entries != gams_gz::idx_entries(m.isize, m.chunk)) return false;
    return true;
}

// the block's k-th chunk (of n_chunks, at least one: the empty block has a chunk of no literals): decoded through put,
// and whether it chains.  base0: the block's first base in the member, n: the block's bases.
template <typename Put>
GAMS_GZ_HD inline bool chunk_chains(const BitReader &r, const Member &m, const DecodeTab &t, uint64_t base0, uint32_t n, uint32_t k,
                                    uint32_t n_chunks, Put put) {
    const uint64_t e0 = base0 / m.chunk;                      // the block's first entry
    const bool last_chunk = k + 1u == n_chunks, last_block = base0 + n >= m.isize;
    uint64_t start;
    if (k == 0) {
        start = (m.n_entries ? r.le32(m.idx + 4u * e0) : 0u);
        if (e0 == 0 && start != 0) return false;
        start += t.hdr_bits;
    } else {
        start = r.le32(m.idx + 4u * (e0 + k));
    }
    if (start > m.body_bits) return false;
    const uint32_t n_sym = n - k * m.chunk < m.chunk ? n - k * m.chunk : m.chunk;
    uint64_t end = 0;
    if (!decode_chunk(r, t, 8u * m.body + start, n_sym, last_chunk, put, &end)) return false;
    end -= 8u * m.body;
    if (!(last_chunk && last_block)) return end == r.le32(m.idx + 4u * (e0 + k + 1u));
    // the body's end: inside the last byte in front of the trailer, the padding zero
    if (end > m.body_bits || end + 8u <= m.body_bits) return false;
    return (r.byte(m.body + (end >> 3)) >> (end & 7u)) == 0u || (end & 7u) == 0u;
}

// the whole member on one core, chunk by chunk, the way the device walks it: out[0, ISIZE) and DONE, or FOREIGN.
// false: the member passed its O(1) checks and ISIZE bases do not fit cap (*n_out = ISIZE).
inline bool gunzip_member(const uint8_t *member, uint64_t n_bytes, uint8_t *out, uint64_t cap, uint64_t *n_out, int *status) {
    const BitReader r{member, n_bytes};
    Member m;
    *n_out = 0;
    *status = kForeign;
    if (!parse_member(r, m)) return true;
    *n_out = m.isize;
    if (m.isize > cap) return false;
    static const struct Crc {
        uint32_t t[256];
        Crc() {
            for (uint32_t i = 0; i < 256; ++i) t[i] = gams_gz::crc_table0(i);
        }
    } T;
    uint32_t crc = 0xFFFFFFFFu;
    DecodeTab t;
    const uint64_t nb = gams_gz::n_blocks(m.isize, m.block);
    for (uint64_t b = 0; b < nb; ++b) {
        const uint64_t base0 = b * m.block;
        const uint32_t n = (uint32_t)(m.isize - base0 < m.block ? m.isize - base0 : m.block);
        const uint64_t at = m.n_entries ? r.le32(m.idx + 4u * (base0 / m.chunk)) : 0u;
        if (at > m.body_bits || !parse_header(r, 8u * m.body + at, t)) return true;
        if ((t.final != 0) != (b + 1 == nb)) return true;
        const uint32_t n_chunks = n ? (n + m.chunk - 1u) / m.chunk : 1u;
        for (uint32_t k = 0; k < n_chunks; ++k) {
            uint8_t *dst = out + base0 + (uint64_t)k * m.chunk;
            if (!chunk_chains(r, m, t, base0, n, k, n_chunks, [dst](uint32_t i, uint8_t v) { dst[i] = v; })) return true;
        }
        for (uint32_t i = 0; i < n; ++i) crc = T.t[(crc ^ out[base0 + i]) & 0xffu] ^ (crc >> 8);
    }
    if (~crc != m.crc) return true;
    *status = kDone;
    return true;
}

}  // namespace gams_gunzip
