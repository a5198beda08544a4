// seq_gz.hip -- gams_gpu_seq_gz: the `seq:{ctg}` values of `gams gen` (gen.rs:153-156 -> redis.rs:137-154) as gzip
// members deflated on the device from a resident seqset; only the finished bytes cross the link.  The members are
// literal-only dynamic-Huffman deflate, one block per `block` bases (seq_gz_code.hpp has the format and the code
// builder, which the host twin gams_seq_gz_host shares: both write the same bytes).  Five stages on the compute stream:
//   hist   one workgroup per block: the 256-bin histogram (LDS atomics over eight interleaved copies, so that the four
//          bases of DNA text do not meet in one bank word) and the block's raw CRC-32, from one read of the bases.  A
//          lane folds its 16-byte pieces, which lie 4096 bytes apart, by Horner's rule -- multiply by x^(8 * 4080),
//          then four table slices (built in LDS) over the piece --, the lanes' terms are shifted to the block's end by
//          a table of x^(128 j) and joined by XOR.  (The upload of the block table, 16 B a block, is timed with it.)
//   codes  one lane per block: gams_gz::build_block -- code lengths, canonical codes, the header's bits
//   sizes  one wave per ctg: the prefix sum of its blocks' bit counts (every block's bit offset in the body), the
//          CRC-32 of the ctg joined from the blocks' raw values by multiplication with x^(8 * bytes behind the block)
//          mod P -- on the device, a few microseconds, no per-block value is read back --, the member's length and,
//          for RESP, the length of its frame.  The host reads two words per ctg back, sums them to out_off and sizes the
//          output from that exact total
//   pack   a small kernel writes the RESP frames, the ten header bytes and the trailers into the zero-filled output;
//          then one workgroup per block encodes its bases through the (code, length) table in LDS: a workgroup prefix
//          sum of the lanes' bit counts per 4096 bases, the lanes' bits ORed into an LDS stage (atomics only on a lane's
//          first and last word), whole words stored coalesced.  A block's first and last word, which it may share with
//          its neighbour, the header or the trailer, are ORed into the output with global atomics; every other word is
//          a plain store inside the block's own bit range
//   copy   the finished bytes to the handle's page-locked buffer of this entry
#include "common.hpp"
#include "seq_gz_code.hpp"
#include "seq_gz_crc.hpp"

#include <algorithm>
#include <string>
#include <vector>

struct gams_seq_gz_state {
    uint32_t block = GAMS_SEQ_GZ_BLOCK;
    uint32_t chunk = GAMS_SEQ_GZ_CHUNK;   // of the indexed members (GAMS_SEQ_GZ_INDEXED)
    char *out = nullptr;
    size_t out_cap = 0;
};

void gams_seq_gz_free(gams_gpu_t *h) {
    gams_seq_gz_state *t = h->seq_gz;
    if (!t) return;
    gams_pool_free(h, true, t->out, t->out_cap);
    delete t;
    h->seq_gz = nullptr;
}

namespace {

using namespace gams_gz;

enum : int { GZ_HIST = 0, GZ_CODES, GZ_SIZES, GZ_PACK, GZ_COPY, GZ_STAGES };

constexpr uint32_t kHistCopies = 8;                  // interleaved: bin s of copy c is word s * 8 + c
constexpr uint32_t kTabStride = 260;                 // words per block of the (length, code) tables
constexpr uint32_t kStageWords = (31 + kTile * 15 + 31) / 32 + 4;   // a tile's bits behind a carry of < 32, and the word they may spill into

// per block of the call: where its bases are, how many, which ctg of the call it belongs to and where in it it begins
struct GzBlocks {
    const uint64_t *src;
    const uint32_t *n, *ctg, *at;
};

__global__ __launch_bounds__(256) void gz_hist_kernel(const uint8_t *seq, GzBlocks B, uint32_t x_gap, const uint32_t *shift16,
                                                       uint32_t *hist, uint32_t *blk_crc) {
    __shared__ uint32_t cnt[256 * kHistCopies];
    __shared__ uint32_t T[4][256];
    __shared__ uint32_t red[4];
    __shared__ uint32_t tail_crc;
    const uint32_t tid = threadIdx.x, b = blockIdx.x;
    for (uint32_t k = 0; k < kHistCopies; ++k) cnt[tid + 256u * k] = 0;
    if (tid == 0) tail_crc = 0;
    crc_slices_build(T, tid);
    const uint32_t n = B.n[b], copy = tid & (kHistCopies - 1);
    const uint8_t *p = seq + B.src[b];
    CrcPieces crc;   // (seq_gz_crc.hpp)
    for (uint32_t base = tid * 16u; base < n; base += kTile) {
        const uint32_t m = n - base < 16u ? n - base : 16u;
        const uint4 v = *reinterpret_cast<const uint4 *>(p + base);   // (a slot's tail may be read past: the seqset carries slack)
        crc.piece(T, x_gap, v, m, base);
        if (m == 16u) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t w = j == 0 ? v.x : j == 1 ? v.y : j == 2 ? v.z : v.w;
#pragma unroll
                for (int k = 0; k < 4; ++k) atomicAdd(&cnt[((w >> (8 * k)) & 0xffu) * kHistCopies + copy], 1u);
            }
        } else {
            const uint64_t lo = ((uint64_t)v.y << 32) | v.x, hi = ((uint64_t)v.w << 32) | v.z;
            for (uint32_t k = 0; k < m; ++k)
                atomicAdd(&cnt[(uint32_t)((k < 8u ? lo >> (8u * k) : hi >> (8u * (k - 8u))) & 0xffu) * kHistCopies + copy], 1u);
        }
    }
    const uint32_t raw = crc.finish(n, shift16, red, &tail_crc);
    uint32_t s = 0;
#pragma unroll
    for (uint32_t k = 0; k < kHistCopies; ++k) s += cnt[tid * kHistCopies + k];
    hist[(uint64_t)b * 256u + tid] = s;
    if (tid == 0) blk_crc[b] = raw;
}

__global__ __launch_bounds__(64) void gz_codes_kernel(uint32_t n_blk, const uint32_t *blk_ctg, const uint32_t *hist, uint32_t *tab,
                                                       uint32_t *hdr, uint32_t *hdr_bits, uint64_t *blk_bits) {
    const uint32_t b = blockIdx.x * 64u + threadIdx.x;
    if (b >= n_blk) return;
    const bool final = b + 1u == n_blk || blk_ctg[b + 1u] != blk_ctg[b];
    uint32_t hb = 0;
    uint64_t bb = 0;
    build_block(hist + (uint64_t)b * 256u, final, tab + (uint64_t)b * kTabStride, hdr + (uint64_t)b * kHdrWords, &hb, &bb);
    hdr_bits[b] = hb;
    blk_bits[b] = bb;
}

// one wave per ctg of the call
__global__ __launch_bounds__(64) void gz_sizes_kernel(const uint32_t *ctg_blk0, const uint32_t *ctg_len, uint32_t block, uint32_t chunk,
                                                       const uint64_t *blk_bits, const uint32_t *blk_crc,
                                                       const unsigned long long *id_off, uint64_t *blk_bit0, uint32_t *ctg_crc,
                                                       uint64_t *sizes) {
    const uint32_t i = blockIdx.x, lane = threadIdx.x;
    const uint32_t b0 = ctg_blk0[i], b1 = ctg_blk0[i + 1u];
    const uint64_t len = ctg_len[i];
    uint64_t run = 0;
    uint32_t raw = 0;
    for (uint32_t base = b0; base < b1; base += 64u) {
        const uint32_t b = base + lane;
        const bool ok = b < b1;
        const uint64_t bits = ok ? blk_bits[b] : 0u;
        const uint64_t inc = wave_incl_scan_u64(bits);
        if (ok) {
            blk_bit0[b] = run + inc - bits;
            const uint64_t stop = (uint64_t)(b - b0 + 1u) * block;
            raw ^= gf2_mul(blk_crc[b], gf2_xpow8(stop < len ? len - stop : 0u));
        }
        run += ((uint64_t)__shfl((uint32_t)(inc >> 32), 63, 64) << 32) | __shfl((uint32_t)inc, 63, 64);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) raw ^= __shfl_xor(raw, d, 64);
    if (lane == 0) {
        const uint64_t member = kHead + idx_extra(len, chunk) + (run + 7u) / 8u + kTail;   // (chunk 0: no index)
        ctg_crc[i] = crc_finish(raw, len);
        sizes[2u * i] = member;
        sizes[2u * i + 1u] = id_off ? resp_front(id_off[i + 1u] - id_off[i], member) + member + 2u : member;
    }
}

__device__ __forceinline__ uint8_t *gz_put_dec(uint8_t *p, uint64_t v) {
    const uint32_t n = dec_len(v);
    for (uint32_t k = n; k-- > 0; v /= 10u) p[k] = (uint8_t)('0' + v % 10u);
    return p + n;
}
__device__ __forceinline__ uint8_t *gz_put(uint8_t *p, const char *s, uint32_t n) {
    for (uint32_t k = 0; k < n; ++k) p[k] = (uint8_t)s[k];
    return p + n;
}

// one lane per ctg: everything of its bytes that is not the deflate body, and where that body begins
__global__ __launch_bounds__(256) void gz_frames_kernel(uint32_t count, const uint64_t *out_off, const uint64_t *sizes,
                                                         const uint32_t *ctg_crc, const uint32_t *ctg_len,
                                                         const unsigned long long *id_off, const char *id_bytes, uint32_t block,
                                                         uint32_t chunk, uint8_t *out, uint64_t *body_bit0) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= count) return;
    const uint64_t member = sizes[2u * i];
    uint8_t *q = out + out_off[i];
    if (id_off) {
        const uint64_t id_n = id_off[i + 1u] - id_off[i];
        q = gz_put(q, "*3\r\n$3\r\nSET\r\n$", 14);
        q = gz_put_dec(q, 4u + id_n);
        q = gz_put(q, "\r\nseq:", 6);
        for (uint64_t k = 0; k < id_n; ++k) *q++ = (uint8_t)id_bytes[id_off[i] + k];
        q = gz_put(q, "\r\n$", 3);
        q = gz_put_dec(q, member);
        q = gz_put(q, "\r\n", 2);
    }
    const uint8_t head[kHead] = {0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 0, 0xff};
    for (uint32_t k = 0; k < kHead; ++k) q[k] = head[k];
    const uint32_t crc = ctg_crc[i], len = ctg_len[i];
    const uint32_t extra = idx_extra(len, chunk);
    if (extra) {   // the index's fixed part; the pack kernel ORs the entries into the zeros behind it
        q[3] = 4;
        const uint32_t xlen = extra - 2u, sub = xlen - 4u;
        const uint8_t fixed[6] = {(uint8_t)xlen, (uint8_t)(xlen >> 8), 'G', 'I', (uint8_t)sub, (uint8_t)(sub >> 8)};
        for (uint32_t k = 0; k < 6; ++k) q[kHead + k] = fixed[k];
        for (uint32_t k = 0; k < 4; ++k) {
            q[kHead + 6u + k] = (uint8_t)(block >> (8u * k));
            q[kHead + 10u + k] = (uint8_t)(chunk >> (8u * k));
        }
    }
    body_bit0[i] = 8u * (uint64_t)(q + kHead + extra - out);
    uint8_t *t = q + member - kTail;
    for (uint32_t k = 0; k < 4; ++k) {
        t[k] = (uint8_t)(crc >> (8u * k));
        t[4u + k] = (uint8_t)(len >> (8u * k));
    }
    if (id_off) {
        t[8] = '\r';
        t[9] = '\n';
    }
}

// The stage holds `total` bits from bit 0 of word 0 (the caller has synchronised behind their writers): its whole
// words go to out[gw ..), the rest becomes the carry in word 0, everything else is zero again.  head_shared: word gw is
// shared with whatever stands in front of the block, and nothing of the block has been stored yet.
__device__ __forceinline__ void gz_flush(uint32_t *stage, uint32_t total, uint32_t *out, uint64_t &gw, uint32_t &carry,
                                         bool &head_shared) {
    const uint32_t n_full = total >> 5;
    for (uint32_t w = threadIdx.x; w < n_full; w += 256u) {
        const uint32_t v = stage[w];
        stage[w] = 0;
        if (w == 0 && head_shared)
            atomicOr(out + gw, v);
        else
            out[gw + w] = v;
    }
    __syncthreads();
    if (threadIdx.x == 0 && n_full) {
        const uint32_t v = stage[n_full];
        stage[n_full] = 0;
        stage[0] = v;
    }
    __syncthreads();
    if (n_full) head_shared = false;
    gw += n_full;
    carry = total & 31u;
}

__global__ __launch_bounds__(256) void gz_pack_kernel(const uint8_t *seq, GzBlocks B, const uint32_t *tab_all, const uint32_t *hdr_all,
                                                       const uint32_t *hdr_bits, const uint64_t *blk_bit0, const uint64_t *body_bit0,
                                                       const uint32_t *ctg_len, uint32_t chunk, uint32_t *out) {
    __shared__ uint32_t tab[kLit];
    __shared__ uint32_t stage[kStageWords];
    __shared__ uint32_t ws[4];
    const uint32_t tid = threadIdx.x, b = blockIdx.x;
    for (uint32_t k = tid; k < kLit; k += 256u) tab[k] = tab_all[(uint64_t)b * kTabStride + k];
    for (uint32_t k = tid; k < kStageWords; k += 256u) stage[k] = 0;
    const uint32_t n = B.n[b];
    const uint8_t *p = seq + B.src[b];
    const uint64_t body = body_bit0[B.ctg[b]], bit0 = body + blk_bit0[b];   // of the output
    // the indexed member: a lane that begins a chunk writes that chunk's entry (chunk divides kTile and is a multiple of 16)
    const uint32_t n_entries = chunk && idx_extra(ctg_len[B.ctg[b]], chunk) ? (uint32_t)idx_entries(ctg_len[B.ctg[b]], chunk) : 0u;
    const bool heads_chunk = n_entries && ((tid * 16u) & (chunk - 1u)) == 0;
    uint64_t gw = bit0 >> 5;
    uint32_t carry = (uint32_t)(bit0 & 31u);
    bool head_shared = carry != 0;
    __syncthreads();
    // the header: word k of it lands carry bits into stage word k
    const uint32_t hb = hdr_bits[b];
    if (tid < (hb + 31u) / 32u) {
        const uint32_t w = hdr_all[(uint64_t)b * kHdrWords + tid];
        atomicOr(&stage[tid], w << carry);
        if (carry) atomicOr(&stage[tid + 1u], w >> (32u - carry));
    }
    __syncthreads();
    gz_flush(stage, carry + hb, out, gw, carry, head_shared);
    for (uint32_t t0 = 0; t0 < n; t0 += kTile) {
        const uint32_t base = t0 + tid * 16u;
        const uint32_t m = base < n ? (n - base < 16u ? n - base : 16u) : 0u;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (m) v = *reinterpret_cast<const uint4 *>(p + base);
        uint32_t mine = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t w = j == 0 ? v.x : j == 1 ? v.y : j == 2 ? v.z : v.w;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if ((uint32_t)(4 * j + k) < m) mine += tab[(w >> (8 * k)) & 0xffu] >> 16;
        }
        uint32_t tile_bits = 0;
        const uint32_t pos = carry + block_excl_scan_256<uint32_t>(mine, ws, tile_bits);
        if (heads_chunk && m) {
            // the block's first lane names the block's first bit, every other one the first bit of its first literal; the
            // entries lie byte-aligned in front of the body, in words that other lanes and the body's first word may share
            const uint32_t v = base == 0 ? (uint32_t)blk_bit0[b] : (uint32_t)(gw * 32u + pos - body);
            const uint64_t a = (body >> 3) - 4ull * n_entries + 4ull * ((B.at[b] + base) / chunk);
            const uint32_t sh = 8u * (uint32_t)(a & 3u);
            atomicOr(out + (a >> 2), v << sh);
            if (sh) atomicOr(out + (a >> 2) + 1u, v >> (32u - sh));
        }
        // the lane's bits: its first and last stage word may be shared with its neighbours, the ones between are its own
        uint32_t sw = pos >> 5, nb = pos & 31u;
        uint64_t acc = 0;
        bool first = true;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t w = j == 0 ? v.x : j == 1 ? v.y : j == 2 ? v.z : v.w;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if ((uint32_t)(4 * j + k) < m) {
                    const uint32_t e = tab[(w >> (8 * k)) & 0xffu];
                    acc |= (uint64_t)(e & 0xffffu) << nb;
                    nb += e >> 16;
                    if (nb >= 32u) {
                        if (first)
                            atomicOr(&stage[sw], (uint32_t)acc);
                        else
                            stage[sw] = (uint32_t)acc;
                        first = false;
                        acc >>= 32;
                        nb -= 32u;
                        ++sw;
                    }
                }
        }
        if (nb && acc) atomicOr(&stage[sw], (uint32_t)acc);
        __syncthreads();
        gz_flush(stage, carry + tile_bits, out, gw, carry, head_shared);
    }
    if (tid == 0) {   // end-of-block: at most 15 bits behind a carry of < 32
        const uint32_t e = tab[256], code = e & 0xffffu;
        stage[0] |= code << carry;
        if (carry) stage[1] |= code >> (32u - carry);
    }
    __syncthreads();
    const uint32_t eob = tab[256] >> 16;
    gz_flush(stage, carry + eob, out, gw, carry, head_shared);
    if (tid == 0 && carry) atomicOr(out + gw, stage[0]);   // the block's last word: the next block, or the trailer, shares it
}

uint32_t blocks_of(uint64_t n, uint32_t per) { return (uint32_t)std::max<uint64_t>(1, (n + per - 1) / per); }

int seq_gz_run(gams_gpu_t *h, gams_seqset_t *s, uint32_t first, uint32_t count, const gams_names_t *ctg_ids, int format,
               const char **out, uint64_t *out_bytes, uint64_t *out_off) {
    const std::string who = "seq_gz";
    const bool resp = (format & ~GAMS_SEQ_GZ_INDEXED) == GAMS_LOADER_RESP;
    if (!h->seq_gz) h->seq_gz = new gams_seq_gz_state();
    gams_seq_gz_state *S = h->seq_gz;
    const uint32_t block = S->block, chunk = (format & GAMS_SEQ_GZ_INDEXED) ? S->chunk : 0u;
    h->k_valid = false;
    h->kq_used = 0;
    *out = S->out;
    *out_bytes = 0;
    out_off[0] = 0;
    if (count == 0) return GAMS_OK;
    const unsigned long long *id_off = nullptr;
    const char *id_bytes = nullptr;
    if (resp) {
        uint32_t n_ids = 0;
        gams_names_view(ctg_ids, &id_off, &id_bytes, &n_ids);
        if (n_ids < count) return gams_fail(h, GAMS_EINVAL, who + ": fewer ctg ids than slots");
    }
    uint64_t n_blk64 = 0;
    for (uint32_t i = 0; i < count; ++i) n_blk64 += n_blocks(s->len[first + i], block);
    if (n_blk64 > 0x7fffffffull) return gams_fail(h, GAMS_EUNSUPPORTED, who + ": more than 2^31 - 1 blocks");
    const uint32_t n_blk = (uint32_t)n_blk64;
    GAMS_HIP(h, hipSetDevice(h->device));
    hipStream_t st = h->compute;
    GAMS_HIP(h, gams_stopwatch_reserve(h, GZ_STAGES));
    const StageClock stage{h, st};

    // what the host knows: the blocks, the ctgs' first blocks and lengths, the shift table of the hist kernel
    struct Desc {
        uint64_t *src;
        uint32_t *n, *ctg, *at, *blk0, *len, *shift16;
    };
    auto desc = [&](Carver &c) {
        Desc d{};
        d.src = c.take<uint64_t>(n_blk);
        d.n = c.take<uint32_t>(n_blk);
        d.ctg = c.take<uint32_t>(n_blk);
        d.at = c.take<uint32_t>(n_blk);
        d.blk0 = c.take<uint32_t>((size_t)count + 1);
        d.len = c.take<uint32_t>(count);
        d.shift16 = c.take<uint32_t>(kShift16);
        return d;
    };
    uint32_t *d_hist = nullptr, *d_crc = nullptr, *d_tab = nullptr, *d_hdr = nullptr, *d_hbits = nullptr, *d_ctg_crc = nullptr;
    uint64_t *d_bits = nullptr, *d_bit0 = nullptr, *d_sizes = nullptr, *d_off = nullptr, *d_body = nullptr;
    auto work = [&](Carver &c) {
        d_hist = c.take<uint32_t>((size_t)n_blk * 256);
        d_crc = c.take<uint32_t>(n_blk);
        d_tab = c.take<uint32_t>((size_t)n_blk * kTabStride);
        d_hdr = c.take<uint32_t>((size_t)n_blk * kHdrWords);
        d_hbits = c.take<uint32_t>(n_blk);
        d_bits = c.take<uint64_t>(n_blk);
        d_bit0 = c.take<uint64_t>(n_blk);
        d_ctg_crc = c.take<uint32_t>(count);
        d_sizes = c.take<uint64_t>((size_t)count * 2);
        d_off = c.take<uint64_t>((size_t)count + 1);
        d_body = c.take<uint64_t>(count);
    };
    const size_t b_desc = layout_bytes(desc), b_sizes = (size_t)count * 16, b_off = ((size_t)count + 1) * 8;
    PoolBlock pin(h, true), d_desc(h, false), d_work(h, false), d_out(h, false);
    GAMS_TRY(h, who, pin.alloc(b_desc + gams_align256(b_sizes) + b_off));
    GAMS_TRY(h, who, d_desc.alloc(b_desc));
    GAMS_TRY(h, who, d_work.alloc(layout_bytes(work)));
    carve(d_work.p, work);
    const Desc hd = carve(pin.p, desc), dd = carve(d_desc.p, desc);
    uint64_t *const h_sizes = reinterpret_cast<uint64_t *>(pin.p + b_desc);
    uint64_t *const h_off = reinterpret_cast<uint64_t *>(pin.p + b_desc + gams_align256(b_sizes));
    uint32_t b = 0;
    for (uint32_t i = 0; i < count; ++i) {
        const uint64_t len = s->len[first + i], nb = n_blocks(len, block);
        hd.blk0[i] = b;
        hd.len[i] = (uint32_t)len;
        for (uint64_t k = 0; k < nb; ++k, ++b) {
            hd.src[b] = s->off[first + i] + k * block;
            hd.n[b] = (uint32_t)std::min<uint64_t>(block, len - k * block);
            hd.ctg[b] = i;
            hd.at[b] = (uint32_t)(k * block);
        }
    }
    hd.blk0[count] = b;
    crc_shift16_fill(hd.shift16);
    const GzBlocks B{dd.src, dd.n, dd.ctg, dd.at};

    const int wrc = gams_seqset_read_begin(h, s);   // the kernels read the sequence bytes
    if (wrc != GAMS_OK) return wrc;
    GAMS_TRY(h, who, hipEventRecord(h->k0, st));
    GAMS_TRY(h, who, stage(GZ_HIST, true));
    GAMS_TRY(h, who, hipMemcpyAsync(d_desc.p, pin.p, b_desc, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(gz_hist_kernel, dim3(n_blk), dim3(256), 0, st, s->d_seq, B, crc_x_gap(), dd.shift16, d_hist, d_crc);
    GAMS_TRY(h, who, hipGetLastError());
    GAMS_TRY(h, who, stage(GZ_HIST, false));
    GAMS_TRY(h, who, stage(GZ_CODES, true));
    hipLaunchKernelGGL(gz_codes_kernel, dim3(blocks_of(n_blk, 64)), dim3(64), 0, st, n_blk, dd.ctg, d_hist, d_tab, d_hdr, d_hbits, d_bits);
    GAMS_TRY(h, who, hipGetLastError());
    GAMS_TRY(h, who, stage(GZ_CODES, false));
    GAMS_TRY(h, who, stage(GZ_SIZES, true));
    hipLaunchKernelGGL(gz_sizes_kernel, dim3(count), dim3(64), 0, st, dd.blk0, dd.len, block, chunk, d_bits, d_crc, id_off, d_bit0, d_ctg_crc,
                       d_sizes);
    GAMS_TRY(h, who, hipGetLastError());
    GAMS_TRY(h, who, hipMemcpyAsync(h_sizes, d_sizes, b_sizes, hipMemcpyDeviceToHost, st));
    GAMS_TRY(h, who, stage(GZ_SIZES, false));
    GAMS_TRY(h, who, hipStreamSynchronize(st));
    uint64_t total = 0;
    for (uint32_t i = 0; i < count; ++i) {
        h_off[i] = total;
        total += h_sizes[2u * i + 1u];
    }
    h_off[count] = total;
    // whole words behind the last byte: a block's last word is ORed as a word
    const size_t out_alloc = (size_t)((total + 3u) & ~3ull) + 16u;
    GAMS_TRY(h, who, d_out.alloc(out_alloc));
    GAMS_TRY(h, who, gams_pool_grow(h, true, &S->out, &S->out_cap, total, total));
    GAMS_TRY(h, who, stage(GZ_PACK, true));
    GAMS_TRY(h, who, hipMemcpyAsync(d_off, h_off, b_off, hipMemcpyHostToDevice, st));
    GAMS_TRY(h, who, hipMemsetAsync(d_out.p, 0, out_alloc, st));
    hipLaunchKernelGGL(gz_frames_kernel, dim3(blocks_of(count, 256)), dim3(256), 0, st, count, d_off, d_sizes, d_ctg_crc, dd.len, id_off,
                       id_bytes, block, chunk, d_out.p, d_body);
    hipLaunchKernelGGL(gz_pack_kernel, dim3(n_blk), dim3(256), 0, st, s->d_seq, B, d_tab, d_hdr, d_hbits, d_bit0, d_body,
                       dd.len, chunk, reinterpret_cast<uint32_t *>(d_out.p));
    GAMS_TRY(h, who, hipGetLastError());
    GAMS_TRY(h, who, stage(GZ_PACK, false));
    GAMS_TRY(h, who, stage(GZ_COPY, true));
    GAMS_TRY(h, who, hipMemcpyAsync(S->out, d_out.p, total, hipMemcpyDeviceToHost, st));
    GAMS_TRY(h, who, stage(GZ_COPY, false));
    GAMS_TRY(h, who, hipEventRecord(h->k1, st));
    GAMS_TRY(h, who, hipStreamSynchronize(st));
    h->kq_used = GZ_STAGES;
    h->kq_staged = true;
    h->k_valid = true;
    *out = S->out;
    *out_bytes = total;
    std::copy(h_off, h_off + count + 1, out_off);
    return GAMS_OK;
}

}  // namespace

extern "C" {

int gams_gpu_seq_gz(gams_gpu_t *h, gams_seqset_t *s, uint32_t first, uint32_t count, const gams_names_t *ctg_ids, int format,
                    const char **out, uint64_t *out_bytes, uint64_t *out_off) {
    if (!h || !s || !out || !out_bytes || !out_off) return gams_fail(h, GAMS_EINVAL, "seq_gz: null argument");
    const int framing = format & ~GAMS_SEQ_GZ_INDEXED;   // the indexed form of either
    if (framing != GAMS_SEQ_GZ_MEMBERS && framing != GAMS_LOADER_RESP) return gams_fail(h, GAMS_EINVAL, "seq_gz: unknown format");
    if (framing == GAMS_LOADER_RESP && !ctg_ids) return gams_fail(h, GAMS_EINVAL, "seq_gz: the SET stream needs the ctg ids");
    if (first > s->n_ctg || count > s->n_ctg - first) return gams_fail(h, GAMS_EINVAL, "seq_gz: slots outside the seqset");
    if (!s->have_bytes) return gams_fail(h, GAMS_ESTATE, "seq_gz: the seqset holds the G/C plane only");
    return seq_gz_run(h, s, first, count, ctg_ids, format, out, out_bytes, out_off);
}

int gams_gpu_seq_gz_set_block(gams_gpu_t *h, uint32_t block) {
    if (!h) return GAMS_EINVAL;
    if (!gams_gz::block_ok(block)) return gams_fail(h, GAMS_EINVAL, "seq_gz_set_block: a multiple of 4096 between 4096 and 2^24");
    if (!h->seq_gz) h->seq_gz = new gams_seq_gz_state();
    h->seq_gz->block = block;
    return GAMS_OK;
}

int gams_gpu_seq_gz_set_chunk(gams_gpu_t *h, uint32_t chunk) {
    if (!h) return GAMS_EINVAL;
    if (!gams_gz::chunk_ok(chunk)) return gams_fail(h, GAMS_EINVAL, "seq_gz_set_chunk: 512, 1024, 2048 or 4096");
    if (!h->seq_gz) h->seq_gz = new gams_seq_gz_state();
    h->seq_gz->chunk = chunk;
    return GAMS_OK;
}

}  // extern "C"
