// seq_gunzip.hip -- gams_seqset_upload_gz: the `seq:{ctg}` values back into the slots of a seqset, inflated on the
// device.  It takes the indexed members of seq_gz_code.hpp (GAMS_SEQ_GZ_INDEXED): literal-only dynamic-Huffman deflate
// with the bit offset of every block and of every `chunk` bases in the FEXTRA field, so that a block's chunks decode
// side by side.  The decoder core is seq_gunzip_code.hpp, which the host twin gams_seq_gunzip_host runs too; it reads
// the member through a bounded reader only and takes a member only if its pieces chain (see there).  The host checks
// the header, the subfield and the trailer of every value in O(1); what fails there is FOREIGN and is not uploaded.
// Four stages on the copy stream, which is where a seqset's uploads are ordered:
//   upload  the taken members back to back (16-byte aligned) behind the ctg and block tables, one copy
//   tables  one lane per block: the block's header into a DecodeTab (the one serial piece: up to 19 + 258 lengths)
//   decode  one workgroup per block: the table into LDS; lane j decodes chunk j into an LDS stage of the block's bases
//           (a word per four bases, chunk j's words rotated by j so that the lanes, which advance in step, write 32
//           different banks); then all 256 threads take the stage in 16-byte pieces: the bases to the slot with 16-byte
//           stores, the plane bits (b & 0xDB) == 0x43 two bytes a piece, the raw CRC-32 by the piece fold of
//           seq_gz_crc.hpp.  A slot's last piece and plane byte are written bytewise: nothing outside the slot changes
//   join    one wave per ctg: the blocks' raw CRCs joined and compared with the trailer, the status byte; the host reads
//           the bytes back
#include "common.hpp"
#include "seq_gunzip_code.hpp"
#include "seq_gz_crc.hpp"

#include <algorithm>
#include <string>
#include <thread>
#include <vector>

namespace {

using namespace gams_gunzip;
using gams_gz::CrcPieces;

enum : int { GU_UPLOAD = 0, GU_TABLES, GU_DECODE, GU_JOIN, GU_STAGES };

// a taken member: what its header says (checked on the host), where its bytes lie in the upload, where its slot begins
struct GunzipCtg {
    Member m;
    uint64_t src, dst;
    uint32_t bytes, blk0, n_blk, pad;
};

constexpr uint32_t kTabPad = (kTabWords + 3u) & ~3u;          // LDS words of the table, the CRC slices behind it
constexpr uint32_t kLdsFixed = kTabPad + 4u * 256u + 8u;      // ... then red[4], tail_crc, and the stage

__global__ __launch_bounds__(64) void gunzip_tables_kernel(uint32_t n_blk, const uint8_t *in, const GunzipCtg *ctgs,
                                                            const uint32_t *blk_ctg, const uint32_t *blk_k, DecodeTab *tabs) {
    const uint32_t b = blockIdx.x * 64u + threadIdx.x;
    if (b >= n_blk) return;
    const GunzipCtg &G = ctgs[blk_ctg[b]];
    const BitReader r{in + G.src, G.bytes};
    const uint64_t base0 = (uint64_t)blk_k[b] * G.m.block;
    const uint64_t at = G.m.n_entries ? r.le32(G.m.idx + 4u * (base0 / G.m.chunk)) : 0u;
    if (at > G.m.body_bits)
        tabs[b].ok = 0;
    else
        parse_header(r, 8u * G.m.body + at, tabs[b]);
}

__global__ __launch_bounds__(256) void gunzip_decode_kernel(const uint8_t *in, const GunzipCtg *ctgs, const uint32_t *blk_ctg,
                                                             const uint32_t *blk_k, const DecodeTab *tabs, const uint32_t *shift16,
                                                             uint32_t x_gap, uint8_t *seq, uint8_t *plane, uint32_t *blk_crc,
                                                             uint32_t *flag) {
    extern __shared__ uint32_t lds[];
    const DecodeTab &tab = *reinterpret_cast<const DecodeTab *>(lds);
    uint32_t(*T)[256] = reinterpret_cast<uint32_t(*)[256]>(lds + kTabPad);
    uint32_t *red = lds + kTabPad + 1024u, *tail_crc = red + 4, *stage = red + 8;
    const uint32_t tid = threadIdx.x, b = blockIdx.x, c = blk_ctg[b], k = blk_k[b];
    const GunzipCtg &G = ctgs[c];
    const Member m = G.m;
    for (uint32_t w = tid; w < kTabWords; w += 256u) lds[w] = reinterpret_cast<const uint32_t *>(tabs + b)[w];
    if (tid == 0) *tail_crc = 0;
    gams_gz::crc_slices_build(T, tid);   // (its barriers publish the table)
    const BitReader r{in + G.src, G.bytes};
    const uint64_t base0 = (uint64_t)k * m.block;
    const uint32_t n = (uint32_t)(m.isize - base0 < m.block ? m.isize - base0 : m.block);
    const uint32_t n_chunks = n ? (n + m.chunk - 1u) / m.chunk : 1u;   // <= 65,536 / 512
    const uint32_t cw = m.chunk >> 2;                                   // words per chunk, a power of two
    bool bad = false;
    if (tab.ok && (tab.final != 0) == (k + 1u == G.n_blk)) {
        if (tid < n_chunks) {
            uint32_t *mine = stage + tid * cw;
            uint32_t acc = 0;
            auto put = [&](uint32_t i, uint8_t v) {
                acc |= (uint32_t)v << (8u * (i & 3u));
                if ((i & 3u) == 3u) {
                    mine[((i >> 2) + tid) & (cw - 1u)] = acc;
                    acc = 0;
                }
            };
            bad = !chunk_chains(r, m, tab, base0, n, tid, n_chunks, put);
            const uint32_t n_sym = n - tid * m.chunk < m.chunk ? n - tid * m.chunk : m.chunk;
            if (n_sym & 3u) mine[((n_sym >> 2) + tid) & (cw - 1u)] = acc;   // (the bytes behind the last base are zero)
        }
    } else {
        bad = tid == 0;
    }
    if (bad) atomicOr(&flag[c], 1u);
    // (the barrier behind the stage's writers.)  A block with a refused header or a chunk that does not chain stores
    // nothing: its stage holds words nobody wrote, and they are not to reach the slot.  The member is flagged already.
    if (__syncthreads_or(bad ? 1 : 0)) {
        if (tid == 0) blk_crc[b] = 0;
        return;
    }
    uint8_t *dst = seq + G.dst + base0;                         // 16-byte aligned: slots on 256 B, blocks multiples of 4096
    uint8_t *pdst = plane + ((G.dst + base0) >> 3);
    CrcPieces crc;
    for (uint32_t base = tid * 16u; base < n; base += gams_gz::kTile) {
        const uint32_t m16 = n - base < 16u ? n - base : 16u;
        const uint32_t j = base / m.chunk, w0 = (base & (m.chunk - 1u)) >> 2;
        const uint32_t *from = stage + j * cw;
        uint4 v;
        v.x = from[(w0 + j) & (cw - 1u)];
        v.y = from[(w0 + 1u + j) & (cw - 1u)];
        v.z = from[(w0 + 2u + j) & (cw - 1u)];
        v.w = from[(w0 + 3u + j) & (cw - 1u)];
        crc.piece(T, x_gap, v, m16, base);
        uint32_t bits = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint32_t w = q == 0 ? v.x : q == 1 ? v.y : q == 2 ? v.z : v.w;
#pragma unroll
            for (int e = 0; e < 4; ++e) bits |= ((((w >> (8 * e)) & 0xDBu) == 0x43u) ? 1u : 0u) << (4 * q + e);
        }
        if (m16 == 16u) {
            *reinterpret_cast<uint4 *>(dst + base) = v;
            *reinterpret_cast<uint16_t *>(pdst + (base >> 3)) = (uint16_t)bits;
        } else {   // the slot's last piece: its bytes and plane bytes alone, the plane bits behind the last base zero
            bits &= (1u << m16) - 1u;
            for (uint32_t e = 0; e < m16; ++e) {
                const uint32_t w = e < 4u ? v.x : e < 8u ? v.y : e < 12u ? v.z : v.w;
                dst[base + e] = (uint8_t)(w >> (8u * (e & 3u)));
            }
            pdst[base >> 3] = (uint8_t)bits;
            if (m16 > 8u) pdst[(base >> 3) + 1u] = (uint8_t)(bits >> 8);
        }
    }
    const uint32_t raw = crc.finish(n, shift16, red, tail_crc);
    if (tid == 0) blk_crc[b] = raw;
}

// one wave per taken member
__global__ __launch_bounds__(64) void gunzip_join_kernel(const GunzipCtg *ctgs, const uint32_t *blk_crc, const uint32_t *flag,
                                                          uint8_t *status) {
    const uint32_t c = blockIdx.x, lane = threadIdx.x;
    const GunzipCtg &G = ctgs[c];
    const uint64_t len = G.m.isize;
    uint32_t raw = 0;
    for (uint32_t k = lane; k < G.n_blk; k += 64u) {
        const uint64_t stop = (uint64_t)(k + 1u) * G.m.block;
        raw ^= gams_gz::gf2_mul(blk_crc[G.blk0 + k], gams_gz::gf2_xpow8(stop < len ? len - stop : 0u));
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) raw ^= __shfl_xor(raw, d, 64);
    if (lane == 0) status[c] = (flag[c] || gams_gz::crc_finish(raw, len) != G.m.crc) ? GAMS_SEQ_GZ_FOREIGN : GAMS_SEQ_GZ_DONE;
}

uint32_t blocks_of(uint64_t n, uint32_t per) { return (uint32_t)std::max<uint64_t>(1, (n + per - 1) / per); }

int upload_gz_run(gams_gpu_t *h, gams_seqset_t *s, uint32_t first, uint32_t count, const uint8_t *const *members,
                  const uint64_t *member_bytes, uint8_t *status, uint32_t *n_foreign) {
    const std::string who = "seqset_upload_gz";
    h->k_valid = false;
    h->kq_used = 0;
    // the O(1) checks: what passes is taken
    std::vector<GunzipCtg> taken;
    std::vector<uint32_t> slot_of;
    uint64_t in_bytes = 0, n_blk64 = 0;
    uint32_t max_block = 0;
    for (uint32_t i = 0; i < count; ++i) {
        status[i] = GAMS_SEQ_GZ_FOREIGN;
        GunzipCtg G{};
        if (!members[i] || member_bytes[i] > 0xffffffffull || !parse_member(BitReader{members[i], member_bytes[i]}, G.m)) continue;
        if (G.m.isize != s->len[first + i])
            return gams_fail(h, GAMS_EINVAL, who + ": the member of slot " + std::to_string(first + i) + " holds " +
                                                 std::to_string(G.m.isize) + " bases, the slot " + std::to_string(s->len[first + i]));
        G.src = in_bytes;
        G.dst = s->off[first + i];
        G.bytes = (uint32_t)member_bytes[i];
        G.blk0 = (uint32_t)n_blk64;
        G.n_blk = (uint32_t)gams_gz::n_blocks(G.m.isize, G.m.block);
        in_bytes += ((uint64_t)G.bytes + 15u) & ~15ull;
        n_blk64 += G.n_blk;
        max_block = std::max(max_block, G.m.block);
        taken.push_back(G);
        slot_of.push_back(i);
    }
    const uint32_t n_taken = (uint32_t)taken.size();
    *n_foreign = count - n_taken;
    if (n_taken == 0) return GAMS_OK;
    if (n_blk64 > 0x7fffffffull) return gams_fail(h, GAMS_EUNSUPPORTED, who + ": more than 2^31 - 1 blocks");
    const uint32_t n_blk = (uint32_t)n_blk64;
    GAMS_HIP(h, hipSetDevice(h->device));
    hipStream_t st = h->copy;
    GAMS_HIP(h, gams_stopwatch_reserve(h, GU_STAGES));
    const StageClock stage{h, st};

    struct Desc {
        GunzipCtg *ctgs;
        uint32_t *blk_ctg, *blk_k, *shift16;
        uint8_t *in;
    };
    auto desc = [&](Carver &c) {
        Desc d{};
        d.ctgs = c.take<GunzipCtg>(n_taken);
        d.blk_ctg = c.take<uint32_t>(n_blk);
        d.blk_k = c.take<uint32_t>(n_blk);
        d.shift16 = c.take<uint32_t>(gams_gz::kShift16);
        d.in = c.take<uint8_t>((size_t)in_bytes);
        return d;
    };
    DecodeTab *d_tabs = nullptr;
    uint32_t *d_crc = nullptr, *d_flag = nullptr;
    uint8_t *d_status = nullptr;
    auto work = [&](Carver &c) {
        d_tabs = c.take<DecodeTab>(n_blk);
        d_crc = c.take<uint32_t>(n_blk);
        d_flag = c.take<uint32_t>(n_taken);
        d_status = c.take<uint8_t>(n_taken);
    };
    const size_t b_desc = layout_bytes(desc);
    PoolBlock pin(h, true, st), d_desc(h, false, st), d_work(h, false, st);
    GAMS_TRY(h, who, pin.alloc(b_desc + gams_align256(n_taken)));
    GAMS_TRY(h, who, d_desc.alloc(b_desc));
    GAMS_TRY(h, who, d_work.alloc(layout_bytes(work)));
    carve(d_work.p, work);
    const Desc hd = carve(pin.p, desc), dd = carve(d_desc.p, desc);
    uint8_t *const h_status = pin.p + b_desc;
    for (uint32_t t = 0; t < n_taken; ++t) {
        hd.ctgs[t] = taken[t];
        for (uint32_t k = 0; k < taken[t].n_blk; ++k) {
            hd.blk_ctg[taken[t].blk0 + k] = t;
            hd.blk_k[taken[t].blk0 + k] = k;
        }
    }
    gams_gz::crc_shift16_fill(hd.shift16);
    {   // the members into the page-locked block, the padding behind each zero; a few threads for a genome's worth
        const unsigned T = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>({8, std::thread::hardware_concurrency(), in_bytes >> 22}));
        auto copy = [&](unsigned w) {
            for (uint32_t t = w; t < n_taken; t += T) {
                uint8_t *q = hd.in + taken[t].src;
                std::memcpy(q, members[slot_of[t]], taken[t].bytes);
                std::memset(q + taken[t].bytes, 0, (size_t)(-(int64_t)taken[t].bytes & 15));
            }
        };
        std::vector<std::thread> pool;
        for (unsigned w = 1; w < T; ++w) pool.emplace_back(copy, w);
        copy(0);
        for (auto &th : pool) th.join();
    }
    const size_t lds_bytes = ((size_t)kLdsFixed + max_block / 4u) * 4u;
    GAMS_TRY(h, who, gams_lds_attr(h, reinterpret_cast<const void *>(gunzip_decode_kernel), lds_bytes));

    // the kernels write the seqset: a writer's bracket (the seqset protocol, common.hpp)
    {
        const int rc = gams_seqset_write_begin(h, s, st);
        if (rc != GAMS_OK) return rc;
    }
    GAMS_TRY(h, who, hipEventRecord(h->k0, st));
    GAMS_TRY(h, who, stage(GU_UPLOAD, true));
    GAMS_TRY(h, who, hipMemcpyAsync(d_desc.p, pin.p, b_desc, hipMemcpyHostToDevice, st));
    GAMS_TRY(h, who, hipMemsetAsync(d_flag, 0, (size_t)n_taken * 4, st));
    GAMS_TRY(h, who, stage(GU_UPLOAD, false));
    GAMS_TRY(h, who, stage(GU_TABLES, true));
    hipLaunchKernelGGL(gunzip_tables_kernel, dim3(blocks_of(n_blk, 64)), dim3(64), 0, st, n_blk, dd.in, dd.ctgs, dd.blk_ctg, dd.blk_k,
                       d_tabs);
    GAMS_TRY(h, who, hipGetLastError());
    GAMS_TRY(h, who, stage(GU_TABLES, false));
    GAMS_TRY(h, who, stage(GU_DECODE, true));
    hipLaunchKernelGGL(gunzip_decode_kernel, dim3(n_blk), dim3(256), lds_bytes, st, dd.in, dd.ctgs, dd.blk_ctg, dd.blk_k, d_tabs,
                       dd.shift16, gams_gz::crc_x_gap(), s->d_seq, s->d_plane, d_crc, d_flag);
    GAMS_TRY(h, who, hipGetLastError());
    GAMS_TRY(h, who, stage(GU_DECODE, false));
    GAMS_TRY(h, who, stage(GU_JOIN, true));
    hipLaunchKernelGGL(gunzip_join_kernel, dim3(n_taken), dim3(64), 0, st, dd.ctgs, d_crc, d_flag, d_status);
    GAMS_TRY(h, who, hipGetLastError());
    GAMS_TRY(h, who, hipMemcpyAsync(h_status, d_status, n_taken, hipMemcpyDeviceToHost, st));
    GAMS_TRY(h, who, stage(GU_JOIN, false));
    GAMS_TRY(h, who, hipEventRecord(h->k1, st));
    {
        const int rc = gams_seqset_write_end(h, s, st);
        if (rc != GAMS_OK) return rc;
    }
    GAMS_TRY(h, who, hipStreamSynchronize(st));
    h->kq_used = GU_STAGES;
    h->kq_staged = true;
    h->k_valid = true;
    for (uint32_t t = 0; t < n_taken; ++t) {
        status[slot_of[t]] = h_status[t];
        if (h_status[t] != GAMS_SEQ_GZ_DONE) ++*n_foreign;
    }
    return GAMS_OK;
}

}  // namespace

extern "C" int gams_seqset_upload_gz(gams_gpu_t *h, gams_seqset_t *s, uint32_t first, uint32_t count, const uint8_t *const *members,
                                     const uint64_t *member_bytes, uint8_t *status, uint32_t *n_foreign) {
    if (!h || !s || !n_foreign || (count && (!members || !member_bytes || !status)))
        return gams_fail(h, GAMS_EINVAL, "seqset_upload_gz: null argument");
    if (first > s->n_ctg || count > s->n_ctg - first) return gams_fail(h, GAMS_EINVAL, "seqset_upload_gz: slots outside the seqset");
    if (!s->have_bytes) return gams_fail(h, GAMS_ESTATE, "seqset_upload_gz: the seqset holds the G/C plane only");
    *n_foreign = 0;
    if (count == 0) return GAMS_OK;
    return upload_gz_run(h, s, first, count, members, member_bytes, status, n_foreign);
}
