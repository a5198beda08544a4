// gen.hip -- the per-base scan of `gams gen` (first "next" row).
//
// Replaces the loop of src/cmd_gams/gen.rs:86-93: every base that is not one of
// A C G T a c g t is "ambiguous"; the valid set is the complement (gen.rs:100-102), then
// fill(fill-1) and excise(min) (gen.rs:103-104) and the --piece split (gen.rs:108-126).
//
// Device: one lane per 16-B chunk, coalesced 16-B loads, SWAR membership test (three
// exact zero-byte tests per dword: G/C class, A class, T class), 16-bit validity mask, and
// the positions where validity flips (a handful per megabase) appended to a small list.
// Host: sort the flips, pair them into spans, fill, excise, split into pieces -- O(#runs).
//
// gams_gpu_gen_text (below the scan) goes from the bytes of a FASTA file to the ctg table and a resident seqset:
//   mark     per 16-KiB block of the input: does it hold a '\n', and is the byte behind its last '\n' a '>'; a byte
//            >= 0x80 or a NUL raises the refusal flag;
//   carry    one workgroup: for every block, is its first byte part of a header line;
//   count    per block: payload bytes (bases) and header lines; white space inside a sequence line raises the flag;
//   offsets  64-bit prefixes of both counts (blk_offsets_scan_kernel);
//   compact  every block stages its bases in LDS and writes its slice of the concatenated base stream in 16-B
//            units; every header line leaves (its position, the bases in front of it) in its slot of the header list;
//   scan     gen_scan_kernel, once, over the whole stream;
//   table    host: runs cut at the chromosome boundaries, fill, excise, --piece, ids from the host's copy of the bytes;
//   place    one lane per 16 B of a ctg's slot: two aligned 16-B loads of the stream combined, one aligned 16-B store,
//            and the two bytes of the G/C plane that describe it.

#include "gen_split.hpp"
#include "text_emit.hpp"

#include <algorithm>
#include <chrono>
#include <unordered_set>

// What gams_gpu_gen_text leaves: the chromosomes (file order), the ctgs (chromosome order, then serial) and the seqset
// (slot k = ctg k) until gams_gen_seqset hands it out.
struct gams_gen {
    std::string names;                 // the ids, one behind the other
    std::vector<uint64_t> name_off;    // n_chr + 1
    std::vector<uint32_t> chr_len;
    std::vector<gams_gen_ctg_t> ctgs;
    gams_seqset_t *set = nullptr;
    bool taken = false;
};

namespace {

// 0x80 in every byte of x that equals `C` after clearing the case bit (0x20); exact for all
// byte values: t's bit 7 is set iff the low 7 bits (without bit 5) differ, x's bit 7 rules out
// bytes >= 0x80.
template <uint32_t C>
__device__ __forceinline__ uint32_t eq_nocase(uint32_t x) {
    constexpr uint32_t c4 = C * 0x01010101u;
    const uint32_t t = ((x & 0x5F5F5F5Fu) ^ c4) + 0x7F7F7F7Fu;
    return ~(t | x | 0x7F7F7F7Fu);
}

__device__ __forceinline__ uint32_t valid_flags(uint32_t x) {
    // G/C/g/c: (b & 0xDB) == 0x43 (see wave_kernels.hpp); A/a: 0x41; T/t: 0x54
    const uint32_t t = ((x & 0x5B5B5B5Bu) ^ 0x43434343u) + 0x7F7F7F7Fu;
    const uint32_t gc = ~(t | x | 0x7F7F7F7Fu);
    return gc | eq_nocase<0x41>(x) | eq_nocase<0x54>(x);
}

__device__ __forceinline__ uint32_t valid_mask16(const uint4 v) {
    uint32_t lo = __builtin_amdgcn_udot4(valid_flags(v.x), 0x08040201u, 0u, false);
    lo = __builtin_amdgcn_udot4(valid_flags(v.y), 0x80402010u, lo, false);
    uint32_t hi = __builtin_amdgcn_udot4(valid_flags(v.z), 0x08040201u, 0u, false);
    hi = __builtin_amdgcn_udot4(valid_flags(v.w), 0x80402010u, hi, false);
    return (lo >> 7) | (hi << 1);
}

// flips[] receives 2*pos + kind: kind 0 = a valid run starts at base pos (0-based),
// kind 1 = a valid run ends just before base pos.  Bases at or beyond len count as invalid.
__global__ __launch_bounds__(256) void gen_scan_kernel(const uint8_t *seq, uint64_t len, uint64_t n_chunks,
                                                       unsigned long long *flips, uint64_t cap,
                                                       unsigned long long *n_flips) {
    const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_chunks) return;
    const uint4 v = load_once16(reinterpret_cast<const uint4 *>(seq) + c);   // a chromosome is scanned once
    uint32_t m = valid_mask16(v);
    const uint64_t b0 = c * 16u;
    if (b0 + 16u > len) m &= (1u << (uint32_t)(len - b0)) - 1u;      // tail of the sequence
    uint32_t prev = 0;                                                // validity of base b0 - 1
    if (c > 0) {
        const uint32_t pb = seq[b0 - 1u] & 0xDFu;
        prev = (pb == 0x41u || pb == 0x43u || pb == 0x47u || pb == 0x54u) ? 1u : 0u;
    }
    const uint32_t shifted = (m << 1) | prev;                         // validity of the base before each base
    uint32_t diff = (m ^ shifted) & 0xFFFFu;                          // bit j: base b0+j differs from base b0+j-1
    // (a flip at base b0+16 belongs to the next chunk)
    while (diff) {
        const uint32_t j = (uint32_t)__ffs((int)diff) - 1u;
        diff &= diff - 1u;
        const uint32_t starts = (m >> j) & 1u;                        // 1: run starts here, 0: run ended
        const unsigned long long at = atomicAdd(n_flips, 1ull);
        if (at < cap) flips[at] = 2ull * (b0 + j) + (starts ? 0ull : 1ull);
    }
    // the end of the sequence closes an open run; a partial last chunk already produced
    // that flip (its masked-off bases read as invalid), a full one has not
    if (b0 + 16u == len && (m >> 15) & 1u) {
        const unsigned long long at = atomicAdd(n_flips, 1ull);
        if (at < cap) flips[at] = 2ull * len + 1ull;
    }
}

// ---------------------------------------------------------------------------
// FASTA bytes -> the concatenated base stream and the header list
// ---------------------------------------------------------------------------
constexpr uint32_t kGenBlk = 256u * 64u;   // input bytes per workgroup, 64 per lane (kIdxBytes of text.hip)

enum : uint32_t {
    GW_BAD = 0,   // a byte >= 0x80 or a NUL
    GW_WS = 1,    // a '\r' that does not end its line, a space, tab, 0x0B or 0x0C inside a sequence line
    GW_PAY = 2,   // bases
    GW_HDR = 3,   // header lines
    GW_COUNT = 8
};

struct GenHdr {
    unsigned long long pos;   // of the '>' in the input
    unsigned long long pay;   // bases in front of it
};

// 0x80 in exactly the zero bytes of y
__device__ __forceinline__ uint32_t gen_zero_bytes(uint32_t y) {
    return ~(((y & 0x7f7f7f7fu) + 0x7f7f7f7fu) | y | 0x7f7f7f7fu);
}

// This lane's 64 bytes and the dword behind them (the input is padded with '\n' to whole blocks and 64 B more).
__device__ __forceinline__ void gen_load(const uint8_t *in, uint64_t p0, uint32_t (&w)[17]) {
#pragma unroll
    for (uint32_t u = 0; u < 4u; ++u) {
        const uint4 v = *reinterpret_cast<const uint4 *>(in + p0 + 16u * u);
        w[4u * u] = v.x;
        w[4u * u + 1u] = v.y;
        w[4u * u + 2u] = v.z;
        w[4u * u + 3u] = v.w;
    }
    w[16] = *reinterpret_cast<const uint32_t *>(in + p0 + 64u);
}

// What a stretch of bytes does to the line state: 0 = it holds no '\n', else 1 + (the byte behind its last '\n' is
// '>': the line open at its end is a header line).
__device__ __forceinline__ uint32_t gen_code(const uint32_t (&w)[17]) {
    uint32_t code = 0;
#pragma unroll
    for (uint32_t i = 0; i < 16u; ++i) {
        const uint32_t m = gen_zero_bytes(w[i] ^ 0x0a0a0a0au);
        if (m) {
            const uint32_t b = (31u - (uint32_t)__clz((int)m)) >> 3;   // the last '\n' of this dword
            const uint32_t nx = b == 3u ? (w[i + 1u] & 0xffu) : ((w[i] >> (8u * (b + 1u))) & 0xffu);
            code = nx == (uint32_t)'>' ? 2u : 1u;
        }
    }
    return code;
}

// The last nonzero code among the lanes in front of this one (0: none) over a workgroup of 256; `all`: among all of
// them.  `ws` is LDS scratch of 4 words; two barriers, may be used back to back.
__device__ __forceinline__ uint32_t block_last_nonzero_256(uint32_t code, uint32_t *ws, uint32_t &all) {
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const unsigned long long bal = __ballot(code != 0u);
    const unsigned long long below = bal & ((1ull << lane) - 1ull);
    const uint32_t got = (uint32_t)__shfl((int)code, below ? 63 - __clzll((long long)below) : 0, 64);
    const uint32_t mine = below ? got : 0u;
    const uint32_t wl = (uint32_t)__shfl((int)code, bal ? 63 - __clzll((long long)bal) : 0, 64);
    if (lane == 0u) ws[wv] = bal ? wl : 0u;
    __syncthreads();
    const uint32_t w0 = ws[0], w1 = ws[1], w2 = ws[2], w3 = ws[3];
    __syncthreads();
    uint32_t carry = 0;
    if (wv > 0u && w0) carry = w0;
    if (wv > 1u && w1) carry = w1;
    if (wv > 2u && w2) carry = w2;
    all = w3 ? w3 : w2 ? w2 : w1 ? w1 : w0;
    return mine ? mine : carry;
}

// mark: the code of every block, and the flag of refused bytes
__global__ __launch_bounds__(256) void gen_mark_kernel(const uint8_t *in, uint32_t *blk_code, unsigned long long *words) {
    __shared__ uint32_t ws[4];
    const uint64_t p0 = ((uint64_t)blockIdx.x * 256u + threadIdx.x) * 64u;
    uint32_t w[17];
    gen_load(in, p0, w);
    uint32_t bad = 0;
#pragma unroll
    for (uint32_t i = 0; i < 16u; ++i) bad |= (w[i] & 0x80808080u) | gen_zero_bytes(w[i]);
    if (bad) words[GW_BAD] = 1ull;
    uint32_t all;
    (void)block_last_nonzero_256(gen_code(w), ws, all);
    if (threadIdx.x == 0u) blk_code[blockIdx.x] = all;
}

// carry: blk_in[b] = the first byte of block b is part of a header line.  One workgroup; the input begins with '>'.
__global__ __launch_bounds__(256) void gen_carry_kernel(const uint32_t *blk_code, uint32_t nb, uint32_t *blk_in) {
    __shared__ uint32_t ws[4];
    const uint32_t per = (nb + 255u) / 256u;
    const uint32_t b0 = min(nb, threadIdx.x * per), b1 = min(nb, b0 + per);
    uint32_t last = 0;
    for (uint32_t b = b0; b < b1; ++b) {
        const uint32_t c = blk_code[b];
        if (c) last = c;
    }
    uint32_t all;
    uint32_t st = block_last_nonzero_256(last, ws, all);
    if (!st) st = 2u;
    for (uint32_t b = b0; b < b1; ++b) {
        blk_in[b] = st == 2u ? 1u : 0u;
        const uint32_t c = blk_code[b];
        if (c) st = c;
    }
}

// One pass over a lane's 64 bytes.  hdr: its first byte is part of a header line (ignored when line_start says that
// the byte begins a line).  Counts the bases and the header lines; kEmit: bases to stage[0 ..), header records to
// hdrs[0 ..) with pos0 = the position of the first byte and pay0 = the bases in front of it.
template <bool kEmit>
__device__ __forceinline__ void gen_walk(const uint32_t (&w)[17], bool hdr, bool line_start, uint32_t &n_pay,
                                         uint32_t &n_hdr, uint32_t &refused, uint8_t *stage, GenHdr *hdrs, uint64_t pos0,
                                         uint64_t pay0) {
#pragma unroll
    for (uint32_t j = 0; j < 64u; ++j) {
        const uint32_t c = (w[j >> 2] >> (8u * (j & 3u))) & 0xffu;
        const uint32_t cn = (w[(j + 1u) >> 2] >> (8u * ((j + 1u) & 3u))) & 0xffu;
        if (line_start) {
            hdr = c == (uint32_t)'>';
            if (hdr) {
                if (kEmit) hdrs[n_hdr] = GenHdr{pos0 + j, pay0 + n_pay};
                ++n_hdr;
            }
        }
        line_start = c == (uint32_t)'\n';
        if (!line_start && !hdr) {
            const bool drop = c == (uint32_t)'\r' && cn == (uint32_t)'\n';   // (the padding makes the input end in '\n')
            if ((c == (uint32_t)'\r' && !drop) || c == (uint32_t)' ' || (c >= 0x09u && c <= 0x0cu)) refused = 1u;
            if (!drop) {
                if (kEmit) stage[n_pay] = (uint8_t)c;
                ++n_pay;
            }
        }
    }
}

struct GenPack {
    const uint8_t *in;
    const uint32_t *blk_in;
    uint32_t *blk_pay, *blk_hdr;                     // count: out
    const unsigned long long *pay_off, *hdr_off;     // compact: in
    uint8_t *cat;
    GenHdr *hdrs;
    unsigned long long *words;
};

// count (kEmit = false) and compact (kEmit = true)
template <bool kEmit>
__global__ __launch_bounds__(256) void gen_pack_kernel(const GenPack a) {
    __shared__ uint32_t ws[4];
    __shared__ __attribute__((aligned(16))) uint8_t stage[kEmit ? kGenBlk + 16u : 16u];
    const uint32_t b = blockIdx.x, tid = threadIdx.x;
    const uint64_t p0 = ((uint64_t)b * 256u + tid) * 64u;
    uint32_t w[17];
    gen_load(a.in, p0, w);
    uint32_t all;
    const uint32_t prev = block_last_nonzero_256(gen_code(w), ws, all);
    const bool hdr = prev ? prev == 2u : a.blk_in[b] != 0u;
    const bool line_start = p0 == 0u || a.in[p0 - 1u] == (uint8_t)'\n';
    uint32_t n_pay = 0, n_hdr = 0, refused = 0;
    gen_walk<false>(w, hdr, line_start, n_pay, n_hdr, refused, nullptr, nullptr, 0u, 0u);
    uint32_t tot_pay, tot_hdr;
    const uint32_t o_pay = block_excl_scan_256<uint32_t>(n_pay, ws, tot_pay);
    const uint32_t o_hdr = block_excl_scan_256<uint32_t>(n_hdr, ws, tot_hdr);
    if (!kEmit) {
        if (refused) a.words[GW_WS] = 1ull;
        if (tid == 0u) {
            a.blk_pay[b] = tot_pay;
            a.blk_hdr[b] = tot_hdr;
        }
        return;
    }
    const unsigned long long base = a.pay_off[b];
    const uint32_t mis = (uint32_t)(base & 15ull);   // the stream's block is 256-B aligned
    n_pay = n_hdr = 0;
    gen_walk<true>(w, hdr, line_start, n_pay, n_hdr, refused, stage + mis + o_pay, a.hdrs + a.hdr_off[b] + o_hdr, p0,
                   base + o_pay);
    __syncthreads();
    stage_flush_256(reinterpret_cast<const char *>(stage), mis, tot_pay, reinterpret_cast<char *>(a.cat) + base);
}

// ---------------------------------------------------------------------------
// the base stream -> the ctgs' slots of the seqset and their G/C plane
// ---------------------------------------------------------------------------
struct GenPlace {
    const uint8_t *cat;
    uint8_t *seq, *plane;
    const unsigned long long *chunk_off;   // n_ctg + 1: 16-B units in front of ctg k
    const unsigned long long *src, *dst;   // of ctg k: first base in the stream, first byte in the seqset (256-B aligned)
    const uint32_t *len;
    uint32_t n_ctg;
    unsigned long long n_chunks;
};

// 0x80 in every byte of x that is one of C G c g: (b & 0xDB) == 0x43 (wave_kernels.hpp)
__device__ __forceinline__ uint32_t gc_flags(uint32_t x) {
    const uint32_t t = ((x & 0x5B5B5B5Bu) ^ 0x43434343u) + 0x7F7F7F7Fu;
    return ~(t | x | 0x7F7F7F7Fu);
}

__global__ __launch_bounds__(256) void gen_place_kernel(const GenPlace a) {
    const uint64_t q = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (q >= a.n_chunks) return;
    uint32_t lo = 0, hi = a.n_ctg;               // chunk_off[lo] <= q < chunk_off[hi]
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (a.chunk_off[mid] <= q)
            lo = mid;
        else
            hi = mid;
    }
    const uint64_t c16 = (q - a.chunk_off[lo]) * 16u;
    const uint32_t rem = a.len[lo] - (uint32_t)c16;      // bases of the ctg from this unit on: >= 1
    const uint64_t s = a.src[lo] + c16;
    const uint32_t sh = (uint32_t)(s & 15u);
    // the unit's 16 bases lie in two aligned units of the stream (its block carries 64 B of slack)
    const uint4 v0 = load_once16(reinterpret_cast<const uint4 *>(a.cat + (s - sh)));
    const uint4 v1 = load_once16(reinterpret_cast<const uint4 *>(a.cat + (s - sh)) + 1);
    const uint32_t d[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
    const uint32_t qd = sh >> 2, r = (sh & 3u) * 8u;
    uint32_t o[4];
#pragma unroll
    for (uint32_t i = 0; i < 4u; ++i) {
        const uint32_t e0 = qd == 0u ? d[i] : qd == 1u ? d[i + 1u] : qd == 2u ? d[i + 2u] : d[i + 3u];
        const uint32_t e1 = qd == 0u ? d[i + 1u] : qd == 1u ? d[i + 2u] : qd == 2u ? d[i + 3u] : d[i + 4u];
        o[i] = (uint32_t)((((uint64_t)e1 << 32) | e0) >> r);
        // bytes past the ctg are zero, like the gaps between the slots
        const uint32_t keep = rem > 4u * i ? min(rem - 4u * i, 4u) : 0u;
        o[i] &= keep >= 4u ? 0xffffffffu : (1u << (8u * keep)) - 1u;
    }
    const uint64_t t = a.dst[lo] + c16;
    *reinterpret_cast<uint4 *>(a.seq + t) = make_uint4(o[0], o[1], o[2], o[3]);
    uint32_t m = __builtin_amdgcn_udot4(gc_flags(o[0]), 0x08040201u, 0u, false);
    m = __builtin_amdgcn_udot4(gc_flags(o[1]), 0x80402010u, m, false);
    uint32_t mh = __builtin_amdgcn_udot4(gc_flags(o[2]), 0x08040201u, 0u, false);
    mh = __builtin_amdgcn_udot4(gc_flags(o[3]), 0x80402010u, mh, false);
    *reinterpret_cast<uint16_t *>(a.plane + (t >> 3)) = (uint16_t)((m >> 7) | (mh << 1));
}

// fill(fill - 1): holes of at most fill-1 bases are closed (gen.rs:103); excise(min): spans shorter than min are
// dropped (gen.rs:104).  Spans are 1-based, inclusive, ascending.
std::vector<std::pair<int64_t, int64_t>> fill_excise(const std::vector<std::pair<int64_t, int64_t>> &spans, int32_t fill,
                                                     int32_t min_len) {
    std::vector<std::pair<int64_t, int64_t>> filled, out;
    for (auto &sp : spans) {
        if (!filled.empty() && sp.first - filled.back().second - 1 <= (int64_t)fill - 1)
            filled.back().second = sp.second;
        else
            filled.push_back(sp);
    }
    for (auto &sp : filled)
        if (sp.second - sp.first + 1 >= (int64_t)min_len) out.push_back(sp);
    return out;
}

// The flips of gen_scan_kernel over d_seq[0, len) on the compute stream, sorted: the list grows once if it was short.
// d_blk is the caller's block for the counter (first 256 B) and the list; t0 / t1 are recorded around the kernel.
int scan_flips(gams_gpu_t *h, const std::string &who, const uint8_t *d_seq, uint64_t len, PoolBlock &d_blk, hipEvent_t t0,
               hipEvent_t t1, std::vector<unsigned long long> &flips) {
    const uint64_t n_chunks = (len + 15) / 16;
    uint64_t fcap = 1u << 16;
    for (int attempt = 0; attempt < 2; ++attempt) {
        GAMS_TRY(h, who, d_blk.alloc(256 + fcap * sizeof(unsigned long long)));
        unsigned long long *const d_n = reinterpret_cast<unsigned long long *>(d_blk.p);
        unsigned long long *const d_flips = reinterpret_cast<unsigned long long *>(d_blk.p + 256);
        GAMS_TRY(h, who, hipMemsetAsync(d_n, 0, sizeof(unsigned long long), h->compute));
        GAMS_TRY(h, who, hipEventRecord(t0, h->compute));
        hipLaunchKernelGGL(gen_scan_kernel, dim3((unsigned)((n_chunks + 255) / 256)), dim3(256), 0, h->compute, d_seq, len,
                           n_chunks, d_flips, fcap, d_n);
        GAMS_TRY(h, who, hipGetLastError());
        GAMS_TRY(h, who, hipEventRecord(t1, h->compute));
        // the counter comes back through the handle's page-locked scratch word
        GAMS_TRY(h, who, hipMemcpyAsync(h->pin_scratch, d_n, sizeof(unsigned long long), hipMemcpyDeviceToHost, h->compute));
        GAMS_TRY(h, who, hipStreamSynchronize(h->compute));
        const unsigned long long nf = h->pin_scratch[0];
        if (nf > fcap) {                 // more flips than the list holds: grow once and rescan
            d_blk.reset();
            fcap = nf;
            continue;
        }
        flips.resize(nf);
        if (nf) GAMS_TRY(h, who, hipMemcpy(flips.data(), d_flips, nf * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        break;
    }
    std::sort(flips.begin(), flips.end());
    if (flips.size() % 2 != 0) return gams_fail(h, GAMS_EHIP, who + ": unpaired run boundary");
    for (size_t i = 0; i < flips.size(); i += 2)
        if ((flips[i] & 1ull) != 0 || (flips[i + 1] & 1ull) != 1)
            return gams_fail(h, GAMS_EHIP, who + ": run boundaries out of order");
    return GAMS_OK;
}

enum { GEN_H2D = 0, GEN_PACK, GEN_SCAN, GEN_TABLE, GEN_PLACE, GEN_STAGES };

}  // namespace

extern "C" int gams_gpu_valid_spans(gams_gpu_t *h, const uint8_t *seq, uint64_t len, int32_t fill, int32_t min_len,
                                    int32_t *span_lo, int32_t *span_hi, uint64_t cap, uint64_t *n_spans) {
    if (!h || !seq || !n_spans) return gams_fail(h, GAMS_EINVAL, "valid_spans: null argument");
    if (len == 0 || len > 0x7fffffffull) return gams_fail(h, GAMS_EINVAL, "valid_spans: length must be 1..2^31-1");
    GAMS_HIP(h, hipSetDevice(h->device));
    const uint64_t n_chunks = (len + 15) / 16;
    // device buffers from the handle's pool (one chromosome after another reuses them): the sequence, and
    // one block holding the flip counter (first 256 B) and the flip list behind it
    const std::string who = "valid_spans";
    PoolBlock d_seq(h, false), d_blk(h, false);
    GAMS_TRY(h, who, d_seq.alloc(n_chunks * 16 + 16));
    GAMS_TRY(h, who, hipMemsetAsync(d_seq.p + (n_chunks - 1) * 16, 0, 32, h->compute));
    GAMS_TRY(h, who, hipMemcpyAsync(d_seq.p, seq, len, hipMemcpyHostToDevice, h->compute));
    std::vector<unsigned long long> flips;
    h->k_valid = false;
    {
        const int rc = scan_flips(h, who, d_seq.p, len, d_blk, h->k0, h->k1, flips);
        if (rc != GAMS_OK) return rc;
    }
    h->k_valid = true;
    h->kq_used = 0;
    d_seq.reset();
    d_blk.reset();
    // valid spans, 1-based inclusive (gen.rs:100-102)
    std::vector<std::pair<int64_t, int64_t>> spans;
    for (size_t i = 0; i < flips.size(); i += 2) spans.emplace_back((int64_t)(flips[i] >> 1) + 1, (int64_t)(flips[i + 1] >> 1));
    uint64_t n = 0;
    for (auto &sp : fill_excise(spans, fill, min_len)) {
        if (span_lo && span_hi && n < cap) {
            span_lo[n] = (int32_t)sp.first;
            span_hi[n] = (int32_t)sp.second;
        }
        ++n;
    }
    *n_spans = n;
    return GAMS_OK;
}

// ---------------------------------------------------------------------------
// gen from the bytes of a FASTA file
// ---------------------------------------------------------------------------
extern "C" int gams_gpu_gen_text(gams_gpu_t *h, const char *bytes, uint64_t n_bytes, const gams_gen_params_t *params,
                                 gams_gen_t **out) {
    const std::string who = "gen_text";
    if (!h || !params || !out || (n_bytes && !bytes)) return gams_fail(h, GAMS_EINVAL, who + ": null argument");
    *out = nullptr;
    if (params->piece < 1 || params->fill < 1 || params->min_len < 1)
        return gams_fail(h, GAMS_EINVAL, who + ": piece, fill and min_len must be at least 1");
    if (n_bytes && bytes[0] != '>') return gams_fail(h, GAMS_EINVAL, who + ": expected '>' at the start of the first record");
    // (the block count is 32 bits, and every launch below stays inside the grid limit)
    if (n_bytes > (1ull << 40)) return gams_fail(h, GAMS_EUNSUPPORTED, who + ": more than 2^40 bytes (use the host path)");
    GAMS_HIP(h, hipSetDevice(h->device));
    struct Owner {   // the result until it is handed out
        gams_gpu_t *h;
        gams_gen_t *g;
        ~Owner() {
            if (g) gams_gen_destroy(h, g);
        }
    } own{h, new gams_gen_t()};
    gams_gen_t *const g = own.g;
    g->name_off.push_back(0);
    h->k_valid = false;
    h->kq_used = 0;
    hipStream_t st = h->compute;
    std::vector<unsigned long long> flips;
    std::vector<GenHdr> hdrs;
    unsigned long long total = 0;
    PoolBlock d_cat(h, false);
    if (n_bytes) GAMS_HIP(h, gams_stopwatch_reserve(h, GEN_STAGES));
    const StageClock stage{h, st};
    if (n_bytes) {
        // 1. the bytes, once; '\n' up to whole blocks and 64 B behind them, so that no kernel below guards a load
        const uint32_t nb = (uint32_t)((n_bytes + kGenBlk - 1) / kGenBlk);
        const uint64_t n_pad = (uint64_t)nb * kGenBlk + 64u;
        PoolBlock d_in(h, false), s0(h, false), d_hdr(h, false), d_flip(h, false);
        GAMS_TRY(h, who, d_in.alloc(n_pad));
        GAMS_TRY(h, who, stage(GEN_H2D, true));
        GAMS_TRY(h, who, hipMemsetAsync(d_in.p + n_bytes, '\n', n_pad - n_bytes, st));
        for (uint64_t o = 0; o < n_bytes; o += 1ull << 28) {
            const size_t n = (size_t)std::min<uint64_t>(1ull << 28, n_bytes - o);
            GAMS_TRY(h, who, hipMemcpyAsync(d_in.p + o, bytes + o, n, hipMemcpyHostToDevice, st));
        }
        GAMS_TRY(h, who, stage(GEN_H2D, false));
        // 2. mark, carry, count, offsets
        unsigned long long *d_words = nullptr, *d_payoff = nullptr, *d_hdroff = nullptr;
        uint32_t *d_code = nullptr, *d_bin = nullptr, *d_bpay = nullptr, *d_bhdr = nullptr;
        auto small = [&](Carver &c) {
            d_words = c.take<unsigned long long>(GW_COUNT);
            d_code = c.take<uint32_t>(nb);
            d_bin = c.take<uint32_t>(nb);
            d_bpay = c.take<uint32_t>(nb);
            d_bhdr = c.take<uint32_t>(nb);
            d_payoff = c.take<unsigned long long>((size_t)nb + 1);
            d_hdroff = c.take<unsigned long long>((size_t)nb + 1);
        };
        GAMS_TRY(h, who, s0.alloc(layout_bytes(small)));
        carve(s0.p, small);
        GAMS_TRY(h, who, stage(GEN_PACK, true));
        GAMS_TRY(h, who, hipMemsetAsync(d_words, 0, GW_COUNT * 8, st));
        hipLaunchKernelGGL(gen_mark_kernel, dim3(nb), dim3(256), 0, st, d_in.p, d_code, d_words);
        hipLaunchKernelGGL(gen_carry_kernel, dim3(1), dim3(256), 0, st, d_code, nb, d_bin);
        GenPack pk{};
        pk.in = d_in.p;
        pk.blk_in = d_bin;
        pk.blk_pay = d_bpay;
        pk.blk_hdr = d_bhdr;
        pk.pay_off = d_payoff;
        pk.hdr_off = d_hdroff;
        pk.words = d_words;
        hipLaunchKernelGGL(gen_pack_kernel<false>, dim3(nb), dim3(256), 0, st, pk);
        hipLaunchKernelGGL(blk_offsets_scan_kernel<uint32_t>, dim3(1), dim3(1024), 0, st, d_bpay, nb, d_payoff, d_words,
                           (uint32_t)GW_PAY);
        hipLaunchKernelGGL(blk_offsets_scan_kernel<uint32_t>, dim3(1), dim3(1024), 0, st, d_bhdr, nb, d_hdroff, d_words,
                           (uint32_t)GW_HDR);
        GAMS_TRY(h, who, hipGetLastError());
        GAMS_TRY(h, who, hipMemcpyAsync(h->pin_scratch, d_words, GW_COUNT * 8, hipMemcpyDeviceToHost, st));
        GAMS_TRY(h, who, hipStreamSynchronize(st));
        if (h->pin_scratch[GW_BAD])
            return gams_fail(h, GAMS_EUNSUPPORTED, who + ": the input holds a byte >= 0x80 or a NUL (use the host path)");
        if (h->pin_scratch[GW_WS])
            return gams_fail(h, GAMS_EUNSUPPORTED, who + ": white space inside a sequence line (use the host path)");
        total = h->pin_scratch[GW_PAY];
        const unsigned long long n_hdr = h->pin_scratch[GW_HDR];
        // 3. compact: the base stream (16-B units, 64 B of slack for the loads of scan and place) and the header list
        GAMS_TRY(h, who, d_cat.alloc(((total + 15u) & ~15ull) + 64u));
        GAMS_TRY(h, who, d_hdr.alloc(std::max<unsigned long long>(n_hdr, 1) * sizeof(GenHdr)));
        pk.cat = d_cat.p;
        pk.hdrs = reinterpret_cast<GenHdr *>(d_hdr.p);
        hipLaunchKernelGGL(gen_pack_kernel<true>, dim3(nb), dim3(256), 0, st, pk);
        GAMS_TRY(h, who, hipGetLastError());
        GAMS_TRY(h, who, stage(GEN_PACK, false));
        hdrs.resize(n_hdr);
        if (n_hdr) GAMS_TRY(h, who, hipMemcpyAsync(hdrs.data(), d_hdr.p, n_hdr * sizeof(GenHdr), hipMemcpyDeviceToHost, st));
        // 4. scan: one pass over the whole stream; this is the host's wait in the middle
        if (total) {
            const int rc = scan_flips(h, who, d_cat.p, total, d_flip, h->kq[GEN_SCAN].first, h->kq[GEN_SCAN].second, flips);
            if (rc != GAMS_OK) return rc;
        } else {
            GAMS_TRY(h, who, stage(GEN_SCAN, true));
            GAMS_TRY(h, who, stage(GEN_SCAN, false));
            GAMS_TRY(h, who, hipStreamSynchronize(st));
        }
        GAMS_TRY(h, who, stage(GEN_TABLE, true));
        // (the input, the small arrays, the header list and the flips go back to the pool here)
    }
    // 5. table: ids from the host's bytes, chromosomes from the header list, runs cut at their boundaries
    const size_t n_chr = hdrs.size();
    {
        std::unordered_set<std::string> seen;
        for (size_t i = 0; i < n_chr; ++i) {
            uint64_t p = hdrs[i].pos + 1, e = p;
            while (e < n_bytes && !gams_fasta_space((uint8_t)bytes[e])) ++e;
            if (e == p) return gams_fail(h, GAMS_EUNSUPPORTED, who + ": a record with an empty id (use the host path)");
            std::string id(bytes + p, bytes + e);
            if (!seen.insert(id).second)
                return gams_fail(h, GAMS_EUNSUPPORTED, who + ": duplicate id " + id + " (use the host path)");
            g->names += id;
            g->name_off.push_back(g->names.size());
            const unsigned long long len = (i + 1 < n_chr ? hdrs[i + 1].pay : total) - hdrs[i].pay;
            if (len > 0x7fffffffull)
                return gams_fail(h, GAMS_EUNSUPPORTED, who + ": " + id + " has more than 2^31 - 1 bases (use the host path)");
            g->chr_len.push_back((uint32_t)len);
        }
    }
    std::vector<unsigned long long> src;   // of ctg k: its first base in the stream
    {
        std::vector<std::pair<int64_t, int64_t>> spans;   // of the chromosome at hand, 1-based inclusive
        size_t c = 0, f = 0;
        auto finish = [&](size_t chr) {                   // fill, excise, --piece (gen.rs:103-126)
            uint32_t serial = 0;
            for (auto &sp : fill_excise(spans, params->fill, params->min_len)) {
                gams_piece_split(sp.first, sp.second, params->piece, [&](int64_t lo, int64_t hi) {
                    g->ctgs.push_back(gams_gen_ctg_t{(uint32_t)chr, ++serial, (int32_t)lo, (int32_t)hi});
                    src.push_back(hdrs[chr].pay + (unsigned long long)(lo - 1));
                });
            }
            spans.clear();
        };
        for (; c < n_chr; ++c) {
            const unsigned long long lo = hdrs[c].pay, hi = lo + g->chr_len[c];
            // the runs that begin in front of this chromosome's end (a run that crosses it is cut, and its rest comes
            // again for the next chromosome)
            while (f < flips.size() && (flips[f] >> 1) < hi) {
                const unsigned long long s = std::max<unsigned long long>(flips[f] >> 1, lo);
                const unsigned long long e = std::min<unsigned long long>(flips[f + 1] >> 1, hi);   // exclusive
                if (e > s) spans.emplace_back((int64_t)(s - lo) + 1, (int64_t)(e - lo));
                if ((flips[f + 1] >> 1) > hi) break;   // the run goes on in the next chromosome
                f += 2;
            }
            finish(c);
        }
    }
    if (g->ctgs.size() > 0xffffffffull) return gams_fail(h, GAMS_EUNSUPPORTED, who + ": more than 2^32 - 1 ctgs");
    const uint32_t n_ctg = (uint32_t)g->ctgs.size();
    std::vector<uint32_t> len(n_ctg);
    for (uint32_t k = 0; k < n_ctg; ++k) len[k] = (uint32_t)(g->ctgs[k].chr_end - g->ctgs[k].chr_start + 1);
    // 6. place: the seqset of the ctgs, bytes and plane, from the stream
    {
        const int rc = gams_seqset_create(h, n_ctg, len.data(), &g->set);
        if (rc != GAMS_OK) return rc;
    }
    if (n_bytes) GAMS_TRY(h, who, stage(GEN_TABLE, false));
    if (n_ctg) {
        gams_seqset_t *const s = g->set;
        std::vector<unsigned long long> chunk_off((size_t)n_ctg + 1);
        chunk_off[0] = 0;
        for (uint32_t k = 0; k < n_ctg; ++k) chunk_off[k + 1] = chunk_off[k] + (len[k] + 15ull) / 16ull;
        PoolBlock d_tab(h, false);
        GenPlace pa{};
        unsigned long long *d_chunk = nullptr, *d_src = nullptr, *d_dst = nullptr;
        uint32_t *d_len = nullptr;
        auto tab = [&](Carver &c) {
            d_chunk = c.take<unsigned long long>((size_t)n_ctg + 1);
            d_src = c.take<unsigned long long>(n_ctg);
            d_dst = c.take<unsigned long long>(n_ctg);
            d_len = c.take<uint32_t>(n_ctg);
        };
        GAMS_TRY(h, who, d_tab.alloc(layout_bytes(tab)));
        carve(d_tab.p, tab);
        {
            // the zeroing of the new buffers, on the copy stream.  (The gate bumps the reader epoch although nothing reads
            // here: harmless, the next burst of gams_seqset_upload_ranges calls orders itself once more.)
            const int rc = gams_seqset_read_begin(h, s);
            if (rc != GAMS_OK) return rc;
        }
        GAMS_TRY(h, who, stage(GEN_PLACE, true));
        GAMS_TRY(h, who, hipMemcpyAsync(d_chunk, chunk_off.data(), ((size_t)n_ctg + 1) * 8, hipMemcpyHostToDevice, st));
        GAMS_TRY(h, who, hipMemcpyAsync(d_src, src.data(), (size_t)n_ctg * 8, hipMemcpyHostToDevice, st));
        GAMS_TRY(h, who, hipMemcpyAsync(d_dst, s->off.data(), (size_t)n_ctg * 8, hipMemcpyHostToDevice, st));
        GAMS_TRY(h, who, hipMemcpyAsync(d_len, len.data(), (size_t)n_ctg * 4, hipMemcpyHostToDevice, st));
        pa.cat = d_cat.p;
        pa.seq = s->d_seq;
        pa.plane = s->d_plane;
        pa.chunk_off = d_chunk;
        pa.src = d_src;
        pa.dst = d_dst;
        pa.len = d_len;
        pa.n_ctg = n_ctg;
        pa.n_chunks = chunk_off[n_ctg];
        hipLaunchKernelGGL(gen_place_kernel, dim3((unsigned)((pa.n_chunks + 255) / 256)), dim3(256), 0, st, pa);
        GAMS_TRY(h, who, hipGetLastError());
        GAMS_TRY(h, who, stage(GEN_PLACE, false));
        // readers on any stream order themselves behind the kernel as behind an upload (the seqset protocol, common.hpp:
        // nothing but the zeroing awaited above was queued on the new buffers, so there was no write_begin to make) ...
        if (!s->uploaded) GAMS_TRY(h, who, hipEventCreateWithFlags(&s->uploaded, hipEventDisableTiming));
        {
            const int rc = gams_seqset_write_end(h, s, st);
            if (rc != GAMS_OK) return rc;
        }
        // ... and an upload behind it as behind a reader: the kernel ran on the compute stream, so the epoch moves on
        // and the next gams_seqset_upload_ranges does not take itself for ordered already
        h->reader_epoch.fetch_add(1, std::memory_order_relaxed);
        GAMS_TRY(h, who, hipStreamSynchronize(st));   // the tables above are the call's
    } else if (n_bytes) {
        GAMS_TRY(h, who, stage(GEN_PLACE, true));
        GAMS_TRY(h, who, stage(GEN_PLACE, false));
    }
    if (n_bytes) {
        h->kq_used = GEN_STAGES;
        h->kq_staged = true;
        h->k_valid = true;
    }
    *out = g;
    own.g = nullptr;
    return GAMS_OK;
}

extern "C" int gams_gen_counts(gams_gpu_t *h, const gams_gen_t *g, uint32_t *n_chr, uint32_t *n_ctg, uint64_t *name_bytes) {
    if (!g) return gams_fail(h, GAMS_EINVAL, "gen_counts: null argument");
    if (n_chr) *n_chr = (uint32_t)g->chr_len.size();
    if (n_ctg) *n_ctg = (uint32_t)g->ctgs.size();
    if (name_bytes) *name_bytes = g->names.size();
    return GAMS_OK;
}

extern "C" int gams_gen_chrs(gams_gpu_t *h, const gams_gen_t *g, char *names, uint64_t *name_off, uint32_t *chr_len) {
    if (!g) return gams_fail(h, GAMS_EINVAL, "gen_chrs: null argument");
    if (names) std::memcpy(names, g->names.data(), g->names.size());
    if (name_off) std::copy(g->name_off.begin(), g->name_off.end(), name_off);
    if (chr_len) std::copy(g->chr_len.begin(), g->chr_len.end(), chr_len);
    return GAMS_OK;
}

extern "C" int gams_gen_ctgs(gams_gpu_t *h, const gams_gen_t *g, gams_gen_ctg_t *ctgs) {
    if (!g || (!ctgs && !g->ctgs.empty())) return gams_fail(h, GAMS_EINVAL, "gen_ctgs: null argument");
    std::copy(g->ctgs.begin(), g->ctgs.end(), ctgs);
    return GAMS_OK;
}

extern "C" int gams_gen_seqset(gams_gpu_t *h, gams_gen_t *g, gams_seqset_t **s) {
    if (!g || !s) return gams_fail(h, GAMS_EINVAL, "gen_seqset: null argument");
    if (g->taken) return gams_fail(h, GAMS_ESTATE, "gen_seqset: the seqset was handed out already");
    *s = g->set;
    g->set = nullptr;
    g->taken = true;
    return GAMS_OK;
}

extern "C" void gams_gen_destroy(gams_gpu_t *h, gams_gen_t *g) {
    if (!g) return;
    if (g->set) gams_seqset_destroy(h, g->set);
    delete g;
}
