// runlist.hip -- the bytes of a runlist JSON file (the set `anno` loads first, anno.rs:84-87: intspan::read_json +
// json2set) to a resident span set, built on the device.
//
//   gams_spans_create_runlist_text   {"chr": "runlist", ...}  ->  gams_spans_t + the chr name table, groups in file order
//   gams_spans_read                  a set back as arrays (group_off, lo, hi)
//
// The file is a flat object of string values.  Everything the kernels do not cover is refused with GAMS_EUNSUPPORTED
// (escapes, bytes >= 0x80, anything but strings as values, white space inside a runlist, negative numbers, a
// duplicate key): the host reader (gams::read_runlist_json) is the judge of what is invalid.
//
// Pipeline (one handle, the compute stream; every workgroup of the text passes takes 16 KiB, a lane 64 B as four 16-B loads):
//   1. mark    the '"' bytes of every block and the refused bytes; a one-workgroup prefix over the blocks.  With no
//              escape in the file a byte is inside a string iff an odd number of quotes precede it, and the string's
//              ordinal is half that number: even ordinals are keys, odd ones values.
//   2. count   with the quotes in front of every lane known: the position of every quote (the keys for the host), the
//              structural bytes outside strings checked against the one their gap may hold and counted per gap, the
//              bytes of the values checked, and the token starts (a value byte behind the opening quote or a ',')
//              counted per lane and per block; a one-workgroup prefix over the blocks.
//   3. parse   the lanes that start tokens parse `a` or `a-b` and store (group << 32 | lo, hi) at the token's number.
//   4. normalise (IntSpan::add_runlist)  a test whether every token already begins beyond its predecessor's end + 1
//              inside its group; if not: a radix sort of the packed keys, the running maximum of (group, hi) -- a
//              segmented running maximum of hi, because the group is the high half and never falls --, run heads where
//              lo > runmax[i - 1] + 1 or the group changes, a prefix sum over the heads, and the compaction: a run's
//              hi is the running maximum at its last token.
//   5. build   the group offsets by a search per group, the 64-bit prefix of the span lengths (cum = that prefix minus
//              its value at the group's first span), the records, the directory headers by build_dir's rule
//              (dir_params), a search per directory slot, and span_cell_kernel of interval.hip.
// Host waits: the quote count, the token count (with the quote positions), the parse flags and the order test, the
// span count after a sort, the end.

#include "interval_kernels.hpp"
#include "text_emit.hpp"

#include <rocprim/rocprim.hpp>

#include <algorithm>
#include <string>
#include <unordered_set>
#include <vector>

namespace {

enum : uint32_t {
    RW_QUOTES = 0,   // '"' bytes of the input
    RW_BAD = 1,      // a byte >= 0x80, a NUL or a backslash
    RW_STRUCT = 2,   // a byte outside the strings that its gap may not hold
    RW_VALUE = 3,    // a byte inside a value that is no digit, '-' or ',', or a ',' in front of the closing quote
    RW_TOKENS = 4,   // tokens
    RW_PARSE = 5,    // a token that is not `a` or `a-b` with 1-10 digits each, a <= b <= INT32_MAX
    RW_UNSORTED = 6, // a token that does not begin beyond its predecessor's end + 1
    RW_SPANS = 7,    // spans after the join
    RW_COUNT = 8
};

enum : int { RL_UPLOAD = 0, RL_MARK, RL_COUNT, RL_PARSE, RL_NORMALISE, RL_BUILD, RL_STAGES };

constexpr uint32_t kBlkBytes = 256u * 64u;   // bytes per workgroup of the text passes

__device__ __forceinline__ uint32_t quote_mask(uint32_t w) { return zero_bytes(w ^ 0x22222222u); }
__device__ __forceinline__ uint32_t refused_mask(uint32_t w) {
    return (w & 0x80808080u) | zero_bytes(w) | zero_bytes(w ^ 0x5c5c5c5cu);
}
__device__ __forceinline__ uint32_t quotes16(const uint4 v) {
    return __popc(quote_mask(v.x)) + __popc(quote_mask(v.y)) + __popc(quote_mask(v.z)) + __popc(quote_mask(v.w));
}
__device__ __forceinline__ bool is_json_ws(uint32_t c) { return c == ' ' || c == '\t' || c == '\n' || c == '\r'; }

// the 64 bytes of a lane at p0 (spaces beyond n16) and their quotes
__device__ __forceinline__ uint32_t rl_load64(const uint8_t *in, uint64_t p0, uint64_t n16, uint4 (&v)[4]) {
    uint32_t c = 0;
#pragma unroll
    for (uint32_t u = 0; u < 4u; ++u) {
        const uint64_t p = p0 + 16u * u;
        v[u] = p < n16 ? *reinterpret_cast<const uint4 *>(in + p) : make_uint4(0x20202020u, 0x20202020u, 0x20202020u, 0x20202020u);
        c += quotes16(v[u]);
    }
    return c;
}

// f(position, byte, quotes in front of it, the byte in front of it) for the 64 bytes of a lane, in order
template <typename F>
__device__ __forceinline__ void rl_walk64(const uint4 (&v)[4], uint64_t p0, uint64_t q, uint32_t prev, F &&f) {
#pragma unroll
    for (uint32_t u = 0; u < 4u; ++u) {
        const uint32_t w4[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
#pragma unroll
        for (uint32_t k = 0; k < 4u; ++k) {
#pragma unroll
            for (uint32_t b = 0; b < 4u; ++b) {
                const uint32_t c = (w4[k] >> (8u * b)) & 0xffu;
                f(p0 + 16u * u + 4u * k + b, c, q, prev);
                q += c == '"' ? 1u : 0u;
                prev = c;
            }
        }
    }
}

// 1. quotes per block, and the flag of refused bytes.  n16: the input rounded up to 16 B (the padding holds spaces)
__global__ __launch_bounds__(256) void rl_mark_kernel(const uint8_t *in, uint64_t n16, uint32_t *blk_q,
                                                      unsigned long long *words) {
    __shared__ uint32_t ws[4];
    const uint64_t p0 = ((uint64_t)blockIdx.x * 256u + threadIdx.x) * 64u;
    uint32_t c = 0, bad = 0;
#pragma unroll
    for (uint32_t u = 0; u < 4u; ++u) {
        const uint64_t p = p0 + 16u * u;
        if (p >= n16) break;
        const uint4 v = *reinterpret_cast<const uint4 *>(in + p);
        c += quotes16(v);
        bad |= refused_mask(v.x) | refused_mask(v.y) | refused_mask(v.z) | refused_mask(v.w);
    }
    if (bad) words[RW_BAD] = 1ull;
    const uint32_t tot = block_sum_256(c, ws);
    if (threadIdx.x == 0) blk_q[blockIdx.x] = tot;
}

struct RlText {
    const uint8_t *in;
    uint64_t n16;
    uint64_t nq;                           // quotes of the input (even, and a multiple of four)
    const unsigned long long *blk_qoff;    // quotes in front of every block
    unsigned long long *qpos;              // nq: the position of every quote
    uint32_t *gap;                         // nq / 2 + 1: structural bytes between string k - 1 and string k
    uint8_t *lane_tok;                     // token starts of every lane
    uint32_t *blk_tok;                     // ... of every block
    const unsigned long long *blk_tokoff;  // tokens in front of every block
    unsigned long long *key;               // per token: group << 32 | lo
    uint32_t *hi;
    uint64_t n_tok;                        // tokens of the input (the size of key / hi)
    unsigned long long *words;
};

// a value byte behind the opening quote or a ',' starts a token; the value "-" is the empty set
__device__ __forceinline__ bool rl_token_start(const uint8_t *in, uint64_t pos, uint32_t c, uint32_t prev) {
    if (prev != '"' && prev != ',') return false;
    return !(c == '-' && prev == '"' && in[pos + 1u] == '"');
}

// 2. the quote positions, the structure outside the strings, the bytes of the values, the token starts
__global__ __launch_bounds__(256) void rl_count_kernel(const RlText a) {
    __shared__ uint32_t ws[4];
    const uint64_t lane = (uint64_t)blockIdx.x * 256u + threadIdx.x, p0 = lane * 64u;
    uint4 v[4];
    const uint32_t c = rl_load64(a.in, p0, a.n16, v);
    uint32_t tot;
    const uint32_t rel = block_excl_scan_256<uint32_t>(c, ws, tot);
    const uint32_t prev0 = p0 > 0 && p0 <= a.n16 ? a.in[p0 - 1u] : (uint32_t)' ';
    uint32_t ntok = 0, bad_struct = 0, bad_value = 0;
    rl_walk64(v, p0, a.blk_qoff[blockIdx.x] + rel, prev0, [&](uint64_t pos, uint32_t ch, uint64_t q, uint32_t prev) {
        if (ch == '"') {
            if (q < a.nq) a.qpos[q] = pos;
        } else if (q & 1u) {
            if (!((q >> 1) & 1u)) {                                 // inside a key: a control character is the host's to judge
                bad_struct |= ch < 0x20u ? 1u : 0u;
            } else {                                                // inside a value
                if (ch == ',')
                    bad_value |= a.in[pos + 1u] == '"' ? 1u : 0u;   // an empty token at the end
                else if (ch != '-' && !is_digit_c((char)ch))
                    bad_value = 1u;
                ntok += rl_token_start(a.in, pos, ch, prev) ? 1u : 0u;
            }
        } else if (!is_json_ws(ch)) {                               // outside: '{', then ':' and ',' in turn, then '}'
            const uint32_t want = q == 0 ? '{' : q == a.nq ? '}' : (((q >> 1) - 1u) & 1u) ? ',' : ':';
            bad_struct |= ch != want ? 1u : 0u;
            if (q <= a.nq) atomicAdd(a.gap + (q >> 1), 1u);
        }
    });
    if (bad_struct) a.words[RW_STRUCT] = 1ull;
    if (bad_value) a.words[RW_VALUE] = 1ull;
    a.lane_tok[lane] = (uint8_t)ntok;
    __syncthreads();                                                // (ws of the scan above is read by every wave first)
    const uint32_t btok = block_sum_256(ntok, ws);
    if (threadIdx.x == 0) a.blk_tok[blockIdx.x] = btok;
}

// 3. one token: `a` or `a-b`, 1-10 digits each, ended by ',' or the closing quote
__device__ __forceinline__ bool rl_parse_token(const uint8_t *in, uint64_t pos, uint64_t end, uint32_t &lo, uint32_t &hi) {
    const char *s = reinterpret_cast<const char *>(in);
    uint64_t p = pos;
    lo = digits(s, p, end);
    bool ok = p > pos && p - pos <= 10u && lo != 0x80000000u;
    hi = lo;
    if (s[p] == '-') {
        const uint64_t b = ++p;
        hi = digits(s, p, end);
        ok = ok && p > b && p - b <= 10u && hi != 0x80000000u;
    }
    return ok && (s[p] == ',' || s[p] == '"') && lo <= hi;
}

__global__ __launch_bounds__(256) void rl_parse_kernel(const RlText a) {
    __shared__ uint32_t wq[4], wt[4];
    const uint64_t lane = (uint64_t)blockIdx.x * 256u + threadIdx.x, p0 = lane * 64u;
    uint4 v[4];
    const uint32_t c = rl_load64(a.in, p0, a.n16, v);
    const uint32_t mine = a.lane_tok[lane];
    uint32_t tot;
    const uint32_t rel = block_excl_scan_256<uint32_t>(c, wq, tot);
    const uint32_t trel = block_excl_scan_256<uint32_t>(mine, wt, tot);
    if (mine == 0u) return;
    const uint32_t prev0 = p0 > 0 && p0 <= a.n16 ? a.in[p0 - 1u] : (uint32_t)' ';
    // the lane's token starts and quotes as bit masks over its 64 bytes, then one parse per start
    const uint64_t q0 = a.blk_qoff[blockIdx.x] + rel;
    uint64_t starts = 0, quotes = 0;
    rl_walk64(v, p0, q0, prev0, [&](uint64_t pos, uint32_t ch, uint64_t q, uint32_t prev) {
        const uint64_t bit = 1ull << (pos - p0);
        if (ch == '"')
            quotes |= bit;
        else if ((q & 1u) && ((q >> 1) & 1u) && rl_token_start(a.in, pos, ch, prev))
            starts |= bit;
    });
    uint64_t t = a.blk_tokoff[blockIdx.x] + trel;
    uint32_t bad = 0;
    while (starts) {
        const uint32_t k = (uint32_t)__builtin_ctzll(starts);
        starts &= starts - 1u;
        const uint64_t q = q0 + (uint64_t)__popcll(quotes & ((1ull << k) - 1u));
        uint32_t lo, hi;
        if (!rl_parse_token(a.in, p0 + k, a.n16 + 16u, lo, hi)) {
            bad = 1u;
            lo = hi = 0u;
        }
        if (t < a.n_tok) {
            a.key[t] = ((unsigned long long)(q >> 2) << 32) | lo;  // the value's ordinal >> 1 = its group
            a.hi[t] = hi;
        }
        ++t;
    }
    if (bad) a.words[RW_PARSE] = 1ull;
}

// 4. is every group a normalised runlist already (lo[i] > hi[i - 1] + 1)?
__global__ __launch_bounds__(256) void rl_sorted_kernel(const unsigned long long *key, const uint32_t *hi, uint64_t n,
                                                        unsigned long long *words) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i == 0 || i >= n) return;
    const unsigned long long k = key[i], kp = key[i - 1u];
    if ((k >> 32) == (kp >> 32) && (uint64_t)(uint32_t)k <= (uint64_t)hi[i - 1u] + 1u) words[RW_UNSORTED] = 1ull;
}

// (group, hi) of the sorted tokens: its running maximum is the running maximum of hi inside the group
__global__ __launch_bounds__(256) void rl_pack_hi_kernel(const unsigned long long *key, const uint32_t *hi, uint64_t n,
                                                         unsigned long long *packed) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    packed[i] = (key[i] & 0xffffffff00000000ull) | hi[i];
}

// run heads: the group changes, or the token begins beyond everything in front of it in its group
__global__ __launch_bounds__(256) void rl_heads_kernel(const unsigned long long *key, const unsigned long long *runmax,
                                                       uint64_t n, uint32_t *head) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    uint32_t hd = 1u;
    if (i) {
        const unsigned long long k = key[i], m = runmax[i - 1u];
        hd = (k >> 32) != (m >> 32) || (uint64_t)(uint32_t)k > (uint64_t)(uint32_t)m + 1u ? 1u : 0u;
    }
    head[i] = hd;
}

// the joined spans: a head gives (group, lo), the last token of a run its hi (the running maximum there)
__global__ __launch_bounds__(256) void rl_join_kernel(const unsigned long long *key, const unsigned long long *runmax,
                                                      const uint32_t *head, const uint32_t *hidx, uint64_t n,
                                                      unsigned long long *out_key, uint32_t *out_hi,
                                                      unsigned long long *words) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint32_t hd = head[i], run = hidx[i] + hd - 1u;      // hidx: heads in front of i
    if (hd) out_key[run] = key[i];
    if (i + 1u == n || head[i + 1u]) out_hi[run] = (uint32_t)runmax[i];
    if (i + 1u == n) words[RW_SPANS] = (unsigned long long)run + 1ull;
}

// 5. group_off[g] = spans of the groups in front of g (a lower bound over the group halves), group_off[n_groups] = m
__global__ __launch_bounds__(256) void rl_group_off_kernel(const unsigned long long *key, uint64_t m, uint32_t n_groups,
                                                           unsigned long long *goff) {
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    if (g > n_groups) return;
    uint64_t a = 0, z = m;
    while (a < z) {
        const uint64_t mid = a + ((z - a) >> 1);
        if ((key[mid] >> 32) < g)
            a = mid + 1u;
        else
            z = mid;
    }
    goff[g] = g == n_groups ? m : a;
}

__global__ __launch_bounds__(256) void rl_len_kernel(const unsigned long long *key, const uint32_t *hi, uint64_t m,
                                                     unsigned long long *len) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= m) return;
    len[i] = (unsigned long long)hi[i] - (uint32_t)key[i] + 1ull;
}

__global__ __launch_bounds__(256) void rl_rec_kernel(const unsigned long long *key, const uint32_t *hi, uint64_t m,
                                                     const unsigned long long *gcum, const unsigned long long *goff,
                                                     SpanRec *rec) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= m) return;
    const unsigned long long k = key[i];
    rec[i] = SpanRec{(int32_t)(uint32_t)k, (int32_t)hi[i], gcum[i] - gcum[goff[k >> 32]]};
}

__global__ __launch_bounds__(256) void rl_groups_kernel(const unsigned long long *key, const unsigned long long *goff,
                                                        uint32_t n_groups, SpanGroup *groups) {
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    if (g >= n_groups) return;
    const uint64_t off = goff[g];
    const uint32_t n = (uint32_t)(goff[g + 1u] - off);
    SpanGroup G;
    G.off = off;
    G.n = n;
    G.pad = 0u;
    G.lo = n ? dir_params((uint32_t)key[off] ^ 0x80000000u, (uint32_t)key[off + n - 1u] ^ 0x80000000u, n)
             : KeyDir{0u, 0u, 0u, 0u};
    groups[g] = G;
}

// slot j of the directory belongs to the group g with off[g] + g <= j, its bucket b = j - off[g] - g:
// dir[b] = spans with biased lo < key0 + (b << shift), dir[nb] = n (build_dir)
__global__ __launch_bounds__(256) void rl_dir_kernel(const SpanGroup *groups, uint32_t n_groups, const SpanRec *rec,
                                                     uint64_t slots, uint32_t *dir) {
    const uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (j >= slots) return;
    uint32_t lo = 0, hi = n_groups;
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (groups[mid].off + mid <= j)
            lo = mid;
        else
            hi = mid;
    }
    const SpanGroup G = groups[lo];
    const uint64_t b = j - (G.off + lo);
    if (b > G.lo.nb || b > G.n) return;                 // (the slots behind a group's nb + 1 entries stay 0)
    uint32_t r = G.n;
    if (b < G.lo.nb) {
        const uint64_t edge = (uint64_t)G.lo.key0 + (b << G.lo.shift);
        uint32_t a = 0, z = G.n;
        while (a < z) {
            const uint32_t mid = a + ((z - a) >> 1);
            if ((uint64_t)((uint32_t)rec[G.off + mid].lo ^ 0x80000000u) < edge)
                a = mid + 1u;
            else
                z = mid;
        }
        r = a;
    }
    dir[j] = r;
}

unsigned blocks256(uint64_t n) { return (unsigned)std::max<uint64_t>(1, (n + 255u) / 256u); }

int runlist_run(gams_gpu_t *h, const char *bytes, uint64_t n_bytes, gams_spans_t **sp_out, gams_names_t **names_out,
                uint32_t *n_groups_out, uint64_t *n_spans_out) {
    const std::string who = "spans_create_runlist_text";
    auto refuse = [&](const char *what) { return gams_fail(h, GAMS_EUNSUPPORTED, who + ": " + what + " (use the host reader)"); };
    if (n_bytes > (1ull << 44)) return refuse("more than 2^44 bytes");
    GAMS_HIP(h, hipSetDevice(h->device));
    hipStream_t st = h->compute;
    const uint64_t n16 = (n_bytes + 15u) & ~15ull, n_pad = n16 + 16u;   // a token is looked at up to 22 bytes past its start
    const uint32_t nbi = (uint32_t)std::max<uint64_t>(1, (n16 + kBlkBytes - 1) / kBlkBytes);
    const uint64_t lanes = (uint64_t)nbi * 256u;
    uint8_t *d_in = nullptr;
    GAMS_TRY(h, who, gams_text_input(h, n_pad, &d_in));
    GAMS_HIP(h, gams_stopwatch_reserve(h, RL_STAGES));
    const StageClock stage{h, st};
    h->k_valid = false;
    h->kq_used = 0;

    // ---- upload, 1. mark
    unsigned long long *d_words = nullptr, *d_bqoff = nullptr, *d_btoff = nullptr;
    uint32_t *d_bq = nullptr, *d_bt = nullptr;
    uint8_t *d_ltok = nullptr;
    PoolBlock s0(h, false);
    auto front = [&](Carver &c) {
        d_words = c.take<unsigned long long>(RW_COUNT);
        d_bq = c.take<uint32_t>(nbi);
        d_bqoff = c.take<unsigned long long>((size_t)nbi + 1);
        d_bt = c.take<uint32_t>(nbi);
        d_btoff = c.take<unsigned long long>((size_t)nbi + 1);
        d_ltok = c.take<uint8_t>(lanes);
    };
    GAMS_TRY(h, who, s0.alloc(layout_bytes(front)));
    carve(s0.p, front);
    GAMS_TRY(h, who, hipEventRecord(h->k0, st));
    GAMS_TRY(h, who, stage(RL_UPLOAD, true));
    GAMS_TRY(h, who, hipMemsetAsync(d_words, 0, RW_COUNT * 8, st));
    if (n_bytes) GAMS_TRY(h, who, hipMemcpyAsync(d_in, bytes, n_bytes, hipMemcpyHostToDevice, st));
    GAMS_TRY(h, who, hipMemsetAsync(d_in + n_bytes, ' ', n_pad - n_bytes, st));
    GAMS_TRY(h, who, stage(RL_UPLOAD, false));
    GAMS_TRY(h, who, stage(RL_MARK, true));
    hipLaunchKernelGGL(rl_mark_kernel, dim3(nbi), dim3(256), 0, st, d_in, n16, d_bq, d_words);
    hipLaunchKernelGGL(blk_offsets_scan_kernel<uint32_t>, dim3(1), dim3(1024), 0, st, d_bq, nbi, d_bqoff, d_words, (uint32_t)RW_QUOTES);
    GAMS_TRY(h, who, hipGetLastError());
    GAMS_TRY(h, who, stage(RL_MARK, false));
    auto read_words = [&]() -> hipError_t {
        hipError_t e = hipMemcpyAsync(h->pin_scratch, d_words, RW_COUNT * 8, hipMemcpyDeviceToHost, st);
        return e == hipSuccess ? hipStreamSynchronize(st) : e;
    };
    GAMS_TRY(h, who, read_words());
    if (h->pin_scratch[RW_BAD]) return refuse("the input holds a byte >= 0x80, a NUL or a backslash");
    const uint64_t nq = h->pin_scratch[RW_QUOTES];
    if (nq & 3u) return refuse("the strings do not pair up as keys and values");
    if (nq / 4u > 0x7fffffffull) return refuse("more than 2^31 - 1 keys");
    const uint32_t n_groups = (uint32_t)(nq / 4u);
    if (nq == 0) {           // no string at all: "{}" between white space is the set with no group
        uint64_t open = 0, close = 0;
        for (uint64_t i = 0; i < n_bytes; ++i) {
            const char c = bytes[i];
            if (c == ' ' || c == '\t' || c == '\n' || c == '\r') continue;
            if (c == '{' && !open && !close)
                ++open;
            else if (c == '}' && open == 1 && !close)
                ++close;
            else
                return refuse("not an object of string values");
        }
        if (!open || !close) return refuse("not an object of string values");
    }

    // ---- 2. count
    unsigned long long *d_qpos = nullptr;
    uint32_t *d_gap = nullptr;
    PoolBlock s1(h, false);
    auto marks = [&](Carver &c) {
        d_qpos = c.take<unsigned long long>(std::max<uint64_t>(nq, 1));
        d_gap = c.take<uint32_t>(nq / 2u + 1u);
    };
    RlText T{};
    T.in = d_in;
    T.n16 = n16;
    T.nq = nq;
    T.blk_qoff = d_bqoff;
    T.lane_tok = d_ltok;
    T.blk_tok = d_bt;
    T.blk_tokoff = d_btoff;
    T.words = d_words;
    std::vector<std::string> keys(n_groups);
    uint64_t n_tok = 0;
    GAMS_TRY(h, who, stage(RL_COUNT, true));
    if (nq) {
        GAMS_TRY(h, who, s1.alloc(layout_bytes(marks)));
        carve(s1.p, marks);
        T.qpos = d_qpos;
        T.gap = d_gap;
        GAMS_TRY(h, who, hipMemsetAsync(d_gap, 0, (nq / 2u + 1u) * 4u, st));
        hipLaunchKernelGGL(rl_count_kernel, dim3(nbi), dim3(256), 0, st, T);
        hipLaunchKernelGGL(blk_offsets_scan_kernel<uint32_t>, dim3(1), dim3(1024), 0, st, d_bt, nbi, d_btoff, d_words, (uint32_t)RW_TOKENS);
        GAMS_TRY(h, who, hipGetLastError());
    }
    GAMS_TRY(h, who, stage(RL_COUNT, false));
    if (nq) {
        GAMS_TRY(h, who, read_words());
        if (h->pin_scratch[RW_STRUCT]) return refuse("not a flat object of string values");
        if (h->pin_scratch[RW_VALUE]) return refuse("a value holds a byte that is no digit, '-' or ',', or an empty token");
        n_tok = h->pin_scratch[RW_TOKENS];
        std::vector<unsigned long long> qpos(nq);
        std::vector<uint32_t> gap(nq / 2u + 1u);
        GAMS_TRY(h, who, hipMemcpy(qpos.data(), d_qpos, nq * 8u, hipMemcpyDeviceToHost));
        GAMS_TRY(h, who, hipMemcpy(gap.data(), d_gap, gap.size() * 4u, hipMemcpyDeviceToHost));
        for (uint32_t g : gap)
            if (g != 1u) return refuse("not a flat object of string values");
        std::unordered_set<std::string> seen;
        for (uint32_t g = 0; g < n_groups; ++g) {
            const uint64_t b = qpos[4ull * g] + 1u, e = qpos[4ull * g + 1u];
            if (b > e || e > n_bytes) return gams_fail(h, GAMS_EHIP, who + ": quote positions out of order");
            keys[g].assign(bytes + b, (size_t)(e - b));
            if (!seen.insert(keys[g]).second) return refuse("a duplicate key");
        }
        if (n_tok > 0xfffffff0ull) return refuse("more than 2^32 - 16 tokens");
    }

    // ---- 3. parse, 4. normalise
    const uint64_t n1 = std::max<uint64_t>(n_tok, 1);
    unsigned long long *d_key = nullptr, *d_key2 = nullptr, *d_pack = nullptr, *d_goff = nullptr;
    uint32_t *d_hi = nullptr, *d_hi2 = nullptr, *d_head = nullptr, *d_hidx = nullptr;
    PoolBlock s2(h, false), s3(h, false), d_tmp(h, false);
    auto tokens = [&](Carver &c) {
        d_key = c.take<unsigned long long>(n1);
        d_hi = c.take<uint32_t>(n1);
        d_pack = c.take<unsigned long long>(n1);        // the running maximum (after a sort), then the prefix of the lengths
        d_goff = c.take<unsigned long long>((size_t)n_groups + 1);
    };
    auto sorted = [&](Carver &c) {
        d_key2 = c.take<unsigned long long>(n1);
        d_hi2 = c.take<uint32_t>(n1);
        d_head = c.take<uint32_t>(n1);
        d_hidx = c.take<uint32_t>(n1);
    };
    GAMS_TRY(h, who, s2.alloc(layout_bytes(tokens)));
    carve(s2.p, tokens);
    T.key = d_key;
    T.hi = d_hi;
    T.n_tok = n_tok;
    GAMS_TRY(h, who, stage(RL_PARSE, true));
    if (n_tok) {
        hipLaunchKernelGGL(rl_parse_kernel, dim3(nbi), dim3(256), 0, st, T);
        hipLaunchKernelGGL(rl_sorted_kernel, dim3(blocks256(n_tok)), dim3(256), 0, st, d_key, d_hi, n_tok, d_words);
        GAMS_TRY(h, who, hipGetLastError());
    }
    GAMS_TRY(h, who, stage(RL_PARSE, false));
    uint64_t m = n_tok;
    GAMS_TRY(h, who, stage(RL_NORMALISE, true));
    if (n_tok) {
        GAMS_TRY(h, who, read_words());
        if (h->pin_scratch[RW_PARSE])
            return refuse("a token that is not `a` or `a-b` of 1-10 digits each with a <= b <= 2147483647");
        if (h->pin_scratch[RW_UNSORTED]) {
            GAMS_TRY(h, who, s3.alloc(layout_bytes(sorted)));
            carve(s3.p, sorted);
            unsigned group_bits = 1;
            while (group_bits < 32u && (n_groups >> group_bits)) ++group_bits;
            const unsigned end_bit = 32u + group_bits;
            const rocprim::maximum<unsigned long long> vmax{};
            size_t b_sort = 0, b_max = 0, b_sum = 0;
            GAMS_TRY(h, who, rocprim::radix_sort_pairs(nullptr, b_sort, d_key, d_key2, d_hi, d_hi2, (size_t)n_tok, 0u, end_bit, st));
            GAMS_TRY(h, who, rocprim::inclusive_scan(nullptr, b_max, d_pack, d_pack, (size_t)n_tok, vmax, st));
            GAMS_TRY(h, who, rocprim::exclusive_scan(nullptr, b_sum, d_head, d_hidx, 0u, (size_t)n_tok, rocprim::plus<uint32_t>(), st));
            GAMS_TRY(h, who, d_tmp.alloc(std::max<size_t>({b_sort, b_max, b_sum, 256})));
            const unsigned nb = blocks256(n_tok);
            GAMS_TRY(h, who, rocprim::radix_sort_pairs(d_tmp.p, b_sort, d_key, d_key2, d_hi, d_hi2, (size_t)n_tok, 0u, end_bit, st));
            hipLaunchKernelGGL(rl_pack_hi_kernel, dim3(nb), dim3(256), 0, st, d_key2, d_hi2, n_tok, d_pack);
            GAMS_TRY(h, who, rocprim::inclusive_scan(d_tmp.p, b_max, d_pack, d_pack, (size_t)n_tok, vmax, st));
            hipLaunchKernelGGL(rl_heads_kernel, dim3(nb), dim3(256), 0, st, d_key2, d_pack, n_tok, d_head);
            GAMS_TRY(h, who, rocprim::exclusive_scan(d_tmp.p, b_sum, d_head, d_hidx, 0u, (size_t)n_tok, rocprim::plus<uint32_t>(), st));
            hipLaunchKernelGGL(rl_join_kernel, dim3(nb), dim3(256), 0, st, d_key2, d_pack, d_head, d_hidx, n_tok, d_key, d_hi, d_words);
            GAMS_TRY(h, who, hipGetLastError());
            GAMS_TRY(h, who, read_words());
            m = h->pin_scratch[RW_SPANS];
            if (m == 0 || m > n_tok) return gams_fail(h, GAMS_EHIP, who + ": span count out of range");
        }
    }
    GAMS_TRY(h, who, stage(RL_NORMALISE, false));

    // ---- 5. the set
    GAMS_TRY(h, who, stage(RL_BUILD, true));
    gams_spans_t *sp = new gams_spans_t();
    sp->n_groups = n_groups;
    sp->m = m;
    const uint64_t slots = m + n_groups + 1;
    auto build = [&]() -> hipError_t {
        hipError_t e = hipMalloc(&sp->d_groups, std::max<size_t>(n_groups, 1) * sizeof(SpanGroup));
        if (e == hipSuccess) e = hipMalloc(&sp->d_rec, std::max<uint64_t>(m, 1) * sizeof(SpanRec));
        if (e == hipSuccess) e = hipMalloc(&sp->d_dir_lo, slots * sizeof(uint32_t));
        if (e == hipSuccess) e = hipMalloc(&sp->d_cells, slots * sizeof(SpanCell));
        if (e == hipSuccess) e = hipMemsetAsync(sp->d_dir_lo, 0, slots * sizeof(uint32_t), st);
        if (e != hipSuccess || n_groups == 0) return e;
        hipLaunchKernelGGL(rl_group_off_kernel, dim3(blocks256((uint64_t)n_groups + 1)), dim3(256), 0, st, d_key, m, n_groups, d_goff);
        if (m) {
            size_t b_len = 0;
            e = rocprim::exclusive_scan(nullptr, b_len, d_pack, d_pack, 0ull, (size_t)m, rocprim::plus<unsigned long long>(), st);
            if (e == hipSuccess && b_len > d_tmp.cap) e = d_tmp.alloc(std::max<size_t>(b_len, 256));
            if (e != hipSuccess) return e;
            hipLaunchKernelGGL(rl_len_kernel, dim3(blocks256(m)), dim3(256), 0, st, d_key, d_hi, m, d_pack);
            e = rocprim::exclusive_scan(d_tmp.p, b_len, d_pack, d_pack, 0ull, (size_t)m, rocprim::plus<unsigned long long>(), st);
            if (e != hipSuccess) return e;
            hipLaunchKernelGGL(rl_rec_kernel, dim3(blocks256(m)), dim3(256), 0, st, d_key, d_hi, m, d_pack, d_goff, sp->d_rec);
        }
        hipLaunchKernelGGL(rl_groups_kernel, dim3(blocks256(n_groups)), dim3(256), 0, st, d_key, d_goff, n_groups, sp->d_groups);
        hipLaunchKernelGGL(rl_dir_kernel, dim3(blocks256(slots)), dim3(256), 0, st, sp->d_groups, n_groups, sp->d_rec, slots, sp->d_dir_lo);
        e = hipGetLastError();
        if (e == hipSuccess) e = gams_spans_launch_cells(sp, st);
        return e;
    };
    hipError_t e = build();
    if (e == hipSuccess) e = stage(RL_BUILD, false);
    if (e == hipSuccess) e = hipEventRecord(h->k1, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    gams_names_t *names = nullptr;
    int rc = GAMS_OK;
    if (e != hipSuccess) {
        rc = gams_fail(h, e == hipErrorOutOfMemory ? GAMS_ENOMEM : GAMS_EHIP, who + ": " + hipGetErrorString(e));
    } else {
        std::vector<const char *> kp(n_groups);
        for (uint32_t g = 0; g < n_groups; ++g) kp[g] = keys[g].c_str();
        rc = gams_names_create(h, n_groups, kp.data(), &names);
    }
    if (rc != GAMS_OK) {
        gams_spans_destroy(h, sp);
        return rc;
    }
    h->kq_used = RL_STAGES;
    h->kq_staged = true;
    h->k_valid = true;
    *sp_out = sp;
    *names_out = names;
    *n_groups_out = n_groups;
    *n_spans_out = m;
    return GAMS_OK;
}

}  // namespace

extern "C" {

int gams_spans_create_runlist_text(gams_gpu_t *h, const char *bytes, uint64_t n_bytes, gams_spans_t **sp,
                                   gams_names_t **chr_names, uint32_t *n_groups, uint64_t *n_spans) {
    if (sp) *sp = nullptr;
    if (chr_names) *chr_names = nullptr;
    if (!h || !sp || !chr_names || !n_groups || !n_spans || (n_bytes && !bytes))
        return gams_fail(h, GAMS_EINVAL, "spans_create_runlist_text: null argument");
    *n_groups = 0;
    *n_spans = 0;
    return runlist_run(h, bytes, n_bytes, sp, chr_names, n_groups, n_spans);
}

int gams_spans_read(gams_gpu_t *h, const gams_spans_t *sp, uint64_t *group_off, int32_t *lo, int32_t *hi, uint64_t cap,
                    uint64_t *n_spans) {
    if (!h || !sp || !group_off || !n_spans) return gams_fail(h, GAMS_EINVAL, "spans_read: null argument");
    *n_spans = sp->m;
    GAMS_HIP(h, hipSetDevice(h->device));
    GAMS_HIP(h, hipStreamSynchronize(h->compute));
    std::vector<SpanGroup> groups(sp->n_groups);
    if (sp->n_groups) GAMS_HIP(h, hipMemcpy(groups.data(), sp->d_groups, groups.size() * sizeof(SpanGroup), hipMemcpyDeviceToHost));
    for (uint32_t g = 0; g < sp->n_groups; ++g) group_off[g] = groups[g].off;
    group_off[sp->n_groups] = sp->m;
    if (cap == 0) return GAMS_OK;
    if (cap < sp->m) return gams_fail(h, GAMS_EINVAL, "spans_read: cap is smaller than the set");
    if (sp->m && (!lo || !hi)) return gams_fail(h, GAMS_EINVAL, "spans_read: null span arrays");
    std::vector<SpanRec> rec(sp->m);
    if (sp->m) GAMS_HIP(h, hipMemcpy(rec.data(), sp->d_rec, rec.size() * sizeof(SpanRec), hipMemcpyDeviceToHost));
    for (uint64_t i = 0; i < sp->m; ++i) {
        lo[i] = rec[i].lo;
        hi[i] = rec[i].hi;
    }
    return GAMS_OK;
}

}  // extern "C"
