// sw.hip -- windows around features: center_sw geometry + range GC + flank statistics.
//
// Replaces, per feature of one ctg (src/cmd_gams/sw.rs:141-184):
//   gams::center_sw         src/libs/window.rs:3-56
//   gams::cache_gc_content  src/libs/utils.rs:141-162   (round4 on return)
//   gams::center_resize     src/libs/window.rs:96-124
//   gams::cache_gc_stat     src/libs/utils.rs:189-213 -> gc_stat utils.rs:164-187
//
// GC of an arbitrary range comes from a prefix index over the whole seqset
// buffer, built once per seqset by two kernels:
//   gc_index_build  one workgroup per 64 KiB segment: 16-bit G/C mask per 16-B
//                   chunk + segment-local prefix (same layout as the wave tile)
//   gc_index_scan   exclusive scan of the segment totals (u64)
// P(y) = seg_base[y >> 16] + (PM[y >> 4] >> 16) + popcount(PM[y >> 4] & low(y & 15))
// and gc_count(range) = P(end+1) - P(start): 6 loads per range (4 B + 8 B each side).
// The parent is a single span, so IntSpan index/slice/at are plain arithmetic.
// Statistics are evaluated in the reference's f32 order (-ffp-contract=off).
//
// `-a count` (rg_count, the ninth column): Lapper::count(win.min(), win.max()) of every window against the
// idx:rg: group of its ctg -- the lookup of `locate --count` (lapper_count, interval_kernels.hpp), run by the
// same thread that holds the window.  sw_kernel<kGc, kCount> is instantiated per action set; without kGc it
// neither needs the gc index nor touches the sequence bytes.  A third flag, kSum, keeps the row in registers and adds it
// into the per-distance summary instead of storing it.  sw_anno_kernel<kGc, kCount> is that summarising
// kernel joined with up to four resident span sets: per row and set the covered share of the window (span_cover_card, the
// lookup of `anno`), summed as the integer the text would print -- the Prop columns of fsw-distance-tag.tera.sql.

#include "interval_kernels.hpp"
#include "text_emit.hpp"

#include "range_batch.hpp"

#include <string>
#include <type_traits>

#include <algorithm>

struct gams_gcindex {
    uint32_t *d_pm = nullptr;        // per 16-B chunk: local prefix << 16 | mask
    uint64_t *d_seg = nullptr;       // per 64 KiB segment: GC count before it
    uint64_t n_chunks = 0, n_segs = 0;
};

namespace {

__device__ __forceinline__ uint32_t gc_nibble(uint32_t x) {
    uint32_t y = (x & 0xDBDBDBDBu) ^ 0x43434343u;
    uint32_t t = (y & 0x7F7F7F7Fu) + 0x7F7F7F7Fu;
    uint32_t f = ~(t | y) & 0x80808080u;
    uint32_t g = f | (f >> 7);
    g |= g >> 14;
    return (g >> 7) & 0xFu;
}

// one workgroup (256 threads) per segment of 4096 chunks = 64 KiB
__global__ __launch_bounds__(256) void gc_index_build(const uint8_t *seq, uint64_t n_chunks, uint32_t *pm,
                                                       uint64_t *seg_tot) {
    __shared__ uint32_t ws[4];
    __shared__ uint32_t msk[4096 + 16];
    const uint32_t tid = threadIdx.x;
    const uint64_t c0 = (uint64_t)blockIdx.x * 4096u;
    const uint4 *src = reinterpret_cast<const uint4 *>(seq);
    // coalesced: in trip q the workgroup reads 256 consecutive chunks (4 KiB)
#pragma unroll 4
    for (uint32_t q = 0; q < 16; ++q) {
        const uint32_t lc = q * 256u + tid;
        const uint64_t c = c0 + lc;
        uint32_t m = 0;
        if (c < n_chunks) {
            const uint4 v = load_once16(src + c);   // the index is built in one pass over the sequence
            m = gc_nibble(v.x) | (gc_nibble(v.y) << 4) | (gc_nibble(v.z) << 8) | (gc_nibble(v.w) << 12);
        }
        msk[lc + (lc >> 8)] = m;  // +1 word per 256: thread t's 16-word run starts on bank 17t
    }
    __syncthreads();
    // thread t owns chunks [16t, 16t+16) of the segment
    uint32_t s = 0;
#pragma unroll
    for (uint32_t q = 0; q < 16; ++q) {
        const uint32_t lc = tid * 16u + q;
        s += __popc(msk[lc + (lc >> 8)]);
    }
    uint32_t tot;
    uint32_t run = block_excl_scan_256<uint32_t>(s, ws, tot);
#pragma unroll
    for (uint32_t q = 0; q < 16; ++q) {
        const uint32_t lc = tid * 16u + q;
        const uint32_t m = msk[lc + (lc >> 8)];
        if (c0 + lc < n_chunks) pm[c0 + lc] = (run << 16) | m;
        run += __popc(m);
    }
    if (tid == 0) seg_tot[blockIdx.x] = tot;  // <= 65536; local prefixes (exclusive) stay below 2^16
}

// single workgroup: in-place exclusive scan of the segment totals
__global__ __launch_bounds__(256) void gc_index_scan(uint64_t *seg, uint64_t n_segs) {
    __shared__ uint64_t ws[4];
    const uint32_t tid = threadIdx.x;
    const uint64_t per = (n_segs + 255u) / 256u;
    const uint64_t b = min((uint64_t)tid * per, n_segs), e = min(b + per, n_segs);
    uint64_t s = 0;
    for (uint64_t i = b; i < e; ++i) s += seg[i];
    uint64_t tot;
    uint64_t run = block_excl_scan_256<uint64_t>(s, ws, tot);
    for (uint64_t i = b; i < e; ++i) {
        const uint64_t v = seg[i];
        seg[i] = run;
        run += v;
    }
}

__device__ __forceinline__ uint64_t gc_before(const uint32_t *pm, const uint64_t *seg, uint64_t y) {
    const uint32_t e = pm[y >> 4];
    return seg[y >> 16] + (e >> 16) + __popc(e & ((1u << (y & 15u)) - 1u));
}

// ---- geometry shared by host (row offsets) and device ------------------------
struct SwGeom {
    int32_t m_s, m_e;  // the M window, chromosome coordinates
    int32_t n_l, n_r;  // number of L and R windows
};

// window.rs:96-124 for a single-span parent [ps,pe] and span [is,ie]
__host__ __device__ inline void center_resize_1(int32_t ps, int32_t pe, int32_t is, int32_t ie, int32_t resize,
                                                int32_t &os, int32_t &oe) {
    const int32_t psize = pe - ps + 1;
    const int32_t half_size = (ie - is + 1) / 2;
    const int32_t mid_left = half_size == 0 ? is : is + half_size - 1;
    const int32_t mid_right = half_size == 0 ? is : is + half_size;
    const int32_t half_resize = resize / 2;
    int32_t left_idx = (mid_left - ps + 1) - half_resize + 1;
    if (left_idx < 1) left_idx = 1;
    int32_t right_idx = (mid_right - ps + 1) + half_resize - 1;
    if (right_idx > psize) right_idx = psize;
    os = ps + left_idx - 1;
    oe = ps + right_idx - 1;
}

// window.rs:3-56: M, then L windows while sw_start >= 1, then R windows while
// sw_end <= parent.size(), at most `max` each
__host__ __device__ inline SwGeom sw_geometry(int32_t ps, int32_t pe, int32_t fs, int32_t fe, int32_t size,
                                              int32_t max) {
    SwGeom g;
    center_resize_1(ps, pe, fs, fe, size, g.m_s, g.m_e);
    const int64_t psize = (int64_t)pe - ps + 1;
    const int64_t m_min_idx = (int64_t)g.m_s - ps + 1, m_max_idx = (int64_t)g.m_e - ps + 1;
    // L: sw_end = m_min_idx - 1 - (d-1)*size, sw_start = sw_end - size + 1 >= 1, sw_end <= psize
    int64_t nl = 0, nr = 0;
    if (max > 0 && size > 0) {
        const int64_t room_l = m_min_idx - 1;  // indices strictly left of M
        nl = room_l >= 0 ? room_l / size : 0;
        if (m_min_idx - 1 > psize) nl = 0;     // first L window already past the end (:33)
        const int64_t room_r = psize - m_max_idx;
        nr = room_r >= 0 ? room_r / size : 0;
        if (m_max_idx + 1 < 1) nr = 0;         // first R window before the start (:30)
        if (nl > max) nl = max;
        if (nr > max) nr = max;
    }
    g.n_l = (int32_t)nl;
    g.n_r = (int32_t)nr;
    return g;
}

__device__ __forceinline__ float round4(float x) {  // utils.rs:135-138 with decimals = 4
    const float y = 10000.0f;
    return roundf(x * y) / y;
}

// one selected ctg of a batched sw call
struct SwCtg {
    uint64_t seq_off;     // buffer offset of ctg base 0
    uint32_t len;
    int32_t chr_start, chr_end;
    uint32_t feat_first;  // index of the ctg's first feature in the call's feature arrays
    uint32_t rg_group;    // its group of the rg index (-a count); >= n_groups: none, counts are 0
    uint32_t pad;
};
static_assert(sizeof(SwCtg) == 32, "tests/layout_main.cpp carves with a stand-in of this size");

struct SwArgs {
    const uint32_t *pm;
    const uint64_t *seg;
    uint64_t seq_off;   // buffer offset of ctg base 0   (sw_kernel: filled per thread from ctgs[])
    uint32_t len;
    int32_t chr_start, chr_end;
    const SwCtg *ctgs;        // sw_kernel: the selected ctgs
    const uint32_t *fctg;     // sw_kernel: selected-ctg number of every feature
    const int32_t *fs, *fe;
    const uint64_t *row_off;  // exclusive prefix of rows per feature
    uint32_t nf;
    int32_t size, max, resize;
    gams_sw_row_t *rows;
    uint64_t cap;
    // -a count: the rg index (interval_kernels.hpp) and the count column, one entry per row
    const CountGroup *cgroups;
    const uint32_t *rg_starts, *rg_stops;
    const BkRec *bk_start, *bk_stop;
    uint32_t n_groups;
    int32_t *cnt;
    // the summarising instantiation: the call's table, (max + 1) groups, its flag word, and the chunks of 256 slots
    unsigned long long *sum, *sum_bad;
    uint64_t sum_chunks;
};

// The span sets of a summarising call with Prop columns, a kernel argument of its own so that SwArgs and
// the instantiations without sets stay what they are: per set the four tables of its gams_spans_t, its groups, and
// set_group[k] = the group of ctg k's chromosome in it (UINT32_MAX: the chromosome is absent, the prop is 0), k as
// a.fctg numbers the ctgs.  prop: the call's Prop sums, (max + 1) x n words, group-major.
struct SwAnnoOne {
    const SpanGroup *groups;
    const SpanRec *rec;
    const uint32_t *dir;
    const SpanCell *cells;
    const uint32_t *set_group;
    uint32_t n_groups, pad;
};
struct SwAnno {
    SwAnnoOne set[GAMS_SW_SUMMARY_MAX_ANNO];
    unsigned long long *prop;
    uint32_t n, pad;
};

// gc_content of chromosome range [s,e] (inclusive) inside the ctg: count / len, f32
__device__ __forceinline__ float range_gc(const SwArgs &a, int32_t s, int32_t e) {
    // parent.index(): from = s - chr_start + 1 (1-based), bytes [from-1, to)
    int64_t b0 = (int64_t)s - a.chr_start, b1 = (int64_t)e - a.chr_start + 1;
    const float flen = (float)(int32_t)(b1 - b0);
    b0 = b0 < 0 ? 0 : (b0 > a.len ? a.len : b0);  // never read outside the ctg
    b1 = b1 < 0 ? 0 : (b1 > a.len ? a.len : b1);
    const uint64_t c = gc_before(a.pm, a.seg, a.seq_off + (uint64_t)b1) -
                       gc_before(a.pm, a.seg, a.seq_off + (uint64_t)b0);
    return (float)(uint32_t)c / flen;
}

// G/C bases in front of ctg byte offset b (clamped into the ctg like range_gc)
__device__ __forceinline__ uint64_t gc_prefix_at(const SwArgs &a, int64_t b) {
    b = b < 0 ? 0 : (b > a.len ? a.len : b);
    return gc_before(a.pm, a.seg, a.seq_off + (uint64_t)b);
}

// one thread per (feature, slot); slot 0 = M, 1..max = L, max+1..2max = R
// All selected ctgs of a call in ONE launch (a ctg's ~400 features are a handful of workgroups: launched
// per ctg the kernel is all launch latency).
// kGc: gc_content and the flank statistics (sw.rs:167-184); kCount: rg_count into a.cnt.  Without kGc the four
// statistics of the row are 0 and nothing reads a.pm / a.seg.
// kSum: the row and its count stay with the thread (r, cnt) for the summary; nothing is stored and a.row_off, a.rows,
// a.cnt and a.cap are not looked at.  gid = the thread's (feature, slot) number; returns whether that slot holds a window.
template <bool kGc, bool kCount, bool kSum>
__device__ __forceinline__ bool sw_row(const SwArgs &a0, uint64_t gid, gams_sw_row_t &r, int32_t &cnt) {
    const uint32_t slots = 1u + 2u * (uint32_t)a0.max;
    const uint64_t f = gid / slots;
    const uint32_t slot = (uint32_t)(gid % slots);
    if (f >= a0.nf) return false;
    const SwCtg cg = a0.ctgs[a0.fctg[f]];
    SwArgs a = a0;
    a.seq_off = cg.seq_off;
    a.len = cg.len;
    a.chr_start = cg.chr_start;
    a.chr_end = cg.chr_end;
    const SwGeom g = sw_geometry(a.chr_start, a.chr_end, a.fs[f], a.fe[f], a.size, a.max);
    int32_t type, dist, ws, we;
    uint64_t row = kSum ? 0ull : a.row_off[f];
    if (slot == 0) {
        type = 0;
        dist = 0;
        ws = g.m_s;
        we = g.m_e;
    } else if (slot <= (uint32_t)a.max) {
        dist = (int32_t)slot;
        if (dist > g.n_l) return false;
        type = 1;
        we = g.m_s - 1 - (dist - 1) * a.size;   // window.rs:24,48-49
        ws = we - a.size + 1;
        row += (uint64_t)dist;
    } else {
        dist = (int32_t)slot - a.max;
        if (dist > g.n_r) return false;
        type = 2;
        ws = g.m_e + 1 + (dist - 1) * a.size;   // window.rs:21,45-46
        we = ws + a.size - 1;
        row += (uint64_t)g.n_l + (uint64_t)dist;
    }
    if (!kSum && row >= a.cap) return false;
    r.feature = (uint32_t)f - cg.feat_first;
    r.type = type;
    r.distance = dist;
    r.start = ws;
    r.end = we;
    if (kCount) { // count_rg(idx:rg:, ctg, Range::from(chr, win.min(), win.max())) = Lapper::count(ws, we)
        cnt = lapper_count(a.cgroups, a.rg_starts, a.rg_stops, a.bk_start, a.bk_stop, a.n_groups, cg.rg_group,
                           (uint32_t)ws, (uint32_t)we);
        if (!kSum) a.cnt[row] = cnt;
    }
    if (!kGc) {
        r.gc_content = r.gc_mean = r.gc_stddev = r.gc_cv = 0.0f;
        if (!kSum) a.rows[row] = r;
        return true;
    }
    r.gc_content = round4(range_gc(a, ws, we));                         // utils.rs:161
    // flank: center_resize(parent, window, resize) cut into size-bp tiles (sw.rs:175-178)
    int32_t rs, re;
    center_resize_1(a.chr_start, a.chr_end, ws, we, a.resize, rs, re);
    const int32_t flen = re - rs + 1;
    const int32_t nt = flen >= a.size ? (flen - a.size) / a.size + 1 : 0;  // sliding(range,size,size)
    const float len = (float)nt;
    // Consecutive tiles share a boundary: one prefix lookup per boundary (nt + 1) instead of two
    // per tile and pass; the tile values are kept for the second pass when they fit.
    constexpr int kKeep = 8;
    float xs[kKeep];
    float sum = 0.0f;
    {
        uint64_t before = gc_prefix_at(a, (int64_t)rs - a.chr_start);
#pragma unroll   // constant indices keep xs[] in registers
        for (int32_t t = 0; t < kKeep; ++t) {
            if (t < nt) {
                const uint64_t upto = gc_prefix_at(a, (int64_t)rs - a.chr_start + (int64_t)(t + 1) * a.size);
                xs[t] = round4((float)(uint32_t)(upto - before) / (float)a.size);
                before = upto;
                sum = sum + xs[t];                                          // stat.rs:3
            }
        }
        for (int32_t t = kKeep; t < nt; ++t) {
            const uint64_t upto = gc_prefix_at(a, (int64_t)rs - a.chr_start + (int64_t)(t + 1) * a.size);
            sum = sum + round4((float)(uint32_t)(upto - before) / (float)a.size);
            before = upto;
        }
    }
    const float mean = sum / len;                                       // stat.rs:5
    float sq = 0.0f;
#pragma unroll
    for (int32_t t = 0; t < kKeep; ++t) {
        if (t < nt) {
            const float d = xs[t] - mean;
            sq = sq + d * d;                                                // stat.rs:12
        }
    }
    for (int32_t t = kKeep; t < nt; ++t) {
        const int32_t ts = rs + t * a.size;
        const float x = round4(range_gc(a, ts, ts + a.size - 1));
        const float d = x - mean;
        sq = sq + d * d;
    }
    const float sd = sqrtf(sq / (len - 1.0f));                          // stat.rs:13
    float cv;                                                           // utils.rs:169-175
    if (mean == 0.0f || mean == 1.0f)
        cv = 0.0f;
    else if (mean <= 0.5f)
        cv = sd / mean;
    else
        cv = sd / (1.0f - mean);
    r.gc_mean = round4(mean);
    r.gc_stddev = round4(sd);
    r.gc_cv = round4(cv);
    if (!kSum) a.rows[row] = r;
    return true;
}

// ---- the per-distance summary of the rows --------------------------------------------------------------
// A group -- one distance of one tag -- is GAMS_SW_SUMMARY_WORDS 64-bit integers: COUNT, the sums S of the four
// statistics' m (sw_f4_units: what sw_put_f4 prints), their four NaN counters, and C, the sum of rg_count.  All integers:
// the result does not depend on the order of the additions.
constexpr uint32_t kSumWords = GAMS_SW_SUMMARY_WORDS;
enum : uint32_t { SUM_COUNT = 0, SUM_S = 1, SUM_NAN = 5, SUM_C = 9 };
// The distances of a call that a workgroup reduces in LDS before it touches global memory: 256 groups x 10 words x 8 B =
// 20 KiB, an eighth of a CU's 160 KiB, so the table never lowers the 8 workgroups of 256 threads a CU holds.  A call with
// more distances (max >= 256) adds to global memory directly.
constexpr uint32_t kSumLdsGroups = 256;
// With n span sets a group has n more words, the Prop sums P_a, kept behind the groups' ten words in the same 20 KiB: the
// call reduces in LDS while (max + 1) x (10 + n) <= 256 x 10 = 2560 words -- max <= 255, 231, 212, 195, 181 for n = 0 .. 4
// -- so the table never grows and the 8 workgroups a CU stay.
constexpr uint32_t kSumLdsWords = kSumLdsGroups * kSumWords;

// one row into group `g` (LDS or global); `bad`: a statistic the text formatter does not cover either
template <bool kGc, bool kCount>
__device__ __forceinline__ void sw_sum_put(unsigned long long *g, const gams_sw_row_t &r, int32_t cnt, bool &bad) {
    atomicAdd(g + SUM_COUNT, 1ull);
    if (kGc) {
        const float v[4] = {r.gc_content, r.gc_mean, r.gc_stddev, r.gc_cv};
#pragma unroll
        for (uint32_t k = 0; k < 4u; ++k) {
            if (v[k] != v[k])
                atomicAdd(g + SUM_NAN + k, 1ull);
            else if (!(v[k] >= 0.0f) || !(v[k] < 1000.0f))     // (sw_put_f4's refusal; -0 passes and adds 0)
                bad = true;
            else if (const uint32_t m = sw_f4_units(v[k]))
                atomicAdd(g + SUM_S + k, (unsigned long long)m);
        }
    }
    if (kCount && cnt) atomicAdd(g + SUM_C, (unsigned long long)(long long)cnt);
}

// The summarising kernel.  The slots are dealt out as in the storing kernel -- 256 consecutive (feature, slot) numbers a
// workgroup and trip -- but a workgroup takes every gridDim.x-th such chunk and keeps its table across them, so the
// global atomics of the flush are paid once per resident workgroup, not once per 256 rows: flushed per chunk, the
// 16 000 chunks of the kept workload queued 1.7e6 atomics on the same 105 words and the stage took 0.37 ms
// (profiles/sw_summary.txt).  The table: the call's distances in LDS, flushed once, non-zero bins only, or -- beyond
// kSumLdsGroups distances -- the call's table in global memory directly.
// The Prop units of the window [ws, we] of ctg k against every set, into the group's n words at p (LDS or global):
// anno.rs:122-140 with the ctg clip left out (a window lies inside its ctg) -- the covered cardinality by span_cover_kernel's
// lookup, two cell records a set, prop = |.| as f32 / len as f32 and the q that `{:.4}` prints.  Zero adds nothing.
__device__ __forceinline__ void sw_sum_put_anno(unsigned long long *p, const SwAnno &an, uint32_t k, int32_t ws, int32_t we) {
    const float len = (float)(int32_t)((int64_t)we - ws + 1);
#pragma unroll
    for (uint32_t s = 0; s < GAMS_SW_SUMMARY_MAX_ANNO; ++s) {
        if (s >= an.n) break;
        const SwAnnoOne &A = an.set[s];
        const uint32_t g = A.set_group[k];
        if (g >= A.n_groups) continue;                         // anno.rs:128: the chromosome is not in the set
        const uint64_t card = span_cover_card(A.groups, A.rec, A.dir, A.cells, g, ws, we);
        const float prop = (float)(int32_t)card / len;
        if (!(prop >= 0.0f && prop <= 1.0f)) continue;         // (cannot happen: card <= len)
        if (const uint32_t q = gams_prop4_units(prop)) atomicAdd(p + s, (unsigned long long)q);
    }
}

template <bool kGc, bool kCount, bool kAnno>
__device__ __forceinline__ void sw_sum_chunks(const SwArgs &a, uint64_t n_chunks, const SwAnno *an) {
    __shared__ unsigned long long bins[kSumLdsWords];
    const uint32_t words = ((uint32_t)a.max + 1u) * kSumWords;
    const uint32_t n_anno = kAnno ? an->n : 0u, pwords = ((uint32_t)a.max + 1u) * n_anno;
    // uniform; with sets, both tables in the same 2560 words (the sum below stays under 2^32: max <= 2^24)
    const bool lds = kAnno ? (uint64_t)words + pwords <= kSumLdsWords : (uint32_t)a.max < kSumLdsGroups;
    bool bad = false;
    if (lds) {
        for (uint32_t i = threadIdx.x; i < words + pwords; i += 256u) bins[i] = 0ull;
        __syncthreads();
    }
    for (uint64_t chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
        gams_sw_row_t r;
        int32_t cnt = 0;
        const uint64_t gid = chunk * 256u + threadIdx.x;
        if (!sw_row<kGc, kCount, true>(a, gid, r, cnt)) continue;
        if (lds)
            sw_sum_put<kGc, kCount>(bins + (uint32_t)r.distance * kSumWords, r, cnt, bad);
        else
            sw_sum_put<kGc, kCount>(a.sum + (uint64_t)(uint32_t)r.distance * kSumWords, r, cnt, bad);
        if constexpr (kAnno) {
            const uint32_t k = a.fctg[gid / (1u + 2u * (uint32_t)a.max)];   // the row's ctg, as sw_row found it
            unsigned long long *const p = lds ? bins + words : an->prop;
            sw_sum_put_anno(p + (uint64_t)(uint32_t)r.distance * n_anno, *an, k, r.start, r.end);
        }
    }
    if (bad) *a.sum_bad = 1ull;
    if (lds) {
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < words; i += 256u) {
            const unsigned long long v = bins[i];
            if (v) atomicAdd(a.sum + i, v);
        }
        if constexpr (kAnno)
            for (uint32_t i = threadIdx.x; i < pwords; i += 256u) {
                const unsigned long long v = bins[words + i];
                if (v) atomicAdd(an->prop + i, v);
            }
    }
}

template <bool kGc, bool kCount, bool kSum = false>
__global__ __launch_bounds__(256) void sw_kernel(const SwArgs a0) {
    if constexpr (kSum) {
        sw_sum_chunks<kGc, kCount, false>(a0, a0.sum_chunks, nullptr);
    } else {
        gams_sw_row_t r;
        int32_t cnt = 0;
        (void)sw_row<kGc, kCount, false>(a0, (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, r, cnt);
    }
}

// the summarising kernel with Prop columns: sw_kernel<kGc, kCount, true> with the sets beside its arguments
template <bool kGc, bool kCount>
__global__ __launch_bounds__(256) void sw_anno_kernel(const SwArgs a0, const SwAnno an) {
    sw_sum_chunks<kGc, kCount, true>(a0, a0.sum_chunks, &an);
}

// the call's table into the accumulator's groups of its tag, unless the call met a value it does not cover
__global__ __launch_bounds__(256) void sw_sum_merge_kernel(const unsigned long long *call, const unsigned long long *bad,
                                                           unsigned long long *acc, uint32_t words) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= words || *bad) return;
    const unsigned long long v = call[i];
    if (v) acc[i] += v;
}

// peak (src/cmd_gams/peak.rs:79) / any caller of cache_gc_content: one lane per range, the ranges of every
// selected ctg in one launch (a.ctgs / a.fctg as in sw_kernel)
__global__ __launch_bounds__(256) void range_gc_kernel(const SwArgs a0, const int32_t *rs, const int32_t *re,
                                                       uint32_t n, float *gc) {
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    const SwCtg cg = a0.ctgs[a0.fctg[q]];
    SwArgs a = a0;
    a.seq_off = cg.seq_off;
    a.len = cg.len;
    a.chr_start = cg.chr_start;
    a.chr_end = cg.chr_end;
    gc[q] = round4(range_gc(a, rs[q], re[q]));                          // utils.rs:157-161
}

// the same over device columns (gams_gpu_peak_text): range q lies in the ctg whose record is entry rctg[q] of the
// three per-ctg columns; a ctg of length 0 has no sequence and gives 0
__global__ __launch_bounds__(256) void range_gc_cols_kernel(const uint32_t *pm, const uint64_t *seg,
                                                            const unsigned long long *seq_off, const uint32_t *len,
                                                            const int32_t *chr_start, const uint32_t *rctg,
                                                            const uint32_t *rs, const uint32_t *re, uint32_t n, float *gc) {
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    const uint32_t c = rctg[q];
    SwArgs a{};
    a.pm = pm;
    a.seg = seg;
    a.seq_off = seq_off[c];
    a.len = len[c];
    a.chr_start = chr_start[c];
    gc[q] = a.len ? round4(range_gc(a, (int32_t)rs[q], (int32_t)re[q])) : 0.0f;
}

}  // namespace

void gams_launch_range_gc_cols(const gams_seqset_t *s, const unsigned long long *seq_off, const uint32_t *len,
                               const int32_t *chr_start, const uint32_t *rctg, const uint32_t *rs, const uint32_t *re,
                               uint32_t n, float *gc, hipStream_t st) {
    hipLaunchKernelGGL(range_gc_cols_kernel, dim3((n + 255u) / 256u), dim3(256), 0, st, s->gcindex->d_pm, s->gcindex->d_seg,
                       seq_off, len, chr_start, rctg, rs, re, n, gc);
}

// lazily built per seqset; owned by the seqset (freed in gams_seqset_destroy)
int gams_seqset_gcindex(gams_gpu_t *h, gams_seqset_t *s) {
    if (!s->have_bytes) return gams_fail(h, GAMS_ESTATE, "the seqset holds the G/C plane only: this call needs the sequence bytes");
    if (s->gcindex) return GAMS_OK;
    int wrc = gams_seqset_read_begin(h, s);   // the build reads the sequence bytes
    if (wrc != GAMS_OK) return wrc;
    gams_gcindex *ix = s->gcindex = new gams_gcindex();   // the seqset's from here on: one way out, gams_seqset_gcindex_free
    ix->n_chunks = s->bytes / 16;
    ix->n_segs = (ix->n_chunks + 4095) / 4096;
    bool launched = false;
    hipError_t e = hipMalloc(&ix->d_pm, ix->n_chunks * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc(&ix->d_seg, (ix->n_segs + 1) * sizeof(uint64_t));
    if (e == hipSuccess) {
        launched = true;
        hipLaunchKernelGGL(gc_index_build, dim3((unsigned)ix->n_segs), dim3(256), 0, h->compute, s->d_seq,
                           ix->n_chunks, ix->d_pm, ix->d_seg);
        hipLaunchKernelGGL(gc_index_scan, dim3(1), dim3(256), 0, h->compute, ix->d_seg, ix->n_segs);
        e = hipGetLastError();
    }
    if (e == hipSuccess) return GAMS_OK;
    (void)hipGetLastError();   // reported below, not left sticky
    gams_seqset_gcindex_free(s);
    return gams_fail(h, launched ? GAMS_EHIP : GAMS_ENOMEM,
                     std::string(launched ? "gcindex: launch: " : "gcindex: hipMalloc: ") + hipGetErrorString(e));
}

void gams_seqset_gcindex_free(gams_seqset_t *s) {
    if (!s->gcindex) return;
    (void)hipFree(s->gcindex->d_pm);
    (void)hipFree(s->gcindex->d_seg);
    delete s->gcindex;
    s->gcindex = nullptr;
}

// ---- the rows as TSV text (sw.rs:152-190, the Display of Sw: data.rs:58-83) -------------------------------------
// "sw:{feature id}:{serial}\t{chr}:{start}-{end}\t{M|L|R}\t{distance}\t{gc_content}\t{gc_mean}\t{gc_stddev}\t{gc_cv}\t{rg_count}\n"
// The action set decides the last five fields: without gc the four statistics are empty ("\t\t\t", data.rs:60-70),
// without count rg_count is empty; with count it is the decimal i32 (data.rs:71-75).  The four floats are round(x, 4) values
// (utils.rs:135-138, :161, :186): the f32 nearest to m / 10^4 for an integer m, and Rust's `{}` prints the shortest
// digits that round-trip -- for m below 10^7 (values below 1000: gc values are below 1, cv a few units) that is m / 10^4
// with its trailing zeros dropped, since no shorter decimal lies within half an ulp of it.  Anything else (a value of
// 1000 or more, a negative coordinate) raises a flag and the host formats the batch as before.
namespace {
constexpr uint32_t kSwTextBlock = 512;     // rows per workgroup of the text kernels (256 threads x 2)
// bytes of a block's text staged in LDS: 96 B a row on average.  A row without its names is at most 88 B
// (-a gc) and 99 B (-a gc -a count: up to 11 more for the count); a block beyond the stage is written to
// global memory directly (sw_text_write_kernel's unstaged branch)
constexpr uint32_t kSwTextStage = 49152;

struct SwTextArgs {
    const gams_sw_row_t *rows;
    uint64_t n_rows;
    const SwCtg *ctgs;
    const uint64_t *ctg_row_off;       // [n_sel + 1]: first row of every selected ctg
    uint32_t n_sel;
    const uint64_t *feat_row_off;      // [nf + 1]: first row of every feature
    const uint32_t *name_off;          // [n_sel + 1] into names
    const char *names;
    const uint32_t *id_off;            // [nf + 1] into ids
    const char *ids;
    uint32_t *len;                     // per row
    uint32_t *blk_len;                 // per block
    unsigned long long *blk_off;       // exclusive prefix, [nb] = all bytes
    uint32_t nb;
    char *text;
    uint64_t text_cap;
    unsigned long long *words;         // [0] = all bytes, [1] = flag (a value this formatter does not cover), [2 + k] = first byte of ctg k
    uint32_t gc;                       // print the four statistics (else four empty fields)
    const int32_t *cnt;                // per row rg_count (nullptr: the field stays empty)
    // gams_gpu_sw_feature_text: the id is composed here, "feature:" + the id of the row's interval + ':' + its 1-based
    // number among the interval's features, and the chromosome is the name of the interval's group; ids / id_off /
    // names / name_off above are unused
    uint32_t dev_ids;
    const unsigned long long *cid_off, *chr_off;   // ctg_ids by interval, chr_names by group
    const char *cid_bytes, *chr_bytes;
    const uint32_t *igrp;                          // per interval: its group
};
// ... with the tenth field (gams_gpu_sw_text_dg): the ΔG of every row, on the device
struct SwTextDgArgs : SwTextArgs {
    const float *dg;
};
__device__ __forceinline__ const float *sw_dg_col(const SwTextArgs &) { return nullptr; }
__device__ __forceinline__ const float *sw_dg_col(const SwTextDgArgs &a) { return a.dg; }

struct SwRowCtx {
    uint32_t k, f, serial;    // selected ctg, feature (index into the call's arrays), 1-based row of the feature
};
__device__ __forceinline__ SwRowCtx sw_row_ctx(const SwTextArgs &a, uint64_t r, const gams_sw_row_t &w) {
    uint32_t lo = 0, hi = a.n_sel;                       // last ctg whose first row <= r
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (a.ctg_row_off[mid] <= r)
            lo = mid;
        else
            hi = mid;
    }
    SwRowCtx c;
    c.k = lo;
    c.f = a.ctgs[lo].feat_first + w.feature;
    c.serial = (uint32_t)(r - a.feat_row_off[c.f]) + 1u;    // sw.rs:148: the serial restarts with every feature
    return c;
}
// the row's text, counted or written; `bad`: a value this formatter does not cover.  kDg: the tenth field behind rg_count,
// dg[r] printed `{:.4}` and empty for NaN (gams_gpu_sw_text_dg); the column is handed in beside SwTextArgs (sw_dg_col)
template <bool kWrite, bool kDg = false>
__device__ __forceinline__ void sw_row_text(const SwTextArgs &a, uint64_t r, RowOut<kWrite> &o, bool &bad,
                                            const float *dg = nullptr) {
    const gams_sw_row_t w = a.rows[r];
    const SwRowCtx c = sw_row_ctx(a, r, w);
    const char *id, *nm;
    uint32_t idn, nmn, num = 0u;                         // num: the feature's number behind a composed id
    if (a.dev_ids) {
        const unsigned long long i0 = a.cid_off[c.k], g0 = a.chr_off[a.igrp[c.k]];
        id = a.cid_bytes + i0;
        idn = (uint32_t)(a.cid_off[c.k + 1u] - i0);
        nm = a.chr_bytes + g0;
        nmn = (uint32_t)(a.chr_off[a.igrp[c.k] + 1u] - g0);
        num = w.feature + 1u;                            // feature.rs:74-86: from 1 on a fresh cnt:feature:
    } else {
        id = a.ids + a.id_off[c.f];
        idn = a.id_off[c.f + 1u] - a.id_off[c.f];
        nm = a.names + a.name_off[c.k];
        nmn = a.name_off[c.k + 1u] - a.name_off[c.k];
    }
    if (w.start < 0 || w.end < 0 || w.distance < 0 || (uint32_t)w.type > 2u) bad = true;
    const uint32_t st = (uint32_t)w.start, en = (uint32_t)w.end, di = (uint32_t)w.distance;
    o.bytes("sw:", 3u);
    if (num) o.bytes("feature:", 8u);
    o.bytes(id, idn);
    if (num) {
        o.ch(':');
        o.dec(num);
    }
    o.ch(':');
    o.dec(c.serial);
    o.ch('\t');
    o.bytes(nm, nmn);
    o.ch(':');
    o.dec(st);
    if (en != st) {
        o.ch('-');
        o.dec(en);
    }
    o.ch('\t');
    o.ch("MLR"[(uint32_t)w.type > 2u ? 0u : (uint32_t)w.type]);
    o.ch('\t');
    o.dec(di);
    o.ch('\t');
    if (a.gc) {
        o.f4(w.gc_content, bad);
        o.ch('\t');
        o.f4(w.gc_mean, bad);
        o.ch('\t');
        o.f4(w.gc_stddev, bad);
        o.ch('\t');
        o.f4(w.gc_cv, bad);
    } else {
        o.bytes("\t\t\t", 3u);                           // four empty statistics
    }
    o.ch('\t');
    if (a.cnt) o.i32(a.cnt[r]);
    if (kDg) {
        o.ch('\t');
        o.dg4(dg[r], bad);
    }
    o.ch('\n');
}

// The two text kernels, instantiated on the argument struct: SwTextArgs, or SwTextDgArgs with the ΔG column.  The type, not
// a flag or a wrapper over a shared body, decides (profiles/seqset_protocol_refactor.txt: the <SwTextArgs> instantiations
// are, instruction for instruction, the kernels that had no column; profiles/dg.txt has what a flag did to them).
template <typename A>
__global__ __launch_bounds__(256) void sw_text_len_kernel(const A a) {
    constexpr bool kDg = std::is_same<A, SwTextDgArgs>::value;
    __shared__ uint32_t ws[4];
    const uint64_t base = (uint64_t)blockIdx.x * kSwTextBlock;
    const uint32_t tid = threadIdx.x;
    uint32_t sum = 0;
    bool bad = false;
#pragma unroll
    for (uint32_t u = 0; u < 2u; ++u) {
        const uint64_t r = base + 2u * tid + u;
        if (r >= a.n_rows) continue;
        RowOut<false> n;
        sw_row_text<false, kDg>(a, r, n, bad, sw_dg_col(a));
        a.len[r] = n.n;
        sum += n.n;
    }
    if (bad) a.words[1] = 1ull;
    const uint32_t tot = block_sum_256(sum, ws);
    if (tid == 0u) a.blk_len[blockIdx.x] = tot;
}

template <typename A>
__global__ __launch_bounds__(256) void sw_text_write_kernel(const A a) {
    constexpr bool kDg = std::is_same<A, SwTextDgArgs>::value;
    __shared__ uint32_t scr[4];
    __shared__ __align__(16) char stage[kSwTextStage + 16];
    const uint64_t base = (uint64_t)blockIdx.x * kSwTextBlock;
    const uint32_t tid = threadIdx.x;
    uint32_t l[2], mine = 0;
#pragma unroll
    for (uint32_t u = 0; u < 2u; ++u) {
        const uint64_t r = base + 2u * tid + u;
        l[u] = r < a.n_rows ? a.len[r] : 0u;
        mine += l[u];
    }
    BlockWriter<uint32_t> w(mine, scr, a.blk_off, a.text, a.text_cap);
    w.stage_if(w.tot <= kSwTextStage, stage);
    uint32_t at = w.rel;
    bool bad = false;
#pragma unroll
    for (uint32_t u = 0; u < 2u; ++u) {
        const uint64_t r = base + 2u * tid + u;
        if (r >= a.n_rows) break;
        w.put(at, [&](char *p) {
            RowOut<true> o{p};
            sw_row_text<true, kDg>(a, r, o, bad, sw_dg_col(a));
        });
        at += l[u];
    }
    w.flush();
}

// where every selected ctg's text begins: the bytes of the rows in front of its first row
__global__ __launch_bounds__(64) void sw_text_ctg_kernel(const SwTextArgs a) {
    const uint32_t k = blockIdx.x, lane = threadIdx.x;
    if (k > a.n_sel) return;
    const uint64_t r = a.ctg_row_off[k];                 // (entry n_sel = all rows)
    const uint64_t b = r / kSwTextBlock;
    unsigned long long off = 0;
    for (uint64_t q = b * kSwTextBlock + lane; q < r; q += 64u) off += a.len[q];
    for (int d = 32; d; d >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)off, d, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(off >> 32), d, 64);
        off += ((unsigned long long)hi << 32) | lo;
    }
    if (lane == 0) a.words[2u + k] = (b < a.nb ? a.blk_off[b] : a.blk_off[a.nb]) + off;
}

// ---- the row offsets of gams_gpu_sw_feature_text, made on the device (what sw_host_rows walks on the host) -------------
// 1 + n_l + n_r of every feature (window.rs:29-41) and their sum per workgroup, carried in 64 bits: 256 features of
// 1 + 2 * max rows each pass 2^32 from max = 2^23 on
__global__ __launch_bounds__(256) void sw_geom_kernel(const SwCtg *ctgs, const uint32_t *fctg, const int32_t *fs,
                                                      const int32_t *fe, uint32_t nf, int32_t size, int32_t max,
                                                      uint32_t *cnt, unsigned long long *blk) {
    __shared__ uint64_t ws[4];
    const uint32_t f = blockIdx.x * 256u + threadIdx.x;
    uint32_t n = 0;
    if (f < nf) {
        const SwCtg cg = ctgs[fctg[f]];
        const SwGeom g = sw_geometry(cg.chr_start, cg.chr_end, fs[f], fe[f], size, max);
        n = 1u + (uint32_t)g.n_l + (uint32_t)g.n_r;
        cnt[f] = n;
    }
    uint64_t tot;
    (void)block_excl_scan_256<uint64_t>((uint64_t)n, ws, tot);
    if (threadIdx.x == 0u) blk[blockIdx.x] = tot;
}

// row_off[f] = the rows in front of feature f: the workgroup's prefix + the scan inside it; row_off[nf] = all rows
__global__ __launch_bounds__(256) void sw_row_off_kernel(const uint32_t *cnt, const unsigned long long *blk_off, uint32_t nf,
                                                         uint32_t nb, unsigned long long *row_off) {
    __shared__ uint64_t ws[4];
    const uint32_t f = blockIdx.x * 256u + threadIdx.x;
    uint64_t tot;
    const uint64_t rel = block_excl_scan_256<uint64_t>(f < nf ? (uint64_t)cnt[f] : 0ull, ws, tot);
    if (f < nf) row_off[f] = blk_off[blockIdx.x] + rel;
    if (f == 0u) row_off[nf] = blk_off[nb];
}

// the first row of every interval (entry n_ctg = all rows): bucket_off[i] <= nf indexes row_off[nf + 1]
__global__ __launch_bounds__(256) void sw_ctg_row_off_kernel(const unsigned long long *row_off, const unsigned long long *bucket_off,
                                                             uint32_t n_ctg, unsigned long long *ctg_row_off) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i <= n_ctg) ctg_row_off[i] = row_off[bucket_off[i]];
}

// ---- the stored rows as the columns of the ΔG kernel (dg.hip): where the bases of row r's window begin in the seqset's
// buffer, and how many they are.  Row r belongs to the last feature whose first row is <= r (every feature has its M row).
__global__ __launch_bounds__(256) void sw_dg_cols_kernel(const gams_sw_row_t *rows, uint64_t n_rows, const SwCtg *ctgs,
                                                         const uint32_t *fctg, const uint64_t *row_off, uint32_t nf,
                                                         unsigned long long *off, uint32_t *len) {
    const uint64_t r = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (r >= n_rows) return;
    uint32_t lo = 0, hi = nf;
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (row_off[mid] <= r)
            lo = mid;
        else
            hi = mid;
    }
    const SwCtg cg = ctgs[fctg[lo]];
    const gams_sw_row_t w = rows[r];
    // (a window lies inside its ctg and has at most `size` <= 65535 bases: anything else would read no byte and answer NaN)
    const bool inside = w.start >= cg.chr_start && w.end <= cg.chr_end && w.end >= w.start && w.end - w.start < 65535;
    off[r] = cg.seq_off + (inside ? (uint64_t)((int64_t)w.start - cg.chr_start) : 0ull);
    len[r] = inside ? (uint32_t)(w.end - w.start + 1) : 0u;
}

struct SwTextReq {                       // what the text entries add to a batch call
    const char *const *chr;              // per selected ctg
    const char *const *feat_id;          // per feature
    const char **text;
    uint64_t *text_bytes;
    const uint64_t **ctg_off;
};

// One call of the batch entries.  What it is asked for: the rows (gams_gpu_sw_batch) or the counts (gams_gpu_sw_count_batch)
// in the caller's array, the rows as text (the text entries) or the rows added into call.summary (the summary entries).
// With dg_table a call also computes the ΔG of every stored row's window: Dg hands the values to the
// caller's array (gams_gpu_sw_dg_batch), Text prints them as the tenth field (gams_gpu_sw_text_dg).
enum class SwMode { Rows, Counts, Text, Summary, Dg };
struct SwReq {
    SwMode mode;
    gams_gpu_t *h;
    gams_seqset_t *s;
    uint32_t n_sel;
    const uint32_t *ctg_index;
    const int32_t *chr_start;
    const uint64_t *feat_off;
    const int32_t *feat_start, *feat_end;
    SwCall call;                         // (rg_group, set_group: per selected ctg)
    uint64_t *n_rows;                    // what every entry passes; below, what the entry of a mode names besides
    gams_sw_row_t *rows = nullptr;       // Rows, Counts: the caller's array of `cap` entries and the first row of every ctg
    int32_t *count = nullptr;
    uint64_t cap = 0;
    uint64_t *row_off = nullptr;
    SwTextReq tx{};                      // Text
    const gams_dg_table_t *dg_table = nullptr;   // Dg, and Text with the ΔG column: the call's terms ...
    float *dg = nullptr;                 // ... Dg: the caller's array of `cap` entries
    SwReq(SwMode mode_, gams_gpu_t *h_, gams_seqset_t *s_, uint32_t n_sel_, const uint32_t *ctg_index_, const int32_t *chr_start_,
          const uint64_t *feat_off_, const int32_t *feat_start_, const int32_t *feat_end_, const SwCall &call_, uint64_t *n_rows_)
        : mode(mode_), h(h_), s(s_), n_sel(n_sel_), ctg_index(ctg_index_), chr_start(chr_start_), feat_off(feat_off_),
          feat_start(feat_start_), feat_end(feat_end_), call(call_), n_rows(n_rows_) {}
    // only *n_rows and row_off are wanted: neither text nor summary, and no array to fill or no room in it
    bool size_query() const {
        if (mode == SwMode::Dg) return !dg || !cap;
        return mode == SwMode::Rows ? !rows || !cap : mode == SwMode::Counts && (!count || !cap);
    }
};

using SwCols = SwStage<SwCtg>;
const std::string kSw = "gpu_sw", kSwText = "gpu_sw_text", kRangeGc = "gpu_range_gc", kSwSum = "gpu_sw_summary";

}  // namespace

// the selected ctgs of a batch call (sw and the range batches): every index names a ctg of a length the kernels carry, and
// `off` (named `off_name` in the messages) begins at 0 and does not decrease
int gams_sw_check_selection(gams_gpu_t *h, const std::string &who, const char *off_name, const gams_seqset_t *s, uint32_t n_sel,
                            const uint32_t *ctg_index, const uint64_t *off) {
    if (off[0] != 0) return gams_fail(h, GAMS_EINVAL, who + ": " + off_name + "[0] must be 0");
    for (uint32_t k = 0; k < n_sel; ++k) {
        if (ctg_index[k] >= s->n_ctg) return gams_fail(h, GAMS_EINVAL, who + ": ctg index out of range");
        if (off[k + 1] < off[k]) return gams_fail(h, GAMS_EINVAL, who + ": " + off_name + " must not decrease");
        const uint32_t len = s->len[ctg_index[k]];
        if (len == 0 || len > 0x7fffffffu) return gams_fail(h, GAMS_EINVAL, who + ": ctg length out of range");
    }
    return GAMS_OK;
}

namespace {
// 1. the arguments; *nf = the features of the call, 0 with GAMS_OK: nothing to do
int sw_check(const SwReq &q, uint32_t *nf) {
    gams_gpu_t *h = q.h;
    *nf = 0;
    if (!h || !q.s || !q.n_rows || (q.n_sel && (!q.ctg_index || !q.chr_start || !q.feat_off)))
        return gams_fail(h, GAMS_EINVAL, "gpu_sw: null argument");
    int rc = gams_sw_call_check(h, kSw, q.call, SWC_WINDOW, q.n_sel);
    if (rc != GAMS_OK) return rc;
    *q.n_rows = 0;
    if (q.row_off)
        for (uint32_t k = 0; k <= q.n_sel; ++k) q.row_off[k] = 0;
    if (q.n_sel == 0) return GAMS_OK;
    if ((rc = gams_sw_check_selection(h, kSw, "feat_off", q.s, q.n_sel, q.ctg_index, q.feat_off)) != GAMS_OK) return rc;
    const uint64_t nf64 = q.feat_off[q.n_sel];
    if (nf64 == 0) return GAMS_OK;
    if (!q.feat_start || !q.feat_end) return gams_fail(h, GAMS_EINVAL, "gpu_sw: null argument");
    if ((rc = gams_sw_call_check(h, kSw, q.call, SWC_MAX | SWC_SLOTS, q.n_sel, true, nf64)) != GAMS_OK) return rc;
    *nf = (uint32_t)nf64;
    return GAMS_OK;
}

// 2. the rows of every feature from the closed form (window.rs:29-41) -> exclusive offsets in in.row_off, the first row
// of every selected ctg in crow (and q.row_off), and the kernel's inputs where `in` has them (a size query has none)
int sw_host_rows(const SwReq &q, uint32_t nf, const SwCols &in, std::vector<uint64_t> &crow, uint64_t *n_rows) {
    const SwCall &c = q.call;
    uint64_t tot = 0;
    for (uint32_t k = 0; k < q.n_sel; ++k) {
        const uint32_t i = q.ctg_index[k];
        const int32_t cs = q.chr_start[k], ce = cs + (int32_t)q.s->len[i] - 1;
        if (q.row_off) q.row_off[k] = tot;
        crow[k] = tot;
        if (in.ctgs)
            in.ctgs[k] = SwCtg{q.s->off[i], q.s->len[i], cs, ce, (uint32_t)q.feat_off[k], c.count() ? c.rg_group[k] : UINT32_MAX, 0u};
        for (uint64_t f = q.feat_off[k]; f < q.feat_off[k + 1]; ++f) {
            // window.rs:98-110: the middle pair of the feature must be members of the ctg span --
            // IntSpan::index of a non-member has no defined answer in the reference to mirror
            const int64_t flen = (int64_t)q.feat_end[f] - q.feat_start[f] + 1, half = flen / 2;
            const int64_t mid_l = half == 0 ? q.feat_start[f] : (int64_t)q.feat_start[f] + half - 1;
            const int64_t mid_r = half == 0 ? q.feat_start[f] : (int64_t)q.feat_start[f] + half;
            if (flen < 1 || mid_l < cs || mid_r > ce)
                return gams_fail(q.h, GAMS_EINVAL, "gpu_sw: feature " + std::to_string(f - q.feat_off[k]) +
                                                       (q.n_sel > 1 ? " of selected ctg " + std::to_string(k) : std::string()) +
                                                       " is empty or has its middle outside the ctg");
            in.row_off[f] = tot;
            const SwGeom g = sw_geometry(cs, ce, q.feat_start[f], q.feat_end[f], c.size, c.max);
            tot += 1u + (uint64_t)g.n_l + (uint64_t)g.n_r;
            if (in.fs) {
                in.fs[f] = q.feat_start[f];
                in.fe[f] = q.feat_end[f];
                in.fctg[f] = k;
            }
        }
    }
    in.row_off[nf] = tot;
    if (q.row_off) q.row_off[q.n_sel] = tot;
    crow[q.n_sel] = tot;
    *n_rows = tot;
    return GAMS_OK;
}

// The sets of a summarising call for the kernel: the set_group columns (n_cols entries each, the caller's host arrays) on
// the device through one page-locked block, and the tables of every gams_spans_t.  Lives until the call has drained.
struct SwAnnoStage {
    PoolBlock dev, pin;
    SwAnno an{};
    explicit SwAnnoStage(gams_gpu_t *h) : dev(h, false), pin(h, true) {}
    const SwAnno *staged() const { return an.n ? &an : nullptr; }   // what sw_launch takes (NULL: no set)
    // the one place the sets of a call are staged; a call without a summary or without sets stages nothing
    int put(gams_gpu_t *h, const SwCall &c, uint32_t n_cols) {
        const uint32_t n = c.summary ? c.n_anno : 0u;
        if (!n) return GAMS_OK;
        const size_t col = gams_align256((size_t)std::max(n_cols, 1u) * 4);
        GAMS_TRY(h, kSwSum, pin.alloc(col * n));
        GAMS_TRY(h, kSwSum, dev.alloc(col * n));
        for (uint32_t a = 0; a < n; ++a) {
            const gams_spans_t *set = c.sets[a];
            std::memcpy(pin.p + a * col, c.set_group[a], (size_t)n_cols * 4);
            an.set[a] = SwAnnoOne{set->d_groups, set->d_rec, set->d_dir_lo, set->d_cells,
                                  reinterpret_cast<const uint32_t *>(dev.p + a * col), set->n_groups, 0u};
        }
        GAMS_TRY(h, kSwSum, hipMemcpyAsync(dev.p, pin.p, col * n, hipMemcpyHostToDevice, h->compute));
        an.n = n;
        an.prop = c.summary->d_call + ((size_t)c.summary->max + 1) * kSumWords + 1;   // behind the call's table and its flag word
        return GAMS_OK;
    }
};

// The twelve instantiations, named here and nowhere else: entry SwCall::variant() of the storing, the summarising and the
// summarising kernel with span sets; and their one launch, 256 threads a workgroup
using SwKernel = void (*)(SwArgs);
using SwAnnoKernel = void (*)(SwArgs, SwAnno);
const SwKernel kSwStoring[4] = {sw_kernel<false, false>, sw_kernel<false, true>, sw_kernel<true, false>, sw_kernel<true, true>};
const SwKernel kSwSumming[4] = {sw_kernel<false, false, true>, sw_kernel<false, true, true>, sw_kernel<true, false, true>,
                                sw_kernel<true, true, true>};
const SwAnnoKernel kSwSummingSets[4] = {sw_anno_kernel<false, false>, sw_anno_kernel<false, true>, sw_anno_kernel<true, false>,
                                        sw_anno_kernel<true, true>};
template <typename... A>
void sw_run(void (*const *table)(A...), const SwCall &c, dim3 grid, hipStream_t st, const A &...a) {
    hipLaunchKernelGGL(table[c.variant()], grid, dim3(256), 0, st, a...);
}

// 3'. the summarising kernel: the call's table zeroed, the rows added into it, the table merged into the tag's groups
// unless the flag word behind it was raised; one read-back, of that word
int sw_sum_launch(gams_gpu_t *h, const SwCall &c, SwArgs &a, dim3 grid, const SwAnno *an) {
    gams_sw_summary_t *sum = c.summary;
    const uint32_t words = ((uint32_t)sum->max + 1u) * kSumWords;
    a.sum = sum->d_call;
    a.sum_bad = sum->d_call + words;
    a.sum_chunks = grid.x;                                     // what the storing kernel launches, walked by ...
    grid.x = std::min<uint32_t>(grid.x, 8u * (uint32_t)std::max(h->cus, 1));   // ... the workgroups a device holds at once
    hipStream_t st = h->compute;
    const uint32_t pwords = ((uint32_t)sum->max + 1u) * sum->n_anno;
    GAMS_TRY(h, kSwSum, hipMemsetAsync(sum->d_call, 0, ((size_t)words + 1 + pwords) * 8, st));
    if (an) {                                                  // (sum->n_anno sets: the entries checked)
        sw_run(kSwSummingSets, c, grid, st, a, *an);
        hipLaunchKernelGGL(sw_sum_merge_kernel, dim3((pwords + 255u) / 256u), dim3(256), 0, st, an->prop, a.sum_bad,
                           sum->d_prop + (size_t)c.tag * pwords, pwords);
    } else
        sw_run(kSwSumming, c, grid, st, a);
    hipLaunchKernelGGL(sw_sum_merge_kernel, dim3((words + 255u) / 256u), dim3(256), 0, st, sum->d_call, a.sum_bad,
                       sum->d_acc + (size_t)c.tag * words, words);
    GAMS_TRY(h, kSwSum, hipGetLastError());
    return GAMS_OK;
}
// ... and the verdict, once the stream has run (the caller's stage mark may lie in between)
int sw_sum_verdict(gams_gpu_t *h, const gams_sw_summary_t *sum) {
    const uint32_t words = ((uint32_t)sum->max + 1u) * kSumWords;
    GAMS_TRY(h, kSwSum, hipMemcpyAsync(h->pin_scratch, sum->d_call + words, 8, hipMemcpyDeviceToHost, h->compute));
    GAMS_TRY(h, kSwSum, hipStreamSynchronize(h->compute));
    if (h->pin_scratch[0])
        return gams_fail(h, GAMS_EUNSUPPORTED, kSwSum + ": a statistic of 1000 or more (or below 0): summarise gams_gpu_sw_batch's "
                                                        "rows on the host");
    return GAMS_OK;
}

// 3. the kernel over the uploaded inputs `d`: n_out rows (and counts), or every row into c.summary (`an`: its staged sets)
int sw_launch(gams_gpu_t *h, const SwCall &c, const gams_seqset_t *s, uint32_t nf, uint64_t n_out, const SwCols &d,
              gams_sw_row_t *d_rows, int32_t *d_cnt, const SwAnno *an) {
    SwArgs a{};
    if (c.gc()) {
        a.pm = s->gcindex->d_pm;
        a.seg = s->gcindex->d_seg;
    }
    if (c.count()) {
        a.cgroups = c.rg_ix->d_cgroups;
        a.rg_starts = c.rg_ix->d_lstart;
        a.rg_stops = c.rg_ix->d_stops;
        a.bk_start = c.rg_ix->d_bk_start;
        a.bk_stop = c.rg_ix->d_bk_stop;
        a.n_groups = c.rg_ix->n_groups;
        a.cnt = d_cnt;
    }
    a.ctgs = d.ctgs;
    a.fs = d.fs;
    a.fe = d.fe;
    a.fctg = d.fctg;
    a.row_off = d.row_off;
    a.nf = nf;
    a.size = c.size;
    a.max = c.max;
    a.resize = c.resize;
    a.rows = d_rows;
    a.cap = n_out;
    const dim3 grid((unsigned)(((uint64_t)nf * (1u + 2u * (uint64_t)c.max) + 255) / 256));
    GAMS_TRY(h, kSw, hipEventRecord(h->k0, h->compute));
    if (c.summary) {
        const int rc = sw_sum_launch(h, c, a, grid, an);
        if (rc != GAMS_OK) return rc;
    } else
        sw_run(kSwStoring, c, grid, h->compute, a);
    GAMS_TRY(h, kSw, hipGetLastError());
    GAMS_TRY(h, kSw, hipEventRecord(h->k1, h->compute));
    h->k_valid = true;
    h->kq_used = 0;
    return GAMS_OK;
}

// the chromosome names and the feature ids of a text call, each as one blob with its offsets, and the longest of each
struct SwTextBlobs {
    std::vector<uint32_t> name_off, id_off;
    std::string names, ids;
    size_t max_name = 0, max_id = 0;
};
int sw_text_blobs(const SwReq &q, uint32_t nf, SwTextBlobs &b) {
    const SwTextReq *tx = &q.tx;
    b.name_off.resize((size_t)q.n_sel + 1);
    b.id_off.resize((size_t)nf + 1);
    for (uint32_t k = 0; k < q.n_sel; ++k) {
        b.name_off[k] = (uint32_t)b.names.size();
        if (!tx->chr[k]) return gams_fail(q.h, GAMS_EINVAL, "gpu_sw_text: null chromosome name");
        const size_t before = b.names.size();
        b.names += tx->chr[k];
        b.max_name = std::max(b.max_name, b.names.size() - before);
    }
    b.name_off[q.n_sel] = (uint32_t)b.names.size();
    for (uint32_t f = 0; f < nf; ++f) {
        b.id_off[f] = (uint32_t)b.ids.size();
        if (!tx->feat_id[f] || b.ids.size() > 0xF0000000ull)
            return gams_fail(q.h, GAMS_EINVAL, "gpu_sw_text: null feature id, or more than 4 GB of ids");
        const size_t before = b.ids.size();
        b.ids += tx->feat_id[f];
        b.max_id = std::max(b.max_id, b.ids.size() - before);
    }
    b.id_off[nf] = (uint32_t)b.ids.size();
    return GAMS_OK;
}

// The back half of both text paths.  sw_text_cols carves what it writes -- row lengths | block lengths and offsets |
// words | text -- behind whatever the caller carved in front, for n_rows rows of at most per_row bytes each in n_sel
// ctgs.  sw_text_tail then queues the length of every row, the blocks' prefix, the rows at their offsets and the first
// byte of every ctg, and reads back the words (total, flag, per-ctg offsets), which say the text's size, and the text into
// the handle's page-locked buffer, valid until the next call.  `ta` comes with its sources filled as well (the rows, the
// ctgs, the row offsets, the ids and names of either kind, gc, cnt).  `stage`, where given, records SWF_TLEN and
// SWF_TWRITE; `advice` ends the refusal's message.
void sw_text_cols(Carver &c, SwTextArgs &ta, uint64_t n_rows, uint32_t n_sel, uint64_t per_row) {
    ta.n_rows = n_rows;
    ta.n_sel = n_sel;
    ta.nb = (uint32_t)((n_rows + kSwTextBlock - 1) / kSwTextBlock);
    ta.text_cap = std::max<uint64_t>(n_rows * per_row, 4096);
    ta.len = c.take<uint32_t>(std::max<uint64_t>(n_rows, 1));
    ta.blk_len = c.take<uint32_t>(std::max(ta.nb, 1u));
    ta.blk_off = c.take<unsigned long long>((size_t)ta.nb + 1);
    ta.words = c.take<unsigned long long>((size_t)n_sel + 3);
    ta.text = c.take<char>(ta.text_cap);
}
// ... and the sources both paths fill alike: the call's rows and counts on the device, their ctgs, the first row of every feature
void sw_text_rows(SwTextArgs &ta, const SwCall &c, const SwCols &d, const gams_sw_row_t *d_rows, const int32_t *d_cnt) {
    ta.rows = d_rows;
    ta.ctgs = d.ctgs;
    ta.feat_row_off = d.row_off;
    ta.gc = c.gc() ? 1u : 0u;
    ta.cnt = d_cnt;
}
struct SwText {
    const char *text;                  // nullptr: no byte
    uint64_t bytes;
    const unsigned long long *words;   // [2 + k] = the first byte of ctg k, [2 + n_sel] = bytes
};
// `dg`, where given: the ΔG of every row on the device, printed as the tenth field (the kernels with the column).
int sw_text_tail(gams_gpu_t *h, const std::string &who, const char *advice, const SwTextArgs &ta, const StageClock *stage,
                 SwText *out, const float *dg = nullptr) {
    hipStream_t st = h->compute;
    const uint32_t nb = ta.nb, n_sel = ta.n_sel;
    const uint64_t text_cap = ta.text_cap;
    const size_t n_words = (size_t)n_sel + 3;
    GAMS_TRY(h, who, hipMemsetAsync(ta.words, 0, gams_align256(n_words * 8), st));
    if (stage) GAMS_TRY(h, who, (*stage)(SWF_TLEN, true));
    const SwTextDgArgs tda{ta, dg};
    if (nb) {
        if (dg)
            hipLaunchKernelGGL(sw_text_len_kernel<SwTextDgArgs>, dim3(nb), dim3(256), 0, st, tda);
        else
            hipLaunchKernelGGL(sw_text_len_kernel<SwTextArgs>, dim3(nb), dim3(256), 0, st, ta);
        hipLaunchKernelGGL(blk_offsets_scan_kernel<uint32_t>, dim3(1), dim3(1024), 0, st, ta.blk_len, nb, ta.blk_off, ta.words, 0u);
    }
    if (stage) {
        GAMS_TRY(h, who, (*stage)(SWF_TLEN, false));
        GAMS_TRY(h, who, (*stage)(SWF_TWRITE, true));
    }
    if (nb) {
        if (dg)
            hipLaunchKernelGGL(sw_text_write_kernel<SwTextDgArgs>, dim3(nb), dim3(256), 0, st, tda);
        else
            hipLaunchKernelGGL(sw_text_write_kernel<SwTextArgs>, dim3(nb), dim3(256), 0, st, ta);
        hipLaunchKernelGGL(sw_text_ctg_kernel, dim3(n_sel + 1), dim3(64), 0, st, ta);
    }
    GAMS_TRY(h, who, hipGetLastError());
    if (stage) GAMS_TRY(h, who, (*stage)(SWF_TWRITE, false));
    GAMS_TRY(h, who, gams_pool_grow(h, true, &h->sw_words, &h->sw_words_bytes, n_words * 8, n_words * 8));
    GAMS_TRY(h, who, hipMemcpyAsync(h->sw_words, ta.words, n_words * 8, hipMemcpyDeviceToHost, st));
    GAMS_TRY(h, who, hipStreamSynchronize(st));
    const uint64_t bytes = h->sw_words[0];
    if (h->sw_words[1] != 0 || bytes > text_cap)
        return gams_fail(h, GAMS_EUNSUPPORTED, who + ": a value this formatter does not cover (a statistic of 1000 or more, a "
                                                     "negative coordinate" + (dg ? ", a dG of 2^20 or more" : "") + "): " + advice);
    GAMS_TRY(h, who, gams_pool_grow(h, true, &h->sw_text, &h->sw_text_bytes, bytes, bytes + bytes / 8 + 4096));
    if (bytes) GAMS_TRY(h, who, hipMemcpyAsync(h->sw_text, ta.text, bytes, hipMemcpyDeviceToHost, st));
    GAMS_TRY(h, who, hipStreamSynchronize(st));
    *out = SwText{bytes ? h->sw_text : nullptr, bytes, h->sw_words};
    return GAMS_OK;
}

// 4. (text entries) the n_out rows on the device -> TSV text in the handle's page-locked buffer
int sw_rows_to_text(const SwReq &q, uint32_t nf, uint64_t n_out, const std::vector<uint64_t> &crow, const SwCols &d,
                    const gams_sw_row_t *d_rows, const int32_t *d_cnt, const float *d_dg) {
    gams_gpu_t *h = q.h;
    const SwTextReq *tx = &q.tx;
    const uint32_t n_sel = q.n_sel;
    SwTextBlobs B;
    const int rc = sw_text_blobs(q, nf, B);
    if (rc != GAMS_OK) return rc;
    // (the tenth field: a tab and at most kGamsDg4MaxLen bytes)
    const uint64_t per_row = B.max_id + B.max_name + (q.call.count() ? 112 : 96) + (d_dg ? 1u + kGamsDg4MaxLen : 0u);
    auto tabs = [&](Carver &c) { return sw_text_tabs_layout(c, n_sel, nf, B.names.size(), B.ids.size()); };
    SwTextArgs ta{};
    auto dev = [&](Carver &c) {   // tables | what the tail writes
        const SwTextTabs t = tabs(c);
        ta.ctg_row_off = t.ctg_row_off;
        ta.name_off = t.name_off;
        ta.names = t.names;
        ta.id_off = t.id_off;
        ta.ids = t.ids;
        sw_text_cols(c, ta, n_out, n_sel, per_row);
    };
    const size_t tab_bytes = layout_bytes(tabs);
    PoolBlock tdev(h, false), tpin(h, true);
    GAMS_TRY(h, kSwText, tpin.alloc(tab_bytes));
    GAMS_TRY(h, kSwText, tdev.alloc(layout_bytes(dev)));
    const SwTextTabs ht = carve(tpin.p, tabs);
    std::memcpy(ht.ctg_row_off, crow.data(), crow.size() * 8);
    std::memcpy(ht.name_off, B.name_off.data(), B.name_off.size() * 4);
    std::memcpy(ht.names, B.names.data(), B.names.size());
    std::memcpy(ht.id_off, B.id_off.data(), B.id_off.size() * 4);
    std::memcpy(ht.ids, B.ids.data(), B.ids.size());
    GAMS_TRY(h, kSwText, hipMemcpyAsync(tdev.p, tpin.p, tab_bytes, hipMemcpyHostToDevice, h->compute));
    carve(tdev.p, dev);
    sw_text_rows(ta, q.call, d, d_rows, d_cnt);
    SwText T{};
    const int rt = sw_text_tail(h, kSwText, "format gams_gpu_sw_batch's rows on the host", ta, nullptr, &T, d_dg);
    if (rt != GAMS_OK) return rt;
    *tx->text = T.text;
    *tx->text_bytes = T.bytes;
    if (tx->ctg_off) *tx->ctg_off = reinterpret_cast<const uint64_t *>(T.words + 2);
    return GAMS_OK;
}

int sw_batch_impl(const SwReq &q) {
    gams_gpu_t *h = q.h;
    const SwCall &c = q.call;
    const bool text = q.mode == SwMode::Text, summary = q.mode == SwMode::Summary;
    uint32_t nf = 0;
    int rc = sw_check(q, &nf);
    if (rc != GAMS_OK || nf == 0) return rc;
    GAMS_HIP(h, hipSetDevice(h->device));
    // Inputs are assembled in one page-locked block (one DMA): ctgs | fs | fe | fctg | off (| the ΔG terms)
    const bool want_dg = q.dg_table != nullptr;
    struct Inputs {
        SwCols cols;
        gams_dg_table_t *tab;            // the ΔG terms of the block carved (nullptr without the column)
    };
    auto inputs = [&](Carver &cv) {
        Inputs i{};
        i.cols = sw_stage_layout<SwCtg>(cv, q.n_sel, nf, true);
        i.tab = want_dg ? cv.take<gams_dg_table_t>(1) : nullptr;
        return i;
    };
    const size_t in_bytes = layout_bytes(inputs);
    const bool size_query = q.size_query();
    PoolBlock dev(h, false), pin(h, true);
    std::vector<uint64_t> crow((size_t)q.n_sel + 1, 0);    // first row of every selected ctg (text mode)
    std::vector<uint64_t> off_host(size_query ? (size_t)nf + 1 : 0);   // a size query: no device, no pinned memory
    SwCols in{};
    in.row_off = off_host.data();
    if (!size_query) {
        GAMS_TRY(h, kSw, pin.alloc(in_bytes));
        const Inputs pinned = carve(pin.p, inputs);
        in = pinned.cols;
        if (want_dg) *pinned.tab = *q.dg_table;
    }
    uint64_t tot = 0;
    if ((rc = sw_host_rows(q, nf, in, crow, &tot)) != GAMS_OK) return rc;
    *q.n_rows = tot;
    if (size_query) return GAMS_OK;
    // the counts and the geometry read no sequence byte: a count-only call leaves the bytes alone
    if (c.gc() && (rc = gams_seqset_gcindex(h, q.s)) != GAMS_OK) return rc;
    if (want_dg && (rc = gams_dg_seq_ready(h, q.s)) != GAMS_OK) return rc;
    // text mode: every row, kept on the device; the summary stores none
    const uint64_t n_out = summary ? 0 : std::min<uint64_t>(tot, text ? tot : q.cap);
    if (want_dg && n_out > 0x7fffff00ull) return gams_fail(h, GAMS_EUNSUPPORTED, "gpu_sw: too many rows for one ΔG launch");
    SwCols d{};
    gams_sw_row_t *d_rows = nullptr;
    int32_t *d_cnt = nullptr;
    unsigned long long *d_dg_off = nullptr;
    uint32_t *d_dg_len = nullptr;
    float *d_dg = nullptr;
    const gams_dg_table_t *d_tab = nullptr;
    auto device = [&](Carver &cv) {   // the inputs | rows | counts (| the ΔG kernel's columns and its values)
        const Inputs i = inputs(cv);
        d = i.cols;
        d_tab = i.tab;
        d_rows = cv.take_tight<gams_sw_row_t>(std::max<uint64_t>(n_out, 1));
        d_cnt = c.count() ? cv.take<int32_t>(std::max<uint64_t>(n_out, 1)) : nullptr;
        if (want_dg) {
            (void)cv.step(gams_align256(cv.off) - cv.off);   // (the rows are carved tight: back onto a 256-B slot)
            d_dg_off = cv.take<unsigned long long>(std::max<uint64_t>(n_out, 1));
            d_dg_len = cv.take<uint32_t>(std::max<uint64_t>(n_out, 1));
            d_dg = cv.take<float>(std::max<uint64_t>(n_out, 1));
        }
    };
    GAMS_TRY(h, kSw, dev.alloc(layout_bytes(device)));
    carve(dev.p, device);
    GAMS_TRY(h, kSw, hipMemcpyAsync(dev.p, pin.p, in_bytes, hipMemcpyHostToDevice, h->compute));
    SwAnnoStage sets(h);
    if ((rc = sets.put(h, c, q.n_sel)) != GAMS_OK) return rc;
    if ((rc = sw_launch(h, c, q.s, nf, n_out, d, d_rows, d_cnt, sets.staged())) != GAMS_OK) return rc;
    if (summary) return sw_sum_verdict(h, c.summary);
    if (want_dg && n_out) {   // 3''. the windows' bytes from the stored rows, and their ΔG
        hipLaunchKernelGGL(sw_dg_cols_kernel, dim3((unsigned)((n_out + 255) / 256)), dim3(256), 0, h->compute, d_rows, n_out,
                           d.ctgs, d.fctg, d.row_off, nf, d_dg_off, d_dg_len);
        gams_launch_dg(h, q.s, d_dg_off, d_dg_len, (uint32_t)n_out, d_tab, d_dg);
        GAMS_TRY(h, kSw, hipGetLastError());
    }
    if (text) return sw_rows_to_text(q, nf, n_out, crow, d, d_rows, d_cnt, d_dg);
    // 5. read back
    if (q.rows) GAMS_TRY(h, kSw, hipMemcpyAsync(q.rows, d_rows, n_out * sizeof(gams_sw_row_t), hipMemcpyDeviceToHost, h->compute));
    if (q.count) GAMS_TRY(h, kSw, hipMemcpyAsync(q.count, d_cnt, n_out * sizeof(int32_t), hipMemcpyDeviceToHost, h->compute));
    if (q.dg) GAMS_TRY(h, kSw, hipMemcpyAsync(q.dg, d_dg, n_out * sizeof(float), hipMemcpyDeviceToHost, h->compute));
    GAMS_TRY(h, kSw, hipStreamSynchronize(h->compute));
    return GAMS_OK;
}
}  // namespace

int gams_launch_sw_cols(gams_gpu_t *h, const SwColsJob &J, const char **text, uint64_t *text_bytes, uint64_t *text_off,
                        uint64_t *n_rows) {
    const SwCall &call = J.call;
    const std::string who = call.summary ? "gpu_sw_feature_summary" : "gpu_sw_feature_text";
    const uint32_t n_ctg = J.n_ctg, nf = J.nf;
    hipStream_t st = h->compute;
    const StageClock stage{h, st};
    // the interval table: a few KB, one copy
    const uint32_t nbf = (nf + 255u) / 256u;
    SwCtg *d_ctgs = nullptr;
    uint32_t *d_cnt_f = nullptr;
    unsigned long long *d_blk = nullptr, *d_blk_off = nullptr, *d_row_off = nullptr, *d_ctg_row_off = nullptr;
    auto geom = [&](Carver &c) {   // ctgs | rows per feature | block sums and prefix | row_off | ctg_row_off
        d_ctgs = c.take<SwCtg>(std::max(n_ctg, 1u));
        d_cnt_f = c.take<uint32_t>(nf);
        d_blk = c.take<unsigned long long>((size_t)nbf + 1);
        d_blk_off = c.take<unsigned long long>((size_t)nbf + 1);
        d_row_off = c.take<unsigned long long>((size_t)nf + 1);
        d_ctg_row_off = c.take<unsigned long long>((size_t)n_ctg + 1);
    };
    PoolBlock g_dev(h, false), g_pin(h, true), r_dev(h, false), t_dev(h, false);
    GAMS_TRY(h, who, g_dev.alloc(layout_bytes(geom)));
    GAMS_TRY(h, who, g_pin.alloc(gams_align256(std::max(n_ctg, 1u) * sizeof(SwCtg))));
    carve(g_dev.p, geom);
    SwCtg *const h_ctgs = reinterpret_cast<SwCtg *>(g_pin.p);
    for (uint32_t i = 0; i < n_ctg; ++i) {
        const uint32_t slot = call.gc() ? J.ctg_index[i] : UINT32_MAX;
        const bool has = slot != UINT32_MAX && J.bucket_off[i + 1] > J.bucket_off[i];   // (checked by the caller)
        h_ctgs[i] = SwCtg{has ? J.s->off[slot] : 0ull,
                          has ? J.s->len[slot] : (uint32_t)((int64_t)J.chr_end[i] - J.chr_start[i] + 1),
                          J.chr_start[i], J.chr_end[i], (uint32_t)J.bucket_off[i], call.count() ? call.rg_group[i] : UINT32_MAX, 0u};
    }
    GAMS_TRY(h, who, hipMemcpyAsync(d_ctgs, h_ctgs, (size_t)n_ctg * sizeof(SwCtg), hipMemcpyHostToDevice, st));
    // 2. geometry: rows per feature -> row_off, ctg_row_off
    GAMS_TRY(h, who, stage(SWF_GEOM, true));
    hipLaunchKernelGGL(sw_geom_kernel, dim3(nbf), dim3(256), 0, st, d_ctgs, J.fctg, J.fs, J.fe, nf, call.size, call.max, d_cnt_f, d_blk);
    hipLaunchKernelGGL(blk_offsets_scan_kernel<unsigned long long>, dim3(1), dim3(1024), 0, st, d_blk, nbf, d_blk_off, J.words, 0u);
    if (!call.summary) {   // (the summary asks where no row lies)
        hipLaunchKernelGGL(sw_row_off_kernel, dim3(nbf), dim3(256), 0, st, d_cnt_f, d_blk_off, nf, nbf, d_row_off);
        hipLaunchKernelGGL(sw_ctg_row_off_kernel, dim3(n_ctg / 256u + 1u), dim3(256), 0, st, d_row_off, J.d_bucket_off, n_ctg,
                           d_ctg_row_off);
    }
    GAMS_TRY(h, who, hipGetLastError());
    GAMS_TRY(h, who, stage(SWF_GEOM, false));
    // 3. the one read-back: the rows and the flags
    GAMS_TRY(h, who, hipMemcpyAsync(h->pin_scratch, J.words, 3 * 8, hipMemcpyDeviceToHost, st));
    GAMS_TRY(h, who, hipStreamSynchronize(st));
    const uint64_t tot = h->pin_scratch[0];
    if (h->pin_scratch[1])
        return gams_fail(h, GAMS_EINVAL, who + ": the feature on line " + std::to_string(h->pin_scratch[2] + 1ull) +
                                             " is empty or has its middle outside its ctg");
    // 4. the rows
    gams_sw_row_t *d_rows = nullptr;
    int32_t *d_cnt = nullptr;
    auto rows = [&](Carver &c) {
        d_rows = c.take<gams_sw_row_t>(std::max<uint64_t>(tot, 1));
        d_cnt = call.count() ? c.take<int32_t>(std::max<uint64_t>(tot, 1)) : nullptr;
    };
    if (!call.summary) {
        GAMS_TRY(h, who, r_dev.alloc(layout_bytes(rows)));
        carve(r_dev.p, rows);
    }
    SwAnnoStage sets(h);
    const int ra = sets.put(h, call, n_ctg);
    if (ra != GAMS_OK) return ra;
    SwCols d{};
    d.ctgs = d_ctgs;
    d.fs = const_cast<int32_t *>(J.fs);
    d.fe = const_cast<int32_t *>(J.fe);
    d.fctg = const_cast<uint32_t *>(J.fctg);
    d.row_off = reinterpret_cast<uint64_t *>(d_row_off);
    GAMS_TRY(h, who, stage(SWF_ROWS, true));
    const int rc = sw_launch(h, call, J.s, nf, tot, d, d_rows, d_cnt, sets.staged());
    if (rc != GAMS_OK) return rc;
    GAMS_TRY(h, who, stage(SWF_ROWS, false));
    if (call.summary) {   // 4'. the rows went into the accumulator: nothing to print
        *n_rows = tot;
        return sw_sum_verdict(h, call.summary);
    }
    // 5. the text, with the ids composed on the device
    const uint64_t per_row = 8ull + J.max_id + 1ull + 10ull + J.max_chr + (call.count() ? 112ull : 96ull);
    SwTextArgs ta{};
    auto txt = [&](Carver &c) { sw_text_cols(c, ta, tot, n_ctg, per_row); };
    GAMS_TRY(h, who, t_dev.alloc(layout_bytes(txt)));
    carve(t_dev.p, txt);
    sw_text_rows(ta, call, d, d_rows, d_cnt);
    ta.ctg_row_off = reinterpret_cast<const uint64_t *>(d_ctg_row_off);
    ta.dev_ids = 1u;
    ta.cid_off = J.id_off;
    ta.cid_bytes = J.id_bytes;
    ta.chr_off = J.chr_off;
    ta.chr_bytes = J.chr_bytes;
    ta.igrp = J.igrp;
    SwText T{};
    const int rt = sw_text_tail(h, who, "use the host path", ta, &stage, &T);
    if (rt != GAMS_OK) return rt;
    *text = T.bytes ? T.text : "";
    *text_bytes = T.bytes;
    *n_rows = tot;
    for (uint32_t i = 0; i <= n_ctg; ++i) text_off[i] = T.words[2u + i];   // (no rows: the words are zero)
    return GAMS_OK;
}

extern "C" int gams_gpu_sw_batch(gams_gpu_t *h, gams_seqset_t *s, uint32_t n_sel, const uint32_t *ctg_index,
                                 const int32_t *chr_start, const uint64_t *feat_off, const int32_t *feat_start,
                                 const int32_t *feat_end, int32_t size, int32_t max, int32_t resize,
                                 gams_sw_row_t *rows, uint64_t cap, uint64_t *row_off, uint64_t *n_rows) {
    const SwCall c(size, max, resize, GAMS_SW_GC);
    SwReq q(SwMode::Rows, h, s, n_sel, ctg_index, chr_start, feat_off, feat_start, feat_end, c, n_rows);
    q.rows = rows;
    q.cap = cap;
    q.row_off = row_off;
    return sw_batch_impl(q);
}

extern "C" int gams_gpu_sw_count_batch(gams_gpu_t *h, gams_seqset_t *s, uint32_t n_sel, const uint32_t *ctg_index,
                                       const int32_t *chr_start, const uint64_t *feat_off, const int32_t *feat_start,
                                       const int32_t *feat_end, int32_t size, int32_t max, gams_index_t *rg_ix,
                                       const uint32_t *rg_group, int32_t *count, uint64_t cap, uint64_t *row_off,
                                       uint64_t *n_rows) {
    if (!rg_ix || (n_sel && !rg_group)) return gams_fail(h, GAMS_EINVAL, "gpu_sw_count: null rg index or rg groups");
    // resize only shapes the gc statistics, which this call does not compute: any value the checks accept
    const SwCall c(size, max, 2, GAMS_SW_COUNT, rg_ix, rg_group);
    SwReq q(SwMode::Counts, h, s, n_sel, ctg_index, chr_start, feat_off, feat_start, feat_end, c, n_rows);
    q.count = count;
    q.cap = cap;
    q.row_off = row_off;
    return sw_batch_impl(q);
}

// ---- the ΔG of the windows: the rows' geometry from the kernel without actions, then dg.hip over them --
// a window has at most `size` bases (M is the feature resized to `size`, window.rs:96-124), so the kernel's limit is one on size
static int sw_dg_check(gams_gpu_t *h, const std::string &who, const gams_dg_table_t *table, int32_t size) {
    const int rc = gams_dg_table_check(h, who, table);
    if (rc != GAMS_OK) return rc;
    if (size > 65535) return gams_fail(h, GAMS_EUNSUPPORTED, who + ": windows of more than 65535 bases");
    return GAMS_OK;
}

extern "C" int gams_gpu_sw_dg_batch(gams_gpu_t *h, gams_seqset_t *s, uint32_t n_sel, const uint32_t *ctg_index,
                                    const int32_t *chr_start, const uint64_t *feat_off, const int32_t *feat_start,
                                    const int32_t *feat_end, int32_t size, int32_t max, const gams_dg_table_t *table,
                                    float *dg, uint64_t cap, uint64_t *row_off, uint64_t *n_rows) {
    const int rc = sw_dg_check(h, "gpu_sw_dg", table, size);
    if (rc != GAMS_OK) return rc;
    // resize only shapes the gc statistics, which this call does not compute: any value the checks accept
    const SwCall c(size, max, 2, 0u);
    SwReq q(SwMode::Dg, h, s, n_sel, ctg_index, chr_start, feat_off, feat_start, feat_end, c, n_rows);
    q.dg_table = table;
    q.dg = dg;
    q.cap = cap;
    q.row_off = row_off;
    return sw_batch_impl(q);
}

// the two text entries: the arguments, the SwReq and the call.  with_dg: the ΔG entry, whose table and size are checked
// between the call's actions and the feature ids
static int sw_text_entry(gams_gpu_t *h, gams_seqset_t *s, uint32_t n_sel, const uint32_t *ctg_index, const char *const *chr,
                         const int32_t *chr_start, const uint64_t *feat_off, const int32_t *feat_start, const int32_t *feat_end,
                         const char *const *feat_id, const SwCall &c, bool with_dg, const gams_dg_table_t *table,
                         const char **text, uint64_t *text_bytes, const uint64_t **ctg_off, uint64_t *n_rows) {
    if (!h || !text || !text_bytes || !n_rows || (n_sel && (!chr || !feat_off)))
        return gams_fail(h, GAMS_EINVAL, "gpu_sw_text: null argument");
    int rc = gams_sw_call_check(h, kSwText, c, SWC_ACTIONS, n_sel);
    if (rc != GAMS_OK) return rc;
    if (with_dg && (rc = sw_dg_check(h, kSwText, table, c.size)) != GAMS_OK) return rc;
    if (n_sel && feat_off[n_sel] && !feat_id) return gams_fail(h, GAMS_EINVAL, "gpu_sw_text: null feature ids");
    SwReq q(SwMode::Text, h, s, n_sel, ctg_index, chr_start, feat_off, feat_start, feat_end, c, n_rows);
    q.tx = SwTextReq{chr, feat_id, text, text_bytes, ctg_off};
    q.dg_table = with_dg ? table : nullptr;
    *text = nullptr;
    *text_bytes = 0;
    return sw_batch_impl(q);
}

extern "C" int gams_gpu_sw_text_actions(gams_gpu_t *h, gams_seqset_t *s, uint32_t n_sel, const uint32_t *ctg_index,
                                        const char *const *chr, const int32_t *chr_start, const uint64_t *feat_off,
                                        const int32_t *feat_start, const int32_t *feat_end, const char *const *feat_id,
                                        int32_t size, int32_t max, int32_t resize, uint32_t actions, gams_index_t *rg_ix,
                                        const uint32_t *rg_group, const char **text, uint64_t *text_bytes,
                                        const uint64_t **ctg_off, uint64_t *n_rows) {
    return sw_text_entry(h, s, n_sel, ctg_index, chr, chr_start, feat_off, feat_start, feat_end, feat_id,
                         SwCall(size, max, resize, actions, rg_ix, rg_group), false, nullptr, text, text_bytes, ctg_off, n_rows);
}

extern "C" int gams_gpu_sw_text_dg(gams_gpu_t *h, gams_seqset_t *s, uint32_t n_sel, const uint32_t *ctg_index,
                                   const char *const *chr, const int32_t *chr_start, const uint64_t *feat_off,
                                   const int32_t *feat_start, const int32_t *feat_end, const char *const *feat_id,
                                   int32_t size, int32_t max, int32_t resize, uint32_t actions, gams_index_t *rg_ix,
                                   const uint32_t *rg_group, const gams_dg_table_t *table, const char **text,
                                   uint64_t *text_bytes, const uint64_t **ctg_off, uint64_t *n_rows) {
    return sw_text_entry(h, s, n_sel, ctg_index, chr, chr_start, feat_off, feat_start, feat_end, feat_id,
                         SwCall(size, max, resize, actions, rg_ix, rg_group), true, table, text, text_bytes, ctg_off, n_rows);
}

extern "C" int gams_gpu_sw_text(gams_gpu_t *h, gams_seqset_t *s, uint32_t n_sel, const uint32_t *ctg_index,
                                const char *const *chr, const int32_t *chr_start, const uint64_t *feat_off,
                                const int32_t *feat_start, const int32_t *feat_end, const char *const *feat_id,
                                int32_t size, int32_t max, int32_t resize, const char **text, uint64_t *text_bytes,
                                const uint64_t **ctg_off, uint64_t *n_rows) {
    return gams_gpu_sw_text_actions(h, s, n_sel, ctg_index, chr, chr_start, feat_off, feat_start, feat_end, feat_id, size,
                                    max, resize, GAMS_SW_GC, nullptr, nullptr, text, text_bytes, ctg_off, n_rows);
}

// ---- the accumulator of the sw summaries -----------------------------------------------------------------------------
// the call's parameters against the accumulator's binding, the tag slot against its tags and the span sets against the
// number it was made for (none of them NULL; need_cols: nor a set_group column): GAMS_EINVAL otherwise
static int sw_summary_check(gams_gpu_t *h, const std::string &who, const SwCall &c, bool need_cols) {
    const gams_sw_summary_t *sum = c.summary;
    if (!sum) return gams_fail(h, GAMS_EINVAL, who + ": null argument");
    if (c.n_anno > GAMS_SW_SUMMARY_MAX_ANNO) return gams_fail(h, GAMS_EINVAL, who + ": more than GAMS_SW_SUMMARY_MAX_ANNO span sets");
    if (c.n_anno != sum->n_anno) return gams_fail(h, GAMS_EINVAL, who + ": the accumulator was created for another number of span sets");
    if (c.n_anno && (!c.sets || !c.set_group)) return gams_fail(h, GAMS_EINVAL, who + ": null span sets or set groups");
    for (uint32_t a = 0; a < c.n_anno; ++a)
        if (!c.sets[a] || (need_cols && !c.set_group[a])) return gams_fail(h, GAMS_EINVAL, who + ": a null span set or set group column");
    if (sum->size != c.size || sum->max != c.max || sum->resize != c.resize || sum->actions != c.actions)
        return gams_fail(h, GAMS_EINVAL, who + ": the accumulator was created for other size, max, resize or actions");
    if (c.tag >= sum->n_tags) return gams_fail(h, GAMS_EINVAL, who + ": tag slot beyond the accumulator's tags");
    return GAMS_OK;
}

int gams_sw_call_check(gams_gpu_t *h, const std::string &who, const SwCall &c, uint32_t parts, uint64_t n_ctgs, bool have_seq,
                       uint64_t nf) {
    if (parts & SWC_ACTIONS) {
        if (!c.known_actions()) return gams_fail(h, GAMS_EINVAL, who + ": unknown action bits");
        if (c.gc() && !have_seq) return gams_fail(h, GAMS_EINVAL, who + ": GAMS_SW_GC without a seqset or the ctgs' slots");
        if (c.count() && (!c.rg_ix || (n_ctgs && !c.rg_group)))
            return gams_fail(h, GAMS_EINVAL, who + ": GAMS_SW_COUNT without an rg index or rg groups");
    }
    if ((parts & SWC_WINDOW) && !c.window_ok())
        return gams_fail(h, GAMS_EINVAL, who + ": size >= 2, max >= 0, resize >= 2 (center_resize of 1 bp is an empty span)");
    if ((parts & SWC_MAX) && !c.max_ok()) return gams_fail(h, GAMS_EUNSUPPORTED, who + ": max beyond 2^24 windows a side");
    if (parts & SWC_SUMMARY) {
        const int rc = sw_summary_check(h, who, c, n_ctgs != 0);
        if (rc != GAMS_OK) return rc;
    }
    if (parts & SWC_SLOTS) {
        const uint64_t threads = nf * (1u + 2u * (uint64_t)c.max);
        if (nf > 0xffffffffull || (threads + 255) / 256 > 0x7fffffffull)
            return gams_fail(h, GAMS_EUNSUPPORTED, who + ": too many feature slots for one launch");
    }
    return GAMS_OK;
}

extern "C" int gams_sw_summary_create(gams_gpu_t *h, int32_t max, uint32_t n_tags, uint32_t actions, int32_t size,
                                      int32_t resize, gams_sw_summary_t **out) {
    return gams_sw_summary_create_anno(h, max, n_tags, actions, size, resize, 0u, out);
}

extern "C" int gams_sw_summary_create_anno(gams_gpu_t *h, int32_t max, uint32_t n_tags, uint32_t actions, int32_t size,
                                           int32_t resize, uint32_t n_anno, gams_sw_summary_t **out) {
    if (!h || !out) return gams_fail(h, GAMS_EINVAL, "sw_summary_create: null argument");
    *out = nullptr;
    if (n_anno > GAMS_SW_SUMMARY_MAX_ANNO)
        return gams_fail(h, GAMS_EINVAL, "sw_summary_create: more than GAMS_SW_SUMMARY_MAX_ANNO span sets");
    const SwCall c(size, max, resize, actions);
    if (n_tags == 0 || !c.window_ok() || !c.max_ok() || !c.known_actions())
        return gams_fail(h, GAMS_EINVAL, "sw_summary_create: n_tags >= 1, size >= 2, 0 <= max <= 2^24, resize >= 2, known action bits");
    GAMS_HIP(h, hipSetDevice(h->device));
    const size_t words = ((size_t)max + 1) * kSumWords;
    gams_sw_summary_t *sum = new gams_sw_summary_t();
    sum->size = size;
    sum->max = max;
    sum->resize = resize;
    sum->actions = actions;
    sum->n_tags = n_tags;
    sum->n_anno = n_anno;
    const size_t pwords = ((size_t)max + 1) * n_anno;          // the Prop sums, beside the ten words of every group
    hipError_t e = hipMalloc(&sum->d_acc, words * n_tags * 8);
    if (e == hipSuccess) e = hipMalloc(&sum->d_call, (words + 1 + pwords) * 8);
    if (e == hipSuccess) e = hipMemsetAsync(sum->d_acc, 0, words * n_tags * 8, h->compute);
    if (e == hipSuccess && pwords) e = hipMalloc(&sum->d_prop, pwords * n_tags * 8);
    if (e == hipSuccess && pwords) e = hipMemsetAsync(sum->d_prop, 0, pwords * n_tags * 8, h->compute);
    if (e != hipSuccess) {
        (void)hipGetLastError();   // reported below, not left sticky
        (void)hipFree(sum->d_acc);
        (void)hipFree(sum->d_call);
        (void)hipFree(sum->d_prop);
        delete sum;
        return gams_fail(h, GAMS_ENOMEM, std::string("sw_summary_create: ") + hipGetErrorString(e));
    }
    *out = sum;
    return GAMS_OK;
}

extern "C" int gams_sw_summary_reset(gams_gpu_t *h, gams_sw_summary_t *sum) {
    if (!h || !sum) return gams_fail(h, GAMS_EINVAL, "sw_summary_reset: null argument");
    GAMS_HIP(h, hipSetDevice(h->device));
    GAMS_TRY(h, kSwSum, hipMemsetAsync(sum->d_acc, 0, ((size_t)sum->max + 1) * kSumWords * sum->n_tags * 8, h->compute));
    if (sum->d_prop)
        GAMS_TRY(h, kSwSum, hipMemsetAsync(sum->d_prop, 0, ((size_t)sum->max + 1) * sum->n_anno * sum->n_tags * 8, h->compute));
    return GAMS_OK;
}

extern "C" int gams_sw_summary_read_anno(gams_gpu_t *h, gams_sw_summary_t *sum, uint64_t *prop) {
    if (!h || !sum || (sum->n_anno && !prop)) return gams_fail(h, GAMS_EINVAL, "sw_summary_read_anno: null argument");
    if (!sum->n_anno) return GAMS_OK;
    GAMS_HIP(h, hipSetDevice(h->device));
    const size_t n = ((size_t)sum->max + 1) * sum->n_tags * sum->n_anno;
    GAMS_TRY(h, kSwSum, hipMemcpyAsync(prop, sum->d_prop, n * 8, hipMemcpyDeviceToHost, h->compute));
    GAMS_TRY(h, kSwSum, hipStreamSynchronize(h->compute));
    return GAMS_OK;
}

extern "C" int gams_sw_summary_read(gams_gpu_t *h, gams_sw_summary_t *sum, uint64_t *count, uint64_t *s, uint64_t *nan,
                                    uint64_t *rg_count) {
    if (!h || !sum) return gams_fail(h, GAMS_EINVAL, "sw_summary_read: null argument");
    GAMS_HIP(h, hipSetDevice(h->device));
    const size_t n = ((size_t)sum->max + 1) * sum->n_tags;
    std::vector<unsigned long long> w(n * kSumWords);
    GAMS_TRY(h, kSwSum, hipMemcpyAsync(w.data(), sum->d_acc, w.size() * 8, hipMemcpyDeviceToHost, h->compute));
    GAMS_TRY(h, kSwSum, hipStreamSynchronize(h->compute));
    for (size_t g = 0; g < n; ++g) {
        const unsigned long long *v = w.data() + g * kSumWords;
        if (count) count[g] = v[SUM_COUNT];
        if (rg_count) rg_count[g] = v[SUM_C];
        for (uint32_t k = 0; k < 4u; ++k) {
            if (s) s[4 * g + k] = v[SUM_S + k];
            if (nan) nan[4 * g + k] = v[SUM_NAN + k];
        }
    }
    return GAMS_OK;
}

extern "C" void gams_sw_summary_destroy(gams_gpu_t *h, gams_sw_summary_t *sum) {
    if (!sum) return;
    if (h) {
        (void)hipSetDevice(h->device);
        (void)hipStreamSynchronize(h->compute);   // a call into it may still be queued
    }
    (void)hipFree(sum->d_acc);
    (void)hipFree(sum->d_call);
    (void)hipFree(sum->d_prop);
    delete sum;
}

extern "C" int gams_gpu_sw_summary_batch_anno(gams_gpu_t *h, gams_seqset_t *s, uint32_t n_sel, const uint32_t *ctg_index,
                                              const int32_t *chr_start, const uint64_t *feat_off, const int32_t *feat_start,
                                              const int32_t *feat_end, int32_t size, int32_t max, int32_t resize,
                                              uint32_t actions, gams_index_t *rg_ix, const uint32_t *rg_group,
                                              gams_sw_summary_t *sum, uint32_t tag, uint32_t n_anno, gams_spans_t *const *sets,
                                              const uint32_t *const *set_group, uint64_t *n_rows) {
    if (!h || !n_rows || (n_sel && !feat_off)) return gams_fail(h, GAMS_EINVAL, "gpu_sw_summary: null argument");
    SwCall c(size, max, resize, actions, rg_ix, rg_group);
    c.summary = sum;
    c.tag = tag;
    c.n_anno = n_anno;
    c.sets = sets;
    c.set_group = set_group;
    const int rc = gams_sw_call_check(h, kSwSum, c, SWC_ACTIONS | SWC_SUMMARY, n_sel);
    if (rc != GAMS_OK) return rc;
    return sw_batch_impl(SwReq(SwMode::Summary, h, s, n_sel, ctg_index, chr_start, feat_off, feat_start, feat_end, c, n_rows));
}

extern "C" int gams_gpu_sw_summary_batch(gams_gpu_t *h, gams_seqset_t *s, uint32_t n_sel, const uint32_t *ctg_index,
                                         const int32_t *chr_start, const uint64_t *feat_off, const int32_t *feat_start,
                                         const int32_t *feat_end, int32_t size, int32_t max, int32_t resize, uint32_t actions,
                                         gams_index_t *rg_ix, const uint32_t *rg_group, gams_sw_summary_t *sum, uint32_t tag,
                                         uint64_t *n_rows) {
    return gams_gpu_sw_summary_batch_anno(h, s, n_sel, ctg_index, chr_start, feat_off, feat_start, feat_end, size, max, resize,
                                          actions, rg_ix, rg_group, sum, tag, 0u, nullptr, nullptr, n_rows);
}

extern "C" int gams_gpu_sw(gams_gpu_t *h, gams_seqset_t *s, uint32_t i, int32_t chr_start,
                           const int32_t *feat_start, const int32_t *feat_end, uint32_t nf, int32_t size,
                           int32_t max, int32_t resize, gams_sw_row_t *rows, uint64_t cap, uint64_t *n_rows) {
    if (!h || !s || !n_rows || (nf && (!feat_start || !feat_end)))
        return gams_fail(h, GAMS_EINVAL, "gpu_sw: null argument");
    const uint64_t feat_off[2] = {0, nf};
    return gams_gpu_sw_batch(h, s, 1, &i, &chr_start, feat_off, feat_start, feat_end, size, max, resize, rows, cap,
                             nullptr, n_rows);
}

// gc_content (round4) of arbitrary chromosome ranges inside ctg i: gams::cache_gc_content
// (src/libs/utils.rs:141-162) as `gams peak` uses it (src/cmd_gams/peak.rs:79).
namespace {
struct RangeGcEntry {   // what gams_range_batch (range_batch.hpp) asks of an entry
    gams_gpu_t *h;
    const RangeBatch &b;
    int admit() const { return GAMS_OK; }
    SwCols inputs(Carver &c, uint32_t n) const { return sw_stage_layout<SwCtg>(c, b.n_sel, n, false); }   // ctgs | rs | re | rctg
    void head(const SwCols &in) const {
        for (uint32_t k = 0; k < b.n_sel; ++k) {
            const uint32_t i = b.ctg_index[k], len = b.s->len[i];
            in.ctgs[k] = SwCtg{b.s->off[i], len, b.chr_start[k], (int32_t)((int64_t)b.chr_start[k] + len - 1), (uint32_t)b.range_off[k], UINT32_MAX, 0u};
        }
    }
    int range(const SwCols &in, uint32_t k, uint64_t q) const {
        in.fs[q] = b.range_start[q];
        in.fe[q] = b.range_end[q];
        in.fctg[q] = k;
        return GAMS_OK;
    }
    int ready() const { return gams_seqset_gcindex(h, b.s); }
    void launch(const SwCols &d, uint32_t n, float *d_gc) const {
        SwArgs a{};
        a.pm = b.s->gcindex->d_pm;
        a.seg = b.s->gcindex->d_seg;
        a.ctgs = d.ctgs;
        a.fctg = d.fctg;
        hipLaunchKernelGGL(range_gc_kernel, dim3((n + 255) / 256), dim3(256), 0, h->compute, a, d.fs, d.fe, n, d_gc);
    }
};
}  // namespace

extern "C" int gams_gpu_range_gc_batch(gams_gpu_t *h, gams_seqset_t *s, uint32_t n_sel, const uint32_t *ctg_index,
                                       const int32_t *chr_start, const uint64_t *range_off, const int32_t *range_start,
                                       const int32_t *range_end, float *gc) {
    const RangeBatch b{s, n_sel, ctg_index, chr_start, range_off, range_start, range_end, gc};
    return gams_range_batch(h, kRangeGc, b, RangeGcEntry{h, b});
}

extern "C" int gams_gpu_range_gc(gams_gpu_t *h, gams_seqset_t *s, uint32_t i, int32_t chr_start,
                                 const int32_t *range_start, const int32_t *range_end, uint32_t n, float *gc) {
    if (!h || !s || (n && (!range_start || !range_end || !gc)))
        return gams_fail(h, GAMS_EINVAL, "gpu_range_gc: null argument");
    const uint64_t range_off[2] = {0, n};
    return gams_gpu_range_gc_batch(h, s, 1, &i, &chr_start, range_off, range_start, range_end, gc);
}
