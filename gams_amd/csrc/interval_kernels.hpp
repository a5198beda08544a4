// interval_kernels.hpp -- device side of the interval index and the span sets, shared by interval.hip (the
// array entries gams_gpu_count / locate / cover) and text.hip (the same lookups behind the text entries): the
// group records, the lookup kernels and their launch on device-resident query columns.  See interval.hip for the
// scheme.
#pragma once

#include "common.hpp"

// bucket directory of one sorted key array of one group (32-bit keys, order-preserving bias applied)
struct KeyDir {
    uint32_t key0;    // smallest key of the group
    uint32_t shift;   // bucket b holds keys in [key0 + (b << shift), key0 + ((b+1) << shift))
    uint32_t nb;      // buckets; nb <= n, dir has nb+1 entries at dir[off + g]
    uint32_t pad;
};

// everything a query needs to know about its group, one 48-B record (one or two lines)
struct IvRec {
    uint32_t start, stop;
    uint64_t orig;
};

struct IndexGroup {
    uint64_t off;     // first interval of the group
    uint32_t n;       // intervals in the group
    uint32_t maxlen;  // max(stop - start), Lapper::max_len
    KeyDir start, stop;       // one bucket per key, rank only (locate's lower bound)
    KeyDir bk_start, bk_stop; // ~2^kCellShift keys per cell, rank + the next seven keys inline (count's two lower bounds)
};

// What a count query needs of its group, one 32-B record (the 80-B IndexGroup costs a second line and
// three more loads per query; random queries are bound by lines moved, not by bytes)
struct CountGroup {
    uint32_t off, n;                 // first interval (m < 2^32), intervals
    uint32_t s_key0, s_nb;           // bucket records over the starts
    uint32_t t_key0, t_nb;           // ... over the stops
    uint32_t s_shift, t_shift;
};

// Bucket record of the count path: everything a lower bound needs in ONE 32-B access -- the rank of
// the first key at or after the bucket's edge and the seven keys that follow it (0xffffffff past the
// group's end).  A key that falls in bucket b is compared with those seven; only when all seven are
// smaller (a cell of more than seven keys: 0.1 % of uniform cells at 2 keys per cell) the search goes on in the key
// array.  Random queries are bound by scattered lines out of the Infinity Cache: the separate
// directory + key array of the locate path cost two lines per bound, this one.
struct BkRec {
    uint32_t rank;
    uint32_t k[7];
};
#ifndef GAMS_CELL_SHIFT
#define GAMS_CELL_SHIFT 1
#endif
static_assert(sizeof(IndexGroup) == 80 && sizeof(CountGroup) == 32 && sizeof(IvRec) == 16 && sizeof(BkRec) == 32,
              "tests/layout_main.cpp carves the index arena with stand-ins of these sizes");
constexpr uint32_t kCellShift = GAMS_CELL_SHIFT;   // about 2^kCellShift keys per cell of the count path's grid

struct SpanRec {
    int32_t lo, hi;   // inclusive
    uint64_t cum;     // covered bases in the group's spans before this one
};

struct SpanGroup {
    uint64_t off;
    uint32_t n;
    uint32_t pad;
    KeyDir lo;
};

struct gams_index {
    uint32_t n_groups = 0;
    uint64_t m = 0;
    IndexGroup *d_groups = nullptr;
    uint32_t *d_stops = nullptr;     // per group, ascending, sorted independently (for count)
    uint32_t *d_lstart = nullptr;    // per group, starts of the (start,stop)-sorted pairs: ascending (both searches)
    IvRec *d_lrec = nullptr;         // the sorted pairs + the caller's index of each, 16 B (locate's scan)
    uint32_t *d_dir_start = nullptr; // m + n_groups entries: group g's directory begins at off[g] + g (locate)
    BkRec *d_bk_start = nullptr;     // 2 * ((m >> kCellShift) + 2*n_groups + 2) records, the starts' and the stops' record of a cell side by side;
    BkRec *d_bk_stop = nullptr;      // = d_bk_start + 1; group g's cells begin at (off[g] >> kCellShift) + 2g
    CountGroup *d_cgroups = nullptr;
    // everything above lives in one pooled HBM block
    uint8_t *arena = nullptr;
    size_t arena_bytes = 0;
};

// One index build, between its two steps (interval.hip): gams_index_build_begin allocates the index and the scratch,
// the caller queues on the compute stream whatever fills cols.off32 (n_groups + 1 offsets), cols.starts_in and cols.stops_in,
// and gams_index_build_run sorts, derives the tables, waits and hands the index out.  gams_index_create is the front
// that fills the columns from host arrays; gams_index_create_range_text (text.hip) fills them by a gather kernel.
// A step that fails has already returned everything to the pools (gams_index_build_fail does that for the caller's
// own errors in between).
struct IndexBuild {
    explicit IndexBuild(gams_gpu_t *h) : scratch(h, false), d_tmp(h, false) {}
    gams_index *ix = nullptr;
    IndexScratch cols{};          // the builder's inputs (off32, starts_in, stops_in), and the radix sort's buffers
    uint64_t bk_slots = 0;
    PoolBlock scratch, d_tmp;     // behind cols; the radix sort's storage
};
int gams_index_build_begin(gams_gpu_t *h, uint32_t n_groups, uint64_t m, IndexBuild *B);
// (done, if given: an event recorded on the compute stream behind the build's last kernel, before the host waits)
int gams_index_build_run(gams_gpu_t *h, IndexBuild *B, uint32_t max_n, gams_index_t **out, hipEvent_t done = nullptr);
int gams_index_build_fail(gams_gpu_t *h, IndexBuild *B, hipError_t err, const char *what);

// Cell record of the anno path, 64 B: everything a "covered bases up to x" lookup needs when x falls in cell b of the
// group's grid (the grid of the `lo` directory, about one span per cell) -- the rank at the cell's edge, the span in
// front of it with the covered bases before that one, and the next five spans inline.  One line per position instead
// of a directory line, a search and a record line; a cell that starts more than five spans falls back to those.
struct SpanCell {
    uint64_t base;        // covered bases in the group's spans before span rank-1 (0 when rank == 0)
    uint32_t rank;        // spans with lo < the cell's edge
    int32_t plo, phi;     // span rank-1; plo > phi when there is none
    int32_t lo[5], hi[5]; // spans rank .. rank+4 (unused entries past the group's end)
    uint32_t pad;
};
static_assert(sizeof(SpanCell) == 64, "SpanCell is one 64-B record");

struct gams_spans {
    uint32_t n_groups = 0;
    uint64_t m = 0;
    SpanGroup *d_groups = nullptr;
    SpanRec *d_rec = nullptr;        // one 16-B record per span: the search and its two follow-up reads share a line
    uint32_t *d_dir_lo = nullptr;
    SpanCell *d_cells = nullptr;     // m + n_groups + 1 records: group g's cell b at off[g] + g + b (like its directory)
};

// interval.hip, for runlist.hip: span_cell_kernel over a set whose groups, records and directory are in place, on `st`
hipError_t gams_spans_launch_cells(const gams_spans_t *sp, hipStream_t st);

namespace {

// the directory header of n ascending keys first .. last: build_dir's rule (interval.hip), on the device
__device__ __forceinline__ KeyDir dir_params(uint32_t first, uint32_t last, uint32_t n) {
    KeyDir d{0u, 0u, 0u, 0u};
    if (n == 0) return d;
    d.key0 = first;
    // 64-bit range: a one-key grid (n == 1, e.g. the cell grid of a one-interval group [0, 2^31 + 1)) needs
    // range >> shift == 0, i.e. shift == 32 when the range has bit 31 set -- a 32-bit shift by 32 is masked
    // to 0 on this hardware and the loop would never end.  Every consumer shifts in 64 bits.
    const uint64_t range = (uint64_t)last - (uint64_t)first;
    while ((range >> d.shift) >= n) ++d.shift;     // (range >> shift) + 1 <= n buckets; ends at shift <= 32
    d.nb = (uint32_t)(range >> d.shift) + 1u;
    return d;
}

// Number of keys < key among the group's n ascending keys a[0..n) (rank of the lower bound).
// BIAS = 0x80000000 compares int32 keys stored as they are (x ^ BIAS is order preserving).
template <uint32_t BIAS>
__device__ __forceinline__ uint32_t dir_lower_bound(const uint32_t *a, const uint32_t *dir, uint32_t n,
                                                    const KeyDir d, uint64_t key) {
    if (n == 0 || key <= (uint64_t)d.key0) return 0;
    const uint64_t b = (key - d.key0) >> d.shift;
    if (b >= d.nb) return n;                       // beyond the last bucket: beyond the largest key
    uint32_t lo = dir[b], hi = dir[b + 1];
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if ((uint64_t)(a[mid] ^ BIAS) < key)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

// lower bound through the bucket records (see BkRec)
__device__ __forceinline__ uint32_t bk_lower_bound(const uint32_t *keys, const BkRec *bk, uint32_t n, const KeyDir d,
                                                   uint64_t key) {
    if (n == 0 || key <= (uint64_t)d.key0) return 0;
    const uint64_t b = (key - d.key0) >> d.shift;
    if (b >= d.nb) return n;
    const uint4 *rp = reinterpret_cast<const uint4 *>(bk + 2u * b);   // the cell's pair of records: starts', stops'
    const uint4 r0 = rp[0], r1 = rp[1];
    const uint32_t rank = r0.x;
    uint32_t c = (uint32_t)((uint64_t)r0.y < key) + (uint32_t)((uint64_t)r0.z < key) + (uint32_t)((uint64_t)r0.w < key) +
                 (uint32_t)((uint64_t)r1.x < key) + (uint32_t)((uint64_t)r1.y < key) + (uint32_t)((uint64_t)r1.z < key) +
                 (uint32_t)((uint64_t)r1.w < key);
    c = min(c, n - rank);                            // padding past the group's end does not count
    if (c < 7u || rank + 7u >= n) return rank + c;
    // A crowded cell (more than seven keys; 5 % of uniform cells, i.e. some lane of nearly every wave): the
    // answer lies between rank + 7 and the next cell's rank.  One load for that rank (the neighbouring
    // record), then the next eight keys in one batch of independent loads -- two round trips instead of the
    // ~12 dependent ones of a binary search over the group, which made every wave of random queries live 26 us
    // (33 dependent loads, profiles/r02_count_latency_chain.txt).  A cell of more than 15 keys goes on with
    // the binary search, inside the cell.
    uint32_t lo = rank + 7u;
    uint32_t hi = b + 1u < d.nb ? reinterpret_cast<const uint32_t *>(bk + 2u * (b + 1u))[0] : n;
    uint32_t cnt = 0;
#pragma unroll
    for (uint32_t i = 0; i < 8u; ++i) {
        const uint32_t k = keys[min(lo + i, n - 1u)];
        cnt += (lo + i < hi && (uint64_t)k < key) ? 1u : 0u;
    }
    if (hi - lo <= 8u) return lo + cnt;
    if (cnt < 8u) return lo + cnt;                   // sorted keys: the first one >= key ends the count
    lo += 8u;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if ((uint64_t)keys[mid] < key)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

// Lapper::count(qs, qe) against group g (g >= n_groups: utils.rs:29-32, ctg not in the index -> 0).  Shared by
// interval_count_kernel and the sw windows' rg_count (sw.hip).
__device__ __forceinline__ int32_t lapper_count(const CountGroup *groups, const uint32_t *starts, const uint32_t *stops,
                                                const BkRec *bk_start, const BkRec *bk_stop, uint32_t n_groups,
                                                uint32_t g, uint32_t qs, uint32_t qe) {
    if (g >= n_groups) return 0;
    const uint4 *gp = reinterpret_cast<const uint4 *>(groups + g);
    const uint4 g0 = gp[0], g1 = gp[1];
    const uint32_t off = g0.x, n = g0.y;
    const KeyDir ds{g0.z, g1.z, g0.w, 0u}, dt{g1.x, g1.w, g1.y, 0u};
    const uint64_t boff = (uint64_t)(off >> kCellShift) + 2ull * g;
    // Lapper::count: first = bsearch_seq(start + 1, stops); last = bsearch_seq(stop, starts)
    // (bk_start = the interleaved array, bk_stop = bk_start + 1: a range shorter than a cell finds both of its
    // records in one 64-B line or in two neighbouring ones)
    const uint32_t first = bk_lower_bound(stops + off, bk_stop + 2u * boff, n, dt, (uint64_t)qs + 1u);
    const uint32_t last = bk_lower_bound(starts + off, bk_start + 2u * boff, n, ds, (uint64_t)qe);
    return (int32_t)((int64_t)last - (int64_t)first);
}

__global__ __launch_bounds__(256) void interval_count_kernel(const CountGroup *groups, const uint32_t *starts,
                                                             const uint32_t *stops, const BkRec *bk_start,
                                                             const BkRec *bk_stop, uint32_t n_groups,
                                                             const uint32_t *group, const uint32_t *qs,
                                                             const uint32_t *qe, uint64_t nq, int32_t *out) {
    const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nq) return;
    out[q] = lapper_count(groups, starts, stops, bk_start, bk_stop, n_groups, group[q], qs[q], qe[q]);
}

__global__ __launch_bounds__(256) void interval_locate_kernel(const IndexGroup *groups, const uint32_t *lstart,
                                                              const IvRec *lrec, const uint32_t *dir_start,
                                                              uint32_t n_groups, const uint32_t *group,
                                                              const uint32_t *qs, const uint32_t *qe, uint64_t nq,
                                                              int64_t *out) {
    const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nq) return;
    const uint32_t g = group[q];
    int64_t hit = -1;
    if (g < n_groups) {
        const IndexGroup G = groups[g];
        const uint32_t s = qs[q], e = qe[q];
        const uint32_t from = s > G.maxlen ? s - G.maxlen : 0u;  // checked_sub(max_len).unwrap_or(0)
        // Lapper::lower_bound: first interval whose start >= from
        const uint64_t hi = G.off + G.n;
        for (uint64_t i = G.off + dir_lower_bound<0u>(lstart + G.off, dir_start + G.off + g, G.n, G.start, from);
             i < hi; ++i) {
            const IvRec r = lrec[i];
            if (r.start < e && r.stop > s) {  // Interval::overlap
                hit = (int64_t)r.orig;
                break;
            }
            if (r.start >= e) break;
        }
    }
    out[q] = hit;
}

// covered positions <= x inside the group's spans
__device__ __forceinline__ uint64_t covered_upto(const SpanRec *rec, const uint32_t *dir, const SpanGroup &G,
                                                 uint32_t g, int32_t x, uint32_t *rank) {
    // spans with lo <= x = keys < x+1 in biased order; directory lookup, then a search over rec[].lo
    const SpanRec *r = rec + G.off;
    uint32_t i = 0;
    const uint64_t key = (uint64_t)((uint32_t)x ^ 0x80000000u) + 1u;
    if (G.n != 0 && key > (uint64_t)G.lo.key0) {
        const uint64_t b = (key - G.lo.key0) >> G.lo.shift;
        if (b >= G.lo.nb) {
            i = G.n;
        } else {
            const uint32_t *d = dir + G.off + g;
            uint32_t lo = d[b], hi = d[b + 1];
            while (lo < hi) {
                const uint32_t mid = lo + ((hi - lo) >> 1);
                if ((uint64_t)((uint32_t)r[mid].lo ^ 0x80000000u) < key)
                    lo = mid + 1;
                else
                    hi = mid;
            }
            i = lo;
        }
    }
    if (rank) *rank = i;
    if (i == 0) return 0;
    const SpanRec s = r[i - 1];
    const int32_t top = s.hi < x ? s.hi : x;
    return s.cum + (uint64_t)((int64_t)top - s.lo + 1);
}

// The same for a second position x2 <= x whose predecessor `rank` (spans with lo <= x) is known: a range is
// short next to the spans' spacing, so the spans with lo <= x2 end zero to two records further down -- a walk
// over neighbouring 16-B records instead of a second directory line + search (two scattered requests less per
// line).  A long walk gives up and searches.
__device__ __forceinline__ uint64_t covered_upto_below(const SpanRec *rec, const uint32_t *dir, const SpanGroup &G,
                                                       uint32_t g, int32_t x2, uint32_t rank) {
    const SpanRec *r = rec + G.off;
    uint32_t i = rank;
    for (int step = 0; step < 6; ++step) {
        if (i == 0) return 0;
        const SpanRec s = r[i - 1];
        if (s.lo <= x2) {
            const int32_t top = s.hi < x2 ? s.hi : x2;
            return s.cum + (uint64_t)((int64_t)top - s.lo + 1);
        }
        --i;
    }
    return covered_upto(rec, dir, G, g, x2, nullptr);
}

// covered positions <= x through the cell records; *cell_no receives the cell (so that a second position in the
// same cell reuses the record), `ok` = false: the cell starts more than five spans, use covered_upto
__device__ __forceinline__ uint64_t covered_cell(const SpanCell &c, uint32_t n, int32_t x, bool &ok) {
    const uint32_t valid = min(5u, n - c.rank);
    uint32_t t = 0;
#pragma unroll
    for (uint32_t u = 0; u < 5u; ++u) t += (u < valid && c.lo[u] <= x) ? 1u : 0u;
    ok = !(t == 5u && c.rank + 5u < n);
    const bool has_pred = c.plo <= c.phi;
    if (t == 0u) {
        if (!has_pred) return 0;
        const int32_t top = c.phi < x ? c.phi : x;
        return c.base + (uint64_t)((int64_t)top - c.plo + 1);
    }
    uint64_t cum = c.base + (has_pred ? (uint64_t)((int64_t)c.phi - c.plo + 1) : 0ull);
#pragma unroll
    for (uint32_t u = 0; u < 4u; ++u)
        if (u + 1u < t) cum += (uint64_t)((int64_t)c.hi[u] - c.lo[u] + 1);
    const int32_t lo = c.lo[t - 1u], hi = c.hi[t - 1u];
    const int32_t top = hi < x ? hi : x;
    return cum + (uint64_t)((int64_t)top - lo + 1);
}

// cell of position x in the group's grid; false: no span of the group has lo <= x (the answer is 0)
__device__ __forceinline__ bool span_cell_of(const SpanGroup &G, int32_t x, uint32_t &b) {
    const uint64_t key = (uint64_t)((uint32_t)x ^ 0x80000000u) + 1u;   // spans with lo <= x = biased keys < key
    if (G.n == 0 || key <= (uint64_t)G.lo.key0) return false;
    const uint64_t bb = (key - 1u - G.lo.key0) >> G.lo.shift;          // the cell x itself falls in
    b = (uint32_t)(bb < G.lo.nb ? bb : G.lo.nb - 1u);                   // past the last cell: the last cell's spans
    return true;
}

__device__ __forceinline__ SpanCell load_cell(const SpanCell *p) {
    const uint4 *q = reinterpret_cast<const uint4 *>(p);
    union {
        uint4 v[4];
        SpanCell c;
    } u;
    u.v[0] = q[0];
    u.v[1] = q[1];
    u.v[2] = q[2];
    u.v[3] = q[3];
    return u.c;
}

// |spans of group G (number g of its set) ∩ [L, H]| for H >= L: one 64-B cell record per end of the range (the same
// record when both ends fall in one cell); a cell that starts more than five spans takes the directory, a search and the
// walk instead.  Shared by span_cover_kernel and the sw summary's Prop columns (sw.hip).
__device__ __forceinline__ uint64_t span_cover_card(const SpanGroup *groups, const SpanRec *rec, const uint32_t *dir,
                                                    const SpanCell *cells, uint32_t g, int32_t L, int32_t H) {
    const SpanGroup G = groups[g];
    uint32_t bh = 0, bl = 0;
    uint64_t upto_h = 0, upto_l = 0;
    bool ok_h = true, ok_l = true;
    const bool any_h = span_cell_of(G, H, bh);
    const bool any_l = L > INT32_MIN && span_cell_of(G, L - 1, bl);
    if (any_h) {
        const SpanCell ch = load_cell(cells + G.off + g + bh);
        upto_h = covered_cell(ch, G.n, H, ok_h);
        if (any_l) {
            if (bl == bh)
                upto_l = covered_cell(ch, G.n, L - 1, ok_l);
            else
                upto_l = covered_cell(load_cell(cells + G.off + g + bl), G.n, L - 1, ok_l);
        }
    }
    if (!(ok_h && ok_l)) {                     // a crowded cell: directory + search + walk
        uint32_t rank_h;
        upto_h = covered_upto(rec, dir, G, g, H, &rank_h);
        upto_l = L > INT32_MIN ? covered_upto_below(rec, dir, G, g, L - 1, rank_h) : 0;
    }
    return upto_h - upto_l;
}

__global__ __launch_bounds__(256) void span_cover_kernel(const SpanGroup *groups, const SpanRec *rec,
                                                         const uint32_t *dir, const SpanCell *cells, uint32_t n_groups,
                                                         const uint32_t *group, const int32_t *clip_lo,
                                                         const int32_t *clip_hi, const int32_t *qs,
                                                         const int32_t *qe, uint64_t nq, float *out) {
    const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nq) return;
    const uint32_t g = group[q];
    const int32_t s = qs[q], e = qe[q];
    float prop = 0.0f;  // anno.rs:128: chr absent from the set
    if (g < n_groups && e >= s) {
        const int32_t L = s > clip_lo[q] ? s : clip_lo[q];
        const int32_t H = e < clip_hi[q] ? e : clip_hi[q];
        uint64_t card = 0;
        if (H >= L) card = span_cover_card(groups, rec, dir, cells, g, L, H);
        const int32_t total = (int32_t)((int64_t)e - s + 1);
        prop = (float)(int32_t)card / (float)total;  // cardinality() as f32 / cardinality() as f32
    }
    out[q] = prop;
}

// The three lookups over query columns already in device memory, queued on `st` (one lane per query).
inline void launch_interval_count(const gams_index_t *ix, const uint32_t *group, const uint32_t *qs, const uint32_t *qe,
                                  uint64_t n, int32_t *out, hipStream_t st) {
    hipLaunchKernelGGL(interval_count_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, ix->d_cgroups,
                       ix->d_lstart, ix->d_stops, ix->d_bk_start, ix->d_bk_stop, ix->n_groups, group, qs, qe, n, out);
}

inline void launch_interval_locate(const gams_index_t *ix, const uint32_t *group, const uint32_t *qs, const uint32_t *qe,
                                   uint64_t n, int64_t *out, hipStream_t st) {
    hipLaunchKernelGGL(interval_locate_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, ix->d_groups,
                       ix->d_lstart, ix->d_lrec, ix->d_dir_start, ix->n_groups, group, qs, qe, n, out);
}

inline void launch_span_cover(const gams_spans_t *sp, const uint32_t *group, const int32_t *clip_lo, const int32_t *clip_hi,
                              const int32_t *qs, const int32_t *qe, uint64_t n, float *out, hipStream_t st) {
    hipLaunchKernelGGL(span_cover_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, sp->d_groups, sp->d_rec,
                       sp->d_dir_lo, sp->d_cells, sp->n_groups, group, clip_lo, clip_hi, qs, qe, n, out);
}

}  // namespace
