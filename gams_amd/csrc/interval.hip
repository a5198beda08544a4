// interval.hip -- sorted-interval binary-search kernels replacing the rust_lapper
// `idx:` index and the IntSpan intersections of `anno`.
//
//   interval_count_kernel   gams::count_rg  (src/libs/utils.rs:24-36) = Lapper::count:
//       #{start < qe} - #{stop <= qs} by two lower bounds over the group's
//       independently sorted starts[] and stops[] (rust-lapper 1.1.0, BITS).
//   interval_locate_kernel  gams::find_one_idx (src/libs/utils.rs:7-22) =
//       Lapper::find(qs,qe).next(): first interval in (start,stop) order with
//       start < qe && stop > qs; the scan begins at lower_bound(qs - max_len)
//       exactly like the crate's iterator and stops at start >= qe.
//   span_cover_kernel       anno (src/cmd_gams/anno.rs:128-139):
//       |set[chr] & [ctg] & [range]| / |range| from a prefix of covered bases
//       over the chr's sorted disjoint spans (two upper bounds per query).
//
// Intervals are half-open [start, stop) with stop = end+1 as the reference
// stores them (src/libs/redis.rs:245-248, 291-294); queries are passed the way
// the reference passes them: (rg.start, rg.end), i.e. the end is exclusive.
// One lane per query; 16 B/query of traffic plus the probed table lines.
//
// Random queries make a plain binary search fetch ~log2(n) scattered cache lines per sorted
// array (measured: 2.8 G queries/s, the L2 line rate).  Every sorted array therefore carries a
// bucket directory: dir[b] = rank of the first key >= key0 + (b << shift), with about one
// bucket per key, so a lower bound is one directory line plus a search inside dir[b]..dir[b+1]
// (typically 0-2 keys, one line).  Skewed keys only lengthen that inner search; the answer is
// the same lower bound either way.

#include "interval_kernels.hpp"

#include <rocprim/rocprim.hpp>   // the segmented LSD radix sort, for groups beyond a workgroup (index_build_kernel does the others)

#include <algorithm>
#include <atomic>
#include <numeric>
#include <thread>

namespace {

__global__ __launch_bounds__(256) void span_cell_kernel(const SpanGroup *groups, uint32_t n_groups, const SpanRec *rec,
                                                        const uint32_t *dir, uint64_t slots, SpanCell *cells) {
    const uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (j >= slots) return;
    uint32_t lo = 0, hi = n_groups;                 // last group with off[g] + g <= j
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (groups[mid].off + mid <= j)
            lo = mid;
        else
            hi = mid;
    }
    const uint32_t g = lo;
    const SpanGroup G = groups[g];
    const uint64_t b = j - (G.off + g);
    if (G.n == 0 || b >= G.lo.nb) return;
    const uint32_t rank = dir[j];                   // spans with biased lo < key0 + (b << shift)
    const SpanRec *r = rec + G.off;
    SpanCell c;
    c.rank = rank;
    c.pad = 0;
    if (rank) {
        const SpanRec p = r[rank - 1u];
        c.base = p.cum;
        c.plo = p.lo;
        c.phi = p.hi;
    } else {
        c.base = 0;
        c.plo = 1;
        c.phi = 0;
    }
#pragma unroll
    for (uint32_t u = 0; u < 5u; ++u) {
        const bool in = rank + u < G.n;
        const SpanRec q = r[in ? rank + u : 0u];
        c.lo[u] = in ? q.lo : 0;
        c.hi[u] = in ? q.hi : 0;
    }
    cells[j] = c;
}


// ---- index build on the device (Lapper::new, src/libs/redis.rs:236-324) -----------------------
// pack (start, stop) into one 64-bit key and number the intervals: a stable sort of the keys inside
// every group is intervals.sort() of rust-lapper (ties keep the caller's order)
__global__ __launch_bounds__(256) void index_pack_kernel(const uint32_t *starts, const uint32_t *stops, uint64_t m,
                                                         uint64_t *key, uint32_t *val) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= m) return;
    key[i] = ((uint64_t)starts[i] << 32) | stops[i];
    val[i] = (uint32_t)i;
}

// sorted keys + permutation -> the ascending starts and the 16-B scan records
__global__ __launch_bounds__(256) void index_unpack_kernel(const uint64_t *key, const uint32_t *perm, uint64_t m,
                                                           uint32_t *lstart, IvRec *lrec) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= m) return;
    const uint64_t k = key[i];
    lstart[i] = (uint32_t)(k >> 32);
    lrec[i] = IvRec{(uint32_t)(k >> 32), (uint32_t)k, (uint64_t)perm[i]};
}

// one wavefront per group: max(stop - start) (Lapper::max_len) and the directory headers
__global__ __launch_bounds__(64) void index_group_kernel(const uint32_t *off32, uint32_t n_groups,
                                                         const IvRec *lrec, const uint32_t *lstart,
                                                         const uint32_t *stops_sorted, IndexGroup *groups,
                                                         CountGroup *cgroups) {
    const uint32_t g = blockIdx.x;
    if (g >= n_groups) return;
    const uint32_t lo = off32[g], hi = off32[g + 1], n = hi - lo;
    uint32_t ml = 0;
    for (uint32_t i = lo + threadIdx.x; i < hi; i += 64u) {
        const IvRec r = lrec[i];
        if (r.stop > r.start) ml = max(ml, r.stop - r.start);
    }
    for (int d = 32; d; d >>= 1) ml = max(ml, (uint32_t)__shfl_xor((int)ml, d, 64));
    if (threadIdx.x == 0) {
        IndexGroup G;
        G.off = lo;
        G.n = n;
        G.maxlen = ml;
        G.start = n ? dir_params(lstart[lo], lstart[hi - 1], n) : KeyDir{0u, 0u, 0u, 0u};
        G.stop = n ? dir_params(stops_sorted[lo], stops_sorted[hi - 1], n) : KeyDir{0u, 0u, 0u, 0u};
        // the count path's bucket records: ONE grid of cells over the group's coordinates for both key
        // arrays, so that the record of the starts and the record of the stops of a cell sit side by side
        G.bk_start = n ? dir_params(min(lstart[lo], stops_sorted[lo]), max(lstart[hi - 1], stops_sorted[hi - 1]), (n >> kCellShift) + 1u)
                       : KeyDir{0u, 0u, 0u, 0u};
        G.bk_stop = G.bk_start;
        groups[g] = G;
        cgroups[g] = CountGroup{lo, n, G.bk_start.key0, G.bk_start.nb, G.bk_stop.key0, G.bk_stop.nb, G.bk_start.shift,
                                G.bk_stop.shift};
    }
}

// bucket directories: slot j of the directory array belongs to the group g with off[g] + g <= j
// (its bucket b = j - off[g] - g); dir[b] = rank of the first key >= key0 + (b << shift), dir[nb] = n
__global__ __launch_bounds__(256) void index_dir_kernel(const uint32_t *off32, uint32_t n_groups, uint64_t slots,
                                                        const IndexGroup *groups, const uint32_t *lstart,
                                                        uint32_t *dir_start) {
    const uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (j >= slots) return;
    uint32_t lo = 0, hi = n_groups;                 // last group with off[g] + g <= j
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if ((uint64_t)off32[mid] + mid <= j)
            lo = mid;
        else
            hi = mid;
    }
    const uint32_t g = lo;
    const IndexGroup G = groups[g];
    const uint32_t b = (uint32_t)(j - ((uint64_t)off32[g] + g));
    auto fill = [&](const uint32_t *keys, const KeyDir d, uint32_t *dir) {
        if (b > d.nb || (G.n == 0 && b > 0)) return;
        uint32_t r = G.n;
        if (b < d.nb) {
            const uint64_t edge = (uint64_t)d.key0 + ((uint64_t)b << d.shift);
            uint32_t a = 0, z = G.n;
            while (a < z) {
                const uint32_t mid = a + ((z - a) >> 1);
                if ((uint64_t)keys[G.off + mid] < edge)
                    a = mid + 1;
                else
                    z = mid;
            }
            r = a;
        }
        dir[j] = G.n == 0 ? 0u : r;
    };
    fill(lstart, G.start, dir_start);
}

// bucket records of the count path: slot j belongs to the group g with off[g]/4 + 2g <= j, bucket b = j - that
__global__ __launch_bounds__(256) void index_bk_kernel(const uint32_t *off32, uint32_t n_groups, uint64_t slots,
                                                       const IndexGroup *groups, const uint32_t *lstart,
                                                       const uint32_t *stops_sorted, BkRec *bk_start, BkRec *bk_stop) {
    const uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (j >= slots) return;
    uint32_t lo = 0, hi = n_groups;
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if ((uint64_t)(off32[mid] >> kCellShift) + 2ull * mid <= j)
            lo = mid;
        else
            hi = mid;
    }
    const uint32_t g = lo;
    const IndexGroup G = groups[g];
    const uint64_t b = j - ((uint64_t)(off32[g] >> kCellShift) + 2ull * g);
    auto fill = [&](const uint32_t *keys, const KeyDir d, BkRec *bk) {
        if (G.n == 0 || b >= d.nb) return;
        const uint64_t edge = (uint64_t)d.key0 + (b << d.shift);
        uint32_t a = 0, z = G.n;
        while (a < z) {
            const uint32_t mid = a + ((z - a) >> 1);
            if ((uint64_t)keys[G.off + mid] < edge)
                a = mid + 1;
            else
                z = mid;
        }
        BkRec r;
        r.rank = a;
#pragma unroll
        for (uint32_t i = 0; i < 7u; ++i) r.k[i] = a + i < G.n ? keys[G.off + a + i] : 0xffffffffu;
        bk[2u * j] = r;                                // cell j: starts' record, stops' record (64 B together)
    };
    fill(lstart, G.bk_start, bk_start);
    fill(stops_sorted, G.bk_stop, bk_stop);
}

// ---- the whole build of ONE group in one workgroup (groups of at most kBuildCap intervals) --------------
// A group of idx:rg:{ctg} / idx:ctg:{chr} is a few thousand intervals: it fits a workgroup's LDS several times
// over, so Lapper::new (redis.rs:253,299: intervals.sort(), the stops sorted on their own, max_len) and every
// table derived from the sorted arrays are made where the data already is, with one pass over HBM in and one
// out -- against eight radix passes of a generic 64-bit segmented sort plus five kernels that each search the
// sorted arrays in global memory again (2.4 ms per 1.25e7 intervals in 4,000 groups).
//   sort      bitonic network over N = 2^ceil(log2 n) slots on the triple (start, stop, position in the
//             caller's order): the position breaks ties, which makes the network's result the STABLE order of
//             intervals.sort(); the stops ride along as a second, keys-only network in the same stages
//             (one barrier per stage for both);
//   outputs   ascending starts, 16-B scan records, sorted stops, max_len, the group's directory headers,
//             the bucket directory (one lower bound per slot, in LDS) and the count path's cell records.
constexpr uint32_t kBuildCap = 8192;
template <uint32_t CAP, uint32_t T>
__global__ __launch_bounds__(T) void index_build_kernel(const uint32_t *off32, uint32_t n_groups, const uint32_t *starts,
                                                        const uint32_t *stops, uint32_t *lstart, IvRec *lrec,
                                                        uint32_t *stops_sorted, IndexGroup *groups, CountGroup *cgroups,
                                                        uint32_t *dir_start, BkRec *bk_start, BkRec *bk_stop) {
    extern __shared__ __align__(16) unsigned char smem_b[];
    uint64_t *key = reinterpret_cast<uint64_t *>(smem_b);            // (start << 32) | stop
    uint32_t *skey = reinterpret_cast<uint32_t *>(key + CAP);        // stops, sorted on their own
    uint16_t *pos = reinterpret_cast<uint16_t *>(skey + CAP);        // position in the caller's order
    uint32_t *scr = reinterpret_cast<uint32_t *>(pos + CAP);         // 96 words: reductions [0, 64), the group record's parameters [64, 96)
    const uint32_t tid = threadIdx.x;
    const uint32_t g = blockIdx.x;
    if (g >= n_groups) return;
    const uint32_t lo = off32[g], n = off32[g + 1] - lo;
    uint32_t N = 4;
    while (N < n) N <<= 1;
    // The ranges of a real group are narrow (a ctg's coordinates: 20-odd bits): when (start - min start),
    // (stop - min stop) and the position fit 64 bits together, the triple is ONE word -- unique, so no tie
    // logic -- and a compare-exchange is two 8-B reads, one compare, two 8-B writes.  Otherwise the triple
    // stays (64-bit key, 16-bit position).
    uint32_t smin = ~0u, smax = 0u, tmin = ~0u, tmax = 0u;
    for (uint32_t i = tid; i < n; i += T) {
        const uint32_t a = starts[lo + i], b = stops[lo + i];
        smin = min(smin, a);
        smax = max(smax, a);
        tmin = min(tmin, b);
        tmax = max(tmax, b);
    }
    for (int d = 32; d; d >>= 1) {
        smin = min(smin, (uint32_t)__shfl_xor((int)smin, d, 64));
        smax = max(smax, (uint32_t)__shfl_xor((int)smax, d, 64));
        tmin = min(tmin, (uint32_t)__shfl_xor((int)tmin, d, 64));
        tmax = max(tmax, (uint32_t)__shfl_xor((int)tmax, d, 64));
    }
    if ((tid & 63u) == 0) {
        scr[(tid >> 6) * 4u + 0u] = smin;     // T / 64 <= 16 waves: scr[0..63] (the parameters below live behind them)
        scr[(tid >> 6) * 4u + 1u] = smax;
        scr[(tid >> 6) * 4u + 2u] = tmin;
        scr[(tid >> 6) * 4u + 3u] = tmax;
    }
    __syncthreads();
    for (uint32_t w = 0; w < T / 64u; ++w) {
        smin = min(smin, scr[w * 4u + 0u]);
        smax = max(smax, scr[w * 4u + 1u]);
        tmin = min(tmin, scr[w * 4u + 2u]);
        tmax = max(tmax, scr[w * 4u + 3u]);
    }
    __syncthreads();
    const uint32_t bs = n ? 32u - (uint32_t)__clz((int)((smax - smin) | 1u)) : 1u;
    const uint32_t bt = n ? 32u - (uint32_t)__clz((int)((tmax - tmin) | 1u)) : 1u;
    const uint32_t bp = 32u - (uint32_t)__clz((int)((N - 1u) | 1u));
    const bool one_word = bs + bt + bp <= 64u;
    for (uint32_t i = tid; i < N; i += T) {
        if (i < n) {
            const uint32_t a = starts[lo + i], b = stops[lo + i];
            key[i] = one_word ? ((uint64_t)(a - smin) << (bt + bp)) | ((uint64_t)(b - tmin) << bp) | i
                              : ((uint64_t)a << 32) | b;
            skey[i] = b;
            pos[i] = (uint16_t)i;
        } else {
            key[i] = ~0ull;                 // pads sort behind every interval: equal keys are ordered by position
            skey[i] = ~0u;
            pos[i] = 0xFFFFu;
        }
    }
    __syncthreads();
    if (one_word) {
        // Slots come in blocks of four (block o = slots 4o .. 4o+3, one thread each): the stages with j = 2 and j = 1 of every level (and
        // the levels k = 2 and k = 4 entirely) never leave them, so they run in registers between one 16-B/32-B
        // read and one write per array -- two barriers and four LDS round trips less per level.
        auto cex = [](uint64_t &x, uint64_t &y, bool up) {
            if ((x > y) == up && x != y) {
                const uint64_t t_ = x;
                x = y;
                y = t_;
            }
        };
        auto cex32 = [](uint32_t &x, uint32_t &y, bool up) {
            if ((x > y) == up && x != y) {
                const uint32_t t_ = x;
                x = y;
                y = t_;
            }
        };
        auto local = [&](uint32_t k) {            // k == 0: levels 2 and 4 from scratch; else stages j = 2, 1 of level k >= 8
            for (uint32_t o = tid; o < (N >> 2); o += T) {
                uint64_t *kp = key + 4u * o;
                uint32_t *sp = skey + 4u * o;
                uint64_t a0 = kp[0], a1 = kp[1], a2 = kp[2], a3 = kp[3];
                uint4 sv = *reinterpret_cast<uint4 *>(sp);
                const bool up = k ? ((4u * o) & k) == 0u : ((4u * o) & 4u) == 0u;
                if (k == 0u) {                     // level 2: pairs (0,1) ascending, (2,3) descending
                    cex(a0, a1, true);
                    cex(a2, a3, false);
                    cex32(sv.x, sv.y, true);
                    cex32(sv.z, sv.w, false);
                }
                cex(a0, a2, up);                   // j = 2
                cex(a1, a3, up);
                cex(a0, a1, up);                   // j = 1
                cex(a2, a3, up);
                cex32(sv.x, sv.z, up);
                cex32(sv.y, sv.w, up);
                cex32(sv.x, sv.y, up);
                cex32(sv.z, sv.w, up);
                kp[0] = a0;
                kp[1] = a1;
                kp[2] = a2;
                kp[3] = a3;
                *reinterpret_cast<uint4 *>(sp) = sv;
            }
            __syncthreads();
        };
        local(0u);
        for (uint32_t k = 8; k <= N; k <<= 1) {
            for (uint32_t j = k >> 1; j >= 4u; j >>= 1) {
                for (uint32_t t = tid; t < (N >> 1); t += T) {
                    const uint32_t i = ((t & ~(j - 1u)) << 1) | (t & (j - 1u));   // bit j clear
                    const uint32_t q = i | j;
                    const bool up = (i & k) == 0u;
                    const uint64_t ka = key[i], kb = key[q];
                    if ((ka > kb) == up && ka != kb) {
                        key[i] = kb;
                        key[q] = ka;
                    }
                    const uint32_t sa = skey[i], sb = skey[q];
                    if ((sa > sb) == up && sa != sb) {
                        skey[i] = sb;
                        skey[q] = sa;
                    }
                }
                __syncthreads();
            }
            local(k);
        }
        // back to (start << 32 | stop) and the position, in place
        const uint64_t mt = bt >= 32u ? 0xFFFFFFFFull : (1ull << bt) - 1ull, mp = (1ull << bp) - 1ull;
        for (uint32_t i = tid; i < n; i += T) {
            const uint64_t c = key[i];
            const uint32_t a = (uint32_t)(c >> (bt + bp)) + smin, b = (uint32_t)((c >> bp) & mt) + tmin;
            key[i] = ((uint64_t)a << 32) | b;
            pos[i] = (uint16_t)(c & mp);
        }
        __syncthreads();
    } else {
        for (uint32_t k = 2; k <= N; k <<= 1) {
            for (uint32_t j = k >> 1; j > 0; j >>= 1) {
                for (uint32_t t = tid; t < (N >> 1); t += T) {
                    const uint32_t i = ((t & ~(j - 1u)) << 1) | (t & (j - 1u));   // bit j clear
                    const uint32_t q = i | j;
                    const bool up = (i & k) == 0u;
                    const uint64_t ka = key[i], kb = key[q];
                    const uint32_t pa = pos[i], pb = pos[q];
                    const bool gt = ka > kb || (ka == kb && pa > pb);
                    if (gt == up) {
                        key[i] = kb;
                        key[q] = ka;
                        pos[i] = (uint16_t)pb;
                        pos[q] = (uint16_t)pa;
                    }
                    const uint32_t sa = skey[i], sb = skey[q];
                    if ((sa > sb) == up && sa != sb) {
                        skey[i] = sb;
                        skey[q] = sa;
                    }
                }
                __syncthreads();
            }
        }
    }
    // sorted arrays out; max(stop - start)
    uint32_t ml = 0;
    for (uint32_t i = tid; i < n; i += T) {
        const uint64_t kk = key[i];
        const uint32_t a = (uint32_t)(kk >> 32), b = (uint32_t)kk;
        lstart[lo + i] = a;
        lrec[lo + i] = IvRec{a, b, (uint64_t)lo + pos[i]};
        stops_sorted[lo + i] = skey[i];
        if (b > a) ml = max(ml, b - a);
    }
    for (int d = 32; d; d >>= 1) ml = max(ml, (uint32_t)__shfl_xor((int)ml, d, 64));
    if ((tid & 63u) == 0) scr[tid >> 6] = ml;
    __syncthreads();
    if (tid == 0) {
        for (uint32_t w = 1; w < T / 64u; ++w) ml = max(ml, scr[w]);
        IndexGroup G;
        G.off = lo;
        G.n = n;
        G.maxlen = ml;
        const KeyDir none{0u, 0u, 0u, 0u};
        const uint32_t s0 = n ? (uint32_t)(key[0] >> 32) : 0u, s1 = n ? (uint32_t)(key[n - 1] >> 32) : 0u;
        const uint32_t t0 = n ? skey[0] : 0u, t1 = n ? skey[n - 1] : 0u;
        G.start = n ? dir_params(s0, s1, n) : none;
        G.stop = n ? dir_params(t0, t1, n) : none;
        G.bk_start = n ? dir_params(min(s0, t0), max(s1, t1), (n >> kCellShift) + 1u) : none;
        G.bk_stop = G.bk_start;
        groups[g] = G;
        cgroups[g] = CountGroup{lo, n, G.bk_start.key0, G.bk_start.nb, G.bk_stop.key0, G.bk_stop.nb, G.bk_start.shift,
                                G.bk_stop.shift};
        scr[64] = G.start.key0;
        scr[65] = G.start.shift;
        scr[66] = G.start.nb;
        scr[67] = G.bk_start.key0;
        scr[68] = G.bk_start.shift;
        scr[69] = G.bk_start.nb;
    }
    __syncthreads();
    if (n == 0) {
        if (tid == 0) dir_start[(uint64_t)lo + g] = 0u;
        return;
    }
    // bucket directory over the starts (locate): slot b of the group's n + 1 at dir_start[lo + g + b]
    {
        const uint32_t key0 = scr[64], shift = scr[65], nb = scr[66];
        for (uint32_t b = tid; b <= nb; b += T) {
            uint32_t r = n;
            if (b < nb) {
                const uint64_t edge = (uint64_t)key0 + ((uint64_t)b << shift);
                uint32_t a = 0, z = n;
                while (a < z) {
                    const uint32_t mid = a + ((z - a) >> 1);
                    if ((key[mid] >> 32) < edge)
                        a = mid + 1;
                    else
                        z = mid;
                }
                r = a;
            }
            dir_start[(uint64_t)lo + g + b] = r;
        }
    }
    // cell records of the count path: cell b of the group at (lo >> kCellShift) + 2g + b, the starts' and the
    // stops' record side by side
    {
        const uint32_t key0 = scr[67], shift = scr[68], nb = scr[69];
        const uint64_t cell0 = (uint64_t)(lo >> kCellShift) + 2ull * g;
        for (uint32_t b = tid; b < nb; b += T) {
            const uint64_t edge = (uint64_t)key0 + ((uint64_t)b << shift);
            BkRec rs, rt;
            {
                uint32_t a = 0, z = n;
                while (a < z) {
                    const uint32_t mid = a + ((z - a) >> 1);
                    if ((key[mid] >> 32) < edge)
                        a = mid + 1;
                    else
                        z = mid;
                }
                rs.rank = a;
#pragma unroll
                for (uint32_t i = 0; i < 7u; ++i) rs.k[i] = a + i < n ? (uint32_t)(key[a + i] >> 32) : 0xffffffffu;
            }
            {
                uint32_t a = 0, z = n;
                while (a < z) {
                    const uint32_t mid = a + ((z - a) >> 1);
                    if ((uint64_t)skey[mid] < edge)
                        a = mid + 1;
                    else
                        z = mid;
                }
                rt.rank = a;
#pragma unroll
                for (uint32_t i = 0; i < 7u; ++i) rt.k[i] = a + i < n ? skey[a + i] : 0xffffffffu;
            }
            bk_start[2u * (cell0 + b)] = rs;
            bk_stop[2u * (cell0 + b)] = rt;
        }
    }
}

template <uint32_t CAP, uint32_t T>
hipError_t index_build_launch(gams_gpu_t *h, hipStream_t st, const uint32_t *off32, uint32_t n_groups, const uint32_t *starts,
                              const uint32_t *stops, gams_index_t *ix) {
    const size_t lds = (size_t)CAP * (8 + 4 + 2) + 96 * 4;
    auto kern = index_build_kernel<CAP, T>;
    hipError_t e = gams_lds_attr(h, reinterpret_cast<const void *>(kern), lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3(n_groups), dim3(T), lds, st, off32, n_groups, starts, stops, ix->d_lstart, ix->d_lrec,
                       ix->d_stops, ix->d_groups, ix->d_cgroups, ix->d_dir_start, ix->d_bk_start, ix->d_bk_stop);
    return hipGetLastError();
}

// Host side of the directory: keys[0..n) ascending (already biased); dir gets nb+1 <= n+1 entries.
KeyDir build_dir(const uint32_t *keys, uint32_t n, uint32_t *dir) {
    KeyDir d{0u, 0u, 0u, 0u};
    if (n == 0) {
        dir[0] = 0;
        return d;
    }
    d.key0 = keys[0];
    const uint64_t range = (uint64_t)keys[n - 1] - (uint64_t)keys[0];
    while ((range >> d.shift) >= n) ++d.shift;     // (range >> shift) + 1 <= n buckets; ends at shift <= 32
    d.nb = (uint32_t)(range >> d.shift) + 1u;
    uint32_t i = 0;
    for (uint32_t b = 0; b < d.nb; ++b) {
        const uint64_t edge = (uint64_t)d.key0 + ((uint64_t)b << d.shift);
        while (i < n && (uint64_t)keys[i] < edge) ++i;
        dir[b] = i;
    }
    dir[d.nb] = n;
    return d;
}

// run fn(g) for every group on up to 16 host threads (the per-group sorts dominate index creation)
template <typename F>
void for_groups(uint32_t n_groups, F fn) {
    const unsigned T = std::max(1u, std::min({16u, std::thread::hardware_concurrency(), n_groups}));
    if (T <= 1) {
        for (uint32_t g = 0; g < n_groups; ++g) fn(g);
        return;
    }
    std::atomic<uint32_t> next{0};
    std::vector<std::thread> pool;
    for (unsigned t = 0; t < T; ++t)
        pool.emplace_back([&] {
            for (uint32_t g = next.fetch_add(1); g < n_groups; g = next.fetch_add(1)) fn(g);
        });
    for (auto &th : pool) th.join();
}

template <typename T>
hipError_t to_device(T **d, const T *hsrc, size_t n) {
    hipError_t e = hipMalloc(d, std::max<size_t>(n, 1) * sizeof(T));
    if (e != hipSuccess) return e;
    if (n) e = hipMemcpy(*d, hsrc, n * sizeof(T), hipMemcpyHostToDevice);
    return e;
}

// Host columns in, one host column out, through the three query kernels.  The queries go in chunks of
// 2^21: chunk c+1 is copied in (copy stream) while chunk c is searched (compute stream) and chunk c-1 is
// copied out (readback stream), two device slots.  With page-locked host arrays (gams_gpu_host_alloc) the
// three overlap and the call runs at the rate of the PCIe link; pageable arrays work, staged by the runtime.
struct QCol {
    const void *host;
    size_t elem;
};

template <typename F>
int query_pipeline(gams_gpu_t *h, uint64_t nq, const QCol *cols, int ncol, void *out_host, size_t out_elem, F launch) {
    const uint64_t CH = std::min<uint64_t>(nq, 1ull << 21);
    const uint64_t nchunk = (nq + CH - 1) / CH;
    const int nslot = nchunk > 1 ? 2 : 1;
    const std::string who = "query";
    size_t slot_bytes = gams_align256(CH * out_elem);
    for (int k = 0; k < ncol; ++k) slot_bytes += gams_align256(CH * cols[k].elem);
    PoolBlock block(h, false, h->copy, h->compute, h->readback);   // the three streams of the pipeline
    GAMS_TRY(h, who, block.alloc(slot_bytes * nslot));
    for (int s = 0; s < 2; ++s)
        for (int k = 0; k < 3; ++k)
            if (!h->q_ev[s][k]) GAMS_TRY(h, who, hipEventCreateWithFlags(&h->q_ev[s][k], hipEventDisableTiming));
    GAMS_TRY(h, who, gams_stopwatch_reserve(h, nchunk));
    const StageClock chunk{h, h->compute};             // one timed pair per chunk
    h->kq_used = 0;
    // whatever the caller queued on the compute stream before (index build, uploads) comes first
    GAMS_TRY(h, who, hipEventRecord(h->k0, h->compute));
    GAMS_TRY(h, who, hipStreamWaitEvent(h->copy, h->k0, 0));
    std::vector<void *> d_in((size_t)ncol);
    for (uint64_t c = 0; c < nchunk; ++c) {
        const int s = (int)(c & 1);
        const uint64_t lo = c * CH, n = std::min<uint64_t>(CH, nq - lo);
        uint8_t *p = block.p + (size_t)s * slot_bytes;
        if (c >= 2) GAMS_TRY(h, who, hipStreamWaitEvent(h->copy, h->q_ev[s][1], 0));       // chunk c-2's kernel has read its inputs
        for (int k = 0; k < ncol; ++k) {
            d_in[(size_t)k] = p;
            GAMS_TRY(h, who, hipMemcpyAsync(p, static_cast<const uint8_t *>(cols[k].host) + lo * cols[k].elem, n * cols[k].elem,
                                 hipMemcpyHostToDevice, h->copy));
            p += gams_align256(CH * cols[k].elem);
        }
        void *d_out = p;
        GAMS_TRY(h, who, hipEventRecord(h->q_ev[s][0], h->copy));
        GAMS_TRY(h, who, hipStreamWaitEvent(h->compute, h->q_ev[s][0], 0));
        if (c >= 2) GAMS_TRY(h, who, hipStreamWaitEvent(h->compute, h->q_ev[s][2], 0));    // chunk c-2's results are out
        GAMS_TRY(h, who, chunk((int)c, true));
        launch(d_in.data(), d_out, n, h->compute);
        GAMS_TRY(h, who, hipGetLastError());
        GAMS_TRY(h, who, chunk((int)c, false));
        GAMS_TRY(h, who, hipEventRecord(h->q_ev[s][1], h->compute));
        GAMS_TRY(h, who, hipStreamWaitEvent(h->readback, h->q_ev[s][1], 0));
        GAMS_TRY(h, who, hipMemcpyAsync(static_cast<uint8_t *>(out_host) + lo * out_elem, d_out, n * out_elem,
                             hipMemcpyDeviceToHost, h->readback));
        GAMS_TRY(h, who, hipEventRecord(h->q_ev[s][2], h->readback));
    }
    h->kq_used = (int)nchunk;
    h->kq_staged = false;
    h->k_valid = true;
    GAMS_TRY(h, who, hipStreamSynchronize(h->readback));
    return GAMS_OK;
}

}  // namespace

// ---- the builder behind gams_index_create (and text.hip's gams_index_create_range_text) ------------------------
// begin: the index's arena and the build's scratch for n_groups groups of m intervals in all (m <= 2^32 - 16, checked by
// the caller).  The caller then fills cols.off32 (n_groups + 1 offsets), cols.starts_in and cols.stops_in (any order inside a
// group) by work queued on the compute stream, and calls run with the largest group's size.
int gams_index_build_begin(gams_gpu_t *h, uint32_t n_groups, uint64_t m, IndexBuild *B) {
    // Lapper::new on the device: intervals.sort() by (start, stop) inside every group = a stable
    // segmented radix sort of the packed 64-bit keys; the stops are also sorted on their own.  The
    // bucket directories and Lapper::max_len come from three small kernels over the sorted arrays.
    B->bk_slots = (m >> kCellShift) + 2ull * n_groups + 2;
    gams_index_t *ix = new gams_index_t();
    B->ix = ix;
    ix->n_groups = n_groups;
    ix->m = m;
    auto arena = [&](Carver &c) { return index_arena_layout<IndexGroup, CountGroup, IvRec, BkRec>(c, n_groups, m, B->bk_slots); };
    auto scratch = [&](Carver &c) { return index_scratch_layout(c, n_groups, m); };
    PoolBlock blk(h, false);
    hipError_t e = blk.alloc(layout_bytes(arena));
    if (e != hipSuccess) return gams_index_build_fail(h, B, e, "hipMalloc(index)");
    ix->arena = blk.release(&ix->arena_bytes);           // the index owns it from here (gams_index_destroy)
    const auto a = carve(ix->arena, arena);
    ix->d_groups = a.groups;
    ix->d_cgroups = a.cgroups;
    ix->d_stops = a.stops;
    ix->d_lstart = a.lstart;
    ix->d_lrec = a.lrec;
    ix->d_dir_start = a.dir_start;
    ix->d_bk_start = a.bk;     // 2 * bk_slots records, interleaved: cell j = [2j] starts, [2j+1] stops
    ix->d_bk_stop = a.bk + 1;
    // scratch: raw columns, packed keys in/out, permutation in/out, 32-bit offsets
    e = B->scratch.alloc(layout_bytes(scratch));
    if (e != hipSuccess) return gams_index_build_fail(h, B, e, "hipMalloc(scratch)");
    B->cols = carve(B->scratch.p, scratch);
    return GAMS_OK;
}

// a failed build: everything of the build back in the pools (each block once its stream has drained), the error reported
int gams_index_build_fail(gams_gpu_t *h, IndexBuild *B, hipError_t err, const char *what) {
    (void)hipGetLastError();
    B->scratch.reset();
    B->d_tmp.reset();
    gams_index_destroy(h, B->ix);
    B->ix = nullptr;
    return gams_fail(h, err == hipErrorOutOfMemory ? GAMS_ENOMEM : GAMS_EHIP,
                     std::string("index_create: ") + what + ": " + hipGetErrorString(err));
}

// run: sorts and tables from the device columns; waits for the build, frees the scratch, hands the index out
int gams_index_build_run(gams_gpu_t *h, IndexBuild *B, uint32_t max_n, gams_index_t **out, hipEvent_t done) {
    gams_index_t *ix = B->ix;
    const uint32_t n_groups = ix->n_groups;
    const uint64_t m = ix->m, bk_slots = B->bk_slots;
    const IndexScratch &c = B->cols;
    size_t tmp_bytes_pairs = 0, tmp_bytes_keys = 0;
    hipStream_t st = h->compute;
    hipError_t e;
    auto fail = [&](hipError_t err, const char *what) { return gams_index_build_fail(h, B, err, what); };
    if (n_groups && max_n <= kBuildCap) {
        // every group fits a workgroup: sort and every derived table in one kernel, one workgroup per group
        if (max_n <= 256)
            e = index_build_launch<256, 128>(h, st, c.off32, n_groups, c.starts_in, c.stops_in, ix);
        else if (max_n <= 1024)
            e = index_build_launch<1024, 512>(h, st, c.off32, n_groups, c.starts_in, c.stops_in, ix);
        else if (max_n <= 2048)
            e = index_build_launch<2048, 1024>(h, st, c.off32, n_groups, c.starts_in, c.stops_in, ix);
        else if (max_n <= 4096)
            e = index_build_launch<4096, 1024>(h, st, c.off32, n_groups, c.starts_in, c.stops_in, ix);
        else
            e = index_build_launch<8192, 1024>(h, st, c.off32, n_groups, c.starts_in, c.stops_in, ix);
        if (e != hipSuccess) return fail(e, "group build");
    } else if (m) {
        // a group beyond the workgroup's LDS: the library's segmented radix sort + the table kernels
        const unsigned blocks = (unsigned)((m + 255) / 256);
        hipLaunchKernelGGL(index_pack_kernel, dim3(blocks), dim3(256), 0, st, c.starts_in, c.stops_in, m, c.key_in,
                           c.val_in);
        if ((e = hipGetLastError()) != hipSuccess) return fail(e, "pack");
        e = rocprim::segmented_radix_sort_pairs(nullptr, tmp_bytes_pairs, c.key_in, c.key_out, c.val_in, c.val_out,
                                                (unsigned)m, n_groups, c.off32, c.off32 + 1, 0, 64, st);
        if (e != hipSuccess) return fail(e, "radix sort (size query)");
        e = rocprim::segmented_radix_sort_keys(nullptr, tmp_bytes_keys, c.stops_in, ix->d_stops, (unsigned)m, n_groups,
                                               c.off32, c.off32 + 1, 0, 32, st);
        if (e != hipSuccess) return fail(e, "radix sort (size query)");
        e = B->d_tmp.alloc(std::max<size_t>(std::max(tmp_bytes_pairs, tmp_bytes_keys), 256));
        if (e != hipSuccess) return fail(e, "hipMalloc(sort storage)");
        e = rocprim::segmented_radix_sort_pairs(B->d_tmp.p, tmp_bytes_pairs, c.key_in, c.key_out, c.val_in, c.val_out,
                                                (unsigned)m, n_groups, c.off32, c.off32 + 1, 0, 64, st);
        if (e != hipSuccess) return fail(e, "radix sort of (start, stop)");
        e = rocprim::segmented_radix_sort_keys(B->d_tmp.p, tmp_bytes_keys, c.stops_in, ix->d_stops, (unsigned)m, n_groups,
                                               c.off32, c.off32 + 1, 0, 32, st);
        if (e != hipSuccess) return fail(e, "radix sort of stops");
        hipLaunchKernelGGL(index_unpack_kernel, dim3(blocks), dim3(256), 0, st, c.key_out, c.val_out, m, ix->d_lstart,
                           ix->d_lrec);
        if ((e = hipGetLastError()) != hipSuccess) return fail(e, "unpack");
    }
    if (n_groups && max_n > kBuildCap) {
        hipLaunchKernelGGL(index_group_kernel, dim3(n_groups), dim3(64), 0, st, c.off32, n_groups, ix->d_lrec,
                           ix->d_lstart, ix->d_stops, ix->d_groups, ix->d_cgroups);
        if ((e = hipGetLastError()) != hipSuccess) return fail(e, "group records");
        const uint64_t slots = m + n_groups;        // the last group's directory ends at m + n_groups (inclusive slot)
        hipLaunchKernelGGL(index_dir_kernel, dim3((unsigned)((slots + 1 + 255) / 256)), dim3(256), 0, st, c.off32,
                           n_groups, slots + 1, ix->d_groups, ix->d_lstart, ix->d_dir_start);
        if ((e = hipGetLastError()) != hipSuccess) return fail(e, "directories");
        hipLaunchKernelGGL(index_bk_kernel, dim3((unsigned)((bk_slots + 255) / 256)), dim3(256), 0, st, c.off32,
                           n_groups, bk_slots, ix->d_groups, ix->d_lstart, ix->d_stops, ix->d_bk_start, ix->d_bk_stop);
        if ((e = hipGetLastError()) != hipSuccess) return fail(e, "bucket records");
    }
    if (done && (e = hipEventRecord(done, st)) != hipSuccess) return fail(e, "index build");
    if ((e = hipStreamSynchronize(st)) != hipSuccess) return fail(e, "index build");
    B->scratch.reset();
    B->d_tmp.reset();
    B->ix = nullptr;
    *out = ix;
    return GAMS_OK;
}

extern "C" {

int gams_index_create(gams_gpu_t *h, uint32_t n_groups, const uint64_t *group_off, const uint32_t *starts,
                      const uint32_t *stops, gams_index_t **out) {
    // the host front: the checks, and the caller's arrays copied into the builder's device columns
    if (!h || !out || !group_off) return gams_fail(h, GAMS_EINVAL, "index_create: null argument");
    const uint64_t m = group_off[n_groups];
    if (m && (!starts || !stops)) return gams_fail(h, GAMS_EINVAL, "index_create: null interval arrays");
    for (uint32_t g = 0; g < n_groups; ++g)
        if (group_off[g] > group_off[g + 1]) return gams_fail(h, GAMS_EINVAL, "index_create: group_off not ascending");
    if (m > 0xfffffff0ull)
        return gams_fail(h, GAMS_EUNSUPPORTED, "index_create: more than 2^32-16 intervals in one index");
    GAMS_HIP(h, hipSetDevice(h->device));
    IndexBuild B(h);
    const int rc = gams_index_build_begin(h, n_groups, m, &B);
    if (rc != GAMS_OK) return rc;
    hipStream_t st = h->compute;
    hipError_t e;
    std::vector<uint32_t> off32((size_t)n_groups + 1);
    for (uint32_t g = 0; g <= n_groups; ++g) off32[g] = (uint32_t)group_off[g];
    if ((e = hipMemcpyAsync(B.cols.off32, off32.data(), off32.size() * 4, hipMemcpyHostToDevice, st)) != hipSuccess)
        return gams_index_build_fail(h, &B, e, "copy offsets");
    uint32_t max_n = 0;
    for (uint32_t g = 0; g < n_groups; ++g) max_n = std::max(max_n, off32[g + 1] - off32[g]);
    if (m) {
        if ((e = hipMemcpyAsync(B.cols.starts_in, starts, m * 4, hipMemcpyHostToDevice, st)) != hipSuccess)
            return gams_index_build_fail(h, &B, e, "copy starts");
        if ((e = hipMemcpyAsync(B.cols.stops_in, stops, m * 4, hipMemcpyHostToDevice, st)) != hipSuccess)
            return gams_index_build_fail(h, &B, e, "copy stops");
    }
    return gams_index_build_run(h, &B, max_n, out);
}

void gams_index_destroy(gams_gpu_t *h, gams_index_t *ix) {
    if (!ix) return;
    if (h) {
        (void)hipSetDevice(h->device);
        (void)hipStreamSynchronize(h->compute);
    }
    gams_pool_free(h, false, ix->arena, ix->arena_bytes);
    delete ix;
}


int gams_gpu_count(gams_gpu_t *h, gams_index_t *ix, const uint32_t *group, const uint32_t *qs,
                   const uint32_t *qe, uint64_t nq, int32_t *count) {
    if (!h || !ix || (nq && (!group || !qs || !qe || !count)))
        return gams_fail(h, GAMS_EINVAL, "gpu_count: null argument");
    if (nq == 0) return GAMS_OK;
    if ((nq + 255) / 256 > 0x7fffffffull) return gams_fail(h, GAMS_EUNSUPPORTED, "gpu_count: too many queries");
    GAMS_HIP(h, hipSetDevice(h->device));
    const QCol cols[3] = {{group, 4}, {qs, 4}, {qe, 4}};
    return query_pipeline(h, nq, cols, 3, count, sizeof(int32_t), [&](void *const *d, void *d_out, uint64_t n, hipStream_t st) {
        launch_interval_count(ix, static_cast<const uint32_t *>(d[0]), static_cast<const uint32_t *>(d[1]),
                              static_cast<const uint32_t *>(d[2]), n, static_cast<int32_t *>(d_out), st);
    });
}

int gams_gpu_locate(gams_gpu_t *h, gams_index_t *ix, const uint32_t *group, const uint32_t *qs,
                    const uint32_t *qe, uint64_t nq, int64_t *hit) {
    if (!h || !ix || (nq && (!group || !qs || !qe || !hit)))
        return gams_fail(h, GAMS_EINVAL, "gpu_locate: null argument");
    if (nq == 0) return GAMS_OK;
    if ((nq + 255) / 256 > 0x7fffffffull) return gams_fail(h, GAMS_EUNSUPPORTED, "gpu_locate: too many queries");
    GAMS_HIP(h, hipSetDevice(h->device));
    const QCol cols[3] = {{group, 4}, {qs, 4}, {qe, 4}};
    return query_pipeline(h, nq, cols, 3, hit, sizeof(int64_t), [&](void *const *d, void *d_out, uint64_t n, hipStream_t st) {
        launch_interval_locate(ix, static_cast<const uint32_t *>(d[0]), static_cast<const uint32_t *>(d[1]),
                               static_cast<const uint32_t *>(d[2]), n, static_cast<int64_t *>(d_out), st);
    });
}

int gams_spans_create(gams_gpu_t *h, uint32_t n_groups, const uint64_t *group_off, const int32_t *lo,
                      const int32_t *hi, gams_spans_t **out) {
    if (!h || !out || !group_off) return gams_fail(h, GAMS_EINVAL, "spans_create: null argument");
    const uint64_t m = group_off[n_groups];
    if (m && (!lo || !hi)) return gams_fail(h, GAMS_EINVAL, "spans_create: null span arrays");
    std::vector<SpanRec> rec(m);
    for (uint32_t g = 0; g < n_groups; ++g) {
        if (group_off[g] > group_off[g + 1]) return gams_fail(h, GAMS_EINVAL, "spans_create: group_off not ascending");
        if (group_off[g + 1] - group_off[g] > 0xfffffff0ull)
            return gams_fail(h, GAMS_EUNSUPPORTED, "spans_create: a group holds more than 2^32-16 spans");
        uint64_t c = 0;
        for (uint64_t i = group_off[g]; i < group_off[g + 1]; ++i) {
            if (hi[i] < lo[i] || (i > group_off[g] && lo[i] <= hi[i - 1]))
                return gams_fail(h, GAMS_EINVAL, "spans_create: spans must be sorted and disjoint");
            rec[i] = SpanRec{lo[i], hi[i], c};
            c += (uint64_t)((int64_t)hi[i] - lo[i] + 1);
        }
    }
    std::vector<SpanGroup> groups(std::max<uint32_t>(n_groups, 1));
    std::vector<uint32_t> dir(m + n_groups + 1);
    for_groups(n_groups, [&](uint32_t g) {
        const uint64_t o = group_off[g];
        const uint32_t n = (uint32_t)(group_off[g + 1] - o);
        std::vector<uint32_t> biased(n);
        for (uint32_t i = 0; i < n; ++i) biased[i] = (uint32_t)lo[o + i] ^ 0x80000000u;
        groups[g].off = o;
        groups[g].n = n;
        groups[g].lo = build_dir(biased.data(), n, dir.data() + o + g);
    });
    GAMS_HIP(h, hipSetDevice(h->device));
    gams_spans_t *sp = new gams_spans_t();
    sp->n_groups = n_groups;
    sp->m = m;
    hipError_t e = to_device(&sp->d_groups, groups.data(), groups.size());
    if (e == hipSuccess) e = to_device(&sp->d_rec, rec.data(), m);
    if (e == hipSuccess) e = to_device(&sp->d_dir_lo, dir.data(), dir.size());
    const uint64_t slots = m + n_groups + 1;
    if (e == hipSuccess) e = hipMalloc(&sp->d_cells, slots * sizeof(SpanCell));
    if (e == hipSuccess && n_groups) {
        hipLaunchKernelGGL(span_cell_kernel, dim3((unsigned)((slots + 255) / 256)), dim3(256), 0, h->compute, sp->d_groups,
                           n_groups, sp->d_rec, sp->d_dir_lo, slots, sp->d_cells);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(h->compute);
    }
    if (e != hipSuccess) {
        (void)hipGetLastError();
        gams_spans_destroy(h, sp);
        return gams_fail(h, e == hipErrorOutOfMemory ? GAMS_ENOMEM : GAMS_EHIP,
                         std::string("spans_create: ") + hipGetErrorString(e));
    }
    *out = sp;
    return GAMS_OK;
}

}  // extern "C"

// for runlist.hip, whose set is built on the device: the cell records of a set whose groups, records and directory are
// in place, queued on `st`
hipError_t gams_spans_launch_cells(const gams_spans_t *sp, hipStream_t st) {
    const uint64_t slots = sp->m + sp->n_groups + 1;
    if (sp->n_groups == 0) return hipSuccess;
    hipLaunchKernelGGL(span_cell_kernel, dim3((unsigned)((slots + 255) / 256)), dim3(256), 0, st, sp->d_groups, sp->n_groups,
                       sp->d_rec, sp->d_dir_lo, slots, sp->d_cells);
    return hipGetLastError();
}

extern "C" {

void gams_spans_destroy(gams_gpu_t *h, gams_spans_t *sp) {
    if (!sp) return;
    if (h) {
        (void)hipSetDevice(h->device);
        (void)hipStreamSynchronize(h->compute);
    }
    (void)hipFree(sp->d_groups);
    (void)hipFree(sp->d_dir_lo);
    (void)hipFree(sp->d_rec);
    (void)hipFree(sp->d_cells);
    delete sp;
}

int gams_gpu_cover(gams_gpu_t *h, gams_spans_t *sp, const uint32_t *group, const int32_t *clip_lo,
                   const int32_t *clip_hi, const int32_t *qs, const int32_t *qe, uint64_t nq, float *prop) {
    if (!h || !sp || (nq && (!group || !clip_lo || !clip_hi || !qs || !qe || !prop)))
        return gams_fail(h, GAMS_EINVAL, "gpu_cover: null argument");
    if (nq == 0) return GAMS_OK;
    if ((nq + 255) / 256 > 0x7fffffffull) return gams_fail(h, GAMS_EUNSUPPORTED, "gpu_cover: too many queries");
    GAMS_HIP(h, hipSetDevice(h->device));
    const QCol cols[5] = {{group, 4}, {clip_lo, 4}, {clip_hi, 4}, {qs, 4}, {qe, 4}};
    return query_pipeline(h, nq, cols, 5, prop, sizeof(float), [&](void *const *d, void *d_out, uint64_t n, hipStream_t st) {
        launch_span_cover(sp, static_cast<const uint32_t *>(d[0]), static_cast<const int32_t *>(d[1]),
                          static_cast<const int32_t *>(d[2]), static_cast<const int32_t *>(d[3]),
                          static_cast<const int32_t *>(d[4]), n, static_cast<float *>(d_out), st);
    });
}

}  // extern "C"
