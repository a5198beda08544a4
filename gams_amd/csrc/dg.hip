// dg.hip -- the nearest-neighbour free energy (src/libs/delta_g.rs: DeltaG::polymer) of many ranges of a seqset.
//
// A range's ΔG is a strictly sequential f32 sum over its dimers, so the parallelism is across ranges: one
// range per lane, 64 consecutive ranges per wave, one wave per workgroup.  A lane must not fetch its own bases a byte at a
// time, so the wave stages its group cooperatively, GAMS_DG_STAGE_BASES bases' worth of aligned 16-B pieces of every range
// per stage:
//   stage   eight lanes per range, eight ranges per trip: coalesced 16-B loads of the pieces that cover the range, 16
//           bases classified at once (dg_code4: 2-bit codes and an invalid mask), the ragged head and tail of the range
//           inside its first and last piece masked before they decide anything, the codes of piece w of range j stored at
//           LDS word w * 65 + j.  The walk's reads (64 lanes, consecutive words) are free of bank conflicts; a staging store
//           puts 4 ranges x 8 pieces of a 32-lane half on banks (w + j) % 32, up to 4 lanes a bank -- one store per
//           seventeen LDS reads of the walk, left as it is (SQ_LDS_BANK_CONFLICT not measured)
//   walk    every lane reads its words back one at a time and adds nn[4 * prev + cur] in order; the sixteen terms sit in
//           LDS (sixteen addresses, sixteen banks; equal addresses broadcast) or in a register read with ds_bpermute
//           (gams_gpu_dg_set_table; profiles/dg.txt has both)
// The accumulator, the last code (the dimer across the seam) and the first code stay in registers from stage to stage; a
// range's invalid flag is one LDS word the staging lanes OR into.  The stage loop runs while any lane has pieces left, so
// a 100-base window and a 65,535-base one go through the same code.  Then the terminal terms, the symmetry term -- even
// lengths only, a per-lane walk from both ends over the bytes that stops at the first mismatch -- and NaN for None.
// Every LDS word read was written in this launch: the flags and the table at its top, the codes by the stage in front.
#include "common.hpp"
#include "dg_code.hpp"
#include "range_batch.hpp"

#include <cmath>
#include <string>

namespace {
constexpr uint32_t kDgPieces = GAMS_DG_STAGE_BASES / 16u;   // 16-B pieces of a range per stage
constexpr uint32_t kDgPitch = 65u;                          // LDS words from piece w to piece w + 1 of a range
const std::string kRangeDg = "gpu_range_dg";

// the dimer term at transposed index i = c(prev) + 4 * c(cur): two bits further up the code word per base
template <bool kPermute>
__device__ __forceinline__ float dg_term(const float *nn_t, float mine, uint32_t i) {
    if (kPermute) return __int_as_float(__builtin_amdgcn_ds_bpermute((int)(i << 2), __float_as_int(mine)));
    return nn_t[i];
}

template <bool kPermute>
__global__ __launch_bounds__(64) void dg_kernel(const uint8_t *seq, const unsigned long long *off, const uint32_t *len,
                                                uint32_t n, const gams_dg_table_t *t, float *dg) {
    __shared__ uint32_t codes[kDgPieces * kDgPitch];
    __shared__ uint32_t flag[64];
    __shared__ float nn_t[16];
    const uint32_t lane = threadIdx.x;
    const uint32_t q = blockIdx.x * 64u + lane;
    const bool live = q < n;
    const unsigned long long o = live ? off[q] : 0ull;
    const uint32_t L = live ? len[q] : 0u;
    const uint32_t head = (uint32_t)o & 15u, tail = (head + L - 1u) & 15u;
    const uint32_t np = L ? (head + L + 15u) >> 4 : 0u;          // the 16-B pieces that cover the range
    const float mine = t->nn[((lane & 3u) << 2) | ((lane >> 2) & 3u)];   // lanes 0..15: the transposed table
    flag[lane] = 0u;
    if (lane < 16u) nn_t[lane] = mine;
    __syncthreads();

    float v = 0.0f;
    uint32_t prev = 0u, first = 0u;
    for (uint32_t s0 = 0u; __any(np > s0); s0 += kDgPieces) {
        // ---- stage: pieces [s0, s0 + kDgPieces) of every range that has them
        for (uint32_t it = 0u; it < 8u; ++it) {
            const uint32_t j = it * 8u + (lane >> 3);
            const uint32_t olo = (uint32_t)__shfl((int)(uint32_t)o, (int)j, 64), ohi = (uint32_t)__shfl((int)(uint32_t)(o >> 32), (int)j, 64);
            const uint32_t lj = (uint32_t)__shfl((int)L, (int)j, 64), npj = (uint32_t)__shfl((int)np, (int)j, 64);
            const unsigned long long oj = ((unsigned long long)ohi << 32) | olo;
            const uint32_t hj = olo & 15u, tj = (hj + lj - 1u) & 15u;
            const uint32_t cnt = npj > s0 ? min(npj - s0, kDgPieces) : 0u;
            const uint4 *src = reinterpret_cast<const uint4 *>(seq) + (oj >> 4) + s0;
            for (uint32_t w = lane & 7u; w < cnt; w += 8u) {
                const uint4 b = src[w];
                uint32_t c0, c1, c2, c3;
                const uint32_t inv = dg_code4(b.x, &c0) | (dg_code4(b.y, &c1) << 4) | (dg_code4(b.z, &c2) << 8) |
                                     (dg_code4(b.w, &c3) << 12);
                // the bytes in front of the range and behind it are not the range's
                const uint32_t lo = s0 + w == 0u ? hj : 0u, hi = s0 + w == npj - 1u ? tj : 15u;
                const uint32_t keep = ((2u << hi) - 1u) & ~((1u << lo) - 1u);
                if (inv & keep) atomicOr(&flag[j], 1u);
                codes[w * kDgPitch + j] = c0 | (c1 << 8) | (c2 << 16) | (c3 << 24);
            }
        }
        __syncthreads();
        // ---- walk: this lane's words, a dimer per base
        const uint32_t cnt = np > s0 ? min(np - s0, kDgPieces) : 0u;
        for (uint32_t w = 0u; __any(w < cnt); ++w) {
            const uint32_t cw = w < cnt ? codes[w * kDgPitch + lane] : 0u;   // (a lane past its pieces reads nothing)
            const uint32_t p = s0 + w;
            const uint32_t lo = p == 0u ? head : 0u, hi = p == np - 1u ? tail : 15u;
            const uint32_t add_lo = p == 0u ? lo + 1u : 0u;            // the range's first base closes no dimer
            const uint32_t add_hi = w < cnt ? hi + 1u : 0u;            // adds for bases [add_lo, add_hi)
            if (p == 0u) first = (cw >> (2u * lo)) & 3u;
            const unsigned long long x = ((unsigned long long)cw << 2) | prev;
#pragma unroll
            for (uint32_t k = 0u; k < 16u; ++k) {
                const float term = dg_term<kPermute>(nn_t, mine, (uint32_t)(x >> (2u * k)) & 15u);
                if (k >= add_lo && k < add_hi) v += term;
            }
            if (w < cnt) prev = (cw >> (2u * hi)) & 3u;
        }
        __syncthreads();
    }

    float out = __int_as_float(0x7fc00000);
    if (live && L >= 3u && flag[lane] == 0u) {
        v += t->init[first];
        v += t->init[prev];
        if (!(L & 1u)) {                                               // its own reverse complement: c[i] + c[L-1-i] == 3
            const uint8_t *a = seq + o;
            uint32_t i = 0u;
            const uint32_t half = L >> 1;
            while (i < half && dg_code1(a[i]) + dg_code1(a[L - 1u - i]) == 3u) ++i;
            if (i == half) v += t->sym;
        }
        out = v;
    }
    if (live) dg[q] = out;
}
}  // namespace

int gams_dg_table_check(gams_gpu_t *h, const std::string &who, const gams_dg_table_t *t) {
    if (!t) return gams_fail(h, GAMS_EINVAL, who + ": null table");
    bool ok = std::isfinite(t->sym);
    for (float x : t->nn) ok = ok && std::isfinite(x);
    for (float x : t->init) ok = ok && std::isfinite(x);
    return ok ? GAMS_OK : gams_fail(h, GAMS_EINVAL, who + ": the table has a non-finite entry");
}

int gams_dg_seq_ready(gams_gpu_t *h, gams_seqset_t *s) {
    if (!s->have_bytes) return gams_fail(h, GAMS_ESTATE, "the seqset holds the G/C plane only: this call needs the sequence bytes");
    return gams_seqset_read_begin(h, s);
}

void gams_launch_dg(gams_gpu_t *h, const gams_seqset_t *s, const unsigned long long *d_off, const uint32_t *d_len, uint32_t n,
                    const gams_dg_table_t *d_table, float *d_dg) {
    if (!n) return;
    const dim3 grid((n + 63u) / 64u);
    if (h->dg_table == GAMS_DG_TABLE_BPERMUTE)
        hipLaunchKernelGGL(dg_kernel<true>, grid, dim3(64), 0, h->compute, s->d_seq, d_off, d_len, n, d_table, d_dg);
    else
        hipLaunchKernelGGL(dg_kernel<false>, grid, dim3(64), 0, h->compute, s->d_seq, d_off, d_len, n, d_table, d_dg);
}

extern "C" int gams_gpu_dg_set_table(gams_gpu_t *h, int placement) {
    if (!h || (placement != GAMS_DG_TABLE_LDS && placement != GAMS_DG_TABLE_BPERMUTE))
        return gams_fail(h, GAMS_EINVAL, "gpu_dg_set_table: unknown placement");
    h->dg_table = placement;
    return GAMS_OK;
}

namespace {
struct DgCols {   // table | off | len
    gams_dg_table_t *table;
    unsigned long long *off;
    uint32_t *len;
};
struct RangeDgEntry {   // what gams_range_batch (range_batch.hpp) asks of an entry
    gams_gpu_t *h;
    const RangeBatch &b;
    const gams_dg_table_t *table;
    int admit() const { return gams_dg_table_check(h, kRangeDg, table); }
    DgCols inputs(Carver &c, uint32_t n) const {
        DgCols k{};
        k.table = c.take<gams_dg_table_t>(1);
        k.off = c.take<unsigned long long>(n);
        k.len = c.take<uint32_t>(n);
        return k;
    }
    void head(const DgCols &in) const { *in.table = *table; }
    int range(const DgCols &in, uint32_t k, uint64_t q) const {
        const uint64_t bases = (uint64_t)((int64_t)b.range_end[q] - b.range_start[q]) + 1u;
        if (bases > kDgMaxBases) return gams_fail(h, GAMS_EUNSUPPORTED, b.which(kRangeDg, k, q) + " has more than 65535 bases");
        in.off[q] = b.s->off[b.ctg_index[k]] + (uint64_t)((int64_t)b.range_start[q] - b.chr_start[k]);
        in.len[q] = (uint32_t)bases;
        return GAMS_OK;
    }
    int ready() const { return gams_dg_seq_ready(h, b.s); }
    void launch(const DgCols &d, uint32_t n, float *d_dg) const { gams_launch_dg(h, b.s, d.off, d.len, n, d.table, d_dg); }
};
}  // namespace

extern "C" int gams_gpu_range_dg_batch(gams_gpu_t *h, gams_seqset_t *s, uint32_t n_sel, const uint32_t *ctg_index,
                                       const int32_t *chr_start, const uint64_t *range_off, const int32_t *range_start,
                                       const int32_t *range_end, const gams_dg_table_t *table, float *dg) {
    const RangeBatch b{s, n_sel, ctg_index, chr_start, range_off, range_start, range_end, dg};
    return gams_range_batch(h, kRangeDg, b, RangeDgEntry{h, b, table});
}
