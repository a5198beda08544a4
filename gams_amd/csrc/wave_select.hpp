// wave_select.hpp -- which tile kernel a wave plan launches, over which tile, in how many threads.
//
// Plain C++17, no HIP: the one list of wave_fast_kernel instantiations the library builds (wave.hip expands it into its
// table of kernel pointers) and the one function that chooses from it.  A new instantiation is one line in
// WAVE_FAST_INSTANCES plus a recipe in tests/wave_instances.py; tests/test_wave_select_cpu.py pins every choice made here.
// Beside the list: wave_select_body (which plans run their plane-fed passes in the narrow body of the headline tile,
// tests/test_wave_body_cpu.py) and wave_select_cut (that body in two waves x 24 windows or one wave x 48,
// tests/test_wave_cut_cpu.py).
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>

#include "../../include/gams_gpu.h"

namespace {

// wave_fast_kernel<W, SIZE, STEP, LAG, NT, NTH>, each tuple with NT false and true.
//   SIZE = 0:            size, step and lag are arguments
//   SIZE, STEP, LAG:     all three baked into the instruction stream (BASELINE's configurations)
//   SIZE, STEP, LAG = 0: size and step baked, the lag an argument (`--lag N` next to the default size: the reference's own
//                        benchmark runs 100 / 5 / 200 and 100 / 20 / 50, doc/benchmark/Atha.md:55,276-280)
// Beside them: wave_fast_taper_kernel<100, 10, 100, NT> (the tapered table of the (12, 100, 10, 100, 256) entry) and
// wave_tile_kernel<KT, WIDE> for KT = unsigned char / unsigned short, WIDE = false / true; and wave_fast_narrow_kernel,
// the (12, 100, 10, 100, 256) tile as 128 threads x 24 windows (wave_select_body below decides who takes it), and
// wave_fast_onewave_kernel, the same tile as 64 threads x 48 windows (wave_select_cut).
#define WAVE_FAST_INSTANCES(X)                                                                        \
    X(20, 0, 0, 0, 256) X(12, 0, 0, 0, 256) X(8, 0, 0, 0, 256) X(4, 0, 0, 0, 256)                     \
    X(28, 100, 1, 100, 64) X(28, 100, 1, 100, 128) X(28, 100, 1, 100, 256)                            \
    X(20, 100, 1, 100, 256) X(12, 100, 1, 100, 256)                                                   \
    X(12, 100, 10, 100, 64) X(12, 100, 10, 100, 128) X(12, 100, 10, 100, 256)                         \
    X(8, 100, 10, 100, 256) X(4, 100, 10, 100, 256)                                                   \
    X(4, 100, 5, 0, 256) X(8, 100, 5, 0, 256) X(12, 100, 5, 0, 256)                                   \
    X(4, 100, 10, 0, 256) X(8, 100, 10, 0, 256) X(12, 100, 10, 0, 256)                                \
    X(4, 100, 20, 0, 256) X(8, 100, 20, 0, 256) X(12, 100, 20, 0, 256)                                \
    X(20, 100, 1, 0, 256)                                                                             \
    X(20, 100, 5, 0, 64) X(20, 100, 5, 0, 128) X(20, 100, 5, 0, 256)                                  \
    X(28, 100, 1, 0, 64) X(28, 100, 1, 0, 128) X(28, 100, 1, 0, 256)

struct WaveInstance {
    int w, size, step, lag, nth;
};
#define WAVE_X_TUPLE(W, SIZE, STEP, LAG, NTH) {W, SIZE, STEP, LAG, NTH},
constexpr WaveInstance kWaveFast[] = {WAVE_FAST_INSTANCES(WAVE_X_TUPLE)};
#undef WAVE_X_TUPLE
constexpr int kWaveFastCount = (int)(sizeof(kWaveFast) / sizeof(kWaveFast[0]));

constexpr uint32_t kMaxTileBytes = 65520;  // chunk prefix is 16 bits
constexpr uint32_t kMaxTw = 8192;          // 2 bits/iteration in a 64-bit register
// sequence loads with the streaming hint once the batch is too large to live in L2 between passes
// (kStreamBytes: twice the 32 MiB of L2)
constexpr uint64_t kStreamBytes = 64ull << 20;

// everything the choice depends on
struct WaveSelectIn {
    gams_wave_params_t prm;
    uint32_t flags;              // GAMS_WAVE_PEAKS | GAMS_WAVE_DENSE
    bool serial, repair;         // influence != 1; ... by guess-and-iterate
    uint32_t depth;              // passes in flight
    uint64_t total_windows;
    uint32_t tw_req, nth_req;    // gams_wave_plan_set_tile / _set_threads (0: the library's choice)
    int taper_req;               // gams_wave_plan_set_taper: -1 auto, 0 off, 1 on
    int cus;                     // compute units of the device
    uint64_t set_bytes;          // size of the seqset
};

enum WaveFamily { kWaveFamDirect, kWaveFamFast, kWaveFamTaper, kWaveFamTile };

struct WaveSelection {
    WaveFamily family = kWaveFamDirect;
    int entry = -1;               // index into kWaveFast (fast and taper), else -1
    bool nt = false;              // the NT half of the pair: streaming loads
    bool k16 = false, wide = false;   // wave_tile_kernel<KT, WIDE>
    uint32_t nth = 256;           // threads per workgroup of the tile kernel (64 / 128: step-1 kernels, W = 28)
    uint32_t tw = 0;              // windows per tile
    uint32_t max_win = 0, max_chunks = 0;
    size_t lds_bytes = 0;
    bool taper = false;           // the tile table ends in W = 8 and W = 4 tiles (wave_fast_taper_kernel)
    bool direct = false;          // halo beyond a tile: one lane per window, no tiling (wave_direct_*_kernel)
};

// a round of workgroup slots: what the taper's threshold and the size of its tails are counted in
inline uint32_t wave_slots(int cus) { return 8u * (uint32_t)std::max(cus, 1); }

// The tapered tile table of the baked W = 12 kernel (wave_fast_taper_kernel): the ctgs holding the last windows of the
// batch are cut into W = 4 tiles, the ones before them into W = 8 tiles.  The two tails are pct4 / pct8 % of a round of
// workgroup slots (whole slots, a tile of that width each) and at most 8 % / 17 % of the batch.
// tests/test_wave_taper_cpu.py holds this arithmetic against the model of tests/taper.py.
struct WaveTaper {
    uint32_t tw4 = 0, tw8 = 0, tw12 = 0;   // windows of a W = 4 / 8 / 12 tile: 256 * W - lag - 1
    uint64_t x4 = 0, y8 = 0;               // windows of the W = 4 tail, and of the W = 8 tail in front of it
};

// % of a round of workgroup slots for the W = 4 / W = 8 tails (defaults 25 / 50 from profiles/r02_taper_sweep.txt:
// 384 Mb 71.6 us without tails, 70.0 at 50/50, 68.5 at 25/50, 70.9 at 100/100; the 120-Mb launch 28.4-28.7 for all)
inline WaveTaper wave_taper_tails(uint64_t total_windows, uint32_t slots, uint32_t lag, int pct4, int pct8) {
    WaveTaper t;
    t.tw12 = 256u * 12u - lag - 1u;
    t.tw8 = 256u * 8u - lag - 1u;
    t.tw4 = 256u * 4u - lag - 1u;
    const uint64_t T = total_windows;
    t.x4 = std::min<uint64_t>((uint64_t)slots * (uint64_t)pct4 / 100 * t.tw4, T * 8 / 100);
    t.y8 = std::min<uint64_t>((uint64_t)slots * (uint64_t)pct8 / 100 * t.tw8, T * 17 / 100);
    return t;
}

// the tile width of a ctg: `after` = the windows from its first window to the end of the batch
inline uint32_t wave_taper_width(const WaveTaper &t, uint64_t after) {
    return after <= t.x4 ? 4u : after <= t.x4 + t.y8 ? 8u : 12u;
}
inline uint32_t wave_taper_tile_windows(const WaveTaper &t, uint32_t w_kind) {
    return w_kind == 4u ? t.tw4 : w_kind == 8u ? t.tw8 : t.tw12;
}

inline size_t wave_lds_bytes(uint32_t max_chunks, uint32_t max_win, bool wide, bool k16) {
    size_t b = 0;
    const size_t mwp = (max_win + 3u) & ~1u;
    b += mwp * (wide ? 8 : 4);                        // Q2
    b += mwp * 4;                                     // Q1
    b += (size_t)((max_chunks + 4) & ~1u) * 4;        // PM
    b += 8 * 8;                                       // scratch
    b += 132 * 4;                                     // PC
    b += (size_t)(max_win + 8) * (k16 ? 2 : 1);       // K
    return (b + 15) & ~(size_t)15;
}

inline size_t wave_fast_lds_bytes(uint32_t max_chunks, uint32_t w, uint32_t lag, bool dense, uint32_t nth = 256) {
    size_t b = (size_t)((((max_chunks + 8u) >> 1) + 16u + 3u) & ~3u) * 4;   // BM: 16 mask bits per chunk + pad
    b += 16 * 4;                                         // scratch
    b += (nth * w + lag + 1u + 31u) & ~15u;              // K (threads past the tile's end still read their slots)
    b += (nth + 16) * 8;                                 // PS: block sums of the baked kernels
    b += nth * 2;                                        // RK: ranks of phase 4b
    if (dense) b += ((nth * w + 15u) & ~15u) + 16u;      // SG (+ the dword behind the last group, read with it)
    return (b + 15) & ~(size_t)15;
}

// What the list holds for these parameters at tile width W.  0: only the entry that takes the parameters as arguments;
// 1: an entry with size, step and lag baked; 2: one with size and step baked, where the lag is an argument and at least
// half of the tile's slots are windows (lag + 1 <= 128 * W).
inline int wave_baked_kind(const gams_wave_params_t &q, int w) {
    int kind = 0;
    for (const WaveInstance &e : kWaveFast) {
        if (e.w != w || e.size != q.size || e.step != q.step) continue;
        if (e.lag != 0 && (uint32_t)e.lag == q.lag) return 1;
        if (e.lag == 0 && q.lag + 1u <= 128u * (uint32_t)w) kind = 2;
    }
    return kind;
}
inline bool wave_is_baked(const gams_wave_params_t &q, int w) { return wave_baked_kind(q, w) != 0; }

// the list entry for tile width W in `nth` threads: the baked form the list has for these parameters, else the one that
// takes them as arguments; -1: none
inline int wave_find_instance(const gams_wave_params_t &q, int w, uint32_t nth) {
    const int kind = wave_baked_kind(q, w);
    for (int i = 0; i < kWaveFastCount; ++i) {
        const WaveInstance &e = kWaveFast[i];
        if (e.w != w || (uint32_t)e.nth != nth) continue;
        if (kind == 0 ? e.size == 0 : e.size == q.size && e.step == q.step && e.lag == (kind == 1 ? (int)q.lag : 0)) return i;
    }
    return -1;
}

// The choice.  false: the ladder arrived at a (W, parameters, threads) the list does not hold -- a slip in the list or
// in the ladder, never a property of the input.
inline bool wave_select(const WaveSelectIn &in, WaveSelection &out) {
    const gams_wave_params_t &q = in.prm;
    const uint32_t tw_req = in.tw_req;
    const uint64_t halo_bytes = (uint64_t)(q.lag + 1) * q.step + (uint64_t)q.size + 32;
    out = WaveSelection{};
    out.nt = in.set_bytes > kStreamBytes;
    // fast kernel: 8-bit counts, 32-bit variance math with 24-bit multiplies
    const bool fast_ok = (!in.serial || in.repair) && q.size <= 255 && q.step <= 32 && (uint64_t)q.lag * q.size <= 65535 &&
                         (uint64_t)q.lag * q.size * q.size < (1ull << 24) && q.lag >= 2;
    const bool step1_prm = q.size == 100 && q.step == 1 && wave_baked_kind(q, 28) != 0;
    if (fast_ok && (tw_req == 0 || tw_req == 1024 || tw_req == 2048 || tw_req == 3072 || tw_req == 5120 ||
                    (tw_req == 7168 && step1_prm))) {
        static const int cand[5] = {28, 20, 12, 8, 4};
        int pick = 0;
        for (int w : cand) {
            const uint64_t tw = 256ull * w;
            if (halo_bytes + tw * q.step > kMaxTileBytes) continue;
            if (tw_req) {
                if (tw_req == tw) pick = w;
                continue;
            }
            // Default W by the number of tiles it would give (a small genome is launch-latency
            // bound and wants many short workgroups; a saturated chip wants the lower instruction
            // count per window of the bigger tiles).  Measured us per pass, W = 4 / 8 / 12, one pass
            // at a time | four in flight:
            //   1.2 M windows   7.9 /  8.2 /  9.3  |  3.02 / 2.84 / 3.07
            //   1.8 M           9.1 /  9.2 / 10.3  |  4.34 / 3.45 / 3.55
            //   2.4 M          11.3 / 10.4 / 11.0  |  5.76 / 4.35 / 4.07
            //   3.6 M          15.0 / 14.2 / 14.2  |  8.42 / 6.44 / 5.91
            //   38 M (384 Mb)   107 /   82 /   77
            // W = 28 / 20 for the baked step-1 kernel (3.8e8 windows: 320 us at W = 28, 334 at W = 20, 503 at
            // W = 12 in round 1; 1.2e7 windows, less than a round of W = 28 tiles: 23.5 vs 21.0 us), otherwise
            // only on request.
            const uint64_t tiles = in.total_windows / tw;
            const bool step1 = q.size == 100 && q.step == 1 && q.lag == 100;   // baked W = 20 fits 64 VGPRs
            const bool flight = in.depth >= 2;
            // (round 3: W = 28 tiles of ONE wave -- 64 threads, 1,691 windows at lag 100 -- from 4,096 such tiles on:
            // 384 Mb 325 -> 285 us, 120 Mb 112 -> 100 us, 12 Mb 21.9 (W = 20) -> 21.2 us; gpurun_out/r3_ab_threads*.log)
            const bool s1w28 = step1 || (q.size == 100 && q.step == 1 && wave_baked_kind(q, 28) == 2);
            // (peaks only: with the dense rows the stores of a whole workgroup's windows are worth more -- 384 Mb --signal
            // 429 us with four waves per tile, 443 with two, 464 with one; gpurun_out/r3_dense_rate2.txt)
            const bool narrow_ok = !(in.flags & GAMS_WAVE_DENSE) && !in.serial;
            if (pick == 0 && w == 28 && s1w28 && in.nth_req == 0 && narrow_ok && q.lag + 1u <= 32u * 28u &&
                in.total_windows / (64u * 28u) >= 4096)
                pick = w;
            if (pick == 0 && w == 28 && s1w28 && tiles >= 4096)
                pick = w;
            if (pick == 0 && w == 20 && (step1 || (q.size == 100 && q.step == 1 && wave_baked_kind(q, 20) == 2)) && tiles >= 1024)
                pick = w;
            // step 5: twice the windows per byte of step 10, W = 20 amortises the per-thread work (384 Mb: 112 -> 108 us at
            // lag 100, 131 -> 114 us at lag 200, one seqset)
            if (pick == 0 && w == 20 && q.size == 100 && q.step == 5 && wave_baked_kind(q, 20) == 2 && tiles >= 2048) pick = w;
            // (step 20 with size 100: 60 KB of bases per W = 12 tile; W = 8 is 2.5 % faster on 384 Mb, HBM bound either way)
            const bool step20 = q.size == 100 && q.step == 20 && wave_baked_kind(q, 8) == 2;
            if (pick == 0 && w == 12 && !step20 && tiles >= (flight ? 768u : 1536u)) pick = w;
            if (pick == 0 && w == 8 && tiles >= (flight ? 512u : 1024u)) pick = w;
            if (pick == 0 && w == 4) pick = w;
        }
        if (pick) {
            // step-1 W = 28 kernels: a tile per one or two waves instead of four (see wave_fast_tile's NTH), while at
            // least half of the tile's slots stay windows
            out.nth = 256;
            if (pick == 28 && q.step == 1 && wave_is_baked(q, pick)) {
                const bool narrow_ok = !(in.flags & GAMS_WAVE_DENSE) && !in.serial;
                const uint32_t want = in.nth_req == 0 ? (narrow_ok ? 64u : 256u) : in.nth_req;   // the library's choice
                if ((want == 64 || want == 128) && q.lag + 1u <= (want / 2u) * 28u) out.nth = want;
            }
            // (diagnostics: the headline kernel in workgroups of one or two waves, on request only -- see DESIGN 3.1)
            if (pick == 12 && q.size == 100 && q.step == 10 && q.lag == 100 && (in.nth_req == 64 || in.nth_req == 128))
                out.nth = in.nth_req;
            // The W = 20 step-5 kernel (lag as an argument) sits between the two regimes: tiles of TWO waves for peaks-only
            // plans over 4,096 such tiles or more (384 Mb 98.0 -> 89.8 us, one wave 94.8; 120 Mb 38.9 -> 38.3 us;
            // gpurun_out/r3_ab_threads5.log)
            if (pick == 20 && q.size == 100 && q.step == 5 && wave_baked_kind(q, 20) == 2) {
                const bool narrow_ok = !(in.flags & GAMS_WAVE_DENSE) && !in.serial;
                const uint32_t want = in.nth_req ? in.nth_req
                                      : narrow_ok && in.total_windows / (128u * 20u) >= 4096 ? 128u : 256u;
                if ((want == 64 || want == 128) && q.lag + 1u <= (want / 2u) * 20u) out.nth = want;
            }
            out.family = kWaveFamFast;
            out.entry = wave_find_instance(q, pick, out.nth);
            if (out.entry < 0) return false;
            // baked kernels: the tile's windows plus the lag+1 in front fill nth*W slots exactly
            out.tw = wave_is_baked(q, pick) ? out.nth * pick - q.lag - 1u : 256u * pick;
            out.max_win = out.tw + q.lag + 1;
            // rounded up to whole rows of one chunk per thread: the baked kernels store every row they load
            out.max_chunks = ((uint32_t)((halo_bytes + (uint64_t)out.tw * q.step + 15) / 16) + 1 + out.nth - 1u) / out.nth * out.nth;
            out.lds_bytes = wave_fast_lds_bytes(out.max_chunks, (uint32_t)pick, q.lag,
                                                (in.flags & GAMS_WAVE_DENSE) != 0 || in.serial, out.nth);
            // a launch of at least a round and a half of workgroups ends in smaller tiles, unless the host
            // keeps passes in flight (their tails overlap anyway, and the small tiles cost 3-4 % more work)
            const uint32_t slots = wave_slots(in.cus);
            const bool headline = q.size == 100 && q.step == 10 && q.lag == 100;
            const bool want = in.taper_req < 0 ? in.depth == 1 : in.taper_req != 0;
            // (not for influence != 1: the dense rows are compacted by wave_compact_kernel, which knows one tile size)
            out.taper = want && !in.serial && tw_req == 0 && pick == 12 && headline && out.nth == 256 &&
                        in.total_windows / out.tw >= slots + slots / 2;
            if (out.taper) out.family = kWaveFamTaper;
            return true;
        }
    }
    uint32_t tw = tw_req;
    if (tw == 0) {
        // default: ~40 KB of bases per tile, 3 workgroups per CU
        uint64_t budget = 40960 > halo_bytes ? 40960 - halo_bytes : 0;
        tw = (uint32_t)std::min<uint64_t>(budget / (uint64_t)q.step, 4096);
    }
    tw = std::min(tw, kMaxTw) & ~255u;
    if (tw < 256) tw = 256;
    while (tw > 256 && halo_bytes + (uint64_t)tw * q.step > kMaxTileBytes) tw -= 256;
    auto go_direct = [&] {
        // (lag+1)*step + size + 256*step beyond the 64-KB tile, or prefix arrays beyond the LDS:
        // untiled kernels; the tile table only serves the peak compaction
        out = WaveSelection{};
        out.nt = in.set_bytes > kStreamBytes;
        out.family = kWaveFamDirect;
        out.direct = true;
        out.tw = 1024;
        return true;
    };
    if (halo_bytes + (uint64_t)tw * q.step > kMaxTileBytes) return go_direct();
    out.family = kWaveFamTile;
    out.tw = tw;
    out.max_win = tw + q.lag + 1;
    out.max_chunks = (uint32_t)((halo_bytes + (uint64_t)tw * q.step + 15) / 16) + 1;
    out.k16 = q.size > 255;
    // narrow integer path: V = n*S2 - S1^2 and the tile prefix of k^2 fit 32 bits
    const uint64_t ns = (uint64_t)q.lag * (uint64_t)q.size;
    const uint64_t q2max = (uint64_t)(out.max_win + 1) * (uint64_t)q.size * (uint64_t)q.size;
    out.wide = !(ns <= 65535 && q2max < (1ull << 32));
    out.lds_bytes = wave_lds_bytes(out.max_chunks, out.max_win, out.wide, out.k16);
    if (out.lds_bytes > 160 * 1024) return go_direct();
    return true;
}

// The narrow body of the headline tile: the tile of the (12, 100, 10, 100, 256) entry -- 3,072 K slots, 2,971 windows --
// is also 128 threads x 24 windows, so a plan of that entry may run its plane-fed passes in wave_fast_narrow_kernel
// (two waves a tile, half the per-thread fixed work per window) over the very same tile table, slots and readers.
struct WaveBody {
    bool narrow = false;          // plane-fed passes of this plan take wave_fast_narrow_kernel
    uint32_t nth = 0, w = 0;      // its threads per workgroup and windows per thread
    size_t lds_bytes = 0;         // its carve: PS and RK for 128 threads (sixteen workgroups fit a CU's 160 KB)
};
constexpr int kWaveNarrowW = 24, kWaveNarrowNth = 128;

// Whether the plan that wave_select() answered `sel` for runs the narrow body, and that body's launch shape.  Only
// the headline entry as the library chose it: peaks only and influence 1 (the dense rows want a whole workgroup's
// stores, see narrow_ok above), no thread-count request, no taper (its W = 8 / W = 4 tiles have no narrow form).
inline WaveBody wave_select_body(const WaveSelectIn &in, const WaveSelection &sel) {
    WaveBody b;
    if (sel.family != kWaveFamFast || sel.entry < 0 || sel.taper) return b;
    const WaveInstance &e = kWaveFast[sel.entry];
    if (!(e.w == 12 && e.size == 100 && e.step == 10 && e.lag == 100 && e.nth == 256)) return b;
    if ((in.flags & GAMS_WAVE_DENSE) || in.serial || in.nth_req != 0) return b;
    b.narrow = true;
    b.nth = (uint32_t)kWaveNarrowNth;
    b.w = (uint32_t)kWaveNarrowW;
    b.lds_bytes = wave_fast_lds_bytes(sel.max_chunks, b.w, (uint32_t)e.lag, false, b.nth);
    return b;
}

// The cuts of the narrow body.  The headline tile's 3,072 K slots are 128 threads x 24 windows (two waves a tile,
// wave_fast_narrow_kernel) and also 64 threads x 48 windows (ONE wave a tile, wave_fast_onewave_kernel): the fixed work
// of a thread is spread over twice the windows again and no workgroup barrier is left.  The one-wave launch lays K over
// the tile's bit stream (every lane holds its bits in registers before any count is stored), has no scratch and no RK,
// and serves the tiles at a ctg start from the baked path too, through a zeroed pad in front of the bit stream: its
// carve is pad | BM | PS, which lets all 32 waves a CU may hold find room in the CU's 160 KB.
enum : int { kWaveCutAuto = 0, kWaveCutTwoWaves = 1, kWaveCutOneWave = 2 };   // GAMS_WAVE_CUT_* of gams_gpu_diag.h
struct WaveCut {
    int cut = 0;                   // kWaveCutTwoWaves / kWaveCutOneWave; 0: the plan has no narrow body
    uint32_t nth = 0, w = 0;       // threads per workgroup and windows per thread of the narrow pass
    size_t lds_bytes = 0;
};
constexpr int kWaveOneWaveW = 48, kWaveOneWaveNth = 64;
// the library's choice (kWaveCutAuto): whichever cut met the project's bar on the headline, profiles/one_wave_cut.txt
constexpr int kWaveCutDefault = kWaveCutOneWave;
constexpr uint32_t kWaveOneWavePad = 128;   // bytes of zeros in front of the bit stream: (lag + 1) * step = 1,010 bits at most

// pad | BM: the tile's plane bytes in the 16-byte pieces of eight chunks wave_fast_tile's plane copy moves
constexpr size_t wave_onewave_bm_bytes() {
    const uint32_t chunks = ((uint32_t)(kWaveOneWaveNth * kWaveOneWaveW) * 10u + 100u + 30u) / 16u + 1u;
    return kWaveOneWavePad + (size_t)((chunks + 7u + 7u) / 8u) * 16u;
}
// K as the one-wave cut reads it: a masked thread still reads the qwords of its second run, 48 t + 120 .. 48 t + 152
constexpr size_t wave_onewave_k_bytes() { return (size_t)(kWaveOneWaveNth - 1) * kWaveOneWaveW + 152u; }
constexpr size_t wave_onewave_lds_bytes() { return wave_onewave_bm_bytes() + (size_t)(kWaveOneWaveNth + 16) * 8u; }

// The cut a narrow pass of the plan runs: `cut_req` (gams_wave_plan_set_cut) when it names one, else the library's choice.
// Nothing (cut 0) for a plan without the narrow body.
inline WaveCut wave_select_cut(const WaveBody &body, int cut_req) {
    WaveCut c;
    if (!body.narrow) return c;
    c.cut = cut_req == kWaveCutAuto ? kWaveCutDefault : cut_req;
    if (c.cut == kWaveCutOneWave) {
        c.nth = (uint32_t)kWaveOneWaveNth;
        c.w = (uint32_t)kWaveOneWaveW;
        c.lds_bytes = wave_onewave_lds_bytes();
    } else {
        c.nth = body.nth;
        c.w = body.w;
        c.lds_bytes = body.lds_bytes;
    }
    return c;
}

// the tile kernel of a selection, spelled the way rocprofv3 prints the instantiation
inline void wave_selection_name(const WaveSelection &s, char *buf, size_t n) {
    const char *nt = s.nt ? "true" : "false";
    if (s.direct)
        std::snprintf(buf, n, "wave_direct_count_kernel + wave_direct_signal_kernel");
    else if (s.taper)
        std::snprintf(buf, n, "wave_fast_taper_kernel<100, 10, 100, %s>", nt);
    else if (s.entry >= 0) {
        const WaveInstance &e = kWaveFast[s.entry];
        std::snprintf(buf, n, "wave_fast_kernel<%d, %d, %d, %d, %s, %d>", e.w, e.size, e.step, e.lag, nt, e.nth);
    } else
        std::snprintf(buf, n, "wave_tile_kernel<%s, %s>", s.k16 ? "unsigned short" : "unsigned char", s.wide ? "true" : "false");
}

}  // namespace
