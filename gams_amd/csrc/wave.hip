// wave.hip -- GC sliding windows + smoothed z-score on gfx950.
//
// Replaces the body of proc_ctg in the reference (src/cmd_gams/wave.rs:138-155):
//   gams::sliding            src/libs/window.rs:78-94
//   bio gc_content per window src/cmd_gams/wave.rs:144-153
//   gams::thresholding_algo  src/libs/stat.rs:16-56
// and the collection of signalled windows (wave.rs:170-187).
//
// One workgroup = one tile of consecutive windows of one ctg, plus the halo of
// lag+1 windows in front of it whose gc values the z-score of the tile's first
// windows needs (z-score state never crosses a ctg: wave.rs:294-297).  Workgroups
// never communicate; every tile writes its peaks into its own fixed slot.
//
// Two tile kernels share that scheme:
//   wave_fast_kernel<W,SIZE,STEP,LAG>  8-bit counts, 32-bit variance math (every BASELINE
//       configuration): 1-bit-per-base stream in LDS, rolling window counts, rolling
//       S1/S2, branch-free integer decision with a rigorous guard band, wave-cooperative
//       exact-order f32 re-evaluation of the windows inside the band.  See its header.
//   wave_tile_kernel<KT,WIDE>          any size/lag up to 65535: chunk prefix PM (prefix<<16 |
//       mask), k[w] = P(w*step+size) - P(w*step), prefix arrays Q1 = sum k, Q2 = sum k^2,
//       same decision + guard band, scalar exact path.
// Signals are bit-identical to thresholding_algo in both (the guard band only decides
// which windows take the exact path).  Parameters whose halo does not fit a tile at all (large
// steps, very large lags) run untiled: wave_direct_count_kernel + wave_direct_signal_kernel.
//
// influence != 1 makes filtered[] (stat.rs:42) a serial recurrence per ctg: those plans guess the signals with the
// influence == 1 kernels and iterate signals -> filtered -> signals to the fixed point, every window in parallel
// (wave_repair.hpp; influence 0 has its own fill-forward filter and a "freeze" guess), then wave_compact_kernel.  The
// round-2 form -- wave_serial_wave_kernel, one wavefront per ctg in exact f32 order (one lane per ctg beyond lag
// 16383) on the counts of a counts-only tile pass -- is what takes over if the sweeps do not settle.
//
// Compile with -ffp-contract=off: the exact paths must not fuse (x-m)*(x-m)+acc.

#include "common.hpp"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <condition_variable>
#include <memory>
#include <mutex>
#include <thread>
#include <type_traits>

#include "wave_kernels.hpp"
#include "wave_repair.hpp"
#include "wave_rows.hpp"
#include "wave_select.hpp"

// The instance list of wave_select.hpp as kernel pointers, a false / true pair (NT) per tuple: every wave_fast_kernel
// and wave_fast_taper_kernel instantiation has the one signature, wave_tile_kernel the other.
using WaveFastFn = void (*)(const WaveTile *, const uint8_t *, WaveArgs);
using WaveTileFn = void (*)(WaveArgs);
#define WAVE_X_PAIR(W, SIZE, STEP, LAG, NTH) \
    {wave_fast_kernel<W, SIZE, STEP, LAG, false, NTH>, wave_fast_kernel<W, SIZE, STEP, LAG, true, NTH>},
static const WaveFastFn kWaveFastFn[kWaveFastCount][2] = {WAVE_FAST_INSTANCES(WAVE_X_PAIR)};
#undef WAVE_X_PAIR
static const WaveFastFn kWaveTaperFn[2] = {wave_fast_taper_kernel<100, 10, 100, false>, wave_fast_taper_kernel<100, 10, 100, true>};
static const WaveFastFn kWaveNarrowFn = wave_fast_narrow_kernel;   // the narrow body of the headline tile (wave_select_body)
static const WaveFastFn kWaveOneWaveFn = wave_fast_onewave_kernel; // ... cut as one wave x 48 windows (wave_select_cut)
static_assert(kOneWaveLds == wave_onewave_lds_bytes() && kOneWavePad == kWaveOneWavePad, "the one-wave carve of wave_select.hpp is the kernel's");
static_assert(kWaveCutAuto == GAMS_WAVE_CUT_AUTO && kWaveCutTwoWaves == GAMS_WAVE_CUT_TWO_WAVES && kWaveCutOneWave == GAMS_WAVE_CUT_ONE_WAVE,
              "wave_select.hpp names the cuts as gams_gpu_diag.h does");
static const WaveTileFn kWaveTileFn[2][2] = {{wave_tile_kernel<uint8_t, false>, wave_tile_kernel<uint8_t, true>},     // [k16][wide]
                                             {wave_tile_kernel<uint16_t, false>, wave_tile_kernel<uint16_t, true>}};


// =============================================================================
// host side
// =============================================================================
// gams_wave_rows_*: the plan's TSV rows made on the device (wave_rows.hpp)
struct WaveRows {
    uint32_t dmax = 0, max_name = 0;
    Kept<uint8_t> arena;                      // RowCtg[n_ctg] | names | gc text table | words[4 + n_ctg + 1]
    RowTabsDev tabs;
    unsigned long long *d_words = nullptr;     // [0] records, [1] text bytes, [2] peaks, [3] fullest tile, [4 ..] ctg_off[n_ctg + 1]
    Kept<uint8_t> tmp;                        // per-record and per-block tables, room for `cap` records
    uint64_t cap = 0;
    Kept<char> d_text;
    Kept<char> h_text{true};                  // page-locked
    Kept<unsigned long long> h_words{true};   // page-locked: [0] records, [1] text bytes, [2] peaks (offsets kernel), [3] fullest tile, [4..] ctg_off
    uint64_t copy_bytes = 0;                  // size of the speculative text copy (held by the captured graphs)
    bool use_graph = true;
    struct RowGraphKey {
        const void *dense, *tmp, *text, *h_text, *peaks, *tile_cnt, *tile_off;
        uint64_t dense_cap, cap, copy_bytes;
        uint32_t tile_cap, nt;
    };
    struct RowGraph {
        hipGraphExec_t exec = nullptr;
        RowGraphKey key{};
    } graph[gams_gpu::kMaxWays];
    uint64_t copied = 0;                      // text bytes the last begin() already sent to the host
    uint64_t last_bytes = 0;                  // text bytes of the previous pass (sizes the speculative copy)
    hipEvent_t done = nullptr;
    bool begun = false;
    void release(gams_gpu_t *h) { gams_free_all(h, arena, tmp, d_text, h_text, h_words); }
};

// gams_wave_signal_text: the `--signal` rows of a pass as text (wave_rows.hpp, sig_*_kernel)
struct WaveSig {
    Kept<uint8_t> arena;                      // SigTile[nt] | blk_len[nt] | blk_off[nt + 2] | RowCtg[n_ctg] | names | gc table | words[n_ctg]
    uint32_t n_tiles = 0;
    SigTile *d_tiles = nullptr;
    uint32_t *d_blk_len = nullptr;
    unsigned long long *d_blk_off = nullptr, *d_words = nullptr;
    RowTabsDev tabs;
    size_t names_cap = 0;
    Kept<char> d_text, h_text{true};                // h_text: page-locked
    Kept<unsigned long long> h_words{true};         // page-locked: words[n_ctg], then ctg_off[n_ctg + 1] made on the host
    void release(gams_gpu_t *h) { gams_free_all(h, arena, d_text, h_text, h_words); }
};

struct Launcher;
struct gams_wave_plan {
    gams_seqset_t *set = nullptr;
    gams_wave_params_t prm{};
    uint32_t flags = 0;
    bool serial = false;          // influence != 1
    bool repair = false;          // ... by guess-and-iterate (wave_repair.hpp): the kernels run as for influence == 1 into
                                  // the dense rows, then filtered[] and the signals are iterated to their fixed point
    Kept<JacTile> d_jtiles;       // repair: tiles of 256 windows
    uint32_t n_jtiles = 0;
    float *d_xtab = nullptr;      // repair: xtab[k] = k as f32 / size as f32, [size + 1] (inside arena_fixed)
    bool jac0 = false;            // repair with influence == 0: fill-forward filter + freeze guess (jac0_* kernels)
    WaveSelection sel;            // the tile kernel and its geometry (wave_select.hpp), made by wave_build_geometry
    WaveFastFn fast_fn = nullptr; // ... as the pointer a pass launches: one of the two is set, neither for sel.direct
    WaveTileFn tile_fn = nullptr;
    WaveBody body;                // plane-fed passes of the headline entry: wave_fast_narrow_kernel over the same tiles (wave_select_body)
    uint64_t total_windows = 0;
    std::vector<WaveCtgDev> ctgs;
    std::vector<WaveTile> tiles;
    // device
    WaveCtgDev *d_ctgs = nullptr;
    WaveTile *d_tiles = nullptr;
    // Outputs of one pass.  A plan of depth D owns D of these "ways"; consecutive gams_wave_run
    // calls rotate over them, each way on its own HIP stream, so that independent passes overlap
    // on the device (a 12-Mb pass alone is launch-latency bound).
    struct Way {
        Kept<gams_peak_t> d_peaks;              // one slot of tile_cap records per tile
        uint32_t *d_tile_cnt = nullptr;         // inside arena_geom
        Kept<unsigned long long> d_counters;    // ring of kCounterRing slots, zeroed once per lap
        uint64_t runs = 0;                      // passes this way has run
        uint32_t last_ring = 0;                 // ring slot of its last pass
        Kept<uint32_t> d_dense_cnt;             // --signal rows / input of the serial kernel
        Kept<int8_t> d_dense_sig;
        Kept<float> d_filtered;
        Kept<uint8_t> d_jac;                    // repair: filtered[] | dirty blocks | control words (one block)
        bool jac0_table = false;                // influence == 0: the freeze table of this way has been filled
        bool jac_serial = false;                // the last pass was handed to the one-wavefront-per-ctg recurrence
        Kept<unsigned long long> h_ctl{true};   // page-locked copy of the control words, made behind every batch of sweeps
        uint32_t jac_sweeps = 0;                // sweeps queued for the way's current pass
        bool jac_settled = true;                // the host has seen a sweep without a flip (or ran the fallback)
        hipEvent_t done = nullptr;              // pipelined mode: recorded behind each run's kernels
        hipEvent_t ran_ev = nullptr;            // lets the readback stream queue behind the last run
        uint64_t seen_upload = 0;               // seqset upload generation this way's stream has waited for
        bool seen_ready = false;                // ... and the plan's const table
        void release(gams_gpu_t *h) { gams_free_all(h, d_peaks, d_counters, d_dense_cnt, d_dense_sig, d_filtered, d_jac, h_ctl); }
    };
    Way way[gams_gpu::kMaxWays];
    uint32_t depth = 1;                         // ways in use
    uint32_t lane = 0;                          // way k runs on stream (lane + k) % kMaxWays (gams_wave_plan_set_lane)
    int taper_req = -1;                         // gams_wave_plan_set_taper: -1 auto, 0 off, 1 on
    int taper4_pct = 25, taper8_pct = 50;       // size of the two tails, % of a round of workgroup slots (gams_wave_plan_set_taper_shape)
    uint32_t queue_threads = gams_gpu::kMaxWays;   // host threads gams_wave_run_n queues from (gams_wave_plan_set_queue_threads)
    uint32_t last_way = 0;                      // way of the most recent run
    uint32_t sel_age = 0;                       // readers look at the run `sel_age` before the most recent one
    hipEvent_t ready = nullptr;                 // recorded on the compute stream behind the const table
    Kept<gams_peak_t> h_peaks{true};            // pinned: packed peaks of the last gams_wave_peaks
    uint32_t tile_cap = 0, tile_cap_req = 0;
    uint32_t tw_req = 0;                        // gams_wave_plan_set_tile request (0: the library's choice)
    uint32_t nth_req = 0;                       // gams_wave_plan_set_threads request (0: the library's choice)
    Kept<gams_peak_t> d_dense;                  // packed copy made by gams_wave_peaks and the rows
    uint64_t dense_cap() const { return d_dense.cap / sizeof(gams_peak_t); }   // ... in records
    uint64_t run_idx = 0;
    int8_t *d_const_sig = nullptr;              // [size+1], see wave_const_table_kernel
    unsigned long long *d_stamps = nullptr;     // diagnostics, [tiles][8]
    unsigned long long *d_tile_off = nullptr;
    // two pooled arenas hold the small tables: `fixed` = ctgs | const_sig (life of the plan),
    // `geom` = tiles | tile_off (+2 totals) | tile_cnt per way (replaced when the tiling changes)
    Kept<uint8_t> arena_fixed, arena_geom;
    bool ran = false;
    struct Launcher *launcher[gams_gpu::kMaxWays - 1] = {};   // extra queueing threads of gams_wave_run_n (made on first use)
    bool pipelined = false;       // gams_wave_plan_set_pipelined: an event per run; readers wait on it
    float g0 = 0, g1 = 0, g2 = 0, g3 = 0;
    float sq[6] = {0, 0, 0, 0, 0, 0};   // aA, aB, gA0, gA1, gB0, gB1 (wave_squared_band)
    WaveRows *rows = nullptr;           // gams_wave_rows_setup
    WaveSig *sigtext = nullptr;         // gams_wave_signal_text
    float guard_safety = 1.5f;          // gams_wave_plan_set_guard
    bool guard_exact = false;           // every window through the exact path
    int input_req = GAMS_WAVE_INPUT_AUTO;   // gams_wave_plan_set_input
    std::atomic<int> last_input{GAMS_WAVE_INPUT_BYTES};   // what the most recently queued pass read (ways queue from several threads)
    int body_req = GAMS_WAVE_BODY_AUTO;     // gams_wave_plan_set_body
    std::atomic<int> last_body{GAMS_WAVE_BODY_WIDE};      // the body of the most recently queued pass
    int cut_req = GAMS_WAVE_CUT_AUTO;       // gams_wave_plan_set_cut
    std::atomic<int> last_cut{GAMS_WAVE_CUT_AUTO};        // the cut of the most recently queued pass (0: not the narrow body)
    // every pooled block of the plan back to the pools (the caller has drained the streams)
    void release(gams_gpu_t *h) {
        if (rows) rows->release(h);
        if (sigtext) sigtext->release(h);
        gams_free_all(h, arena_fixed, arena_geom, d_jtiles, d_dense, h_peaks);
        for (Way &w : way) w.release(h);
    }
};
static void wave_launcher_stop(gams_wave_plan_t *p);


namespace {

constexpr uint32_t kCounterRing = 128;       // one counter slot (kShards lines) per run: no per-run memset
constexpr size_t kSlotWords = (size_t)kShards * kShardWords;
constexpr uint32_t kOffOneGroup = 32768;   // tables up to here: wave_offsets_kernel (one workgroup, one launch)

// What the readers queue behind a pass, in order: kernels and copies to the host, launched on `st` as they come
// (graph == nullptr) or added to `graph` as a chain of nodes.  Argument blocks are read when the launch / the node is made.
// The first failure stays in `err` and nothing is queued behind it.
struct Chain {
    hipStream_t st;
    hipGraph_t graph = nullptr;
    hipGraphNode_t last = nullptr;
    hipError_t err = hipSuccess;
    void kernel(const void *fn, unsigned grid, unsigned block, void **args) {
        if (err != hipSuccess) return;
        if (!graph) {
            err = hipLaunchKernel(fn, dim3(grid), dim3(block), args, 0, st);
            return;
        }
        hipKernelNodeParams kp{};
        kp.func = const_cast<void *>(fn);
        kp.gridDim = dim3(grid);
        kp.blockDim = dim3(block);
        kp.sharedMemBytes = 0;
        kp.kernelParams = args;
        kp.extra = nullptr;
        hipGraphNode_t node = nullptr;
        err = hipGraphAddKernelNode(&node, graph, last ? &last : nullptr, last ? 1 : 0, &kp);
        last = node;
    }
    void copy(void *dst, const void *src, size_t bytes) {
        if (err != hipSuccess || bytes == 0) return;
        if (!graph) {
            err = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st);
            return;
        }
        hipGraphNode_t node = nullptr;
        err = hipGraphAddMemcpyNode1D(&node, graph, last ? &last : nullptr, last ? 1 : 0, dst, src, bytes, hipMemcpyDeviceToHost);
        last = node;
    }
    // exclusive prefix of n counts, the total and the maximum into tot[0..1]: one workgroup, or spans of kOffSpan
    // counts in three launches (wave_kernels.hpp)
    void offsets(const uint32_t *cnt, uint32_t n, unsigned long long *off, unsigned long long *tot) {
        void *all4[] = {&cnt, &n, &off, &tot}, *cnt_n_off[] = {&cnt, &n, &off}, *n_off_tot[] = {&n, &off, &tot};
        if (n <= kOffOneGroup) {
            kernel(reinterpret_cast<const void *>(wave_offsets_kernel), 1, 1024, all4);
            return;
        }
        const unsigned spans = (n + kOffSpan - 1u) / kOffSpan;
        kernel(reinterpret_cast<const void *>(wave_offsets_sum_kernel), spans, 1024, cnt_n_off);
        kernel(reinterpret_cast<const void *>(wave_offsets_base_kernel), 1, 1024, n_off_tot);
        kernel(reinterpret_cast<const void *>(wave_offsets_scan_kernel), spans, 1024, cnt_n_off);
    }
    // the tile slots of way `w` packed into d_dense (at most dense_cap records): the tiles' offsets, with the total and
    // the fullest tile in the two words behind them, then the gather
    void gather(const gams_wave_plan_t *p, const gams_wave_plan::Way &w) {
        const gams_peak_t *slots = w.d_peaks;
        uint32_t tile_cap = p->tile_cap;
        const uint32_t *tile_cnt = w.d_tile_cnt;
        const unsigned long long *tile_off = p->d_tile_off;
        gams_peak_t *dense = p->d_dense;
        unsigned long long dense_cap = p->dense_cap();
        void *args[] = {&slots, &tile_cap, &tile_cnt, &tile_off, &dense, &dense_cap};
        kernel(reinterpret_cast<const void *>(wave_gather_kernel), (unsigned)p->tiles.size(), 64, args);
    }
    void pack(const gams_wave_plan_t *p, const gams_wave_plan::Way &w) {
        const uint32_t nt = (uint32_t)p->tiles.size();
        offsets(w.d_tile_cnt, nt, p->d_tile_off, p->d_tile_off + nt);
        gather(p, w);
    }
};

// Guard band of the integer decision, in units of D = |n*k - S1| (see DESIGN.md
// "z-score guard band" for the derivation).  u = 2^-24.
void wave_guard_band(const gams_wave_params_t &p, double safety, bool all_exact, float g[4]) {
    const double u = std::ldexp(1.0, -24);
    const double n = (double)p.lag, sz = (double)p.size;
    const double thr = std::fabs((double)p.threshold);
    // The squared-domain decision divides by thr*sqrt(n/(n-1)): thresholds outside [1e-6, 1e6]
    // (and non-finite or negative ones) are not worth a fast path, every window is exact.
    if (all_exact || !(std::isfinite(p.threshold)) || p.threshold < 1e-6f || p.threshold > 1e6f || p.lag < 2) {
        g[0] = INFINITY;  // every window takes the exact path
        g[1] = g[2] = g[3] = 0.0f;
        return;
    }
    const double gam = 1.01 * (n + 1.0) * u / (1.0 - (n + 1.0) * u);  // f32 sequential mean
    const double kap = std::sqrt(n / (n - 1.0));
    const double eta = 1.01 * ((n + 3.0) / 2.0 + 2.0) * u;              // sq sum, /, sqrt, *thr
    g[1] = (float)(safety * (gam + 2.0 * u + thr * kap * gam * (1.0 + eta)));
    g[2] = (float)(safety * (eta + 8.0 * u));
    g[3] = (float)(safety * 3.0 * u);
    g[0] = (float)(safety * (2.0 * thr * kap * u * n * sz) + 1e-3);
}

// The same band for z_decide (wave_kernels.hpp): with g = g2 + g3, c = g0 + g1*S1 and
// sb = thr*sqrt(n/(n-1)),   A = D*(1-g)/((1+g) sb) - c/((1+g) sb),   B = D*(1+g)/((1-g) sb) + c/((1-g) sb).
// The kernel's own roundings (one fma for c, one for A or B, 2u on V) are covered by rounding the
// multiplier of A down and everything else up by a few u here, so that a decided window is
// decided under the exact-arithmetic band above: A_f^2 > V_f implies A^2 > V, B_f^2 < V_f implies B^2 < V.
void wave_squared_band(const gams_wave_params_t &p, const float g[4], float sq[6]) {
    for (int i = 0; i < 6; ++i) sq[i] = 0.0f;
    if (!(g[0] < INFINITY)) return;
    const double u = std::ldexp(1.0, -24);
    const double n = (double)p.lag;
    const double sb = std::fabs((double)p.threshold) * std::sqrt(n / (n - 1.0));
    const double gg = (double)g[2] + (double)g[3];
    const double lo = 1.0 - 5.0 * u, hi = 1.0 + 7.0 * u;
    sq[0] = (float)((1.0 - gg) / ((1.0 + gg) * sb) * lo);   // aA
    sq[1] = (float)((1.0 + gg) / ((1.0 - gg) * sb) * hi);   // aB
    sq[2] = (float)((double)g[0] / ((1.0 + gg) * sb) * hi); // gA0
    sq[3] = (float)((double)g[1] / ((1.0 + gg) * sb) * hi); // gA1
    sq[4] = (float)((double)g[0] / ((1.0 - gg) * sb) * hi); // gB0
    sq[5] = (float)((double)g[1] / ((1.0 - gg) * sb) * hi); // gB1
}

void wave_fill_tiles(gams_wave_plan_t *p) {
    p->tiles.clear();
    for (uint32_t c = 0; c < p->set->n_ctg; ++c) {
        const uint32_t n = p->ctgs[c].n_win;
        for (uint32_t w = 0; w < n; w += p->sel.tw)
            p->tiles.push_back(WaveTile{c, w, n, 0u, p->ctgs[c].seq_off, p->ctgs[c].win_base});
    }
}

// Tapered tile table for the baked W = 12 kernel: the ctgs holding the last windows of the batch are
// cut into W = 4 tiles, the ones before them into W = 8 tiles (see wave_fast_taper_kernel).  The two
// tails are a quarter / half a round of workgroup slots, and at most 8 % / 17 % of the batch: the arithmetic is
// wave_taper_tails / wave_taper_width of wave_select.hpp (plain C++, pinned on the CPU).
void wave_fill_tiles_tapered(gams_wave_plan_t *p, uint32_t slots) {
    const uint64_t T = p->total_windows;
    // gams_wave_plan_set_taper_shape (0..100)
    const WaveTaper t = wave_taper_tails(T, slots, p->prm.lag, p->taper4_pct, p->taper8_pct);
    p->tiles.clear();
    for (uint32_t c = 0; c < p->set->n_ctg; ++c) {
        const uint32_t n = p->ctgs[c].n_win;
        const uint64_t after = T - p->ctgs[c].win_base;           // windows from this ctg's first to the end of the batch
        const uint32_t w_kind = wave_taper_width(t, after);
        const uint32_t tw = wave_taper_tile_windows(t, w_kind);
        for (uint32_t w = 0; w < n; w += tw)
            p->tiles.push_back(WaveTile{c, w, n, w_kind, p->ctgs[c].seq_off, p->ctgs[c].win_base});
    }
}

// The plan's tile kernel, its geometry and its tile table from wave_select(); the kernel's dynamic-LDS limit is raised
// here (the callers have set the device), so that a pass only launches.
int wave_build_geometry(gams_gpu_t *h, gams_wave_plan_t *p, uint32_t tw_req) {
    const WaveSelectIn in{p->prm,  p->flags,   p->serial,    p->repair, p->depth,     p->total_windows,
                          tw_req,  p->nth_req, p->taper_req, h->cus,    p->set->bytes};
    WaveSelection s;
    if (!wave_select(in, s)) return gams_fail(h, GAMS_ESTATE, "wave: the instance list lacks the selected kernel");
    p->sel = s;
    p->fast_fn = s.entry < 0 ? nullptr : s.taper ? kWaveTaperFn[s.nt] : kWaveFastFn[s.entry][s.nt];
    p->tile_fn = s.family == kWaveFamTile ? kWaveTileFn[s.k16][s.wide] : nullptr;
    if (p->fast_fn) GAMS_HIP(h, gams_lds_attr(h, reinterpret_cast<const void *>(p->fast_fn), s.lds_bytes));
    if (p->tile_fn) GAMS_HIP(h, gams_lds_attr(h, reinterpret_cast<const void *>(p->tile_fn), s.lds_bytes));
    p->body = wave_select_body(in, s);
    if (p->body.narrow) {
        GAMS_HIP(h, gams_lds_attr(h, reinterpret_cast<const void *>(kWaveNarrowFn), p->body.lds_bytes));
        GAMS_HIP(h, gams_lds_attr(h, reinterpret_cast<const void *>(kWaveOneWaveFn), wave_onewave_lds_bytes()));
    }
    if (s.taper)
        wave_fill_tiles_tapered(p, wave_slots(h->cus));
    else
        wave_fill_tiles(p);
    return GAMS_OK;
}

void wave_set_band(gams_wave_plan_t *p) {
    float g[4];
    wave_guard_band(p->prm, (double)p->guard_safety, p->guard_exact, g);
    p->g0 = g[0];
    p->g1 = g[1];
    p->g2 = g[2];
    p->g3 = g[3];
    wave_squared_band(p->prm, g, p->sq);
}

// the stream way k runs on: the handle's compute stream, or one of its auxiliary streams
hipStream_t wave_stream(gams_gpu_t *h, const gams_wave_plan_t *p, uint32_t k) {
    const uint32_t si = (p->lane + k) % (uint32_t)gams_gpu::kMaxWays;
    return si == 0 ? h->compute : h->aux[si - 1];
}

// the way the readers look at
gams_wave_plan::Way &wave_read_way(gams_wave_plan_t *p) {
    return p->way[(p->last_way + p->depth - (p->sel_age % p->depth)) % p->depth];
}
uint32_t wave_read_way_index(const gams_wave_plan_t *p) {
    return (p->last_way + p->depth - (p->sel_age % p->depth)) % p->depth;
}

int wave_sync_ways(gams_gpu_t *h, gams_wave_plan_t *p) {
    for (uint32_t k = 0; k < p->depth; ++k) GAMS_HIP(h, hipStreamSynchronize(wave_stream(h, p, k)));
    return GAMS_OK;
}

// A freed arena anew: a block of the bytes `layout` takes, carved by it.  (Sizing runs the layout over no block, which
// leaves its pointers null should the request fail.)
template <typename F>
hipError_t wave_arena(gams_gpu_t *h, Kept<uint8_t> &arena, F layout) {
    arena.free(h);
    const size_t bytes = layout_bytes(layout);
    const hipError_t e = arena.reserve(h, bytes);
    if (e == hipSuccess) carve(arena, layout);
    return e;
}

int wave_upload_geometry(gams_gpu_t *h, gams_wave_plan_t *p) {
    const size_t nt = std::max<size_t>(p->tiles.size(), 1);
    for (auto &w : p->way) w.d_tile_cnt = nullptr;
    auto geom = [&](Carver &c) {
        p->d_tiles = c.take<WaveTile>(nt);
        p->d_tile_off = c.take<unsigned long long>(nt + 2);   // + the two totals
        for (uint32_t k = 0; k < p->depth; ++k) p->way[k].d_tile_cnt = c.take<uint32_t>(nt);
    };
    GAMS_HIP(h, wave_arena(h, p->arena_geom, geom));
    if (p->flags & GAMS_WAVE_PEAKS) {
        // a slot of tw/8 records per tile (typical density is 1-2 % of the windows); a tile that
        // overflows makes the first reader regrow the slots to the fullest tile and run again (wave_regrow_slots)
        p->d_dense.free(h);
        p->tile_cap = std::max<uint32_t>(p->tile_cap_req ? p->tile_cap_req : p->sel.tw / 8u, 16u);
        for (auto &w : p->way) w.d_peaks.free(h);
        const size_t slots = nt * (size_t)p->tile_cap * sizeof(gams_peak_t);
        for (uint32_t k = 0; k < p->depth; ++k) GAMS_HIP(h, p->way[k].d_peaks.reserve(h, slots));
    }
    if (!p->tiles.empty())
        GAMS_HIP(h, hipMemcpy(p->d_tiles, p->tiles.data(), p->tiles.size() * sizeof(WaveTile),
                              hipMemcpyHostToDevice));
    return GAMS_OK;
}

// The repair path's device tables of one way, carved from one pooled block
struct JacBufs {
    float *f;                        // filtered[], one per row
    uint32_t *fblk;                  // per block of kJacTile rows: 1 + the sweep in which filtered last changed there
    unsigned long long *ctl;         // kJacWords control words
    // influence == 0 only
    int32_t *lastu, *tile_last;
    unsigned long long *freeze;
    int8_t *ftab;
    uint8_t *frow;
    size_t bytes;
};
JacBufs wave_jac_carve(uint8_t *base, uint64_t total_windows, const gams_wave_plan_t *p = nullptr) {
    Carver c(base);
    JacBufs z{};
    z.f = c.take<float>(std::max<uint64_t>(total_windows, 1));
    z.fblk = c.take<uint32_t>((size_t)(total_windows / kJacTile + 2));
    z.ctl = c.take<unsigned long long>(kJacWords);
    if (p && p->jac0) {
        const size_t size1 = (size_t)p->prm.size + 1;
        z.lastu = c.take<int32_t>(std::max<uint64_t>(total_windows, 1));
        z.tile_last = c.take<int32_t>(std::max<size_t>(p->n_jtiles, 1));
        z.freeze = c.take<unsigned long long>(std::max<size_t>(p->set->n_ctg, 1) * 2);
        z.ftab = c.take<int8_t>(size1 * size1);
        z.frow = c.take<uint8_t>(size1);
    }
    z.bytes = c.bytes();
    return z;
}

// per-way buffers that do not depend on the tiling: counter ring, dense rows, filtered[]
int wave_alloc_ways(gams_gpu_t *h, gams_wave_plan_t *p) {
    const uint64_t base = std::max<uint64_t>(p->total_windows, 1);
    const bool need_dense = (p->flags & GAMS_WAVE_DENSE) || p->serial || p->sel.direct;
    for (uint32_t k = 0; k < p->depth; ++k) {
        gams_wave_plan::Way &w = p->way[k];
        if (!w.d_counters) {
            const size_t ring = kCounterRing * kSlotWords * sizeof(unsigned long long);
            GAMS_HIP(h, w.d_counters.reserve(h, ring));
            // queued in front of the way's first run on its own stream
            GAMS_HIP(h, hipMemsetAsync(w.d_counters, 0, ring, wave_stream(h, p, k)));
            w.runs = 0;
        }
        if (need_dense && !w.d_dense_cnt) {
            GAMS_HIP(h, w.d_dense_cnt.reserve(h, base * sizeof(uint32_t)));
            GAMS_HIP(h, w.d_dense_sig.reserve(h, base));
        }
        if (p->serial && !p->repair && !w.d_filtered)
            GAMS_HIP(h, w.d_filtered.reserve(h, base * sizeof(float)));
        if (p->repair && !w.d_jac) {
            const size_t jac = wave_jac_carve(nullptr, p->total_windows, p).bytes;
            GAMS_HIP(h, w.d_jac.reserve(h, jac));
            GAMS_HIP(h, w.h_ctl.reserve(h, kJacWords * 8));
        }
    }
    return GAMS_OK;
}

// ---- what the readers of a pass share ---------------------------------------------------------------------------
// Buffers are sized from two device-written words, the peaks of the pass and of its fullest tile: are they something
// a pass over this plan can produce?  (A tile signals at most its own windows, all tiles together at most the batch's.)
bool wave_totals_plausible(const gams_wave_plan_t *p, uint64_t total, uint64_t worst) {
    return worst <= p->sel.tw && total <= p->total_windows && total <= (uint64_t)p->tiles.size() * worst;
}

// Some tile signalled more windows than its slot holds.  The device has reported the fullest tile (runs are
// deterministic, so that is what the slots need -- at GRCh38 step 1 a slot of tw records per tile would be ~50 GB per
// way) and every pass still held is run again into the new slots: same inputs, same results.  The run counter only
// steps back by the passes repeated, so the way rotation and the history gams_wave_plan_select sees stay.
int wave_regrow_slots(gams_gpu_t *h, gams_wave_plan_t *p, uint64_t worst) {
    p->tile_cap_req = (uint32_t)std::min<uint64_t>(p->sel.tw, (worst + 15u) & ~(uint64_t)15u);
    const uint32_t age = p->sel_age;
    const uint32_t again = (uint32_t)std::min<uint64_t>(p->depth, p->run_idx);
    int rc = wave_sync_ways(h, p);
    if (rc == GAMS_OK) rc = wave_upload_geometry(h, p);
    if (rc == GAMS_OK) {
        p->run_idx -= again;
        for (uint32_t k = 0; k < again && rc == GAMS_OK; ++k) rc = gams_wave_run(h, p);
        p->sel_age = age;
    }
    return rc;
}

// the first d_dense of a tiling: typical density is 1-3 % of the windows; a fuller result makes its reader regrow it
int wave_first_dense(gams_gpu_t *h, gams_wave_plan_t *p) {
    if (p->d_dense) return GAMS_OK;
    const size_t want = (size_t)(p->total_windows / 16 + 4096) * sizeof(gams_peak_t);
    GAMS_HIP(h, p->d_dense.reserve(h, want));
    return GAMS_OK;
}

}  // namespace

extern "C" {

int64_t gams_window_count(int64_t len, int32_t size, int32_t step) {
    if (size <= 0 || step <= 0) return -1;
    if (len < size) return 0;
    return (len - size) / step + 1;  // window.rs:78-94 in closed form
}

int gams_wave_plan_create(gams_gpu_t *h, gams_seqset_t *s, const gams_wave_params_t *params, uint32_t flags,
                          gams_wave_plan_t **out) {
    if (!h || !s || !params || !out) return gams_fail(h, GAMS_EINVAL, "wave_plan_create: null argument");
    if (!(flags & (GAMS_WAVE_PEAKS | GAMS_WAVE_DENSE)))
        return gams_fail(h, GAMS_EINVAL, "wave_plan_create: flags must request PEAKS and/or DENSE");
    if (params->size <= 0 || params->step <= 0)
        return gams_fail(h, GAMS_EINVAL, "wave: size and step must be positive");
    if (params->lag == 0) return gams_fail(h, GAMS_ESHORT, "wave: lag == 0 (the reference panics, stat.rs:30)");
    if (params->size > 65535 || params->lag > 65535)
        return gams_fail(h, GAMS_EUNSUPPORTED, "wave: size and lag are limited to 65535");
    GAMS_HIP(h, hipSetDevice(h->device));
    gams_wave_plan_t *p = new gams_wave_plan_t();
    p->set = s;
    p->prm = *params;
    p->flags = flags;
    p->serial = !(params->influence == 1.0f);
    p->ctgs.resize(s->n_ctg);
    uint64_t base = 0;
    for (uint32_t c = 0; c < s->n_ctg; ++c) {
        const int64_t n = gams_window_count(s->len[c], params->size, params->step);
        if (n < (int64_t)params->lag) {
            delete p;
            return gams_fail(h, GAMS_ESHORT,
                             "wave: ctg " + std::to_string(c) + " has " + std::to_string(n) +
                                 " windows < lag (the reference panics, stat.rs:30)");
        }
        p->ctgs[c] = WaveCtgDev{s->off[c], base, s->len[c], (uint32_t)n};
        base += (uint64_t)n;
    }
    p->total_windows = base;
    // influence != 1: guess-and-iterate while a tile's history (256 + lag + 1 floats) fits a comfortable share of the
    // LDS; the one-wavefront-per-ctg recurrence beyond that
    p->repair = p->serial && params->lag >= 2 && params->lag <= 16000;
    p->jac0 = p->repair && params->influence == 0.0f && params->size <= 400;   // (a (size + 1)^2 table)
    int rc = wave_build_geometry(h, p, 0);
    if (rc != GAMS_OK) {
        delete p;
        return rc;
    }
    wave_set_band(p);
    // from here on the plan takes blocks and events: every early return gives the half-built plan to gams_wave_plan_destroy
    auto destroy = [h](gams_wave_plan_t *q) { gams_wave_plan_destroy(h, q); };
    std::unique_ptr<gams_wave_plan_t, decltype(destroy)> half_built(p, destroy);
    const size_t size1 = (size_t)params->size + 1;
    auto fixed = [&](Carver &c) {
        p->d_ctgs = c.take<WaveCtgDev>(std::max<size_t>(s->n_ctg, 1));
        p->d_const_sig = c.take<int8_t>(size1);
        p->d_xtab = p->repair ? c.take<float>(size1) : nullptr;
    };
    GAMS_HIP(h, wave_arena(h, p->arena_fixed, fixed));
    if (p->repair) {
        // the data value of a window with k G/C bases, as the reference computes it: k as f32 / size as f32
        std::vector<float> xt(size1);
        for (size_t k = 0; k < xt.size(); ++k) xt[k] = (float)k / (float)params->size;
        GAMS_HIP(h, hipMemcpy(p->d_xtab, xt.data(), xt.size() * sizeof(float), hipMemcpyHostToDevice));
        std::vector<JacTile> jt;
        for (uint32_t c = 0; c < s->n_ctg; ++c)
            for (uint32_t w0 = 0; w0 < p->ctgs[c].n_win; w0 += kJacTile)
                jt.push_back(JacTile{c, w0, p->ctgs[c].n_win, 0u, p->ctgs[c].win_base});
        p->n_jtiles = (uint32_t)jt.size();
        const size_t jt_bytes = std::max<size_t>(jt.size(), 1) * sizeof(JacTile);
        GAMS_HIP(h, p->d_jtiles.reserve(h, jt_bytes));
        if (!jt.empty()) GAMS_HIP(h, hipMemcpy(p->d_jtiles, jt.data(), jt.size() * sizeof(JacTile), hipMemcpyHostToDevice));
    }
    if (s->n_ctg) GAMS_HIP(h, hipMemcpy(p->d_ctgs, p->ctgs.data(), s->n_ctg * sizeof(WaveCtgDev), hipMemcpyHostToDevice));
    rc = wave_upload_geometry(h, p);
    if (rc != GAMS_OK) return rc;
    rc = wave_alloc_ways(h, p);
    if (rc != GAMS_OK) return rc;
    hipLaunchKernelGGL(wave_const_table_kernel, dim3((params->size + 256) / 256), dim3(256), 0, h->compute,
                       p->d_const_sig, (uint32_t)params->size, params->lag, params->threshold);
    GAMS_HIP(h, hipGetLastError());
    GAMS_HIP(h, hipEventCreateWithFlags(&p->ready, hipEventDisableTiming));
    GAMS_HIP(h, hipEventRecord(p->ready, h->compute));
    p->way[0].seen_ready = true;   // same stream
    *out = half_built.release();
    return GAMS_OK;
}

void gams_wave_plan_destroy(gams_gpu_t *h, gams_wave_plan_t *p) {
    if (!p) return;
    wave_launcher_stop(p);
    if (h) {
        (void)hipSetDevice(h->device);
        for (uint32_t k = 0; k < p->depth; ++k)
            if (wave_stream(h, p, k)) (void)hipStreamSynchronize(wave_stream(h, p, k));
        if (h->readback) (void)hipStreamSynchronize(h->readback);
    }
    p->release(h);
    if (p->rows) {
        if (p->rows->done) (void)hipEventDestroy(p->rows->done);
        for (auto &g : p->rows->graph)
            if (g.exec) (void)hipGraphExecDestroy(g.exec);
        delete p->rows;
    }
    delete p->sigtext;
    for (auto &w : p->way) {
        if (w.done) (void)hipEventDestroy(w.done);
        if (w.ran_ev) (void)hipEventDestroy(w.ran_ev);
    }
    if (p->ready) (void)hipEventDestroy(p->ready);
    (void)hipFree(p->d_stamps);
    delete p;
}

uint64_t gams_wave_total_windows(const gams_wave_plan_t *p) { return p ? p->total_windows : 0; }

uint32_t gams_wave_ctg_windows(const gams_wave_plan_t *p, uint32_t i) {
    return (p && i < p->ctgs.size()) ? p->ctgs[i].n_win : 0;
}

// The tiling again, after a setter changed what it depends on, and everything that is sized by it.  `same_taper_ok`: nothing
// else to do when the table is tapered, or not, as before.
static int wave_retile(gams_gpu_t *h, gams_wave_plan_t *p, uint32_t tile_windows, bool same_taper_ok = false) {
    int rc = wave_sync_ways(h, p);
    if (rc != GAMS_OK) return rc;
    const bool before = p->sel.taper;
    rc = wave_build_geometry(h, p, tile_windows);
    if (rc != GAMS_OK) return rc;
    p->tw_req = tile_windows;
    if (same_taper_ok && p->sel.taper == before) return GAMS_OK;       // same tile table
    p->ran = false;
    (void)hipFree(p->d_stamps);                     // sized for the old tiling
    p->d_stamps = nullptr;
    rc = wave_upload_geometry(h, p);
    // a requested tile can move the plan from the tiled to the untiled kernels (prefix arrays beyond
    // the LDS), which need the dense rows
    if (rc == GAMS_OK) rc = wave_alloc_ways(h, p);
    return rc;
}

int gams_wave_plan_set_tile(gams_gpu_t *h, gams_wave_plan_t *p, uint32_t tile_windows) {
    if (!h || !p) return gams_fail(h, GAMS_EINVAL, "wave_plan_set_tile: null argument");
    GAMS_HIP(h, hipSetDevice(h->device));
    return wave_retile(h, p, tile_windows);
}

int gams_wave_plan_set_threads(gams_gpu_t *h, gams_wave_plan_t *p, uint32_t threads) {
    if (!h || !p) return gams_fail(h, GAMS_EINVAL, "wave_plan_set_threads: null argument");
    if (threads != 0 && threads != 64 && threads != 128 && threads != 256)
        return gams_fail(h, GAMS_EINVAL, "wave_plan_set_threads: 0 (the library's choice), 64, 128 or 256");
    p->nth_req = threads;
    return gams_wave_plan_set_tile(h, p, p->tw_req);
}

int gams_wave_plan_set_guard(gams_gpu_t *h, gams_wave_plan_t *p, float safety, int all_exact) {
    if (!h || !p) return gams_fail(h, GAMS_EINVAL, "wave_plan_set_guard: null argument");
    if (!(safety >= 1.0f) || !(safety <= 1e6f))
        return gams_fail(h, GAMS_EINVAL, "wave_plan_set_guard: safety must be in [1, 1e6]");
    p->guard_safety = safety;
    p->guard_exact = all_exact != 0;
    wave_set_band(p);
    return GAMS_OK;
}

// ---- influence != 1: guess-and-iterate (wave_repair.hpp) ------------------------------------------------------
constexpr uint32_t kJacFirstBatch = 6;      // sweeps queued with the pass (3-5 settle the usual case), then batches of 8

static JacArgs wave_jac_args(gams_wave_plan_t *p, uint32_t k) {
    gams_wave_plan::Way &w = p->way[k];
    const JacBufs z = wave_jac_carve(w.d_jac, p->total_windows, p);
    JacArgs a{};
    a.tiles = p->d_jtiles;
    a.n_tiles = p->n_jtiles;
    a.cnt = w.d_dense_cnt;
    a.sig = w.d_dense_sig;
    a.xtab = p->d_xtab;
    a.f = z.f;
    a.fblk = z.fblk;
    a.ctl = z.ctl;
    a.lag = p->prm.lag;
    a.sweep = 0;
    a.thr = p->prm.threshold;
    a.influence = p->prm.influence;
    a.lastu = z.lastu;
    a.tile_last = z.tile_last;
    a.freeze = z.freeze;
    a.ftab = z.ftab;
    a.frow = z.frow;
    a.size1 = (uint32_t)p->prm.size + 1u;
    a.n_ctg = p->set->n_ctg;
    return a;
}

// the peaks of the dense rows into the tile slots (what the readers pack)
static int wave_compact_dense(gams_gpu_t *h, gams_wave_plan_t *p, uint32_t k, hipStream_t st) {
    gams_wave_plan::Way &w = p->way[k];
    if (!(p->flags & GAMS_WAVE_PEAKS) || p->tiles.empty()) return GAMS_OK;
    hipLaunchKernelGGL(wave_compact_kernel, dim3((unsigned)p->tiles.size()), dim3(256), 0, st, p->d_ctgs, p->d_tiles, p->sel.tw,
                       w.d_dense_cnt, w.d_dense_sig, w.d_peaks, p->tile_cap, w.d_tile_cnt);
    GAMS_HIP(h, hipGetLastError());
    return GAMS_OK;
}

// The recurrence of influence != 1 in exact f32 order over the dense counts of way k: one wavefront per ctg with the last
// lag + 1 filtered values in an LDS ring, or one lane per ctg with `filtered` (a float per window) beyond the ring.
static int wave_serial_recurrence(gams_gpu_t *h, gams_wave_plan_t *p, uint32_t k, hipStream_t st, float *filtered) {
    gams_wave_plan::Way &w = p->way[k];
    const gams_wave_params_t &q = p->prm;
    const uint32_t n = p->set->n_ctg;
    if (q.lag + 1u <= kSerialRing) {
        const size_t ring = (size_t)((q.lag + 1u + 63u) & ~63u) * sizeof(float);
        GAMS_HIP(h, gams_lds_attr(h, reinterpret_cast<const void *>(wave_serial_wave_kernel), kSerialRing * sizeof(float)));
        hipLaunchKernelGGL(wave_serial_wave_kernel, dim3(n), dim3(64), ring, st, p->d_ctgs, n, w.d_dense_cnt,
                           w.d_dense_sig, q.lag, q.threshold, q.influence, (float)q.size);
    } else {
        hipLaunchKernelGGL(wave_serial_kernel, dim3((n + 63) / 64), dim3(64), 0, st, p->d_ctgs, n, w.d_dense_cnt,
                           w.d_dense_sig, filtered, q.lag, q.threshold, q.influence, (float)q.size);
    }
    GAMS_HIP(h, hipGetLastError());
    return GAMS_OK;
}

// queue `n` more sweeps on way k's stream (first: with the initialisation in front), then the compaction of the dense
// rows and the copy of the control words
static int wave_jac_sweeps(gams_gpu_t *h, gams_wave_plan_t *p, uint32_t k, uint32_t n, bool first) {
    gams_wave_plan::Way &w = p->way[k];
    hipStream_t st = wave_stream(h, p, k);
    JacArgs a = wave_jac_args(p, k);
    const unsigned grid = std::max(p->n_jtiles, 1u);
    const size_t lds = ((size_t)kJacTile + a.lag + 1) * sizeof(float);
    GAMS_HIP(h, gams_lds_attr(h, reinterpret_cast<const void *>(jac_eval_kernel), lds));
    if (first) {
        hipLaunchKernelGGL(jac_init_kernel, dim3(grid), dim3(256), 0, st, a);
        if (p->jac0 && !w.jac0_table) {
            // the decisions behind a freeze point, once per way (the parameters belong to the plan)
            GAMS_HIP(h, hipMemsetAsync(const_cast<uint8_t *>(a.frow), 1, a.size1, st));
            hipLaunchKernelGGL(jac0_table_kernel, dim3((a.size1 * a.size1 + 255u) / 256u), dim3(256), 0, st,
                               const_cast<int8_t *>(a.ftab), const_cast<uint8_t *>(a.frow), a.xtab, a.size1, a.lag, a.thr);
            w.jac0_table = true;
        }
    }
    const uint32_t max_sweeps = p->jac0 ? kJacMaxSweeps0 : kJacMaxSweeps;
    if (p->n_jtiles)
        for (uint32_t i = 0; i < n && w.jac_sweeps < max_sweeps; ++i, ++w.jac_sweeps) {
            a.sweep = w.jac_sweeps;
            if (p->jac0) {
                const unsigned g0 = (grid + kJac0Group - 1u) / kJac0Group;
                hipLaunchKernelGGL(jac0_scan_kernel, dim3(g0), dim3(256), 0, st, a);
                hipLaunchKernelGGL(jac0_fill_kernel, dim3(g0), dim3(256), 0, st, a);
            } else {
                hipLaunchKernelGGL(jac_filter_kernel, dim3(grid), dim3(256), 0, st, a);
            }
            hipLaunchKernelGGL(jac_eval_kernel, dim3(grid), dim3(256), lds, st, a);
        }
    GAMS_HIP(h, hipGetLastError());
    int rc = wave_compact_dense(h, p, k, st);
    if (rc != GAMS_OK) return rc;
    GAMS_HIP(h, hipMemcpyAsync(w.h_ctl, a.ctl, kJacWords * 8, hipMemcpyDeviceToHost, st));
    return GAMS_OK;
}

// Has way k's pass reached its fixed point?  Waits for what is queued, looks at the control words, queues more sweeps
// while a sweep still flipped signals, and after kJacMaxSweeps (or at a run of thousands of signalled windows) lets the
// one-wavefront-per-ctg recurrence compute the batch from the counts.  Every reader of a pass calls this first.
static int wave_jac_settle(gams_gpu_t *h, gams_wave_plan_t *p, uint32_t k) {
    if (!p->repair) return GAMS_OK;
    gams_wave_plan::Way &w = p->way[k];
    if (w.jac_settled || p->n_jtiles == 0) return GAMS_OK;
    hipStream_t st = wave_stream(h, p, k);
    for (;;) {
        GAMS_HIP(h, hipStreamSynchronize(st));
        bool fixed = false;
        for (uint32_t i = 0; i < w.jac_sweeps && !fixed; ++i) fixed = w.h_ctl[i] == 0ull;
        const bool abandon = w.h_ctl[kJacAbandon] != 0ull;
        if (fixed && !abandon) break;
        if (abandon || w.jac_sweeps >= (p->jac0 ? kJacMaxSweeps0 : kJacMaxSweeps)) {
            int rc = wave_serial_recurrence(h, p, k, st, wave_jac_carve(w.d_jac, p->total_windows).f);
            if (rc != GAMS_OK) return rc;
            rc = wave_compact_dense(h, p, k, st);
            if (rc != GAMS_OK) return rc;
            GAMS_HIP(h, hipStreamSynchronize(st));
            w.jac_serial = true;
            break;
        }
        // (influence 0: the dense regime takes tens of sweeps, a host round trip per batch: 8, 16, 32, 32, ...)
        int rc = wave_jac_sweeps(h, p, k, !p->jac0 ? 8u : w.jac_sweeps < 14u ? 8u : w.jac_sweeps < 30u ? 16u : 32u, false);
        if (rc != GAMS_OK) return rc;
    }
    w.jac_settled = true;
    return GAMS_OK;
}

int gams_wave_plan_settled(gams_gpu_t *h, gams_wave_plan_t *p, uint32_t *sweeps, int *serial) {
    if (!h || !p || !sweeps || !serial) return gams_fail(h, GAMS_EINVAL, "wave_plan_settled: null argument");
    if (!p->ran) return gams_fail(h, GAMS_ESTATE, "wave_plan_settled: no run to read");
    GAMS_HIP(h, hipSetDevice(h->device));
    const uint32_t k = wave_read_way_index(p);
    const int rc = wave_jac_settle(h, p, k);
    if (rc != GAMS_OK) return rc;
    *sweeps = p->repair ? p->way[k].jac_sweeps : 0u;
    *serial = p->repair ? (p->way[k].jac_serial ? 1 : 0) : (p->serial ? 1 : 0);
    return GAMS_OK;
}

// the argument block of the tile kernels for a pass on way `w` that takes counter slot `slot`
static WaveArgs wave_args(const gams_wave_plan_t *p, const gams_wave_plan::Way &w, uint32_t slot, bool use_plane) {
    const gams_wave_params_t &q = p->prm;
    WaveArgs a{};
    a.seq = p->set->d_seq;
    a.plane = use_plane ? p->set->d_plane : nullptr;
    a.ctgs = p->d_ctgs;
    a.tiles = p->d_tiles;
    a.size = (uint32_t)q.size;
    a.step = (uint32_t)q.step;
    a.lag = q.lag;
    a.tw = p->sel.tw;
    a.max_chunks = p->sel.max_chunks;
    a.max_win = p->sel.max_win;
    a.flags = p->serial ? GAMS_WAVE_DENSE : p->flags;
    a.no_signal = (q.lag < 2 || (p->serial && !p->repair)) ? 1u : 0u;
    a.thr = q.threshold;
    a.thr_abs = std::fabs(q.threshold);
    a.fsize = (float)q.size;
    a.flag_f = (float)q.lag;
    a.cvar = q.lag > 1 ? (float)((double)q.lag / ((double)q.lag - 1.0)) : 0.0f;
    a.g0 = p->g0;
    a.g1 = p->g1;
    a.g2 = p->g2;
    a.g3 = p->g3;
    a.aA = p->sq[0];
    a.aB = p->sq[1];
    a.gA0 = p->sq[2];
    a.gA1 = p->sq[3];
    a.gB0 = p->sq[4];
    a.gB1 = p->sq[5];
    a.peaks = w.d_peaks;
    a.tile_cap = p->tile_cap;
    a.counters = w.d_counters + kSlotWords * slot;
    a.const_sig = p->d_const_sig;
    a.stamps = p->d_stamps;
    a.tile_cnt = w.d_tile_cnt;
    a.dense_cnt = w.d_dense_cnt;
    a.dense_sig = w.d_dense_sig;
    return a;
}

// One pass on way k: touches only that way's state and its stream (run_n drives different ways
// from different host threads); everything else it reads is fixed once the plan exists.
static int wave_pass_on_way(gams_gpu_t *h, gams_wave_plan_t *p, uint32_t k) {
    gams_wave_plan::Way &w = p->way[k];
    hipStream_t st = wave_stream(h, p, k);
    h->reader_epoch.fetch_add(1, std::memory_order_relaxed);   // a reader of the seqset is about to be queued
    // inputs: the way's stream queues behind the uploads and the plan's const table (no host wait)
    if (st == h->compute) {
        int wrc = gams_seqset_wait_uploads(h, p->set);
        if (wrc != GAMS_OK) return wrc;
    } else if (w.seen_upload != p->set->upload_gen && p->set->uploaded) {
        GAMS_HIP(h, hipStreamWaitEvent(st, p->set->uploaded, 0));
    }
    w.seen_upload = p->set->upload_gen;
    if (!w.seen_ready) {
        GAMS_HIP(h, hipStreamWaitEvent(st, p->ready, 0));
        w.seen_ready = true;
    }
    const uint32_t slot = (uint32_t)(w.runs % kCounterRing);
    if (slot == 0 && w.runs > 0)
        GAMS_HIP(h, hipMemsetAsync(w.d_counters, 0, kCounterRing * kSlotWords * sizeof(unsigned long long), st));
    ++w.runs;
    w.last_ring = slot;
    if (p->pipelined && !w.done) GAMS_HIP(h, hipEventCreateWithFlags(&w.done, hipEventDisableTiming));
    if (p->tiles.empty()) {
        // nothing to launch, whatever input or body was asked for: no kernel ran, so not the narrow one
        p->last_body.store(GAMS_WAVE_BODY_WIDE, std::memory_order_relaxed);
        p->last_cut.store(GAMS_WAVE_CUT_AUTO, std::memory_order_relaxed);
        if (p->pipelined) GAMS_HIP(h, hipEventRecord(w.done, st));
        return GAMS_OK;
    }
    const gams_wave_params_t &q = p->prm;
    // The tiled fast kernels stream the seqset's G/C plane when it describes the bytes right now (every upload so
    // far brought both); everything else reads the bytes.  Decided when the pass is queued: a later upload queues
    // itself behind this pass (gams_order_after_readers) and changes the state for the passes after it.
    const bool fast_tile = p->fast_fn != nullptr;
    const bool plane_fit = fast_tile && p->set->plane_ok && p->set->d_plane != nullptr;
    if (p->input_req == GAMS_WAVE_INPUT_PLANE && !plane_fit)
        return gams_fail(h, GAMS_ESTATE, fast_tile ? "wave: the seqset's G/C plane is stale" : "wave: this plan's kernels read the sequence bytes, not the G/C plane");
    const bool use_plane = plane_fit && (p->input_req != GAMS_WAVE_INPUT_BYTES || !p->set->have_bytes);
    if (!use_plane && !p->set->have_bytes)
        return gams_fail(h, GAMS_ESTATE, "wave: the seqset holds the G/C plane only and this plan needs the sequence bytes");
    if (p->input_req == GAMS_WAVE_INPUT_BYTES && use_plane)
        return gams_fail(h, GAMS_ESTATE, "wave: the seqset holds the G/C plane only, the bytes were asked for");
    p->last_input.store(use_plane ? GAMS_WAVE_INPUT_PLANE : GAMS_WAVE_INPUT_BYTES, std::memory_order_relaxed);
    // The headline entry's plane-fed passes run the narrow body (128 threads x 24 windows over the same tiles); passes
    // that read the bytes -- a stale plane, forced bytes -- keep the wide kernel, which holds the byte body.
    const bool narrow_fit = use_plane && p->body.narrow;
    if (p->body_req == GAMS_WAVE_BODY_NARROW && !narrow_fit)
        return gams_fail(h, GAMS_ESTATE, p->body.narrow ? "wave: the narrow body reads the G/C plane, this pass reads the bytes"
                                                        : "wave: this plan has no narrow body");
    const bool narrow = narrow_fit && p->body_req != GAMS_WAVE_BODY_WIDE;
    p->last_body.store(narrow ? GAMS_WAVE_BODY_NARROW : GAMS_WAVE_BODY_WIDE, std::memory_order_relaxed);
    // ... in one of its two cuts of the tile: two waves x 24 windows or one wave x 48 (wave_select_cut)
    if (p->cut_req == GAMS_WAVE_CUT_ONE_WAVE && !narrow_fit)
        return gams_fail(h, GAMS_ESTATE, p->body.narrow ? "wave: the one-wave cut reads the G/C plane, this pass reads the bytes"
                                                        : "wave: this plan has no narrow body to cut");
    const WaveCut cut = narrow ? wave_select_cut(p->body, p->cut_req) : WaveCut{};
    p->last_cut.store(cut.cut, std::memory_order_relaxed);
    const WaveArgs a = wave_args(p, w, slot, use_plane);
    const unsigned nt = (unsigned)p->tiles.size();
    if (p->sel.direct) {
        const uint64_t total = p->total_windows;
        const unsigned blocks = (unsigned)((total + 255) / 256);
        hipLaunchKernelGGL(wave_direct_count_kernel, dim3(blocks), dim3(256), 0, st, p->set->d_seq, p->d_ctgs,
                           p->set->n_ctg, total, (uint32_t)q.size, (uint32_t)q.step, w.d_dense_cnt);
        GAMS_HIP(h, hipGetLastError());
        if (!p->serial || p->repair) {
            hipLaunchKernelGGL(wave_direct_signal_kernel, dim3(blocks), dim3(256), 0, st, p->d_ctgs, p->set->n_ctg,
                               total, w.d_dense_cnt, w.d_dense_sig, q.lag, q.threshold, (float)q.size,
                               q.lag < 2 ? 1u : 0u);
            GAMS_HIP(h, hipGetLastError());
        }
    } else if (narrow) {
        const WaveFastFn cut_fn = cut.cut == GAMS_WAVE_CUT_ONE_WAVE ? kWaveOneWaveFn : kWaveNarrowFn;
        hipLaunchKernelGGL(cut_fn, dim3(nt), dim3(cut.nth), cut.lds_bytes, st, a.tiles, a.seq, a);
        GAMS_HIP(h, hipGetLastError());
    } else if (p->fast_fn) {
        hipLaunchKernelGGL(p->fast_fn, dim3(nt), dim3(p->sel.nth), p->sel.lds_bytes, st, a.tiles, a.seq, a);
        GAMS_HIP(h, hipGetLastError());
    } else {
        hipLaunchKernelGGL(p->tile_fn, dim3(nt), dim3(256), p->sel.lds_bytes, st, a);
        GAMS_HIP(h, hipGetLastError());
    }
    int rc = GAMS_OK;
    if (p->sel.direct && !p->serial) {
        rc = wave_compact_dense(h, p, k, st);
        if (rc != GAMS_OK) return rc;
    }
    if (p->repair) {
        // influence != 1, guess-and-iterate (wave_repair.hpp): the dense rows hold the counts and the S1 signals; a first
        // batch of sweeps is queued behind them -- no host wait here; whoever reads the pass checks that it settled
        // (wave_jac_settle) and queues more sweeps if it did not
        w.jac_sweeps = 0;
        w.jac_settled = false;
        w.jac_serial = false;
        rc = wave_jac_sweeps(h, p, k, kJacFirstBatch, true);
        if (rc != GAMS_OK) return rc;
    } else if (p->serial) {
        rc = wave_serial_recurrence(h, p, k, st, w.d_filtered);
        if (rc == GAMS_OK) rc = wave_compact_dense(h, p, k, st);
        if (rc != GAMS_OK) return rc;
    }
    // An event per run costs a marker packet between back-to-back launches (measured: 8.8 ->
    // 11.7 us per 12-Mb pass), so it is only recorded for plans that overlap several runs.
    if (p->pipelined) GAMS_HIP(h, hipEventRecord(w.done, st));
    return GAMS_OK;
}

// wait for the run the readers look at: its own event in pipelined mode, else its whole stream
static int wave_wait_last_run(gams_gpu_t *h, gams_wave_plan_t *p) {
    gams_wave_plan::Way &w = wave_read_way(p);
    if (p->pipelined && w.done)
        GAMS_HIP(h, hipEventSynchronize(w.done));
    else
        GAMS_HIP(h, hipStreamSynchronize(wave_stream(h, p, wave_read_way_index(p))));
    return GAMS_OK;
}

int gams_wave_plan_set_input(gams_gpu_t *h, gams_wave_plan_t *p, int mode) {
    if (!h || !p) return gams_fail(h, GAMS_EINVAL, "wave_plan_set_input: null argument");
    if (mode != GAMS_WAVE_INPUT_AUTO && mode != GAMS_WAVE_INPUT_BYTES && mode != GAMS_WAVE_INPUT_PLANE)
        return gams_fail(h, GAMS_EINVAL, "wave_plan_set_input: mode is 0 (auto), 1 (bytes) or 2 (plane)");
    p->input_req = mode;
    return GAMS_OK;
}

int gams_wave_plan_last_input(gams_gpu_t *h, gams_wave_plan_t *p, int *input) {
    if (!h || !p || !input) return gams_fail(h, GAMS_EINVAL, "wave_plan_last_input: null argument");
    if (!p->ran) return gams_fail(h, GAMS_ESTATE, "wave_plan_last_input: no run yet");
    *input = p->last_input.load(std::memory_order_relaxed);
    return GAMS_OK;
}

int gams_wave_plan_set_body(gams_gpu_t *h, gams_wave_plan_t *p, int mode) {
    if (!h || !p) return gams_fail(h, GAMS_EINVAL, "wave_plan_set_body: null argument");
    if (mode != GAMS_WAVE_BODY_AUTO && mode != GAMS_WAVE_BODY_WIDE && mode != GAMS_WAVE_BODY_NARROW)
        return gams_fail(h, GAMS_EINVAL, "wave_plan_set_body: mode is 0 (auto), 1 (wide) or 2 (narrow)");
    p->body_req = mode;
    return GAMS_OK;
}

int gams_wave_plan_last_body(gams_gpu_t *h, gams_wave_plan_t *p, int *body) {
    if (!h || !p || !body) return gams_fail(h, GAMS_EINVAL, "wave_plan_last_body: null argument");
    if (!p->ran) return gams_fail(h, GAMS_ESTATE, "wave_plan_last_body: no run yet");
    *body = p->last_body.load(std::memory_order_relaxed);
    return GAMS_OK;
}

int gams_wave_plan_set_cut(gams_gpu_t *h, gams_wave_plan_t *p, int mode) {
    if (!h || !p) return gams_fail(h, GAMS_EINVAL, "wave_plan_set_cut: null argument");
    if (mode != GAMS_WAVE_CUT_AUTO && mode != GAMS_WAVE_CUT_TWO_WAVES && mode != GAMS_WAVE_CUT_ONE_WAVE)
        return gams_fail(h, GAMS_EINVAL, "wave_plan_set_cut: mode is 0 (auto), 1 (two waves) or 2 (one wave)");
    p->cut_req = mode;
    return GAMS_OK;
}

int gams_wave_plan_last_cut(gams_gpu_t *h, gams_wave_plan_t *p, int *cut) {
    if (!h || !p || !cut) return gams_fail(h, GAMS_EINVAL, "wave_plan_last_cut: null argument");
    if (!p->ran) return gams_fail(h, GAMS_ESTATE, "wave_plan_last_cut: no run yet");
    *cut = p->last_cut.load(std::memory_order_relaxed);
    return GAMS_OK;
}

int gams_wave_plan_set_pipelined(gams_gpu_t *h, gams_wave_plan_t *p, int enable) {
    if (!h || !p) return gams_fail(h, GAMS_EINVAL, "wave_plan_set_pipelined: null argument");
    p->pipelined = enable != 0;
    return GAMS_OK;
}

int gams_wave_run(gams_gpu_t *h, gams_wave_plan_t *p) {
    if (!h || !p) return gams_fail(h, GAMS_EINVAL, "wave_run: null argument");
    GAMS_HIP(h, hipSetDevice(h->device));
    const uint32_t k = (uint32_t)(p->run_idx % p->depth);
    int rc = wave_pass_on_way(h, p, k);
    if (rc != GAMS_OK) return rc;
    ++p->run_idx;
    p->last_way = k;
    p->sel_age = 0;
    p->ran = true;
    return GAMS_OK;
}

// A queueing thread of gams_wave_run_n.  It lives as long as the plan (binding a new host thread
// to the device costs ~100 us, more than a short batch), sleeps between batches and, once armed,
// spins until the caller has queued the first round.
struct Launcher {
    std::thread th;
    std::mutex mu;
    std::condition_variable cv;
    bool armed = false, quit = false, finished = true;
    std::atomic<int> go{0};            // 0: wait, 1: run the job, 2: skip it
    gams_gpu_t *h = nullptr;
    gams_wave_plan_t *p = nullptr;
    uint64_t first = 0;
    uint32_t rest = 0;
    uint32_t share = 0, shares = 1;    // this thread queues the ways k with k % shares == share
    int rc = GAMS_OK;
};

static inline void cpu_relax() {
#if defined(__x86_64__) || defined(__i386__)
    __builtin_ia32_pause();
#else
    std::this_thread::yield();
#endif
}

// passes first .. first+rest-1 whose way belongs to `share` (way order is kept per way)
static int wave_queue_share(gams_gpu_t *h, gams_wave_plan_t *p, uint64_t first, uint32_t rest, uint32_t share,
                            uint32_t shares) {
    for (uint32_t j = 0; j < rest; ++j) {
        const uint32_t k = (uint32_t)((first + j) % p->depth);
        if (k % shares != share) continue;
        const int rc = wave_pass_on_way(h, p, k);
        if (rc != GAMS_OK) return rc;
    }
    return GAMS_OK;
}

static void wave_launcher_main(Launcher *L, int device) {
    const bool bound = hipSetDevice(device) == hipSuccess;
    std::unique_lock<std::mutex> lk(L->mu);
    for (;;) {
        L->cv.wait(lk, [&] { return L->armed || L->quit; });
        if (L->quit) return;
        L->armed = false;
        lk.unlock();
        int g;
        while ((g = L->go.load(std::memory_order_acquire)) == 0) cpu_relax();   // a few microseconds
        int rc = GAMS_OK;
        if (g == 1) rc = bound ? wave_queue_share(L->h, L->p, L->first, L->rest, L->share, L->shares) : GAMS_EHIP;
        lk.lock();
        L->rc = rc;
        L->finished = true;
        L->cv.notify_all();
    }
}

static void wave_launcher_stop(gams_wave_plan_t *p) {
    for (Launcher *&L : p->launcher) {
        if (!L) continue;
        {
            std::lock_guard<std::mutex> lk(L->mu);
            L->quit = true;
        }
        L->cv.notify_all();
        L->th.join();
        delete L;
        L = nullptr;
    }
}

int gams_wave_run_n(gams_gpu_t *h, gams_wave_plan_t *p, uint32_t n) {
    if (!h || !p) return gams_fail(h, GAMS_EINVAL, "wave_run_n: null argument");
    // One host thread queues a pass every ~3.3 us (hipLaunchKernelGGL); with three or four passes
    // in flight that is slower than the device drains them (2.85 us per 12-Mb pass), so a batch is
    // queued by several threads: the caller keeps way 0, launcher threads take the other ways
    // (K = 1000 passes at depth 4: 4.4 / 3.1 / 3.0 / 3.0 us per pass with 1 / 2 / 3 / 4 threads;
    // K = 200: 3.8 / 3.8 / 3.6 / 3.5).  The first round goes through gams_wave_run on the caller.
    const uint32_t shares = std::min(p->queue_threads, p->depth);   // default: one queueing thread per way
    const bool threaded = p->depth >= 3 && shares >= 2 && n >= 4 * p->depth;
    if (!threaded) {
        for (uint32_t i = 0; i < n; ++i) {
            int rc = gams_wave_run(h, p);
            if (rc != GAMS_OK) return rc;
        }
        return GAMS_OK;
    }
    const uint32_t lead = p->depth;
    const uint32_t rest = n - lead;
    const uint64_t first = p->run_idx + lead;     // index of the first pass the threads share
    for (uint32_t t = 1; t < shares; ++t) {
        Launcher *&L = p->launcher[t - 1];
        if (!L) {
            L = new Launcher();
            L->th = std::thread(wave_launcher_main, L, h->device);
        }
        {
            std::lock_guard<std::mutex> lk(L->mu);
            L->h = h;
            L->p = p;
            L->first = first;
            L->rest = rest;
            L->share = t;
            L->shares = shares;
            L->go.store(0, std::memory_order_relaxed);
            L->finished = false;
            L->armed = true;
        }
        L->cv.notify_all();                        // wakes up while the first round is queued
    }
    int rc = GAMS_OK;
    for (uint32_t i = 0; i < lead && rc == GAMS_OK; ++i) rc = gams_wave_run(h, p);
    for (uint32_t t = 1; t < shares; ++t)
        p->launcher[t - 1]->go.store(rc == GAMS_OK ? 1 : 2, std::memory_order_release);
    if (rc == GAMS_OK) rc = wave_queue_share(h, p, first, rest, 0u, shares);
    for (uint32_t t = 1; t < shares; ++t) {
        Launcher *L = p->launcher[t - 1];
        std::unique_lock<std::mutex> lk(L->mu);
        L->cv.wait(lk, [&] { return L->finished; });
        if (rc == GAMS_OK) rc = L->rc;
    }
    if (rc != GAMS_OK) return rc;
    p->run_idx = first + rest;
    p->last_way = (uint32_t)((p->run_idx - 1) % p->depth);
    p->sel_age = 0;
    p->ran = true;
    return GAMS_OK;
}

int gams_wave_plan_set_depth(gams_gpu_t *h, gams_wave_plan_t *p, uint32_t depth) {
    if (!h || !p) return gams_fail(h, GAMS_EINVAL, "wave_plan_set_depth: null argument");
    if (depth < 1 || depth > (uint32_t)gams_gpu::kMaxWays)
        return gams_fail(h, GAMS_EINVAL, "wave_plan_set_depth: depth must be 1.." + std::to_string(gams_gpu::kMaxWays));
    GAMS_HIP(h, hipSetDevice(h->device));
    int rc = wave_sync_ways(h, p);                  // the ways of the old depth (wave_retile waits over the new ones)
    if (rc != GAMS_OK) return rc;
    for (uint32_t k = 1; k < depth; ++k)
        if (!h->aux[k - 1]) GAMS_HIP(h, hipStreamCreateWithFlags(&h->aux[k - 1], hipStreamNonBlocking));
    p->depth = depth;
    p->ran = false;
    p->run_idx = 0;
    p->last_way = 0;
    p->sel_age = 0;
    return wave_retile(h, p, p->tw_req);            // the default tile depends on the depth
}

int gams_wave_plan_set_taper(gams_gpu_t *h, gams_wave_plan_t *p, int mode) {
    if (!h || !p) return gams_fail(h, GAMS_EINVAL, "wave_plan_set_taper: null argument");
    if (mode < -1 || mode > 1) return gams_fail(h, GAMS_EINVAL, "wave_plan_set_taper: mode must be -1 (auto), 0 or 1");
    GAMS_HIP(h, hipSetDevice(h->device));
    p->taper_req = mode;
    return wave_retile(h, p, p->tw_req, true);
}

int gams_wave_plan_set_taper_shape(gams_gpu_t *h, gams_wave_plan_t *p, int pct4, int pct8) {
    if (!h || !p) return gams_fail(h, GAMS_EINVAL, "wave_plan_set_taper_shape: null argument");
    if (pct4 < 0 || pct4 > 100 || pct8 < 0 || pct8 > 100)
        return gams_fail(h, GAMS_EINVAL, "wave_plan_set_taper_shape: percentages must be 0..100");
    GAMS_HIP(h, hipSetDevice(h->device));
    p->taper4_pct = pct4;
    p->taper8_pct = pct8;
    return wave_retile(h, p, p->tw_req);
}

int gams_wave_plan_tiles(gams_gpu_t *h, gams_wave_plan_t *p, uint32_t *out, uint64_t cap, uint64_t *n) {
    if (!h || !p || !n || (cap && !out)) return gams_fail(h, GAMS_EINVAL, "wave_plan_tiles: null argument");
    // the host's copy of the table the tile kernel reads: no device work
    *n = p->tiles.size();
    const uint64_t m = std::min<uint64_t>(cap, p->tiles.size());
    for (uint64_t i = 0; i < m; ++i) {
        const WaveTile &t = p->tiles[i];
        out[3 * i] = t.ctg;
        out[3 * i + 1] = t.w0;
        out[3 * i + 2] = t.pad;                    // W of a tapered table's tile, 0 in every other table
    }
    return GAMS_OK;
}

int gams_wave_plan_set_queue_threads(gams_gpu_t *h, gams_wave_plan_t *p, uint32_t n) {
    if (!h || !p) return gams_fail(h, GAMS_EINVAL, "wave_plan_set_queue_threads: null argument");
    if (n < 1 || n > (uint32_t)gams_gpu::kMaxWays)
        return gams_fail(h, GAMS_EINVAL, "wave_plan_set_queue_threads: 1..4");
    p->queue_threads = n;
    return GAMS_OK;
}

int gams_wave_plan_kernel_name(gams_gpu_t *h, gams_wave_plan_t *p, char *buf, size_t n) {
    if (!h || !p || !buf || n == 0) return gams_fail(h, GAMS_EINVAL, "wave_plan_kernel_name: null argument");
    // of a repair pass's kernels (counts + S1 signals, sweeps) the one that takes longest; else the recurrence, else the
    // plan's tile kernel
    if (p->repair)
        std::snprintf(buf, n, "jac_eval_kernel");
    else if (p->serial)
        std::snprintf(buf, n, "%s", p->prm.lag + 1u <= kSerialRing ? "wave_serial_wave_kernel" : "wave_serial_kernel");
    else
        wave_selection_name(p->sel, buf, n);
    return GAMS_OK;
}

int gams_wave_plan_set_lane(gams_gpu_t *h, gams_wave_plan_t *p, uint32_t lane) {
    if (!h || !p) return gams_fail(h, GAMS_EINVAL, "wave_plan_set_lane: null argument");
    if (lane >= (uint32_t)gams_gpu::kMaxWays)
        return gams_fail(h, GAMS_EINVAL, "wave_plan_set_lane: lane must be 0.." + std::to_string(gams_gpu::kMaxWays - 1));
    GAMS_HIP(h, hipSetDevice(h->device));
    int rc = wave_sync_ways(h, p);
    if (rc != GAMS_OK) return rc;
    for (uint32_t k = 1; k < (uint32_t)gams_gpu::kMaxWays; ++k)
        if (!h->aux[k - 1]) GAMS_HIP(h, hipStreamCreateWithFlags(&h->aux[k - 1], hipStreamNonBlocking));
    p->lane = lane;
    // the ways now run on other streams: they have to queue behind the uploads and the const table again
    for (auto &w : p->way) {
        w.seen_upload = 0;
        w.seen_ready = false;
    }
    p->set->dirty = true;
    return GAMS_OK;
}

int gams_wave_plan_select(gams_gpu_t *h, gams_wave_plan_t *p, uint32_t age) {
    if (!h || !p) return gams_fail(h, GAMS_EINVAL, "wave_plan_select: null argument");
    if (age >= p->depth || age >= p->run_idx)
        return gams_fail(h, GAMS_ESTATE, "wave_plan_select: that run is no longer (or not yet) held");
    p->sel_age = age;
    return GAMS_OK;
}

int gams_wave_peaks(gams_gpu_t *h, gams_wave_plan_t *p, const gams_peak_t **peaks, uint64_t *n_peaks) {
    if (!h || !p || !peaks || !n_peaks) return gams_fail(h, GAMS_EINVAL, "wave_peaks: null argument");
    if (!(p->flags & GAMS_WAVE_PEAKS)) return gams_fail(h, GAMS_ESTATE, "wave_peaks: plan has no PEAKS output");
    if (!p->ran) return gams_fail(h, GAMS_ESTATE, "wave_peaks: no run to read");
    GAMS_HIP(h, hipSetDevice(h->device));
    const size_t nt = p->tiles.size();
    if (nt == 0) {
        *peaks = nullptr;
        *n_peaks = 0;
        return GAMS_OK;
    }
    for (int attempt = 0; attempt < 2; ++attempt) {
        {
            const int src = wave_jac_settle(h, p, wave_read_way_index(p));   // influence != 1: the pass has reached its fixed point
            if (src != GAMS_OK) return src;
        }
        // two words behind the offsets (re-read every attempt: a regrow replaces the arena)
        unsigned long long *const d_totals = p->d_tile_off + nt;
        // The readback stream queues behind the run (pipelined: behind this plan's run only, later
        // runs of other plans keep going); the host waits once, for the two totals.
        gams_wave_plan::Way &w = wave_read_way(p);
        if (p->pipelined && w.done) {
            GAMS_HIP(h, hipStreamWaitEvent(h->readback, w.done, 0));
        } else {
            if (!w.ran_ev) GAMS_HIP(h, hipEventCreateWithFlags(&w.ran_ev, hipEventDisableTiming));
            GAMS_HIP(h, hipEventRecord(w.ran_ev, wave_stream(h, p, wave_read_way_index(p))));
            GAMS_HIP(h, hipStreamWaitEvent(h->readback, w.ran_ev, 0));
        }
        {
            const int drc = wave_first_dense(h, p);
            if (drc != GAMS_OK) return drc;
        }
        Chain ch{h->readback};
        ch.pack(p, w);
        GAMS_HIP(h, ch.err);
        GAMS_HIP(h, hipMemcpyAsync(h->pin_scratch, d_totals, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost,
                                   h->readback));
        GAMS_HIP(h, hipStreamSynchronize(h->readback));
        const uint64_t total = h->pin_scratch[0];
        const uint64_t worst = h->pin_scratch[1];
        // (values no pass over this plan can produce are refused instead of allocating and copying by them)
        if (!wave_totals_plausible(p, total, worst))
            return gams_fail(h, GAMS_EHIP,
                             "wave_peaks: inconsistent peak counts from the device (total " + std::to_string(total) +
                                 ", fullest tile " + std::to_string(worst) + ", " + std::to_string(p->total_windows) +
                                 " windows in " + std::to_string(nt) + " tiles of at most " + std::to_string(p->sel.tw) + ")");
        if (worst > p->tile_cap) {
            const int rc = wave_regrow_slots(h, p, worst);
            if (rc != GAMS_OK) return rc;
            continue;
        }
        if (total) {
            const size_t grown = (total + total / 4 + 1024) * sizeof(gams_peak_t);
            if (total > p->dense_cap()) {
                GAMS_HIP(h, p->d_dense.grow(h, total * sizeof(gams_peak_t), grown));
                ch.gather(p, w);
                GAMS_HIP(h, ch.err);
            }
            GAMS_HIP(h, p->h_peaks.grow(h, total * sizeof(gams_peak_t), grown));
            GAMS_HIP(h, hipMemcpyAsync(p->h_peaks, p->d_dense, total * sizeof(gams_peak_t), hipMemcpyDeviceToHost,
                                       h->readback));
            GAMS_HIP(h, hipStreamSynchronize(h->readback));
        }
        *peaks = p->h_peaks;   // NULL when there is none
        *n_peaks = total;
        return GAMS_OK;
    }
    return gams_fail(h, GAMS_EHIP, "wave_peaks: peak buffer overflow persisted");
}

// ---- rows as text ---------------------------------------------------------------------------------
}  // extern "C"
namespace {
// What the row kernels print from, built on the host: the chromosome names in one blob with a RowCtg per ctg
// (ctgs of one chromosome share its name; one copy per distinct pointer is not worth the bookkeeping: a few bytes
// per ctg), and the gc text table, Rust's `{}` of the f32 k / size (what wave.rs:196 prints) for every count k.
struct RowTabs {
    std::vector<RowCtg> rc;
    std::string blob;
    std::vector<uint8_t> gct;
    // "" or what `who` has to report (GAMS_EUNSUPPORTED)
    std::string fill(const char *who, uint32_t n_ctg, const char *const *chr, const int32_t *chr_start, int32_t size) {
        rc.assign(std::max<uint32_t>(n_ctg, 1), RowCtg{});
        for (uint32_t c = 0; c < n_ctg; ++c) {
            const size_t len = std::strlen(chr[c]);
            size_t at = blob.find(chr[c]);
            if (at == std::string::npos || len == 0) {
                at = blob.size();
                blob += chr[c];
            }
            rc[c] = RowCtg{(uint32_t)at, (uint32_t)len, chr_start[c], 0u};
        }
        gct.assign(((size_t)size + 1) * kGcStride, 0);
        for (int32_t k = 0; k <= size; ++k) {
            char t[32];
            const uint32_t len = gams_fmt_f32_short((float)k / (float)size, t);     // gc_content as wave.rs prints it
            if (len == 0u || len > kGcStride - 1) return std::string(who) + ": gc_content text too long";
            gct[(size_t)k * kGcStride] = (uint8_t)len;
            std::memcpy(&gct[(size_t)k * kGcStride + 1], t, len);
        }
        return "";
    }
    // the three tables' place in their owner's arena, with room for names_cap bytes of names
    RowTabsDev take(Carver &c, size_t names_cap) const {
        RowTabsDev d;
        d.ctgs = c.take<RowCtg>(rc.size());
        d.names = c.take<char>(names_cap);
        d.gctab = c.take<uint8_t>(gct.size());
        return d;
    }
    // ... and their bytes, copied before the call returns, or queued on `st` (the tables must outlive that copy)
    hipError_t upload(const RowTabsDev &d) const {
        return each(d, [](void *dst, const void *src, size_t n) { return hipMemcpy(dst, src, n, hipMemcpyHostToDevice); });
    }
    hipError_t upload_async(const RowTabsDev &d, hipStream_t st) const {
        return each(d, [st](void *dst, const void *src, size_t n) { return hipMemcpyAsync(dst, src, n, hipMemcpyHostToDevice, st); });
    }
    template <typename Copy>
    hipError_t each(const RowTabsDev &d, Copy copy) const {
        hipError_t e = copy(d.ctgs, rc.data(), rc.size() * sizeof(RowCtg));
        if (e == hipSuccess && !blob.empty()) e = copy(d.names, blob.data(), blob.size());
        if (e == hipSuccess) e = copy(d.gctab, gct.data(), gct.size());
        return e;
    }
};

// where every ctg's rows begin, from where those of the ctgs that have rows do (~0: a ctg without): it begins where the
// next one does, the last at the text's end
void rows_fill_ctg_off(unsigned long long *off, uint32_t n_ctg, unsigned long long bytes) {
    off[n_ctg] = bytes;
    for (uint32_t c = n_ctg; c-- > 0;)
        if (off[c] == ~0ull) off[c] = off[c + 1];
}

// what both text entries ask of the chromosome table (GAMS_EINVAL): "" or what `who` has to report
std::string rows_check_chr(const char *who, const gams_wave_plan_t *p, const char *const *chr, const int32_t *chr_start) {
    for (uint32_t c = 0; c < p->set->n_ctg; ++c) {
        if (!chr[c]) return std::string(who) + ": null chromosome name";
        if (chr_start[c] < 0 || (int64_t)chr_start[c] + p->ctgs[c].len >= 0x7FFFFFFFll)
            return std::string(who) + ": chromosome coordinates must be in [0, 2^31)";
    }
    return "";
}

struct RowTables {
    uint8_t *flags;
    int2 *headpos, *blk_head;
    uint32_t *tailwin, *len, *blk_len;
    unsigned long long *blk_off;
    uint32_t nb_cap;
    size_t bytes;
};
RowTables rows_carve(uint8_t *base, uint64_t cap) {
    const uint32_t nb = (uint32_t)((cap + kRowsBlock - 1) / kRowsBlock);
    Carver c(base);
    RowTables t{};
    t.headpos = c.take<int2>(cap);
    t.tailwin = c.take<uint32_t>(cap);
    t.len = c.take<uint32_t>(cap);
    t.flags = c.take<uint8_t>(cap);
    t.blk_head = c.take<int2>(nb);
    t.blk_len = c.take<uint32_t>(nb);
    t.blk_off = c.take<unsigned long long>((size_t)nb + 2);
    t.nb_cap = nb;
    t.bytes = c.bytes();
    return t;
}

// The kernels and copies of one rows pass over way `wi`, in order: launched on `st` as they are (graph == nullptr), or
// added to `graph` as a chain of nodes.  (Built node by node rather than by stream capture: a capture is invalidated
// by what OTHER host threads do meanwhile, and the host layer runs one thread per handle.)
int rows_emit(gams_gpu_t *h, gams_wave_plan_t *p, uint32_t wi, hipStream_t st, uint64_t copy_bytes, hipGraph_t graph) {
    WaveRows *r = p->rows;
    gams_wave_plan::Way &w = p->way[wi];
    const RowTables t = rows_carve(r->tmp, r->cap);
    const uint32_t n_ctg = p->set->n_ctg;
    RowArgs a{};
    a.rec = p->d_dense;
    a.n_rec = p->d_tile_off + p->tiles.size();   // the total behind the tiles' offsets
    a.cap = std::min<uint64_t>(r->cap, p->dense_cap());
    a.tile_cap = p->tile_cap;
    a.ctgs = r->tabs.ctgs;
    a.n_ctg = n_ctg;
    a.names = r->tabs.names;
    a.gctab = r->tabs.gctab;
    a.size = (uint32_t)p->prm.size;
    a.step = (uint32_t)p->prm.step;
    a.dmax = r->dmax;
    a.flags = t.flags;
    a.headpos = t.headpos;
    a.blk_head = t.blk_head;
    a.tailwin = t.tailwin;
    a.len = t.len;
    a.blk_len = t.blk_len;
    a.blk_off = t.blk_off;
    a.nb_cap = t.nb_cap;
    a.text = r->d_text;
    a.text_cap = r->d_text.cap;
    a.words = r->d_words;
    Chain ch{st, graph};
    void *args_rows[] = {&a};
    const uint32_t nb = t.nb_cap;
    ch.pack(p, w);
    ch.kernel(reinterpret_cast<const void *>(rows_link_kernel), nb, 256, args_rows);
    ch.kernel(reinterpret_cast<const void *>(rows_heads_kernel), 1, 1024, args_rows);
    ch.kernel(reinterpret_cast<const void *>(rows_tail_kernel), (unsigned)((r->cap + 255) / 256), 256, args_rows);
    ch.kernel(reinterpret_cast<const void *>(rows_len_kernel), nb, 256, args_rows);
    ch.offsets(t.blk_len, nb, t.blk_off, t.blk_off + nb);
    ch.kernel(reinterpret_cast<const void *>(rows_write_kernel), nb, 256, args_rows);
    // the words (sizes, totals, per-ctg offsets: one block) and -- sized by the previous pass -- the text itself go to the
    // host behind the kernels
    ch.copy(r->h_words, r->d_words, ((size_t)n_ctg + 1 + 4) * 8);
    ch.copy(r->h_text, r->d_text, copy_bytes);
    if (ch.err != hipSuccess) {
        (void)hipGetLastError();
        return gams_fail(h, GAMS_EHIP, std::string("wave_rows: ") + hipGetErrorString(ch.err));
    }
    return GAMS_OK;
}

// queue everything of one rows pass on the readback stream, behind the run the readers look at.  The dozen launches
// and copies are one graph per way (a plan's buffers do not move between passes; the graph is rebuilt when one does): one
// call instead of ten on the host thread that also queues the passes themselves.
int rows_queue(gams_gpu_t *h, gams_wave_plan_t *p) {
    WaveRows *r = p->rows;
    const uint32_t wi = wave_read_way_index(p);
    gams_wave_plan::Way &w = p->way[wi];
    {
        const int src = wave_jac_settle(h, p, wi);      // influence != 1: the pass has reached its fixed point
        if (src != GAMS_OK) return src;
    }
    // The rows go on the stream the pass itself ran on: ordered behind it without an event, and the rows of plans
    // on different lanes run side by side (eight short dependent kernels and a 2-MB copy per batch: on one shared
    // stream they were 117 us per batch for three plans in flight, the passes themselves 22).
    hipStream_t st = wave_stream(h, p, wi);
    {
        const int drc = wave_first_dense(h, p);
        if (drc != GAMS_OK) return drc;
    }
    const uint64_t cap = std::min<uint64_t>(p->dense_cap(), 0x7FFFFF00ull);
    if (r->cap < cap) {   // (in records: the block is replaced even where the pool had rounded it up far enough)
        r->tmp.free(h);
        r->cap = 0;
        const size_t tables = rows_carve(nullptr, cap).bytes;
        GAMS_HIP(h, r->tmp.reserve(h, tables));
        r->cap = cap;
    }
    const uint64_t want_text = std::max<uint64_t>(r->cap * ((uint64_t)r->max_name + 44u), 1u << 20);
    GAMS_HIP(h, r->d_text.reserve(h, want_text));
    // the text's speculative copy: sized by the previous pass, kept while it still fits (the graph holds the size)
    uint64_t copy_bytes = r->copy_bytes;
    if (r->last_bytes && (copy_bytes < r->last_bytes || copy_bytes > 2 * r->last_bytes + (1u << 20)))
        copy_bytes = std::min<uint64_t>(r->d_text.cap, (r->last_bytes + r->last_bytes / 8 + 65536) & ~(uint64_t)65535);
    GAMS_HIP(h, r->h_text.reserve(h, copy_bytes));
    r->copy_bytes = copy_bytes;
    r->copied = copy_bytes;
    const WaveRows::RowGraphKey key{p->d_dense, r->tmp, r->d_text, r->h_text, w.d_peaks, w.d_tile_cnt, p->d_tile_off, p->dense_cap(),
                          r->cap, copy_bytes, p->tile_cap, (uint32_t)p->tiles.size()};
    WaveRows::RowGraph &g = r->graph[wi];
    bool launched = false;
    if (r->use_graph) {
        if (!g.exec || std::memcmp(&g.key, &key, sizeof key) != 0) {
            if (g.exec) (void)hipGraphExecDestroy(g.exec);
            g.exec = nullptr;
            hipGraph_t graph = nullptr;
            hipError_t e = hipGraphCreate(&graph, 0);
            if (e == hipSuccess && rows_emit(h, p, wi, st, copy_bytes, graph) != GAMS_OK) e = hipErrorUnknown;
            if (e == hipSuccess) e = hipGraphInstantiate(&g.exec, graph, nullptr, nullptr, 0);
            if (graph) (void)hipGraphDestroy(graph);
            if (e != hipSuccess) {
                (void)hipGetLastError();
                g.exec = nullptr;
                r->use_graph = false;       // this runtime will not take the graph: plain launches from here on
            } else {
                g.key = key;
            }
        }
        if (g.exec) {
            GAMS_HIP(h, hipGraphLaunch(g.exec, st));
            launched = true;
        }
    }
    if (!launched) {
        const int rc = rows_emit(h, p, wi, st, copy_bytes, nullptr);
        if (rc != GAMS_OK) return rc;
    }
    if (!r->done) GAMS_HIP(h, hipEventCreateWithFlags(&r->done, hipEventDisableTiming));
    GAMS_HIP(h, hipEventRecord(r->done, st));
    r->begun = true;
    return GAMS_OK;
}
}  // namespace
extern "C" {

int gams_wave_rows_setup(gams_gpu_t *h, gams_wave_plan_t *p, const char *const *chr, const int32_t *chr_start,
                         float coverage) {
    if (!h || !p || (p->set->n_ctg && (!chr || !chr_start))) return gams_fail(h, GAMS_EINVAL, "wave_rows_setup: null argument");
    if (!(p->flags & GAMS_WAVE_PEAKS)) return gams_fail(h, GAMS_ESTATE, "wave_rows_setup: plan has no PEAKS output");
    const gams_wave_params_t &q = p->prm;
    // merge_ints (wave.rs:217-252) links windows i < j iff they intersect and size / |intersection| >= coverage
    // (both ratios are that one: all windows have one size).  The device makes rows when every intersecting
    // pair links, i.e. when the smallest possible ratio -- at distance 1 -- already passes.
    const int64_t dmax = ((int64_t)q.size + q.step - 1) / q.step - 1;
    if (dmax >= 1) {
        const float inter = (float)(int32_t)(q.size - q.step);
        if (!((float)q.size / inter >= coverage))
            return gams_fail(h, GAMS_EUNSUPPORTED,
                             "wave_rows_setup: this --coverage links only some of the overlapping windows; merge the "
                             "peaks on the host (gams_wave_peaks)");
    }
    const uint32_t n_ctg = p->set->n_ctg;
    {
        const std::string bad = rows_check_chr("wave_rows_setup", p, chr, chr_start);
        if (!bad.empty()) return gams_fail(h, GAMS_EINVAL, bad);
    }
    GAMS_HIP(h, hipSetDevice(h->device));
    if (p->rows) {                       // set up again (other names / coverage): drop the old tables
        GAMS_HIP(h, hipStreamSynchronize(h->readback));
        WaveRows *r = p->rows;
        r->arena.free(h);
        r->h_words.free(h);
        for (auto &g : r->graph) {
            if (g.exec) (void)hipGraphExecDestroy(g.exec);
            g.exec = nullptr;
        }
    } else {
        p->rows = new WaveRows();
    }
    WaveRows *r = p->rows;
    r->dmax = (uint32_t)dmax;
    r->begun = false;
    RowTabs tabs;
    const std::string bad = tabs.fill("wave_rows_setup", n_ctg, chr, chr_start, q.size);
    if (!bad.empty()) return gams_fail(h, GAMS_EUNSUPPORTED, bad);
    r->max_name = 0;
    for (const RowCtg &c : tabs.rc) r->max_name = std::max(r->max_name, c.name_len);
    const size_t n_words = (size_t)n_ctg + 1 + 4;
    auto arena = [&](Carver &c) {
        r->tabs = tabs.take(c, std::max<size_t>(tabs.blob.size(), 1));
        r->d_words = c.take<unsigned long long>(n_words);
    };
    GAMS_HIP(h, wave_arena(h, r->arena, arena));
    GAMS_HIP(h, tabs.upload(r->tabs));
    GAMS_HIP(h, r->h_words.reserve(h, n_words * 8));
    return GAMS_OK;
}

int gams_wave_rows_begin(gams_gpu_t *h, gams_wave_plan_t *p) {
    if (!h || !p) return gams_fail(h, GAMS_EINVAL, "wave_rows_begin: null argument");
    if (!p->rows) return gams_fail(h, GAMS_ESTATE, "wave_rows_begin: call gams_wave_rows_setup first");
    if (!p->ran) return gams_fail(h, GAMS_ESTATE, "wave_rows_begin: no run to read");
    GAMS_HIP(h, hipSetDevice(h->device));
    if (p->tiles.empty()) {
        p->rows->begun = true;
        return GAMS_OK;
    }
    return rows_queue(h, p);
}

int gams_wave_rows_end(gams_gpu_t *h, gams_wave_plan_t *p, const char **text, uint64_t *text_bytes,
                       const uint64_t **ctg_off) {
    if (!h || !p || !text || !text_bytes) return gams_fail(h, GAMS_EINVAL, "wave_rows_end: null argument");
    if (!p->rows || !p->rows->begun) return gams_fail(h, GAMS_ESTATE, "wave_rows_end: no gams_wave_rows_begin to finish");
    GAMS_HIP(h, hipSetDevice(h->device));
    WaveRows *r = p->rows;
    const uint32_t n_ctg = p->set->n_ctg;
    r->begun = false;
    if (p->tiles.empty()) {
        for (uint32_t c = 0; c <= n_ctg; ++c) r->h_words[4 + c] = 0;
        *text = nullptr;
        *text_bytes = 0;
        if (ctg_off) *ctg_off = reinterpret_cast<const uint64_t *>(r->h_words + 4);
        return GAMS_OK;
    }
    for (int attempt = 0; attempt < 4; ++attempt) {
        GAMS_HIP(h, hipEventSynchronize(r->done));
        const uint64_t n_rec = r->h_words[0], bytes = r->h_words[1], total = r->h_words[2], worst = r->h_words[3];
        if (!wave_totals_plausible(p, total, worst))
            return gams_fail(h, GAMS_EHIP, "wave_rows: inconsistent peak counts from the device");
        int rc = GAMS_OK;
        if (worst > p->tile_cap) {
            rc = wave_regrow_slots(h, p, worst);   // ... then the rows once more
        } else if (total > p->dense_cap() || total > r->cap) {
            if (total > 0x7FFFFF00ull) return gams_fail(h, GAMS_EUNSUPPORTED, "wave_rows: more than 2^31 peaks in one pass");
            const size_t grown = (total + total / 4 + 1024) * sizeof(gams_peak_t);
            p->d_dense.free(h);
            GAMS_HIP(h, p->d_dense.reserve(h, grown));
        } else if (bytes > r->d_text.cap) {
            return gams_fail(h, GAMS_EHIP, "wave_rows: text beyond its bound");
        } else {
            (void)n_rec;
            if (bytes > r->copied) {
                // the speculative copy fell short (the first pass, or more text than last time): the rest now
                if (r->h_text.cap < bytes) {
                    // the new block first: the old one still holds the part already copied
                    Kept<char> blk{true};
                    GAMS_HIP(h, blk.reserve(h, bytes + bytes / 4 + 4096));
                    if (r->copied) std::memcpy(blk, r->h_text, r->copied);
                    std::swap(blk, r->h_text);
                    blk.free(h);
                }
                GAMS_HIP(h, hipMemcpyAsync(r->h_text + r->copied, r->d_text + r->copied, bytes - r->copied,
                                           hipMemcpyDeviceToHost, h->readback));
                GAMS_HIP(h, hipStreamSynchronize(h->readback));
            }
            r->last_bytes = bytes;
            unsigned long long *off = r->h_words + 4;
            rows_fill_ctg_off(off, n_ctg, bytes);
            *text = bytes ? r->h_text.p : nullptr;
            *text_bytes = bytes;
            if (ctg_off) *ctg_off = reinterpret_cast<const uint64_t *>(off);
            return GAMS_OK;
        }
        if (rc != GAMS_OK) return rc;
        rc = rows_queue(h, p);
        if (rc != GAMS_OK) return rc;
    }
    return gams_fail(h, GAMS_EHIP, "wave_rows: buffers kept overflowing");
}

int gams_wave_signal_text(gams_gpu_t *h, gams_wave_plan_t *p, const char *const *chr, const int32_t *chr_start,
                          const char **text, uint64_t *text_bytes, const uint64_t **ctg_off) {
    if (!h || !p || !text || !text_bytes || !ctg_off || (p->set->n_ctg && (!chr || !chr_start)))
        return gams_fail(h, GAMS_EINVAL, "wave_signal_text: null argument");
    if (!(p->flags & GAMS_WAVE_DENSE)) return gams_fail(h, GAMS_ESTATE, "wave_signal_text: plan has no DENSE output");
    if (!p->ran) return gams_fail(h, GAMS_ESTATE, "wave_signal_text: no run to read");
    const gams_wave_params_t &q = p->prm;
    const uint32_t n_ctg = p->set->n_ctg;
    {
        const std::string bad = rows_check_chr("wave_signal_text", p, chr, chr_start);
        if (!bad.empty()) return gams_fail(h, GAMS_EINVAL, bad);
    }
    GAMS_HIP(h, hipSetDevice(h->device));
    {
        int wrc = wave_jac_settle(h, p, wave_read_way_index(p));
        if (wrc == GAMS_OK) wrc = wave_wait_last_run(h, p);
        if (wrc != GAMS_OK) return wrc;
    }
    // names, gc text table (as gams_wave_rows_setup), tiles of kSigRows windows
    RowTabs tabs;
    const std::string bad = tabs.fill("wave_signal_text", n_ctg, chr, chr_start, q.size);
    if (!bad.empty()) return gams_fail(h, GAMS_EUNSUPPORTED, bad);
    if (!p->sigtext) p->sigtext = new WaveSig();
    WaveSig *g = p->sigtext;
    if (!g->arena || g->names_cap < tabs.blob.size()) {
        std::vector<SigTile> st;
        for (uint32_t c = 0; c < n_ctg; ++c)
            for (uint32_t w0 = 0; w0 < p->ctgs[c].n_win; w0 += kSigRows)
                st.push_back(SigTile{c, w0, p->ctgs[c].n_win, 0u, p->ctgs[c].win_base});
        g->n_tiles = (uint32_t)st.size();
        g->names_cap = std::max<size_t>(tabs.blob.size(), 64) * 2;
        const size_t nt = std::max<size_t>(st.size(), 1);
        auto arena = [&](Carver &c) {
            g->d_tiles = c.take<SigTile>(nt);
            g->d_blk_len = c.take<uint32_t>(nt);
            g->d_blk_off = c.take<unsigned long long>(nt + 2);
            g->tabs = tabs.take(c, g->names_cap);
            g->d_words = c.take<unsigned long long>(std::max<size_t>(n_ctg, 1));
        };
        GAMS_HIP(h, wave_arena(h, g->arena, arena));
        if (!st.empty()) GAMS_HIP(h, hipMemcpy(g->d_tiles, st.data(), st.size() * sizeof(SigTile), hipMemcpyHostToDevice));
        g->h_words.free(h);
        GAMS_HIP(h, g->h_words.reserve(h, ((size_t)2 * n_ctg + 2) * 8));
    }
    *text = nullptr;
    *text_bytes = 0;
    unsigned long long *off = g->h_words + n_ctg;          // ctg_off[n_ctg + 1]
    if (g->n_tiles == 0) {
        for (uint32_t c = 0; c <= n_ctg; ++c) off[c] = 0;
        *ctg_off = reinterpret_cast<const uint64_t *>(off);
        return GAMS_OK;
    }
    hipStream_t st = h->readback;
    GAMS_HIP(h, tabs.upload_async(g->tabs, st));
    GAMS_HIP(h, hipMemsetAsync(g->d_words, 0xFF, std::max<size_t>(n_ctg, 1) * 8, st));
    gams_wave_plan::Way &w = wave_read_way(p);
    SigArgs a{};
    a.tiles = g->d_tiles;
    a.n_tiles = g->n_tiles;
    a.cnt = w.d_dense_cnt;
    a.sig = w.d_dense_sig;
    a.ctgs = g->tabs.ctgs;
    a.names = g->tabs.names;
    a.gctab = g->tabs.gctab;
    a.size = (uint32_t)q.size;
    a.step = (uint32_t)q.step;
    a.blk_len = g->d_blk_len;
    a.blk_off = g->d_blk_off;
    a.words = g->d_words;
    unsigned long long *const d_totals = g->d_blk_off + g->n_tiles;
    Chain ch{st};
    void *args_sig[] = {&a};                     // (read at each launch: the write kernel sees the text set below)
    ch.kernel(reinterpret_cast<const void *>(sig_len_kernel), g->n_tiles, 256, args_sig);
    ch.offsets(g->d_blk_len, g->n_tiles, g->d_blk_off, d_totals);
    ch.copy(h->pin_scratch, d_totals, 2 * sizeof(unsigned long long));
    GAMS_HIP(h, ch.err);
    GAMS_HIP(h, hipStreamSynchronize(st));       // (`tabs` lives on this call's stack until here)
    const uint64_t total = h->pin_scratch[0];
    GAMS_HIP(h, g->d_text.grow(h, total, total + total / 16 + 4096));
    GAMS_HIP(h, g->h_text.grow(h, total, total + total / 16 + 4096));
    a.text = g->d_text;
    a.text_cap = total;
    ch.kernel(reinterpret_cast<const void *>(sig_write_kernel), g->n_tiles, 256, args_sig);
    ch.copy(g->h_words, g->d_words, std::max<size_t>(n_ctg, 1) * 8);
    ch.copy(g->h_text, g->d_text, total);
    GAMS_HIP(h, ch.err);
    GAMS_HIP(h, hipStreamSynchronize(st));
    std::copy(g->h_words.p, g->h_words.p + n_ctg, off);    // where the rows of the ctgs that have a window begin
    rows_fill_ctg_off(off, n_ctg, total);
    *text = g->h_text;
    *text_bytes = total;
    *ctg_off = reinterpret_cast<const uint64_t *>(off);
    return GAMS_OK;
}

int gams_wave_dense(gams_gpu_t *h, gams_wave_plan_t *p, uint32_t i, uint32_t *gc_count, int8_t *signal) {
    if (!h || !p) return gams_fail(h, GAMS_EINVAL, "wave_dense: null argument");
    if (!(p->flags & GAMS_WAVE_DENSE)) return gams_fail(h, GAMS_ESTATE, "wave_dense: plan has no DENSE output");
    if (!p->ran) return gams_fail(h, GAMS_ESTATE, "wave_dense: no run to read");
    if (i >= p->ctgs.size()) return gams_fail(h, GAMS_EINVAL, "wave_dense: ctg index out of range");
    GAMS_HIP(h, hipSetDevice(h->device));
    {
        int wrc = wave_jac_settle(h, p, wave_read_way_index(p));
        if (wrc == GAMS_OK) wrc = wave_wait_last_run(h, p);
        if (wrc != GAMS_OK) return wrc;
    }
    const WaveCtgDev &c = p->ctgs[i];
    if (c.n_win == 0) return GAMS_OK;
    gams_wave_plan::Way &w = wave_read_way(p);
    if (gc_count)
        GAMS_HIP(h, hipMemcpy(gc_count, w.d_dense_cnt + c.win_base, (size_t)c.n_win * sizeof(uint32_t),
                              hipMemcpyDeviceToHost));
    if (signal)
        GAMS_HIP(h, hipMemcpy(signal, w.d_dense_sig + c.win_base, (size_t)c.n_win, hipMemcpyDeviceToHost));
    return GAMS_OK;
}

int gams_wave_plan_set_stamps(gams_gpu_t *h, gams_wave_plan_t *p, int enable) {
    if (!h || !p) return gams_fail(h, GAMS_EINVAL, "wave_plan_set_stamps: null argument");
    GAMS_HIP(h, hipSetDevice(h->device));
    {
        int src = wave_sync_ways(h, p);
        if (src != GAMS_OK) return src;
    }
    (void)hipFree(p->d_stamps);
    p->d_stamps = nullptr;
    if (enable) {
        const size_t n = std::max<size_t>(p->tiles.size(), 1) * 16;
        GAMS_HIP(h, hipMalloc(&p->d_stamps, n * sizeof(unsigned long long)));
        GAMS_HIP(h, hipMemsetAsync(p->d_stamps, 0, n * sizeof(unsigned long long), h->compute));
        GAMS_HIP(h, hipStreamSynchronize(h->compute));
    }
    return GAMS_OK;
}

int gams_wave_stamps(gams_gpu_t *h, gams_wave_plan_t *p, double *mean_cycles, uint64_t *span_cycles) {
    if (!h || !p || !mean_cycles || !span_cycles) return gams_fail(h, GAMS_EINVAL, "wave_stamps: null argument");
    if (!p->d_stamps) return gams_fail(h, GAMS_ESTATE, "wave_stamps: stamps are off");
    GAMS_HIP(h, hipSetDevice(h->device));
    {
        int src = wave_sync_ways(h, p);
        if (src != GAMS_OK) return src;
    }
    const size_t nt = p->tiles.size();
    std::vector<unsigned long long> st(std::max<size_t>(nt, 1) * 16);
    GAMS_HIP(h, hipMemcpy(st.data(), p->d_stamps, st.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    for (int k = 0; k < 8; ++k) mean_cycles[k] = 0.0;
    size_t used = 0;
    unsigned long long r_lo = ~0ull, r_hi = 0, r_sum = 0;
    double cyc_sum = 0.0;
    for (size_t t = 0; t < nt; ++t) {
        const unsigned long long *w = &st[t * 16];
        bool ok = w[8] != 0 && w[9] >= w[8];
        for (int k = 0; k < 6; ++k) ok &= w[k] != 0 && w[k + 1] >= w[k] && w[k + 1] - w[k] < (1ull << 28);
        if (!ok) continue;
        ++used;
        for (int k = 0; k < 6; ++k) mean_cycles[k] += (double)(w[k + 1] - w[k]);
        mean_cycles[6] += (double)(w[6] - w[0]);
        r_lo = std::min(r_lo, w[8]);
        r_hi = std::max(r_hi, w[9]);
        r_sum += w[9] - w[8];
        cyc_sum += (double)(w[6] - w[0]);
    }
    if (used)
        for (int k = 0; k < 7; ++k) mean_cycles[k] /= (double)used;
    // shader clock in GHz = cycles / (ticks * 10 ns)
    mean_cycles[7] = r_sum ? cyc_sum / ((double)r_sum * 10.0) : 0.0;
    // high half: launch span in 10-ns ticks; low half: sum of workgroup lifetimes in ticks / 16
    *span_cycles = used ? (((r_hi - r_lo) & 0xffffffffull) << 32) | ((r_sum >> 4) & 0xffffffffull) : 0;
    return GAMS_OK;
}

int gams_wave_stamps_raw(gams_gpu_t *h, gams_wave_plan_t *p, uint64_t *out, uint64_t n_words) {
    if (!h || !p || !out) return gams_fail(h, GAMS_EINVAL, "wave_stamps_raw: null argument");
    if (!p->d_stamps) return gams_fail(h, GAMS_ESTATE, "wave_stamps_raw: stamps are off");
    GAMS_HIP(h, hipSetDevice(h->device));
    {
        int src = wave_sync_ways(h, p);
        if (src != GAMS_OK) return src;
    }
    const uint64_t n = std::min<uint64_t>(n_words, (uint64_t)p->tiles.size() * 16);
    GAMS_HIP(h, hipMemcpy(out, p->d_stamps, n * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return GAMS_OK;
}

int gams_wave_exact_count(gams_gpu_t *h, gams_wave_plan_t *p, uint64_t *n_exact) {
    if (!h || !p || !n_exact) return gams_fail(h, GAMS_EINVAL, "wave_exact_count: null argument");
    GAMS_HIP(h, hipSetDevice(h->device));
    gams_wave_plan::Way &w = wave_read_way(p);
    GAMS_HIP(h, hipStreamSynchronize(wave_stream(h, p, wave_read_way_index(p))));
    std::vector<unsigned long long> cnt(kSlotWords);
    GAMS_HIP(h, hipMemcpy(cnt.data(), w.d_counters + kSlotWords * w.last_ring,
                          kSlotWords * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    uint64_t tot = 0;
    for (uint32_t sh = 0; sh < kShards; ++sh) tot += cnt[sh * kShardWords + 1];
    *n_exact = tot;
    return GAMS_OK;
}

int gams_gpu_wave(gams_gpu_t *h, const uint8_t *seq, uint32_t len, const gams_wave_params_t *params,
                  uint32_t *gc_count, int8_t *signal, uint32_t *n_windows) {
    if (!h || !seq || !params) return gams_fail(h, GAMS_EINVAL, "gpu_wave: null argument");
    gams_seqset_t *s = nullptr;
    int rc = gams_seqset_create(h, 1, &len, &s);
    if (rc != GAMS_OK) return rc;
    rc = gams_seqset_upload(h, s, 0, seq);
    gams_wave_plan_t *p = nullptr;
    if (rc == GAMS_OK) rc = gams_wave_plan_create(h, s, params, GAMS_WAVE_DENSE, &p);
    if (rc == GAMS_OK) rc = gams_wave_run(h, p);
    if (rc == GAMS_OK) rc = gams_wave_dense(h, p, 0, gc_count, signal);
    if (rc == GAMS_OK && n_windows) *n_windows = gams_wave_ctg_windows(p, 0);
    if (p) gams_wave_plan_destroy(h, p);
    gams_seqset_destroy(h, s);
    return rc;
}

}  // extern "C"
