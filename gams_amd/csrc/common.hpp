// common.hpp -- shared host/device plumbing of libgams_gpu (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/gams_gpu.h"
#include "../../include/gams_gpu_diag.h"
#include "layout.hpp"

struct gams_gpu {
    int device = 0;
    hipStream_t compute = nullptr;  // every kernel of the library runs here
    hipStream_t copy = nullptr;     // H2D staging of seq: bytes
    hipEvent_t copy2_ev = nullptr;  // gams_seqset_upload_all: joins the second DMA queue (the readback stream) into `copy`
    hipStream_t readback = nullptr; // packing + D2H of a finished run's results (waits on that run only)
    // a wave plan of depth D rotates its runs over `compute` and aux[0..D-2] (gams_wave_plan_set_depth)
    static constexpr int kMaxWays = 4;
    hipStream_t aux[kMaxWays - 1] = {};
    hipEvent_t aux_ev[kMaxWays - 1] = {};
    hipEvent_t rd_ev[kMaxWays] = {};   // uploads queue behind every stream that may still read a seqset
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    hipEvent_t k0 = nullptr, k1 = nullptr;  // around the kernel of the last query-style call
    bool k_valid = false;
    // chunked query calls (gams_gpu_count / locate / cover): per-slot ordering events and one timed pair
    // per chunk; gams_gpu_last_kernel_ms sums the pairs of the last call when kq_used > 0
    hipEvent_t q_ev[2][3] = {};
    std::vector<std::pair<hipEvent_t, hipEvent_t>> kq;
    int kq_used = 0;
    bool kq_staged = false;   // the pairs are the stages of a range loader call (text.hip), not the chunks of a query call
    // pinned staging ring of the copy stream: the CPU fills slot k+1 while the DMA drains slot k
    static constexpr int kStageSlots = 4;
    static constexpr size_t kStageBytes = 16u << 20;
    // (a slot is kStageBytes of bases followed by kStagePlane bytes of their G/C plane)
    static constexpr size_t kStagePlane = kStageBytes / 8;
    uint8_t *stage[kStageSlots] = {};
    hipEvent_t stage_free[kStageSlots] = {};
    int stage_next = 0;
    unsigned long long *pin_scratch = nullptr;   // 4 KiB of pinned host memory for few-word readbacks
    int cus = 0;
    uint64_t hbm = 0;
    char arch[64] = {0};
    std::string err;
    std::mutex err_mu;
    // Freed HBM / pinned-host blocks kept for the next batch: hipMalloc of a few hundred MB and
    // hipHostMalloc of the peak buffer cost milliseconds each (13 ms + 5 ms per 384-Mb batch).
    struct Block {
        void *p;
        size_t bytes;
    };
    std::vector<Block> dev_pool, pin_pool;
    std::vector<Block> host_blocks;   // page-locked blocks handed out by gams_gpu_host_alloc (their pooled sizes)
    // gams_gpu_sw_text: the last call's text and words (total, flag, per-ctg offsets), page-locked, valid until the next call
    char *sw_text = nullptr;
    size_t sw_text_bytes = 0;
    unsigned long long *sw_words = nullptr;
    size_t sw_words_bytes = 0;
    // gams_gpu_locate_text / count_text / anno_text: the cached device copy of the input and each entry's last text
    struct gams_text_state *text = nullptr;
    // gams_gpu_seq_gz: its block size and the page-locked bytes of its last call (seq_gz.hip)
    struct gams_seq_gz_state *seq_gz = nullptr;
    // hipFuncAttributeMaxDynamicSharedMemorySize belongs to the kernel FUNCTION (per device), not to a plan:
    // the largest value any launch on this handle has asked for, per function; only ever raised (gams_lds_attr)
    // counts the launches that read a seqset (any stream of the handle): gams_seqset_upload_image queues the
    // copy stream behind the handle's streams only when a reader was launched since it last did so
    std::atomic<uint64_t> reader_epoch{1};
    std::unordered_map<const void *, size_t> lds_attr;
    std::mutex lds_mu;
    int dg_table = GAMS_DG_TABLE_LDS;   // where the ΔG kernel keeps its dimer terms (gams_gpu_dg_set_table)
};

// Make sure launches of `func` on the handle's device may use `bytes` of dynamic LDS.  Plans with different
// tile sizes / lags share one kernel function; lowering the attribute behind another plan's back would fail
// that plan's next launch, so the recorded maximum only grows.
inline hipError_t gams_lds_attr(gams_gpu_t *h, const void *func, size_t bytes) {
    std::lock_guard<std::mutex> lk(h->lds_mu);
    size_t &have = h->lds_attr[func];
    if (bytes <= have) return hipSuccess;
    const hipError_t e = hipFuncSetAttribute(func, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e == hipSuccess) have = bytes;
    return e;
}

// Pooled allocation on the handle's device (pinned = page-locked host memory).  *cap is the size
// of the block handed out (>= bytes); pass it back to gams_pool_free.
hipError_t gams_pool_alloc(gams_gpu_t *h, bool pinned, size_t bytes, void **out, size_t *cap);
void gams_pool_free(gams_gpu_t *h, bool pinned, void *p, size_t cap);
// text.hip: return the text entries' buffers to the pools (gams_gpu_destroy)
void gams_text_free(gams_gpu_t *h);
// text.hip, for runlist.hip: the text entries' cached device copy of an input, grown to hold `bytes`
hipError_t gams_text_input(gams_gpu_t *h, size_t bytes, uint8_t **d_in);
// text.hip, for seq_gz.hip: a name table's device bytes -- name i is bytes[off[i] .. off[i + 1]) -- and its size
void gams_names_view(const gams_names_t *nm, const unsigned long long **off, const char **bytes, uint32_t *n);
// seq_gz.hip: return the entry's buffer to the pool (gams_gpu_destroy)
void gams_seq_gz_free(gams_gpu_t *h);

inline int gams_fail(gams_gpu_t *h, int code, const std::string &msg) {
    (void)hipGetLastError();   // a failed HIP call is reported through the code; it must not stay sticky
    if (h) {
        std::lock_guard<std::mutex> lk(h->err_mu);   // gams_wave_run_n queues from two host threads
        h->err = msg;
    }
    return code;
}

#define GAMS_HIP(h, call)                                                           \
    do {                                                                            \
        hipError_t e_ = (call);                                                     \
        if (e_ != hipSuccess) {                                                     \
            (void)hipGetLastError(); /* reported here; not left sticky */           \
            return gams_fail((h), GAMS_EHIP,                                        \
                             std::string(#call) + ": " + hipGetErrorString(e_));    \
        }                                                                           \
    } while (0)

// The check of a call whose scratch is owned by PoolBlocks (below): report and return, the destructors give back.
// `who` names the entry (a std::string).  An out-of-memory failure is GAMS_ENOMEM, every other one GAMS_EHIP.
#define GAMS_TRY(h, who, call)                                                                   \
    do {                                                                                         \
        hipError_t e_ = (call);                                                                  \
        if (e_ != hipSuccess)                                                                    \
            return gams_fail((h), e_ == hipErrorOutOfMemory ? GAMS_ENOMEM : GAMS_EHIP,           \
                             (who) + ": " + #call + ": " + hipGetErrorString(e_));               \
    } while (0)

// The stopwatch of the staged calls: gams_gpu::kq holds one timed pair of events per stage (per chunk of a query call).
// gams_stopwatch_reserve grows it to n pairs; a StageClock records the event that opens or closes stage k on its stream.
inline hipError_t gams_stopwatch_reserve(gams_gpu_t *h, size_t n) {
    while (h->kq.size() < n) {
        hipEvent_t a = nullptr, b = nullptr;
        hipError_t e = hipEventCreate(&a);
        if (e == hipSuccess) e = hipEventCreate(&b);
        if (e != hipSuccess) return e;
        h->kq.emplace_back(a, b);
    }
    return hipSuccess;
}
struct StageClock {
    gams_gpu_t *h;
    hipStream_t st;
    hipError_t operator()(int k, bool open) const {
        return hipEventRecord(open ? h->kq[(size_t)k].first : h->kq[(size_t)k].second, st);
    }
};

// One pooled block for the length of a call (or of a build).  A block goes back to the pool only after every stream
// that had work queued on it has drained: the streams named at construction (h->compute unless others are given).
struct PoolBlock {
    gams_gpu_t *h;
    bool pinned;
    hipStream_t drain[3];
    uint8_t *p = nullptr;
    size_t cap = 0;
    PoolBlock(gams_gpu_t *h_, bool pinned_, hipStream_t a = nullptr, hipStream_t b = nullptr, hipStream_t c = nullptr)
        : h(h_), pinned(pinned_), drain{a ? a : h_->compute, b, c} {}
    PoolBlock(const PoolBlock &) = delete;
    PoolBlock &operator=(const PoolBlock &) = delete;
    ~PoolBlock() { reset(); }
    hipError_t alloc(size_t bytes) {
        reset();
        return gams_pool_alloc(h, pinned, bytes, reinterpret_cast<void **>(&p), &cap);
    }
    void reset() {   // back to the pool now
        if (!p) return;
        for (hipStream_t st : drain)
            if (st) (void)hipStreamSynchronize(st);
        gams_pool_free(h, pinned, p, cap);
        p = nullptr;
        cap = 0;
    }
    uint8_t *release(size_t *cap_out) {   // to an owner that outlives the call
        uint8_t *const q = p;
        *cap_out = cap;
        p = nullptr;
        return q;
    }
};

// A buffer the handle keeps between calls and only ever grows: nothing to do if it holds `need` bytes; otherwise the old
// block goes back and one of `want` bytes takes its place (contents are not kept; p = nullptr, cap = 0 on failure).
template <typename T>
hipError_t gams_pool_grow(gams_gpu_t *h, bool pinned, T **p, size_t *cap, size_t need, size_t want) {
    if (*cap >= need) return hipSuccess;
    gams_pool_free(h, pinned, *p, *cap);
    *p = nullptr;
    *cap = 0;
    return gams_pool_alloc(h, pinned, want, reinterpret_cast<void **>(p), cap);
}

// One pooled block that its owner (a wave plan, its ways, its rows) keeps between calls.  Nothing here waits for a
// stream: the owner drains whatever may still use the block before it grows or frees it.  Reads as its pointer.
template <typename T>
struct Kept {
    T *p = nullptr;
    size_t cap = 0;   // bytes
    bool pinned;
    explicit Kept(bool pinned_ = false) : pinned(pinned_) {}
    operator T *() const { return p; }
    // gams_pool_grow: nothing to do if the block holds `need` bytes, else one of `want` bytes takes its place
    hipError_t grow(gams_gpu_t *h, size_t need, size_t want) { return gams_pool_grow(h, pinned, &p, &cap, need, want); }
    // ... without headroom: on an empty or freed block, the request for `bytes`
    hipError_t reserve(gams_gpu_t *h, size_t bytes) { return grow(h, bytes, bytes); }
    void free(gams_gpu_t *h) {
        gams_pool_free(h, pinned, p, cap);
        p = nullptr;
        cap = 0;
    }
};
// an owner's release(h): its blocks back to the pools, in the order given
template <typename... K>
void gams_free_all(gams_gpu_t *h, K &...blocks) {
    (blocks.free(h), ...);
}

struct gams_gcindex;  // sw.hip: prefix index over the seqset buffer

struct gams_seqset {
    uint32_t n_ctg = 0;
    std::vector<uint32_t> len;      // bases per ctg
    std::vector<uint64_t> off;      // byte offset of ctg i inside d_seq (256-B aligned)
    uint64_t bytes = 0;             // bytes in use (with tail slack for 16-B over-reads)
    size_t cap = 0;                 // size of the pooled block behind d_seq
    uint8_t *d_seq = nullptr;
    // the 1-bit G/C plane of d_seq: byte o of d_seq is bit o & 7 of d_plane[o >> 3] (ctgs stay on their 256-B
    // boundaries = 32 plane bytes, gap bits zero, an eighth of the byte slack behind).  plane_ok: it describes the
    // bytes (every upload so far brought both); have_bytes: d_seq holds the sequence (false: plane-only seqset).
    // Host state, read when a pass is queued: the streams order the copies themselves (`uploaded`).
    uint8_t *d_plane = nullptr;
    size_t plane_cap = 0;
    bool plane_ok = false, have_bytes = true;
    hipEvent_t uploaded = nullptr;    // recorded on the copy stream after the last upload; kernels wait on it
    bool dirty = false;               // an upload happened since the last wait was queued (compute stream)
    uint64_t upload_gen = 0;          // counts uploads; streams other than `compute` compare it with what they saw
    uint64_t ordered_epoch = 0;       // gams_gpu::reader_epoch when an upload last queued itself behind the readers
    gams_gcindex *gcindex = nullptr;  // built lazily by gams_gpu_sw, dropped by every upload
};

// The seqset protocol (api.hip).  d_seq / d_plane are written on one stream and read on others, and only events order them.
//   A writer (an upload, the device inflate, the place stage of gen) brackets what it queues on its stream `st`:
//   gams_seqset_write_begin drops the G/C index of the old bytes (after draining `compute`, which may still use it), makes
//   sure `uploaded` exists and queues `st` behind everything queued so far on the streams that run readers (`compute` and
//   the auxiliary ones); gams_seqset_write_end records `uploaded` on `st`, sets `dirty` and counts the upload in
//   `upload_gen`.  Nothing else writes the two buffers or these fields (gams_seqset_create, whose buffers nobody has seen
//   yet, keeps lines of its own).
//   A reader on the compute stream calls gams_seqset_read_begin before it queues a kernel that reads either buffer: it
//   bumps gams_gpu::reader_epoch and, if the seqset is `dirty`, makes `compute` wait for `uploaded`.  (The ways of a wave
//   plan run on streams of their own and compare `upload_gen`: wave.hip, which bumps the epoch itself and calls
//   gams_seqset_wait_uploads, the wait alone, on its compute branch.)
//   The epoch is what lets a burst of gams_seqset_upload_ranges calls pay the ordering once (once_per_epoch): a writer that
//   ordered itself at epoch e is still behind every reader while the epoch is e.  That holds only if EVERY reader bumps it,
//   which is why readers go through the one gate and do not type the two steps out.
int gams_seqset_write_begin(gams_gpu_t *h, gams_seqset_t *s, hipStream_t st, bool once_per_epoch = false);
int gams_seqset_write_end(gams_gpu_t *h, gams_seqset_t *s, hipStream_t st);
int gams_seqset_read_begin(gams_gpu_t *h, gams_seqset_t *s);
int gams_seqset_wait_uploads(gams_gpu_t *h, gams_seqset_t *s);   // the wait of read_begin without the bump: wave.hip only
int gams_stage_ring(gams_gpu_t *h);   // allocate the pinned staging slots on first use
int gams_seqset_gcindex(gams_gpu_t *h, gams_seqset_t *s);
void gams_seqset_gcindex_free(gams_seqset_t *s);
// sw.hip, for text.hip: gc[q] = round4(gc_content) of chromosome range [rs[q], re[q]] inside the ctg rctg[q] names,
// one lane per range on `st`, over device columns: ctg c begins at byte seq_off[c] of the seqset's buffer, has len[c]
// bases (0: no sequence, gc = 0) and starts at chr_start[c].  The seqset's gc index must exist (gams_seqset_gcindex).
// A range that leaves its ctg is clamped into it (never read outside); the caller checks.
void gams_launch_range_gc_cols(const gams_seqset_t *s, const unsigned long long *seq_off, const uint32_t *len,
                               const int32_t *chr_start, const uint32_t *rctg, const uint32_t *rs, const uint32_t *re,
                               uint32_t n, float *gc, hipStream_t st);

// dg.hip: the nearest-neighbour ΔG.  The table of a call: not NULL, every entry finite (GAMS_EINVAL under
// the entry `who` names); the seqset's bytes: present (GAMS_ESTATE) and the compute stream behind their uploads; and the
// kernel on the compute stream over device columns: dg[q] of the len[q] <= 65535 bases at byte off[q] of the seqset's
// buffer, NaN for None, with the table in device memory.
int gams_dg_table_check(gams_gpu_t *h, const std::string &who, const gams_dg_table_t *t);
int gams_dg_seq_ready(gams_gpu_t *h, gams_seqset_t *s);
void gams_launch_dg(gams_gpu_t *h, const gams_seqset_t *s, const unsigned long long *d_off, const uint32_t *d_len, uint32_t n,
                    const gams_dg_table_t *d_table, float *d_dg);
// sw.hip, for range_batch.hpp as well: the selected ctgs of a batch call against the seqset, `off` (named off_name in the
// messages) from 0 and not decreasing, under the entry `who` names
int gams_sw_check_selection(gams_gpu_t *h, const std::string &who, const char *off_name, const gams_seqset_t *s, uint32_t n_sel,
                            const uint32_t *ctg_index, const uint64_t *off);

// The accumulator of the sw summaries (sw.hip): n_tags x (max + 1) groups of GAMS_SW_SUMMARY_WORDS 64-bit
// integers in device memory, and the table of one call ((max + 1) groups, then a flag word) that the summarising
// sw_kernel adds into and that is merged into a tag's groups only when the call met no value it does not cover.
struct gams_sw_summary {
    int32_t size = 0, max = 0, resize = 0;
    uint32_t actions = 0, n_tags = 0;
    unsigned long long *d_acc = nullptr, *d_call = nullptr;
    // with span sets (gams_sw_summary_create_anno): the Prop sums, n_tags x (max + 1) x n_anno words beside d_acc, and
    // (max + 1) x n_anno more words of the call's table behind its flag word
    uint32_t n_anno = 0;
    unsigned long long *d_prop = nullptr;
};

// What every sw call shares, whichever entry it came through and wherever its columns live: filled once, at the extern "C"
// entry, and carried from there (SwReq in sw.hip, SwFeatJob in text.hip, SwColsJob below hold one each).
struct SwCall {
    int32_t size = 0, max = 0, resize = 0;
    uint32_t actions = 0;
    const gams_index_t *rg_ix = nullptr;        // GAMS_SW_COUNT: the rg index and (host) the group of every selected ctg / interval
    const uint32_t *rg_group = nullptr;
    gams_sw_summary_t *summary = nullptr;       // the summary entries: the rows go into tag slot `tag` of it and are never stored
    uint32_t tag = 0;
    // the _anno entries: the span sets of the Prop columns and, per set, a host column of groups (set_group[a][k] = the group
    // of ctg / interval k's chromosome in set a, UINT32_MAX: absent); n_anno 0: none
    uint32_t n_anno = 0;
    gams_spans_t *const *sets = nullptr;
    const uint32_t *const *set_group = nullptr;

    SwCall() = default;
    // (the rg index and groups are kept only where the call counts)
    SwCall(int32_t size_, int32_t max_, int32_t resize_, uint32_t actions_, const gams_index_t *ix = nullptr, const uint32_t *group = nullptr)
        : size(size_), max(max_), resize(resize_), actions(actions_), rg_ix(count() ? ix : nullptr), rg_group(count() ? group : nullptr) {}
    bool gc() const { return (actions & GAMS_SW_GC) != 0; }
    bool count() const { return (actions & GAMS_SW_COUNT) != 0; }
    uint32_t variant() const { return (gc() ? 2u : 0u) | (count() ? 1u : 0u); }   // the kernel tables' index
    bool known_actions() const { return (actions & ~(GAMS_SW_GC | GAMS_SW_COUNT)) == 0; }
    // size or resize 1: half_resize = 0 makes center_resize slice [mid+1, mid-1] (window.rs:113-123), an empty span whose
    // min()/max() the reference then asks for -- no defined answer to mirror
    bool window_ok() const { return size >= 2 && max >= 0 && resize >= 2; }
    // one thread per (feature, slot): more than 2^24 windows a side cannot exist in a ctg of < 2^31 bases and would overflow
    bool max_ok() const { return max <= (1 << 24); }
};
// The one check of a call's shared parameters, for the entry `who` names.  The entries differ in what of their own they
// test in between, so each names the `parts` to test at that point; inside a call they are tested in the enumerators' order:
// the action bits, GC without a seqset (have_seq: what the entry found; entries without that rule pass true), COUNT without
// an rg index or (n_ctgs != 0) rg groups, the three lower bounds -- GAMS_EINVAL --, max beyond 2^24 (GAMS_EUNSUPPORTED),
// the call against the accumulator's binding, tags and number of span sets, none of them NULL nor (n_ctgs != 0) a set_group
// column (GAMS_EINVAL), and the slots of `nf` features against one launch (GAMS_EUNSUPPORTED).
enum : uint32_t { SWC_ACTIONS = 1u, SWC_WINDOW = 2u, SWC_MAX = 4u, SWC_SUMMARY = 8u, SWC_SLOTS = 16u };
int gams_sw_call_check(gams_gpu_t *h, const std::string &who, const SwCall &c, uint32_t parts, uint64_t n_ctgs,
                       bool have_seq = true, uint64_t nf = 0);

// sw.hip, for text.hip (gams_gpu_sw_feature_text): stages 2-5 of that entry over device columns -- the rows of every
// feature (sw_geometry), their 64-bit prefix and the first row of every interval, one read-back of the total and the
// flags, sw_kernel, and the text with the ids composed on the device.  Interval i of the ctg index owns features
// [bucket_off[i], bucket_off[i + 1]) of fs / fe / fctg (device, nf entries; fctg[f] = i), in file order.
// With call.summary the stages stop before the text; the name tables and the text outputs of the launcher are unused (NULL).
struct SwColsJob {
    SwCall call;                                // (rg_group, set_group: per interval)
    gams_seqset_t *s;                           // NULL without GAMS_SW_GC; its gc index exists (gams_seqset_gcindex)
    uint32_t n_ctg, nf;
    const int32_t *fs, *fe;                     // device
    const uint32_t *fctg;                       // device
    const unsigned long long *d_bucket_off;     // device, n_ctg + 1
    const unsigned long long *bucket_off;       // host, n_ctg + 1
    const uint32_t *ctg_index;                  // host, per interval: the seqset slot (UINT32_MAX: none)
    const int32_t *chr_start, *chr_end;         // host, per interval
    const uint32_t *igrp;                       // device, per interval: its group of the ctg index = its chromosome name
    const unsigned long long *chr_off, *id_off; // device: the name tables' offsets (chr_names by group, ctg_ids by interval)
    const char *chr_bytes, *id_bytes;
    uint32_t max_chr, max_id;                   // the longest name of each table, in bytes
    // device, 3 words: [0] receives the rows; [1] != 0: a kept feature has its middle outside its ctg, [2] = the
    // smallest such line number (both written by the caller's gather, queued in front)
    unsigned long long *words;
};

// the timed pairs of the handle (gams_gpu::kq) these stages record: behind the range loader's lines .. order (0 .. 6)
enum : int { SWF_GATHER = 7, SWF_GEOM, SWF_ROWS, SWF_TLEN, SWF_TWRITE, SWF_STAGES };
// *text (the handle's page-locked sw text, valid until the next sw call), text_off[n_ctg + 1], *n_rows.  GAMS_EINVAL for
// the flag in words[1] (the message names the line), GAMS_EUNSUPPORTED for what the formatter does not cover.  With
// J.call.summary the stages end behind SWF_ROWS and only *n_rows is written.
int gams_launch_sw_cols(gams_gpu_t *h, const SwColsJob &J, const char **text, uint64_t *text_bytes, uint64_t *text_off,
                        uint64_t *n_rows);

// 16 bytes of sequence that this kernel will not read again: non-temporal load (global_load ... nt).
// A pure streaming read runs at 7.06 TB/s with the hint, 6.3 TB/s without (profiles/r02_stream_read.txt).
__device__ __forceinline__ uint4 load_once16(const uint4 *p) {
    typedef unsigned v4u_ __attribute__((ext_vector_type(4)));
    const v4u_ t = __builtin_nontemporal_load(reinterpret_cast<const v4u_ *>(p));
    return make_uint4(t.x, t.y, t.z, t.w);
}

// ---------------------------------------------------------------------------
// wave64 / workgroup scan primitives (device)
// ---------------------------------------------------------------------------
// Inclusive add-scan across the 64 lanes of a wavefront with DPP row shifts and
// the GFX9 row broadcasts: 6 VALU adds, no LDS traffic.
__device__ __forceinline__ uint32_t wave_incl_scan_u32(uint32_t x) {
    int v = (int)x;
    v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, false);  // row_shr:1
    v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, false);  // row_shr:2
    v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, false);  // row_shr:4
    v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, false);  // row_shr:8
    v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false);  // row_bcast:15 -> rows 1,3
    v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, false);  // row_bcast:31 -> rows 2,3
    return (uint32_t)v;
}

// 64-bit variant (only the wide z-score path needs it): shuffle based.
__device__ __forceinline__ uint64_t wave_incl_scan_u64(uint64_t x) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        uint32_t lo = __shfl_up((uint32_t)x, d, 64);
        uint32_t hi = __shfl_up((uint32_t)(x >> 32), d, 64);
        uint64_t y = ((uint64_t)hi << 32) | lo;
        if (lane >= d) x += y;
    }
    return x;
}

__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t x) { return wave_incl_scan_u32(x); }
__device__ __forceinline__ uint64_t wave_incl_scan(uint64_t x) { return wave_incl_scan_u64(x); }

// Exclusive scan over a 256-thread workgroup (4 waves).  `ws` is LDS scratch of
// 4 elements; the call contains two barriers and may be used back to back.
template <typename T, int NTH = 256>
__device__ __forceinline__ T block_excl_scan_256(T v, T *ws, T &total) {
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    T inc = wave_incl_scan(v);
    if (lane == 63) ws[wv] = inc;
    __syncthreads();
    // (NTH = 64 / 128: workgroups of one or two waves, the missing waves count as empty)
    T w0 = ws[0], w1 = NTH > 64 ? ws[1] : (T)0, w2 = NTH > 128 ? ws[2] : (T)0, w3 = NTH > 128 ? ws[3] : (T)0;
    __syncthreads();
    T base = (wv > 0 ? w0 : (T)0) + (wv > 1 ? w1 : (T)0) + (wv > 2 ? w2 : (T)0);
    total = w0 + w1 + w2 + w3;
    return base + inc - v;
}

