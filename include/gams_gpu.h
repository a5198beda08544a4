/*
 * gams_gpu.h -- C ABI of the MI355X (gfx950) engine behind the `gams` hot path.
 *
 * This is the drop-in boundary: what a Rust host would bind with `extern "C"`
 * in place of the CPU loops inside the reference's per-ctg workers.  No torch
 * types, no C++ types: plain pointers and sizes.  All pointers are caller-owned
 * HOST memory unless a function says "device-resident"; the library owns every
 * byte of device memory, per handle.  A handle is not thread-safe; use one
 * handle per host worker thread (the reference runs one ctg per worker,
 * src/cmd_gams/wave.rs:288-299).  Every entry returns 0 on success or a
 * GAMS_E* code; gams_gpu_last_error() gives the message (the reference
 * panics instead: src/gams.rs:57, src/libs/stat.rs:30).
 *
 * Reference interfaces replaced (paths under wang-q/gams @ 2024-10-22):
 *   gams_gpu_wave*            src/cmd_gams/wave.rs:138-155  (sliding + gc_content + thresholding_algo)
 *                             = src/libs/window.rs:78-94, bio gc_content, src/libs/stat.rs:16-56
 *   gams_gpu_sw(_batch, _text) src/cmd_gams/sw.rs:141-184   (center_sw + cache_gc_content + cache_gc_stat; _text: + the rows' text, :152-190)
 *   gams_gpu_sw_text_actions, gams_gpu_sw_count_batch: + rg_count (sw.rs:28-32 `--action count`, fixed as count_rg)
 *                             = src/libs/window.rs:3-56,96-124, src/libs/utils.rs:141-213
 *   gams_dg_*, gams_gpu_range_dg_batch, gams_gpu_sw_dg_batch, gams_gpu_sw_text_dg: src/libs/delta_g.rs (DeltaG::polymer; as a
 *                             column of sw it is this project's own: `--action gibbs` is declared upstream and never filled)
 *   gams_gpu_count            src/libs/utils.rs:24-36       (count_rg -> Lapper::count)
 *   gams_gpu_locate           src/libs/utils.rs:7-22        (find_one_idx -> Lapper::find().next())
 *   gams_gpu_cover            src/cmd_gams/anno.rs:128-139  (IntSpan intersect cardinalities)
 *   gams_gpu_valid_spans      src/cmd_gams/gen.rs:86-104    (ambiguous-base scan, fill, excise)
 *   gams_gpu_gen_text         src/cmd_gams/gen.rs:67-157    (one FASTA file: records, the scan, fill, excise, --piece, the ctgs' bases)
 *   gams_gpu_locate_text      src/cmd_gams/locate.rs:84-141 (locate -f: lines, Range::from_str, find_one_idx, rows)
 *   gams_gpu_count_text       src/cmd_gams/locate.rs:84-141 (locate --count: the same with count_rg, utils.rs:24-36)
 *   gams_gpu_anno_text        src/cmd_gams/anno.rs:95-142   (one input file: fields, extract_ctg_id, cover, rows)
 *   gams_gpu_peak_text        src/libs/utils.rs:83-116 read_peak + src/cmd_gams/peak.rs:41-160 (one wave TSV: fields,
 *                             find_one_idx, drop-first, sort by start, cache_gc_content, neighbours, the Peak rows)
 *   gams_index_create_range_files, gams_gpu_loader_text: src/cmd_gams/rg.rs:40-82, feature.rs:47-96 (several files:
 *                             read_range per file, the serials behind cnt:, the records' JSON / TSV / SET commands)
 *
 * Measurement and tuning entries (event stopwatch, phase stamps, guard-band and tile knobs, kernel
 * names) are NOT part of this surface: they live in gams_gpu_diag.h, which a host need not bind.
 *
 * Environment: the library neither reads nor writes the process environment.  Kernel arguments in
 * device memory (HIP_FORCE_DEV_KERNARG=1, set by the host BEFORE its first HIP call) shorten every
 * launch by the PCIe round trip of the argument fetch (12-Mb pass 9.5 -> 7.8 us); see INTEGRATION.md.
 */
#ifndef GAMS_GPU_H
#define GAMS_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GAMS_OK 0
#define GAMS_EINVAL 1       /* bad argument */
#define GAMS_ENODEV 2       /* no usable HIP device */
#define GAMS_ENOMEM 3       /* host or device allocation failed */
#define GAMS_EHIP 4         /* a HIP call failed (message has the HIP error) */
#define GAMS_ESHORT 5       /* a ctg has fewer windows than lag: the reference panics (stat.rs:30) */
#define GAMS_EUNSUPPORTED 6 /* outside what the kernels implement (sizes / lags beyond 65535, counts beyond 2^31) */
#define GAMS_ESTATE 7       /* call order violated (e.g. results read before run) */

typedef struct gams_gpu gams_gpu_t;
typedef struct gams_seqset gams_seqset_t;
typedef struct gams_wave_plan gams_wave_plan_t;
typedef struct gams_index gams_index_t;
typedef struct gams_spans gams_spans_t;
typedef struct gams_names gams_names_t;
typedef struct gams_gen gams_gen_t;
typedef struct gams_sw_summary gams_sw_summary_t;

/* ---- handle ------------------------------------------------------------ */
int gams_gpu_create(int device, gams_gpu_t **h);
void gams_gpu_destroy(gams_gpu_t *h);
const char *gams_gpu_last_error(gams_gpu_t *h);
/* name (e.g. "gfx950"), CU count, HBM bytes of the device behind the handle */
int gams_gpu_device_info(gams_gpu_t *h, char *arch, size_t arch_len,
                         int32_t *compute_units, uint64_t *hbm_bytes);
/* block until everything queued on the handle's streams has finished */
int gams_gpu_sync(gams_gpu_t *h);
/* Freed HBM and pinned-host blocks stay cached on the handle for the next batch (at most 16
 * blocks, a quarter of the HBM, 1 GiB pinned); this returns them to the driver now.
 * cached_bytes (may be NULL) receives what was held. */
int gams_gpu_release_cached(gams_gpu_t *h, uint64_t *cached_bytes);
/* Page-locked host memory for query / result columns: gams_gpu_count, gams_gpu_locate and gams_gpu_cover
 * move their columns in chunks (copy in, search, copy out on three streams); from page-locked arrays the
 * three overlap and a call runs at the rate of the PCIe link.  Any host memory works. */
int gams_gpu_host_alloc(gams_gpu_t *h, uint64_t bytes, void **p);
/* Blocks come from (and go back to) the handle's pool of page-locked memory, so asking for the same columns batch
 * after batch does not pin them again.  Free with the handle that allocated, while it is alive (h == NULL: the
 * block is released to the system; that is also the way to free one after its handle is gone). */
void gams_gpu_host_free(gams_gpu_t *h, void *p);

/* window.rs:78-94: number of size/step windows over `len` bases (-1: bad size/step) */
int64_t gams_window_count(int64_t len, int32_t size, int32_t step);

/* ---- ctg sequences resident in HBM ------------------------------------- */
/* A seqset is the device image of a batch of `seq:{ctg}` values (gunzipped
 * bases, 1 B/base, redis.rs:142-146): one contiguous HBM buffer, every ctg
 * starting on a 256-B boundary.  lengths[i] = bases of ctg i. */
int gams_seqset_create(gams_gpu_t *h, uint32_t n_ctg, const uint32_t *lengths,
                       gams_seqset_t **s);
/* copy ctg `i` (lengths[i] bytes) host -> HBM on the handle's copy stream */
int gams_seqset_upload(gams_gpu_t *h, gams_seqset_t *s, uint32_t i,
                       const uint8_t *seq);
/* copy every ctg of the set (seqs[i] -> lengths[i] bytes; NULL allowed where lengths[i] == 0):
 * the batch form of the per-ctg GET loop (wave.rs:134-136).  Several host threads fill pinned
 * staging buffers in the device layout, one DMA per 16 MiB; returns once everything is queued. */
int gams_seqset_upload_all(gams_gpu_t *h, gams_seqset_t *s, const uint8_t *const *seqs);
/* Where the library put the ctgs: offsets[i] (n_ctg entries, may be NULL) = byte offset of ctg i in the
 * device buffer, *bytes (may be NULL) = the buffer's size in use.  A host that produces the bases itself
 * -- gunzip of the `seq:` values, redis.rs:142-161 -- writes them at these offsets of a page-locked
 * block of *bytes bytes (gams_gpu_host_alloc) and hands ranges of that image to
 * gams_seqset_upload_image: no staging copy between the inflate and the DMA. */
int gams_seqset_layout(gams_gpu_t *h, const gams_seqset_t *s, uint64_t *offsets, uint64_t *bytes);
/* DMA bytes [lo, hi) of `image` (a host image of the device buffer, laid out as gams_seqset_layout says)
 * to the same bytes of the device buffer, on the handle's copy stream; returns once queued.  The image must
 * stay untouched until the next gams_gpu_sync / a reader of the seqset has finished.  Page-locked images
 * (gams_gpu_host_alloc) go at the rate of the link; pageable ones work but stage through the driver.
 * Bytes between ctgs (alignment gaps) are never counted: they may hold anything. */
int gams_seqset_upload_image(gams_gpu_t *h, gams_seqset_t *s, const uint8_t *image, uint64_t lo, uint64_t hi);
/* The 1-bit G/C plane of n bases: bit i & 7 of plane[i >> 3] says (seq[i] & 0xDB) == 0x43, i.e. base i is one
 * of C, G, c, g; ceil(n / 8) bytes are written, bits past n are zero.  Host code, no device involved.  Next to
 * its bytes a seqset keeps this plane (the same offsets divided by 8): gams_seqset_upload and
 * gams_seqset_upload_all produce it while they stage the bytes, and `wave` passes of the tiled fast kernels
 * stream it instead of the bytes.  An upload that brings bytes without their plane (gams_seqset_upload_image)
 * marks the plane stale, and passes read the bytes again until gams_seqset_upload_all has renewed it. */
int gams_gc_plane(const uint8_t *seq, uint64_t n, uint8_t *plane);
/* gams_seqset_upload_image for a host that also, or only, holds the plane: bytes [lo, hi) of `image` and / or
 * plane bytes [lo / 8, ceil(hi / 8)) of `plane_image` (a host image of the plane: byte o of the device buffer
 * is bit o & 7 of plane_image[o >> 3], bits of alignment gaps zero) go to the device; lo must be a multiple of
 * 8, either pointer may be NULL, not both.  image == NULL makes the seqset PLANE-ONLY: `wave` answers through
 * the tiled fast kernels, and whatever needs the bytes (gams_gpu_sw*, gams_gpu_range_gc*, wave parameters
 * outside the fast kernels) returns GAMS_ESTATE until gams_seqset_upload_all has brought them.
 * plane_image == NULL is gams_seqset_upload_image. */
int gams_seqset_upload_ranges(gams_gpu_t *h, gams_seqset_t *s, const uint8_t *image, const uint8_t *plane_image,
                              uint64_t lo, uint64_t hi);
/* Wait for the uploads queued so far and copy ctg i back: its lengths[i] bases to seq and / or the ceil(lengths[i] / 8)
 * bytes of its G/C plane to plane (either may be NULL).  What a host that fills a store needs after gams_gpu_gen_text.
 * GAMS_ESTATE for the bases of a plane-only seqset and for the plane while it is stale. */
int gams_seqset_download(gams_gpu_t *h, gams_seqset_t *s, uint32_t i, uint8_t *seq, uint8_t *plane);
void gams_seqset_destroy(gams_gpu_t *h, gams_seqset_t *s);

/* ---- wave (GC windows + smoothed z-score) ------------------------------- */
typedef struct {
    int32_t size;      /* --size      (wave.rs:125) */
    int32_t step;      /* --step      (wave.rs:126) */
    uint32_t lag;      /* --lag       (wave.rs:127) */
    float threshold;   /* --threshold (wave.rs:128) */
    float influence;   /* --influence (wave.rs:129) */
} gams_wave_params_t;

/* one signalled window, as wave.rs:170-187 collects them */
typedef struct {
    uint32_t ctg;      /* index into the seqset */
    uint32_t window;   /* k: bases [k*step, k*step+size) of the ctg */
    uint32_t gc_count; /* #{G,C,g,c}; gc_content = gc_count as f32 / size as f32 */
    int32_t signal;    /* +1 crest, -1 trough */
} gams_peak_t;

#define GAMS_WAVE_PEAKS 1u /* compacted (ctg, window, gc_count, signal) of signal != 0 */
#define GAMS_WAVE_DENSE 2u /* every window: gc_count u32 + signal i8 (--signal, wave.rs:158-168) */

/* Geometry + device buffers for running `params` over every ctg of `s`.
 * GAMS_ESHORT if any ctg has fewer than `lag` windows (the reference panics). */
int gams_wave_plan_create(gams_gpu_t *h, gams_seqset_t *s,
                          const gams_wave_params_t *params, uint32_t flags,
                          gams_wave_plan_t **p);
void gams_wave_plan_destroy(gams_gpu_t *h, gams_wave_plan_t *p);
/* total windows over all ctgs, and windows of ctg i */
uint64_t gams_wave_total_windows(const gams_wave_plan_t *p);
uint32_t gams_wave_ctg_windows(const gams_wave_plan_t *p, uint32_t i);
/* One pass: queue the kernels on the compute stream (asynchronous). */
int gams_wave_run(gams_gpu_t *h, gams_wave_plan_t *p);
/* n passes queued back to back (the loop a host would write, without its per-call overhead) */
int gams_wave_run_n(gams_gpu_t *h, gams_wave_plan_t *p, uint32_t n);
/* Passes in flight.  With depth D (1..4, default 1) consecutive gams_wave_run calls of the plan
 * rotate over D HIP streams and D sets of output buffers, so that independent passes (batch
 * after batch of ctgs, wave.rs:288-299 hands them to workers the same way) overlap on the device:
 * a 12-Mb pass alone is launch-latency bound (8.2 us; 3.3 us each at depth 4).  The readers
 * (gams_wave_peaks, gams_wave_dense, gams_wave_exact_count) return the most recent run;
 * gams_wave_plan_select(age) points them at the run `age` runs earlier (age < depth).
 * Changing the depth drops the results held so far. */
int gams_wave_plan_set_depth(gams_gpu_t *h, gams_wave_plan_t *plan, uint32_t depth);
int gams_wave_plan_select(gams_gpu_t *h, gams_wave_plan_t *plan, uint32_t age);
/* Several plans in flight on one handle (batch k+1 computing while batch k is read back): a plan's
 * runs go to HIP stream (lane + way) % 4 of the handle, lane 0 by default.  Plans on different lanes
 * overlap on the device exactly like the ways of one plan; the readers wait for their own plan only.
 * Call while the plan is idle (it waits for the plan's queued runs). */
int gams_wave_plan_set_lane(gams_gpu_t *h, gams_wave_plan_t *plan, uint32_t lane);
/* Pipelined plans record an event behind every run, and gams_wave_peaks / gams_wave_dense wait
 * for that run only (so a host can keep several plans in flight on one handle: upload of batch
 * k+1 and its kernel overlap the readback and formatting of batch k).  Off by default: the
 * event costs a marker packet between back-to-back launches. */
int gams_wave_plan_set_pipelined(gams_gpu_t *h, gams_wave_plan_t *p, int enable);
/* Wait for the last run and fetch its compacted peaks, ordered by (ctg, window).
 * *peaks points into plan-owned host memory, valid until the next run. */
int gams_wave_peaks(gams_gpu_t *h, gams_wave_plan_t *p,
                    const gams_peak_t **peaks, uint64_t *n_peaks);
/* The rows of `gams wave` as TSV text, made on the device (wave.rs:157-252: crests and troughs separately,
 * overlapping windows merged into "{chr}(+):{min}-{max}", every row "...\t{gc_content}\t{signal}\n" in window
 * order, gc_content printed like Rust's `{}` of an f32) -- what the host otherwise derives from gams_wave_peaks.
 * setup: once per plan; chr[i] / chr_start[i] = chromosome name and first chromosome coordinate of ctg i
 *   (chr_id, chr_start of its Ctg record); coverage = --coverage.  GAMS_EUNSUPPORTED when that coverage links
 *   only some of the overlapping windows (> size / (size - step): merge gams_wave_peaks on the host then).
 * begin: queue the packing of the selected run's peaks, the rows and their copy to the host behind that run;
 *   returns at once, so several plans can have their rows in flight while later passes compute.
 * end: wait for this plan's rows.  *text (text_bytes bytes, no header line, no terminating NUL) and *ctg_off
 *   (n_ctg + 1 offsets: the rows of ctg i are text[ctg_off[i] .. ctg_off[i+1])) point into plan-owned
 *   page-locked memory, valid until the plan's next gams_wave_rows_begin. */
int gams_wave_rows_setup(gams_gpu_t *h, gams_wave_plan_t *p, const char *const *chr,
                         const int32_t *chr_start, float coverage);
int gams_wave_rows_begin(gams_gpu_t *h, gams_wave_plan_t *p);
int gams_wave_rows_end(gams_gpu_t *h, gams_wave_plan_t *p, const char **text, uint64_t *text_bytes,
                       const uint64_t **ctg_off);
/* `wave --signal` (wave.rs:158-168: a row for EVERY window, "{chr}:{start}-{end}\t{gc_content}\t{signal}\n") as text made
 * on the device from the dense rows of the selected run of a plan with GAMS_WAVE_DENSE.  chr[i] / chr_start[i] as in
 * gams_wave_rows_setup.  Waits for the run; *text (text_bytes bytes, no header line, no NUL) and *ctg_off (n_ctg + 1
 * offsets: the rows of ctg i are text[ctg_off[i] .. ctg_off[i+1])) point into plan-owned page-locked memory, valid
 * until the next call on this plan.  120 Mb at step 10 are 1.2e7 rows and 310 MB of text. */
int gams_wave_signal_text(gams_gpu_t *h, gams_wave_plan_t *p, const char *const *chr, const int32_t *chr_start,
                          const char **text, uint64_t *text_bytes, const uint64_t **ctg_off);
/* Wait for the last run and copy ctg i's dense rows (either pointer may be NULL). */
int gams_wave_dense(gams_gpu_t *h, gams_wave_plan_t *p, uint32_t i,
                    uint32_t *gc_count, int8_t *signal);

/* Convenience, one ctg from host memory (what wave.rs:143-155 computes):
 * gc_count / signal receive n = gams_window_count(len,size,step) items. */
int gams_gpu_wave(gams_gpu_t *h, const uint8_t *seq, uint32_t len,
                  const gams_wave_params_t *params, uint32_t *gc_count,
                  int8_t *signal, uint32_t *n_windows);

/* ---- sw (windows around features) --------------------------------------- */
typedef struct {
    uint32_t feature;  /* index into the feature arrays */
    int32_t type;      /* 0 = M, 1 = L, 2 = R  (window.rs:13-15) */
    int32_t distance;  /* 0 for M, 1..max */
    int32_t start;     /* chromosome coordinates, 1-based inclusive */
    int32_t end;
    float gc_content;  /* round4 (utils.rs:161) */
    float gc_mean;     /* round4 (utils.rs:186) */
    float gc_stddev;
    float gc_cv;
} gams_sw_row_t;

/* Features are inclusive chromosome ranges whose middle lies inside the ctg (GAMS_EINVAL otherwise:
 * center_resize takes parent.index(mid), window.rs:98-111, undefined for a non-member); size and
 * resize >= 2.
 * rows per feature = 1 + nL + nR (window.rs:29-41); writes at most `cap` rows
 * in the reference's order (feature order, then M, L1.., R1..). ctg i of `s`
 * spans chromosome coordinates [chr_start, chr_start+len-1]. */
int gams_gpu_sw(gams_gpu_t *h, gams_seqset_t *s, uint32_t i, int32_t chr_start,
                const int32_t *feat_start, const int32_t *feat_end, uint32_t nf,
                int32_t size, int32_t max, int32_t resize, gams_sw_row_t *rows,
                uint64_t cap, uint64_t *n_rows);

/* The same over several ctgs of the seqset in ONE launch and one pair of transfers (a ctg's few hundred
 * features are a handful of workgroups: called per ctg the kernel is all launch latency).  ctg_index[k]
 * (k < n_sel) names a ctg of `s`, chr_start[k] its first chromosome coordinate; its features are
 * feat_start / feat_end [feat_off[k], feat_off[k+1]) (feat_off[0] = 0).  Rows come out in (k, feature, M,
 * L1.., R1..) order, `feature` counting from 0 inside each selected ctg; row_off (n_sel + 1 entries, may be
 * NULL) receives where the rows of selected ctg k begin.  rows == NULL or cap == 0: size query (n_rows and
 * row_off only, nothing runs on the device).  gams_gpu_sw is this call with n_sel = 1. */
int gams_gpu_sw_batch(gams_gpu_t *h, gams_seqset_t *s, uint32_t n_sel, const uint32_t *ctg_index,
                      const int32_t *chr_start, const uint64_t *feat_off, const int32_t *feat_start,
                      const int32_t *feat_end, int32_t size, int32_t max, int32_t resize,
                      gams_sw_row_t *rows, uint64_t cap, uint64_t *row_off, uint64_t *n_rows);

/* The rows of gams_gpu_sw_batch as the TSV text of `gams sw` (sw.rs:152-190 and the Display of Sw, data.rs:58-83:
 * "sw:{feature id}:{serial}\t{chr}:{start}-{end}\t{M|L|R}\t{distance}\t{gc_content}\t{gc_mean}\t{gc_stddev}\t{gc_cv}\t\n",
 * the last field -- rg_count -- empty: gams_gpu_sw_text_actions fills it), formatted on the device.  chr[k] = chromosome name of selected ctg k,
 * feat_id[f] = id of feature f ("feature:{ctg}:{serial}", feature.rs:81-83), both NUL-terminated.  *text
 * (text_bytes bytes, no header, no NUL) and *ctg_off (n_sel + 1 offsets: the rows of selected ctg k are
 * text[ctg_off[k] .. ctg_off[k+1])) point into page-locked memory owned by the handle, valid until the handle's next
 * gams_gpu_sw_text.  GAMS_EUNSUPPORTED if a statistic is 1000 or more or a coordinate negative (the formatter
 * prints the four round4 values as m / 10^4 with the trailing zeros dropped, which is what Rust's `{}` prints for them
 * below 1000): format the rows of gams_gpu_sw_batch on the host then. */
int gams_gpu_sw_text(gams_gpu_t *h, gams_seqset_t *s, uint32_t n_sel, const uint32_t *ctg_index,
                     const char *const *chr, const int32_t *chr_start, const uint64_t *feat_off,
                     const int32_t *feat_start, const int32_t *feat_end, const char *const *feat_id,
                     int32_t size, int32_t max, int32_t resize, const char **text, uint64_t *text_bytes,
                     const uint64_t **ctg_off, uint64_t *n_rows);

/* `gams sw --action` (sw.rs:28-32, :116-119): the action set of a call, a mask of these bits.  `gibbs` is accepted
 * upstream and computes nothing: it has no bit. */
#define GAMS_SW_GC 1u    /* gc_content, gc_mean, gc_stddev, gc_cv (fields 5-8) */
#define GAMS_SW_COUNT 2u /* rg_count (field 9) */

/* gams_gpu_sw_text with an action set.  Without GAMS_SW_GC fields 5-8 are empty ("\t\t\t", data.rs:60-70) and the
 * call reads no sequence byte (the seqset need not be uploaded); without GAMS_SW_COUNT field 9 is empty.  With
 * GAMS_SW_COUNT field 9 is count_rg(idx:rg:, ctg, Range::from(chr, win.min(), win.max())) (utils.rs:24-36) =
 * Lapper::count(start, end) of the window against group rg_group[k] of rg_ix for the windows of selected ctg k --
 * the range's end is exclusive there, as in `locate --count`; rg_group[k] >= the index's groups (e.g. UINT32_MAX):
 * no group, the count is 0.  GAMS_EINVAL for bits beyond the two flags and for GAMS_SW_COUNT without rg_ix (or
 * without rg_group when n_sel > 0).  Output and ownership as for gams_gpu_sw_text, which is this call with
 * GAMS_SW_GC and no index. */
int gams_gpu_sw_text_actions(gams_gpu_t *h, gams_seqset_t *s, uint32_t n_sel, const uint32_t *ctg_index,
                             const char *const *chr, const int32_t *chr_start, const uint64_t *feat_off,
                             const int32_t *feat_start, const int32_t *feat_end, const char *const *feat_id,
                             int32_t size, int32_t max, int32_t resize, uint32_t actions, gams_index_t *rg_ix,
                             const uint32_t *rg_group, const char **text, uint64_t *text_bytes,
                             const uint64_t **ctg_off, uint64_t *n_rows);
/* The rg_count of every window of gams_gpu_sw_batch (same arguments without resize, same row order, row_off and size
 * query: count == NULL or cap == 0), rg_ix / rg_group as in gams_gpu_sw_text_actions: count[r] for row r.  Reads no
 * sequence byte.  What a host formatter needs next to the rows when the text entry returns GAMS_EUNSUPPORTED. */
int gams_gpu_sw_count_batch(gams_gpu_t *h, gams_seqset_t *s, uint32_t n_sel, const uint32_t *ctg_index,
                            const int32_t *chr_start, const uint64_t *feat_off, const int32_t *feat_start,
                            const int32_t *feat_end, int32_t size, int32_t max, gams_index_t *rg_ix,
                            const uint32_t *rg_group, int32_t *count, uint64_t cap, uint64_t *row_off,
                            uint64_t *n_rows);

/* ---- sw summary: the rows reduced per distance on the device (templates/dql/fsw-distance.tera.sql) ---- */
/* What the user plots is not the rows but their table per distance: avg(gc_content), avg(gc_mean), avg(gc_stddev),
 * avg(gc_cv) and count, L and R together; fsw-distance-tag.tera.sql is the same per (tag, distance).  The accumulator
 * below holds that table as exact integers in device memory: n_tags x (max + 1) groups, group (t, d) at words
 * [(t * (max + 1) + d) * GAMS_SW_SUMMARY_WORDS ..), each
 *   [0] COUNT, the rows; [1..4] S, the sum of m over the rows for gc_content, gc_mean, gc_stddev, gc_cv, a statistic
 *   being printed as m / 10^4 (the integer the text entries print); [5..8] the rows whose statistic is NaN (left out of
 *   S); [9] C, the sum of rg_count.
 * A -0 adds 0.  Without GAMS_SW_GC words 1..8 stay 0, without GAMS_SW_COUNT word 9.  The sums are integers, so neither
 * the order of the calls nor of the additions inside one shows in them.  An accumulator is bound to size, max, resize
 * and actions: a call with other values is GAMS_EINVAL.  It belongs to the handle it was made on. */
#define GAMS_SW_SUMMARY_WORDS 10u
/* GAMS_EINVAL: n_tags == 0, size < 2, max < 0 or beyond 2^24, resize < 2, unknown action bits.  All groups start at 0. */
int gams_sw_summary_create(gams_gpu_t *h, int32_t max, uint32_t n_tags, uint32_t actions, int32_t size, int32_t resize,
                           gams_sw_summary_t **out);
int gams_sw_summary_reset(gams_gpu_t *h, gams_sw_summary_t *sum);   /* every group back to 0 */
/* The raw integers, one small read-back; n = n_tags * (max + 1) groups in (tag, distance) order: count[n], sum[4 * n]
 * and nan[4 * n] (group-major: the four statistics of a group side by side), rg_count[n].  Any of the four may be NULL. */
int gams_sw_summary_read(gams_gpu_t *h, gams_sw_summary_t *sum, uint64_t *count, uint64_t *s, uint64_t *nan,
                         uint64_t *rg_count);
void gams_sw_summary_destroy(gams_gpu_t *h, gams_sw_summary_t *sum);
/* The rows gams_gpu_sw_text_actions prints for these arguments (it takes them without the names and ids), added into tag
 * slot `tag` of `sum` and never stored: for hosts that hold their features as arrays.  *n_rows = the rows of the call.
 * Checks and return codes as for gams_gpu_sw_text_actions, and GAMS_EINVAL for tag >= n_tags and for size, max, resize
 * or actions other than the accumulator's.  GAMS_EUNSUPPORTED where that entry answers it for a statistic (a non-NaN
 * value outside [0, 1000)): the accumulator is then as it was before the call -- summarise the rows of
 * gams_gpu_sw_batch on the host. */
int gams_gpu_sw_summary_batch(gams_gpu_t *h, gams_seqset_t *s, uint32_t n_sel, const uint32_t *ctg_index,
                              const int32_t *chr_start, const uint64_t *feat_off, const int32_t *feat_start,
                              const int32_t *feat_end, int32_t size, int32_t max, int32_t resize, uint32_t actions,
                              gams_index_t *rg_ix, const uint32_t *rg_group, gams_sw_summary_t *sum, uint32_t tag,
                              uint64_t *n_rows);

/* ---- the Prop columns of fsw-distance-tag.tera.sql: AVG_{prefix}Prop per span set ----
 * The reference's rows pass `gams anno <runlist.json> stdin -H` once per set before they are loaded; to anno a row is its
 * window {chr}:{start}-{end} in its ctg, and prop = |set[chr] n window| as f32 / |window| as f32 (anno.rs:122-140; 0 when
 * the chromosome is absent from the set), printed {:.4} = q / 10^4.  An accumulator made for n_anno sets keeps, beside
 * the ten words of every group, P_a = the exact sum of q over the group's rows for set a; the layout above,
 * GAMS_SW_SUMMARY_WORDS and gams_sw_summary_read are unchanged, gams_sw_summary_reset zeroes the Prop sums too.
 * The sets are resident gams_spans_t (gams_spans_create, gams_spans_create_runlist_text), shared by any number of calls.
 * The Prop sums do not depend on the action mask: coverage reads no sequence byte. */
#define GAMS_SW_SUMMARY_MAX_ANNO 4u
/* gams_sw_summary_create for n_anno sets (0: that entry itself); GAMS_EINVAL also for n_anno > GAMS_SW_SUMMARY_MAX_ANNO */
int gams_sw_summary_create_anno(gams_gpu_t *h, int32_t max, uint32_t n_tags, uint32_t actions, int32_t size, int32_t resize,
                                uint32_t n_anno, gams_sw_summary_t **out);
/* The Prop sums: prop[(g * n_anno) + a] for group g of the n = n_tags * (max + 1) groups in (tag, distance) order and set
 * a (group-major).  Nothing is written for an accumulator without sets. */
int gams_sw_summary_read_anno(gams_gpu_t *h, gams_sw_summary_t *sum, uint64_t *prop);
/* gams_gpu_sw_summary_batch with the sets: sets[a] and set_group[a], a host column indexed as ctg_index is --
 * set_group[a][k] = the group of selected ctg k's chromosome in sets[a], UINT32_MAX (or anything >= the set's groups) for
 * an absent chromosome, which adds 0.  GAMS_EINVAL for n_anno other than the accumulator's (so the entries without sets
 * refuse an accumulator made with sets), for n_anno > GAMS_SW_SUMMARY_MAX_ANNO and for a NULL set or column; on every
 * code but GAMS_OK the accumulator, Prop sums included, is as it was before the call. */
int gams_gpu_sw_summary_batch_anno(gams_gpu_t *h, gams_seqset_t *s, uint32_t n_sel, const uint32_t *ctg_index,
                                   const int32_t *chr_start, const uint64_t *feat_off, const int32_t *feat_start,
                                   const int32_t *feat_end, int32_t size, int32_t max, int32_t resize, uint32_t actions,
                                   gams_index_t *rg_ix, const uint32_t *rg_group, gams_sw_summary_t *sum, uint32_t tag,
                                   uint32_t n_anno, gams_spans_t *const *sets, const uint32_t *const *set_group,
                                   uint64_t *n_rows);

/* gc_content (round4, utils.rs:141-162) of n chromosome ranges inside ctg i: what `gams peak`
 * asks per merged peak (peak.rs:79; second "next" row of SURVEY section 8f). */
int gams_gpu_range_gc(gams_gpu_t *h, gams_seqset_t *s, uint32_t i, int32_t chr_start,
                      const int32_t *range_start, const int32_t *range_end, uint32_t n,
                      float *gc);
/* The same for the ranges of several ctgs of the seqset in one launch (ctg_index / chr_start / range_off as in
 * gams_gpu_sw_batch): gc[q] for range q of the concatenated list. */
int gams_gpu_range_gc_batch(gams_gpu_t *h, gams_seqset_t *s, uint32_t n_sel, const uint32_t *ctg_index,
                            const int32_t *chr_start, const uint64_t *range_off, const int32_t *range_start,
                            const int32_t *range_end, float *gc);

/* ---- nearest-neighbour free energy (src/libs/delta_g.rs: DeltaG) of ranges and sw windows ----
 * The ΔG of a polymer is the sum of its dimers' terms, in sequence order and in f32, then the terminal terms of its first
 * and last base, then the symmetry term when it equals its reverse complement (delta_g.rs:78-115).  None -- fewer than 3
 * bases, or a byte that is none of ACGTacgt -- is a quiet NaN here.  The 21 terms depend on temperature and salt alone:
 * the host makes them once and every call takes them as data, so an answer is a function of (table, bytes). */
typedef struct {
    float nn[16];  /* dimer XY at 4 * c(X) + c(Y), A C G T = 0 1 2 3 */
    float init[4]; /* terminal term by base */
    float sym;     /* symmetry term */
} gams_dg_table_t;
/* init_delta_g (delta_g.rs:118-207) in f32, the reference's order.  Host code, no device involved.  GAMS_EINVAL for a
 * non-finite temp, and for a non-finite salt or salt <= 0.  DeltaG::new() is (37, 1). */
int gams_dg_table(float temp, float salt, gams_dg_table_t *table);
/* DeltaG::polymer over n bytes, *dg = NaN for None: the host twin of the device entries below, bit for bit.  Host code;
 * any length. */
int gams_dg_polymer_host(const gams_dg_table_t *table, const uint8_t *seq, uint64_t n, float *dg);
/* The ΔG of chromosome ranges inside ctgs of the seqset, in one launch: arguments, checks, codes and messages as for
 * gams_gpu_range_gc_batch; dg[q] for range q of the concatenated list.  GAMS_EINVAL also for a NULL table or a table with
 * a non-finite entry, GAMS_EUNSUPPORTED for a range of more than 65535 bases (the sum is one serial chain: this is for
 * oligos and windows), GAMS_ESTATE for a plane-only seqset. */
int gams_gpu_range_dg_batch(gams_gpu_t *h, gams_seqset_t *s, uint32_t n_sel, const uint32_t *ctg_index,
                            const int32_t *chr_start, const uint64_t *range_off, const int32_t *range_start,
                            const int32_t *range_end, const gams_dg_table_t *table, float *dg);
/* The ΔG of every window of gams_gpu_sw_batch (same arguments without resize, same row order, row_off and size query:
 * dg == NULL or cap == 0): dg[r] = the ΔG of the bases [start, end] of row r, the window its range column prints.
 * Table, length limit and plane-only seqsets as for gams_gpu_range_dg_batch. */
int gams_gpu_sw_dg_batch(gams_gpu_t *h, gams_seqset_t *s, uint32_t n_sel, const uint32_t *ctg_index,
                         const int32_t *chr_start, const uint64_t *feat_off, const int32_t *feat_start,
                         const int32_t *feat_end, int32_t size, int32_t max, const gams_dg_table_t *table, float *dg,
                         uint64_t cap, uint64_t *row_off, uint64_t *n_rows);
/* gams_gpu_sw_text_actions with the ΔG of every window as a tenth field: every row ends "...\t{rg_count}\t{dg}\n", dg the
 * f32 of gams_gpu_sw_dg_batch printed with four decimals ({:.4}: the exact value rounded half to even, "-0.0000" keeps its
 * sign) and empty for None.  Action sets, checks, output and ownership as for gams_gpu_sw_text_actions (the text lives in
 * the same buffer of the handle, valid until its next sw text call); the column always reads the sequence bytes.
 * GAMS_EUNSUPPORTED also when some |dg| reaches 2^20, which takes a caller's own table. */
int gams_gpu_sw_text_dg(gams_gpu_t *h, gams_seqset_t *s, uint32_t n_sel, const uint32_t *ctg_index,
                        const char *const *chr, const int32_t *chr_start, const uint64_t *feat_off,
                        const int32_t *feat_start, const int32_t *feat_end, const char *const *feat_id,
                        int32_t size, int32_t max, int32_t resize, uint32_t actions, gams_index_t *rg_ix,
                        const uint32_t *rg_group, const gams_dg_table_t *table, const char **text,
                        uint64_t *text_bytes, const uint64_t **ctg_off, uint64_t *n_rows);

/* ---- sorted-interval index (replaces rust_lapper `idx:`) ---------------- */
/* m intervals [start, stop) (stop = end+1, redis.rs:245-248,291-294) grouped
 * in `n_groups` groups (one per ctg for idx:rg:, one per chr for idx:ctg:);
 * group g owns intervals [group_off[g], group_off[g+1]).  Any order inside a
 * group: the library sorts. */
int gams_index_create(gams_gpu_t *h, uint32_t n_groups, const uint64_t *group_off,
                      const uint32_t *starts, const uint32_t *stops,
                      gams_index_t **ix);
void gams_index_destroy(gams_gpu_t *h, gams_index_t *ix);
/* Lapper::count(qs,qe) per query against its group (utils.rs:35).
 * group[q] >= n_groups (e.g. UINT32_MAX) -> 0 (utils.rs:29-32).
 * The count is #{start < qe} - #{stop <= qs}, the starts and the stops each
 * sorted on their own.  Of a reversed query (qe <= qs) or over reversed
 * intervals (stop < start) it is that signed difference, which can be
 * negative; the reference itself has no defined answer there. */
int gams_gpu_count(gams_gpu_t *h, gams_index_t *ix, const uint32_t *group,
                   const uint32_t *qs, const uint32_t *qe, uint64_t nq,
                   int32_t *count);
/* Lapper::find(qs,qe).next() per query (utils.rs:16): index (into the
 * caller's original interval order) of the first hit in (start,stop) order,
 * or -1.  Among equal (start, stop) pairs the one earliest in the caller's
 * order is returned: the build sorts like the stable intervals.sort() of
 * redis.rs:253,299, whatever the size of the group. */
int gams_gpu_locate(gams_gpu_t *h, gams_index_t *ix, const uint32_t *group,
                    const uint32_t *qs, const uint32_t *qe, uint64_t nq,
                    int64_t *hit);

/* ---- runlist coverage (anno) -------------------------------------------- */
/* Sorted, disjoint, inclusive spans per chr group (intspan runlists). */
int gams_spans_create(gams_gpu_t *h, uint32_t n_groups, const uint64_t *group_off,
                      const int32_t *lo, const int32_t *hi, gams_spans_t **sp);
void gams_spans_destroy(gams_gpu_t *h, gams_spans_t *sp);
/* anno.rs:128-139: prop = |set[group] & [clip_lo,clip_hi] & [qs,qe]| as f32 /
 * |[qs,qe]| as f32; group >= n_groups -> 0.0 */
int gams_gpu_cover(gams_gpu_t *h, gams_spans_t *sp, const uint32_t *group,
                   const int32_t *clip_lo, const int32_t *clip_hi,
                   const int32_t *qs, const int32_t *qe, uint64_t nq,
                   float *prop);

/* ---- text in, text out: locate -f, locate --count, anno ------------------------- */
/* A device-resident map from a byte string to its position in names[0..n) (NUL-terminated), which also keeps the
 * names' bytes so that kernels can print them.  Lookup is exact byte equality; a duplicate name is GAMS_EINVAL.
 * Uses: chromosome name -> group of a ctg index or a span set; ctg id -> ctg slot (anno); ctg slot -> id (locate). */
int gams_names_create(gams_gpu_t *h, uint32_t n, const char *const *names, gams_names_t **out);
/* The names of a table back (one that gams_spans_create_runlist_text made, for instance): *n names, *n_bytes bytes;
 * with `bytes` / `off` not NULL the names' bytes back to back (no NUL between) and the n + 1 offsets into them. */
int gams_names_read(gams_gpu_t *h, const gams_names_t *nm, uint32_t *n, uint64_t *n_bytes, char *bytes, uint64_t *off);
void gams_names_destroy(gams_gpu_t *h, gams_names_t *nm);

/* The three entries below take the bytes of an input file (n_bytes, any host memory; page-locked memory from
 * gams_gpu_host_alloc copies at the rate of the link; more than 4 GiB works) and return its finished rows.  Lines are
 * those of Rust's BufRead::lines(): split on '\n', one '\r' before a '\n' dropped, a last line without '\n' counted
 * (it keeps any '\r'), nothing after a final '\n'.  *text (text_bytes bytes, rows in input-line order, no NUL) points
 * into page-locked memory owned by the handle, valid until the next call of the same entry on that handle; *n_rows
 * counts the rows, a header row included.
 * GAMS_EUNSUPPORTED (nothing is printed; run the host path instead): a byte >= 0x80 or a NUL in the input, more than
 * 2^32 - 1 lines, and the entry-specific cases below. */
/* locate -f (locate.rs:84-141, utils.rs:7-22).  rg = the bytes of a line up to its first '\t' (locate.rs:89-91),
 * parsed like intspan's Range::from_str ([name.]chr[(strand)]:start[-end], 1-10 digits, runs of '-'/'_' between the
 * numbers, values <= INT32_MAX).  Invalid lines, lines whose chromosome is not in chr_names, and lines that
 * gams_gpu_locate does not locate (Lapper::find(start, end) against half-open [start, end + 1): a point range on a
 * ctg start is not located) print nothing; every other prints "{rg}\t{ctg_id}\n" (locate.rs:139).  chr_names[g]
 * names group g of ctg_ix; ctg_ids[i] names interval i of ctg_ix in the caller's original order (what
 * gams_gpu_locate returns), so ctg_ids has one name per interval (GAMS_EINVAL otherwise). */
int gams_gpu_locate_text(gams_gpu_t *h, gams_index_t *ctg_ix, const gams_names_t *chr_names, const gams_names_t *ctg_ids,
                         const char *bytes, uint64_t n_bytes, const char **text, uint64_t *text_bytes, uint64_t *n_rows);
/* locate --count (utils.rs:24-36): the lines locate_text locates print "{rg}\t{count}\n" (locate.rs:137), count =
 * gams_gpu_count of the range against group rg_group[i] of rg_ix, i the located interval of ctg_ix (rg_group has one
 * entry per interval of ctg_ix).  GAMS_EUNSUPPORTED if a located interval has rg_group[i] == UINT32_MAX: the host
 * path reports such a ctg as "not found in idx". */
int gams_gpu_count_text(gams_gpu_t *h, gams_index_t *ctg_ix, const gams_names_t *chr_names, gams_index_t *rg_ix,
                        const uint32_t *rg_group, const char *bytes, uint64_t n_bytes, const char **text,
                        uint64_t *text_bytes, uint64_t *n_rows);
/* anno over one input file (anno.rs:95-142).  With `header` the first line prints "{line}\t{prefix}Prop\n"
 * (anno.rs:98-110).  Every other line is split on '\t': field idx_id or idx_range (1-based) missing, or either
 * index 0, is GAMS_EINVAL (the reference panics, anno.rs:115).  The ctg id is the first match of (?i)ctg:[\w_]+:\d+
 * in field idx_id (utils.rs:118-129); no match, or an invalid range in field idx_range, drops the line.  If the
 * range's chromosome names span group g of sp (chr_names[g]), the id must be in ctg_ids (GAMS_EINVAL otherwise, the
 * reference panics, redis.rs:133-134) and prop is gams_gpu_cover of the range clipped to [ctg_start[k], ctg_end[k]],
 * k the id's slot; otherwise prop is 0.  Each row is "{line}\t{prop:.4}\n" with {:.4} exact (round half to even on
 * the binary value).  GAMS_EUNSUPPORTED for a reversed range (start > end) on a chromosome of the set, whose prop
 * the reference computes as 0/0, and for any prop that is not a finite value in [0, 1]. */
int gams_gpu_anno_text(gams_gpu_t *h, gams_spans_t *sp, const gams_names_t *chr_names, const gams_names_t *ctg_ids,
                       const int32_t *ctg_start, const int32_t *ctg_end, const char *bytes, uint64_t n_bytes, int header,
                       const char *prefix, uint32_t idx_id, uint32_t idx_range, const char **text, uint64_t *text_bytes,
                       uint64_t *n_rows);

/* ---- text in, span set out: the runlist JSON of anno (anno.rs:84-87: intspan::read_json, then json2set) ---- */
/* The bytes of a runlist JSON file -- one flat object {"chr": "runlist", ...} -- to a span set that behaves under
 * gams_gpu_cover and gams_gpu_anno_text exactly like one from gams_spans_create on the normalised spans
 * (IntSpan::add_runlist: the union of the spans, overlapping and adjacent ones joined).  Group g is the g-th key of
 * the object in file order and *chr_names names the groups in that order (for gams_gpu_anno_text); *n_groups and
 * *n_spans receive the sizes.  A runlist is tokens separated by ',', each `a` or `a-b` of 1-10 decimal digits with
 * a <= b <= INT32_MAX, in any order; the values "" and "-" are the empty set.  White space between the strings is
 * free (compact, pretty-printed, CRLF); "{}" is a set with no group.
 * GAMS_EUNSUPPORTED (run the host reader instead, which is the judge of what is invalid: this entry never answers
 * GAMS_EINVAL for the file's content): a backslash, a byte >= 0x80 or a NUL anywhere; a control character (below
 * 0x20) inside a key; anything that is not a flat
 * object of string values (a nested value, a number, null, an array, a missing brace, text behind the '}'); inside
 * a runlist any byte that is no digit, '-' or ',' (white space included), an empty token, more than 10 digits, a
 * value above INT32_MAX, a > b, a negative number; a duplicate key; more than 2^32 - 16 tokens.
 * On any return but GAMS_OK nothing is created, *sp and *chr_names are NULL and the handle stays usable.  Release
 * with gams_spans_destroy and gams_names_destroy. */
int gams_spans_create_runlist_text(gams_gpu_t *h, const char *bytes, uint64_t n_bytes, gams_spans_t **sp,
                                   gams_names_t **chr_names, uint32_t *n_groups, uint64_t *n_spans);
/* A span set as arrays, for hosts and tests: group_off[n_groups + 1], and lo / hi (cap entries each) when
 * cap >= *n_spans.  cap = 0 is the size query: only group_off and *n_spans are written.  GAMS_EINVAL for a cap
 * between 1 and the set's size. */
int gams_spans_read(gams_gpu_t *h, const gams_spans_t *sp, uint64_t *group_off, int32_t *lo, int32_t *hi, uint64_t cap,
                    uint64_t *n_spans);

/* ---- text in, index out: the rg loader (utils.rs:39-67 read_range, then redis.rs:288-299) ---- */
/* The two entries below take the bytes of ONE .rg file (lines, refused bytes and the 2^32 - 1 line limit as above) and
 * bucket its ranges per ctg the way gams::read_range does.  The WHOLE line goes through Range::from_str (utils.rs:50;
 * unlike locate -f nothing is cut at a tab, so "I:1-100\tfoo" is invalid).  A valid line is located as gams_gpu_locate
 * locates (group of its chromosome in chr_names, start, end) in ctg_ix; invalid lines, unknown chromosomes and
 * unlocated lines (the point range on a ctg start among them) are skipped.  Of the located lines of a ctg the first
 * in file order is dropped (`.entry().and_modify(push).or_default()` creates the bucket with it and pushes nothing)
 * and the rest are kept, so a ctg with one located line has a bucket, and the bucket is empty.  Drop-first is per file:
 * two files concatenated are not two files loaded.  Bucket / group i belongs to interval i of ctg_ix in the caller's
 * original order (what gams_gpu_locate returns); n_ctg = the intervals of ctg_ix.  GAMS_EUNSUPPORTED also for more than
 * 2^32 - 16 kept ranges (the limit of gams_index_create).  Zero bytes: GAMS_OK, nothing kept. */
/* The buckets as arrays.  bucket_off has n_ctg + 1 entries; seen[i] (seen may be NULL) is 1 if ctg i had a located line,
 * i.e. has a bucket; the kept ranges of bucket i are start/end/line[bucket_off[i] .. bucket_off[i+1]) in file order,
 * line = the 0-based line number.  cap == 0 is the size query: bucket_off, seen and *n_kept only.  A cap smaller than
 * *n_kept is GAMS_EINVAL (with *n_kept set).  Two calls return identical arrays. */
int gams_gpu_read_range_text(gams_gpu_t *h, gams_index_t *ctg_ix, const gams_names_t *chr_names, const char *bytes,
                             uint64_t n_bytes, uint64_t *bucket_off, uint8_t *seen, int32_t *start, int32_t *end,
                             uint32_t *line, uint64_t cap, uint64_t *n_kept);
/* The rg index of the file: n_ctg groups, group i = bucket i's ranges as [start, end + 1) (redis.rs:291-294), in the
 * same canonical order gams_index_create gives the same buckets.  rg_group[i] (n_ctg entries) is i if ctg i has a
 * bucket and UINT32_MAX otherwise: the table gams_gpu_count_text and gams_gpu_sw_text_actions take.  Destroy *rg_ix with
 * gams_index_destroy. */
int gams_index_create_range_text(gams_gpu_t *h, gams_index_t *ctg_ix, const gams_names_t *chr_names, const char *bytes,
                                 uint64_t n_bytes, gams_index_t **rg_ix, uint32_t *rg_group, uint64_t *n_kept);

/* ---- several files in one load: `gams rg f1 f2 ...` / `gams feature f1 f2 ...` (rg.rs:40, feature.rs:47) ---- */
/* The two entries below take n_files files, file f = bytes[f][0 .. n_bytes[f]) (bytes[f] may be NULL where n_bytes[f] is
 * 0), and load them as the reference does, one after another: lines are per file (a last line without '\n' ends at its
 * file's end and never joins the next file's first line; an empty file has no lines), every line is parsed and located as
 * above, and of the located lines of a ctg the first IN EACH FILE is dropped.  The kept lines of a ctg are ordered by
 * (file, line).  No file, or one: exactly the load of zero bytes, or of that file's bytes.
 * GAMS_EUNSUPPORTED as for the one-file entries -- a byte >= 0x80 or a NUL in any file, 2^32 - 1 lines in all, 2^32 - 16
 * kept -- and for more than 2^24 (file, ctg) pairs, n_files * n_ctg (the tables by them). */
/* The rg index of the load: group i = the kept ranges of ctg i from all files as [start, end + 1); rg_group as in
 * gams_index_create_range_text (i if ctg i had a located line in any file).  With one file the result is that entry's. */
int gams_index_create_range_files(gams_gpu_t *h, gams_index_t *ctg_ix, const gams_names_t *chr_names, uint32_t n_files,
                                  const char *const *bytes, const uint64_t *n_bytes, gams_index_t **rg_ix, uint32_t *rg_group,
                                  uint64_t *n_kept);

#define GAMS_LOADER_RG 0      /* kind: the records of `gams rg` */
#define GAMS_LOADER_FEATURE 1 /*       the records of `gams feature` (with length and tag) */
#define GAMS_LOADER_RECORDS 0 /* format: "{id}\t{json}\n" */
#define GAMS_LOADER_TSV 1     /*         the values of the record in field order, tab-separated (tsv.rs), no header */
#define GAMS_LOADER_RESP 2    /*         "*3\r\n$3\r\nSET\r\n${len(id)}\r\n{id}\r\n${len(json)}\r\n{json}\r\n" */
/* The records the loaders SET (rg.rs:62-82, feature.rs:73-96), as text written on the device.  ctg_ix, chr_names, ctg_ids
 * as for gams_gpu_locate_text; tag (tag_bytes bytes, no NUL needed) is used by GAMS_LOADER_FEATURE only.
 * serial_base[i] (NULL: all 0) is cnt:{kind}:{ctg i} before the load, i an interval of ctg_ix in the caller's order; the
 * k-th kept line (from 1) of ctg i in (file, line) order gets serial serial_base[i] + k, which is what incr_sn_n and
 * `serial - cnt` give over successive files; serial_next[i] (serial_next may be NULL) is the counter after the load.  A
 * negative base, or a serial beyond INT32_MAX, is GAMS_EINVAL.
 * id = "{rg|feature}:{ctg_id}:{serial}".  range = Range::to_string() of the parsed line -- "name." if the name is not
 * empty, the chromosome, "(strand)" if not empty, ':', start, and "-end" only when end != start --, canonical and not
 * echoed ("I:007_9 " prints "I:7-9").  json = {"id":"..","range":".."} or, for a feature,
 * {"id":"..","range":"..","length":N,"tag":".."} with N = end - start + 1 as a signed i32 (data.rs:16-28, serde's field
 * order).  Inside the JSON '"' and '\' get a backslash; nowhere else.
 * Rows are grouped by (file, interval of ctg_ix in the caller's order), in line order inside a group: those of file f and
 * interval i are text[text_off[f * n_ctg + i] .. text_off[f * n_ctg + i + 1]) (text_off has n_files * n_ctg + 1 entries; a
 * host that prints file by file with the ctgs in id order has the reference's SET order).  n_in_file[f] (may be NULL)
 * counts the kept lines of file f, *n_rows all of them.  *text (text_bytes bytes, no NUL) is page-locked memory of this
 * entry's own on the handle, valid until its next call.  Two calls return identical text.  No file, only empty files or
 * nothing kept: GAMS_OK, no rows, text_off all zero, serial_next = serial_base.
 * GAMS_EUNSUPPORTED (run the host path) as above, and: a kept line whose name or strand holds a byte < 0x20 (serde_json
 * escapes those) or 2^30 bytes; a tag with a byte < 0x20 or >= 0x80, or of 2^30 bytes.  ctg ids are printed as given.
 * gams_gpu_last_stage_ms then reports ten stages: the loader's lines, parse, locate, first, keep, offsets, order, then
 * serials, row lengths, write (seven when nothing was kept; GAMS_ESTATE for an input without lines). */
int gams_gpu_loader_text(gams_gpu_t *h, gams_index_t *ctg_ix, const gams_names_t *chr_names, const gams_names_t *ctg_ids,
                         uint32_t n_files, const char *const *bytes, const uint64_t *n_bytes, int kind, const char *tag,
                         uint64_t tag_bytes, int format, const int32_t *serial_base, const char **text, uint64_t *text_bytes,
                         uint64_t *text_off, int32_t *serial_next, uint64_t *n_in_file, uint64_t *n_rows);

/* ---- text in, text out: peak (utils.rs:83-116 read_peak, then peak.rs:41-160) ---- */
/* The bytes of ONE wave TSV ("{range}\t{gc_content}\t{signal}" rows; lines, refused bytes and the 2^32 - 1 line limit as
 * for the text entries above) -> the rows `gams peak` makes of it, as gams_host_peak prints them:
 *   "peak:{ctg_id}:{serial}\t{range}\t{length}\t{gc}\t{signal}\t{left_wave_length}\t{left_amplitude}\t{left_signal}\t"
 *   "{right_wave_length}\t{right_amplitude}\t{right_signal}\n"
 * ctg_ix, chr_names, ctg_ids as for gams_gpu_locate_text.  ctg_index[i], chr_start[i], chr_end[i] describe interval i of
 * ctg_ix in the caller's original order: the slot of s that holds the ctg's bases (UINT32_MAX: none; otherwise a slot
 * of chr_end - chr_start + 1 bases, GAMS_EINVAL if not) and the ctg's place on its chromosome.
 * parts[0], the line up to its first '\t', goes through Range::from_str; an invalid one (the header row) skips the
 * line.  A line with a valid range and fewer than three fields is GAMS_EINVAL, located or not (the reference panics,
 * utils.rs:102).  The strand is dropped, the range is located as gams_gpu_locate locates; unknown chromosomes and
 * unlocated lines are skipped.  Of the located lines of a ctg the first in file order is dropped (utils.rs:109-112, as
 * in the rg loader): it is never looked at again, and a ctg with one located line prints nothing.  The kept peaks of a
 * ctg are ordered by start, ties in file order (peak.rs:49, a stable sort), and numbered from 1.  Every kept peak must
 * lie inside its ctg (chr_start <= start <= end <= chr_end) and its ctg must have a sequence: GAMS_EINVAL otherwise.
 * gc = gams_gpu_range_gc of the range.  With k the peak's rank among the n of its ctg: left_wave_length = start -
 * (k ? end[k-1] : chr_start) + 1, left_amplitude = |gc - gc[k-1]| (0 for k = 0), left_signal = the third field of peak
 * k - 1 (its own for k = 0); the right side mirrors it with start[k+1] / chr_end.  Wave lengths are signed i32.
 * {range} is the range reprinted with the strand cleared: the "name." prefix if the name is not empty, the chromosome,
 * ':', start, and "-end" only when end != start; gc and the amplitudes print as Rust's `{}` prints an f32 (shortest
 * round trip), the signals are echoed.
 * *text (text_bytes bytes, no NUL; page-locked memory owned by the handle, valid until the next call of this entry on
 * the handle) holds the rows grouped by ctg in the caller's order: those of interval i are text[text_off[i] ..
 * text_off[i+1]) (text_off has n_ctg + 1 entries; `gams peak` prints the ctgs in id order).  *n_rows counts the rows.
 * Two calls return identical text.  Zero bytes or no kept peak: GAMS_OK, no rows, text_off all zero.
 * GAMS_ESTATE for a seqset without the sequence bytes (plane-only).  GAMS_EUNSUPPORTED (nothing is printed; run the
 * host path) also when (ctg, start, line) does not fit a 64-bit sort key -- bits(n_ctg) + 31 + bits(lines - 1) > 64 --
 * and for a gc or amplitude the device formatters do not cover (none on valid input). */
int gams_gpu_peak_text(gams_gpu_t *h, gams_seqset_t *s, gams_index_t *ctg_ix, const gams_names_t *chr_names,
                       const gams_names_t *ctg_ids, const uint32_t *ctg_index, const int32_t *chr_start,
                       const int32_t *chr_end, const char *bytes, uint64_t n_bytes, const char **text,
                       uint64_t *text_bytes, uint64_t *text_off, uint64_t *n_rows);

/* The records `gams peak` stores (peak.rs:68-78,163-171: SET peak:{ctg_id}:{serial} serde_json(Peak)), as text written on
 * the device.  Inputs, checks and return codes are exactly those of gams_gpu_peak_text; format is one of GAMS_LOADER_RECORDS
 * / _TSV / _RESP (anything else: GAMS_EINVAL):
 *   TSV      the row of gams_gpu_peak_text, byte for byte, but for the serial;
 *   RECORDS  "{id}\t{json}\n";
 *   RESP     "*3\r\n$3\r\nSET\r\n${len(id)}\r\n{id}\r\n${len(json)}\r\n{json}\r\n", the lengths in bytes as written.
 * serial_base[i] (NULL: all 0) is cnt:peak:{ctg i} before the load, i an interval of ctg_ix in the caller's order; the k-th
 * kept peak (from 1) of ctg i in sorted order gets serial serial_base[i] + k (peak.rs:71-77); serial_next[i] (serial_next
 * may be NULL) is the counter afterwards, the base for a ctg without kept peaks.  A negative base, or a serial beyond
 * INT32_MAX, is GAMS_EINVAL (decided before any row is written; the handle stays usable).
 * json = {"id":"peak:{ctg_id}:{serial}","range":"{range}","length":N,"gc":F,"signal":"S","left_wave_length":N,
 * "left_amplitude":F,"left_signal":"S","right_wave_length":N,"right_amplitude":F,"right_signal":"S"} (data.rs:30-43, serde's
 * field order, no spaces), the fields those of the TSV row.  Inside its strings '"' and '\' get a backslash (the ctg id, the
 * name prefix, the signals).  A float prints as serde_json prints an f32 (ryu: shortest round trip, always a decimal point):
 * for 0 and for [1e-5, 1] -- every gc and amplitude -- the text of the TSV row with ".0" behind one without a point ("0.0",
 * "1.0", "0.0268").  Parity with serde_json / ryu is their documented behaviour, not pinned against a run.
 * GAMS_EUNSUPPORTED (nothing is printed; run the host path) for what gams_gpu_peak_text refuses; in RECORDS and RESP only,
 * for a kept line whose name prefix or signal holds a byte < 0x20 (serde_json writes \uXXXX and the short escapes) or 2^30
 * bytes; and for a float outside the set above (NaN, -0, a nonzero value below 1e-5: ryu's exponent form).
 * *text (text_bytes bytes, no NUL) is page-locked memory of this entry's own on the handle, valid until its next call: a
 * text of gams_gpu_peak_text stays valid across it.  text_off (n_ctg + 1 entries), *n_rows, the grouping of the rows and
 * the ten stages of gams_gpu_last_stage_ms as for gams_gpu_peak_text.  Two calls return identical text.  Zero bytes or no
 * kept peak: GAMS_OK, no rows, text_off all zero, serial_next = serial_base. */
int gams_gpu_peak_records_text(gams_gpu_t *h, gams_seqset_t *s, gams_index_t *ctg_ix, const gams_names_t *chr_names,
                               const gams_names_t *ctg_ids, const uint32_t *ctg_index, const int32_t *chr_start,
                               const int32_t *chr_end, const char *bytes, uint64_t n_bytes, int format,
                               const int32_t *serial_base, const char **text, uint64_t *text_bytes,
                               uint64_t *text_off, int32_t *serial_next, uint64_t *n_rows);

/* ---- text in, text out: sw from a feature file (feature.rs:50-54 read_range, then sw.rs:132-191) ---- */
/* The bytes of ONE range file (lines, refused bytes and limits as for the rg loader above) -> the rows `gams sw` prints
 * for the features `gams feature` would have stored from it.  ctg_ix, chr_names, ctg_ids, ctg_index, chr_start, chr_end
 * as for gams_gpu_peak_text (chr_names names every group of ctg_ix); size, max, resize, actions, rg_ix as for
 * gams_gpu_sw_text_actions, rg_group[i] belonging to interval i of ctg_ix.
 * The file is read as gams_gpu_read_range_text reads it: the whole line through Range::from_str, located by overlap, the
 * first located line of a ctg dropped.  The kept lines of a ctg keep file order; the k-th of them, from 1, is the
 * feature "feature:{ctg_id}:{k}" (feature.rs:74-86 on a fresh cnt:feature:).  Every kept feature prints the rows of
 * sw.rs:141-191, byte-equal to what gams_gpu_sw_text_actions prints for the same features and ids.
 * *text (text_bytes bytes, no NUL; page-locked memory owned by the handle, valid until the handle's next sw call) holds
 * the rows grouped by interval in the caller's order: those of interval i are text[text_off[i] .. text_off[i+1])
 * (text_off has n_ctg + 1 entries; `gams sw` prints the ctgs in id order).  *n_features = the kept lines ("There are N
 * features in this file"), *n_rows the rows.  Two calls return identical text.  Zero bytes or no kept line: GAMS_OK,
 * no rows, text_off all zero.
 * Without GAMS_SW_GC no sequence byte is read: s and ctg_index may be NULL.  With it, a ctg that has kept features needs a
 * slot of chr_end - chr_start + 1 bases.
 * GAMS_EINVAL: null arguments; size < 2, max < 0 or resize < 2; unknown action bits; GAMS_SW_COUNT without rg_ix; a kept
 * feature whose middle pair lies outside its ctg (located by overlap does not imply it; the message names the smallest
 * such line; a dropped first line is never looked at); with GAMS_SW_GC a ctg with kept features and no slot, or a slot
 * of another length.  GAMS_ESTATE: GAMS_SW_GC on a seqset without the sequence bytes.  GAMS_EUNSUPPORTED (nothing is
 * printed; run the host path): what the rg loader refuses, a value the sw formatter does not cover, more feature
 * slots than one launch takes, max beyond 2^24.
 * gams_gpu_last_stage_ms then reports twelve stages: the loader's lines, parse, locate, first, keep, offsets, order,
 * then gather, geometry, rows, text lengths, text write (seven when no line is kept). */
int gams_gpu_sw_feature_text(gams_gpu_t *h, gams_seqset_t *s, gams_index_t *ctg_ix, const gams_names_t *chr_names,
                             const gams_names_t *ctg_ids, const uint32_t *ctg_index, const int32_t *chr_start,
                             const int32_t *chr_end, const char *bytes, uint64_t n_bytes,
                             int32_t size, int32_t max, int32_t resize, uint32_t actions,
                             gams_index_t *rg_ix, const uint32_t *rg_group,
                             const char **text, uint64_t *text_bytes, uint64_t *text_off,
                             uint64_t *n_features, uint64_t *n_rows);
/* From the bytes of ONE range file to the sw summary: the rows gams_gpu_sw_feature_text would print for the same
 * arguments (it takes them without the text outputs), added into tag slot `tag` of `sum` on the device and never stored
 * -- no row buffer, no text, no read-back but the counts and two flag words.  Drop-first is per file and per ctg, as
 * there; several files, tagged or not, are several calls into one accumulator (feature ids play no part in the table).
 * *n_features = the kept lines, *n_rows = the rows added.  Checks and return codes as for gams_gpu_sw_feature_text, and
 * GAMS_EINVAL for tag >= n_tags and for size, max, resize or actions other than the accumulator's; on any code but
 * GAMS_OK the accumulator is as it was before the call.  GAMS_EUNSUPPORTED (run the host path) for what the loader
 * refuses and for a non-NaN statistic outside [0, 1000).
 * gams_gpu_last_stage_ms then reports ten stages: the loader's lines, parse, locate, first, keep, offsets, order, then
 * gather, geometry, rows (seven when no line is kept). */
int gams_gpu_sw_feature_summary(gams_gpu_t *h, gams_seqset_t *s, gams_index_t *ctg_ix, const gams_names_t *chr_names,
                                const gams_names_t *ctg_ids, const uint32_t *ctg_index, const int32_t *chr_start,
                                const int32_t *chr_end, const char *bytes, uint64_t n_bytes,
                                int32_t size, int32_t max, int32_t resize, uint32_t actions,
                                gams_index_t *rg_ix, const uint32_t *rg_group, gams_sw_summary_t *sum, uint32_t tag,
                                uint64_t *n_features, uint64_t *n_rows);

/* gams_gpu_sw_feature_summary with span sets (see gams_gpu_sw_summary_batch_anno): set_group[a][i] for interval i of
 * ctg_ix in the caller's order, as ctg_index is.  The same stages. */
int gams_gpu_sw_feature_summary_anno(gams_gpu_t *h, gams_seqset_t *s, gams_index_t *ctg_ix, const gams_names_t *chr_names,
                                     const gams_names_t *ctg_ids, const uint32_t *ctg_index, const int32_t *chr_start,
                                     const int32_t *chr_end, const char *bytes, uint64_t n_bytes,
                                     int32_t size, int32_t max, int32_t resize, uint32_t actions,
                                     gams_index_t *rg_ix, const uint32_t *rg_group, gams_sw_summary_t *sum, uint32_t tag,
                                     uint32_t n_anno, gams_spans_t *const *sets, const uint32_t *const *set_group,
                                     uint64_t *n_features, uint64_t *n_rows);

/* ---- text in, text out: locate --seq (locate.rs:124-134) ---- */
/* The bytes of ONE range file (lines, refused bytes and the 2^32 - 1 line limit as for gams_gpu_locate_text) -> the bases
 * of its ranges as FASTA, copied on the device out of a resident seqset.  ctg_ix, chr_names as for gams_gpu_locate_text;
 * ctg_index, chr_start, chr_end as for gams_gpu_peak_text: per interval of ctg_ix in the caller's order, the slot of s
 * that holds the ctg's bases (UINT32_MAX: none) and the ctg's place on its chromosome.
 * rg = the bytes of a line up to its first '\t', parsed like Range::from_str; the strand is not used by the lookup; a
 * line is located as gams_gpu_locate locates.  Invalid lines, unknown chromosomes and unlocated lines (the point range on
 * a ctg start among them) print nothing.  Every located line prints ">" rg "\n" bases "\n" (locate.rs:134): rg echoed
 * byte for byte as it stands in the file, name prefix and strand kept; bases = bytes [start - chr_start, end - chr_start]
 * of the ctg's slot, copied verbatim -- the sequence bytes are not interpreted, so lower case, N and any byte value,
 * 0 and >= 0x80 included, pass through (the refused bytes are refused in the input, not in the sequences).  Nothing is
 * reverse-complemented and nothing is wrapped, as in the reference.
 * *text (text_bytes bytes, rows in input-line order, no NUL) is page-locked memory owned by the handle, a buffer of this
 * entry's own, valid until the next call of this entry on the handle; *n_rows counts the records.  Two calls return
 * identical text.  Zero bytes, or no located line: GAMS_OK, no rows, *text_bytes == 0.
 * GAMS_EINVAL: null arguments; a located line that does not satisfy chr_start <= start <= end <= chr_end of its ctg (the
 * reference panics on the slice, locate.rs:133; a range that spans a ctg boundary is located to the ctg in front and
 * lands here; a reversed range that is located does too) -- the message names the smallest such line, 0-based; a located
 * ctg with no slot, or with a slot whose length is not chr_end - chr_start + 1 (a ctg no line is located to may have
 * either).  GAMS_ESTATE: a seqset without the sequence bytes (plane-only).  GAMS_EUNSUPPORTED (nothing is printed; run
 * the host path): a byte >= 0x80 or a NUL in the input, more than 2^32 - 1 lines.
 * All byte arithmetic is 64-bit: a row alone may be 2^31 bytes and the text may pass 4 GiB, as far as one device
 * allocation and one page-locked buffer hold it; no test runs a text beyond 4 GiB.
 * gams_gpu_last_stage_ms then reports six stages: lines (upload + line index), parse, locate, lengths (row lengths and
 * the checks), offsets (the per-line offsets), copy (GAMS_ESTATE when no line was located: nothing was copied). */
int gams_gpu_locate_seq_text(gams_gpu_t *h, gams_seqset_t *s, gams_index_t *ctg_ix, const gams_names_t *chr_names,
                             const uint32_t *ctg_index, const int32_t *chr_start, const int32_t *chr_end,
                             const char *bytes, uint64_t n_bytes,
                             const char **text, uint64_t *text_bytes, uint64_t *n_rows);

/* ---- gen: valid regions of a chromosome (first "next" row of SURVEY section 8f) ---- */
/* gen.rs:86-104: bases other than A C G T a c g t are ambiguous; the valid set is their
 * complement after fill(fill-1) and excise(min_len).  Writes up to `cap` spans (1-based,
 * inclusive, ascending); *n_spans is the full count (call with cap = 0 to size). */
int gams_gpu_valid_spans(gams_gpu_t *h, const uint8_t *seq, uint64_t len, int32_t fill,
                         int32_t min_len, int32_t *span_lo, int32_t *span_hi, uint64_t cap,
                         uint64_t *n_spans);

/* ---- gen from the bytes of a FASTA file (gen.rs:67-157) ---- */
/* The bytes of ONE FASTA file (any host memory, as for the text entries; they cross the link once) -> the chromosomes,
 * the ctg table, and a seqset of the ctgs' bases with its G/C plane, built on the device from the copy just uploaded.
 * Lines are split on '\n'; a last line without '\n' counts.  A line whose first byte is '>' starts a record: its id is
 * the bytes behind the '>' up to the first ASCII white space or the line's end.  Every other line contributes its bytes
 * as bases, without a '\r' that stands directly before the '\n' or at the end of the input; a '>' that is not in column
 * 0 is a base (an ambiguous one); empty lines contribute nothing; a record without bases is a chromosome of length 0
 * without ctgs.  Zero bytes: GAMS_OK, no chromosomes.  Otherwise the first byte must be '>' (GAMS_EINVAL; the reference
 * panics); piece, fill or min_len < 1 is GAMS_EINVAL.
 * Bases other than A C G T a c g t are ambiguous; per chromosome the valid set is their complement after fill(fill - 1)
 * and excise(min_len), and a valid span longer than `piece` is cut into pieces of `piece` bases, the last one taking the
 * remainder (gen.rs:86-126: gams_gpu_valid_spans per chromosome and the split).  Chromosomes come in file order; ctgs in
 * chromosome order, then ascending serial, which counts from 1 inside each chromosome; the id of a ctg is
 * "ctg:{name of chr}:{serial}"; chr_start / chr_end are 1-based, inclusive.  Ctg k of the table is slot k of the seqset.
 * GAMS_EUNSUPPORTED (run the host path): a byte >= 0x80 or a NUL; inside a sequence line a '\r' anywhere else, a space, a
 * tab, 0x0B or 0x0C (the reference trims trailing white space; the host path does); an empty id; a duplicate id; a
 * chromosome of more than INT32_MAX bases; more than 2^32 - 1 ctgs; more than 2^40 bytes of input.  Two calls on the same bytes return identical tables
 * and identical device bytes. */
typedef struct {
    int32_t piece, fill, min_len; /* --piece, --fill, --min (gen.rs:28-50) */
} gams_gen_params_t;
typedef struct {
    uint32_t chr, serial; /* chromosome (file order) and serial inside it, from 1 */
    int32_t chr_start, chr_end;
} gams_gen_ctg_t;
int gams_gpu_gen_text(gams_gpu_t *h, const char *bytes, uint64_t n_bytes, const gams_gen_params_t *params,
                      gams_gen_t **g);
/* sizes of the result (any pointer may be NULL): chromosomes, ctgs, and the bytes of all ids together */
int gams_gen_counts(gams_gpu_t *h, const gams_gen_t *g, uint32_t *n_chr, uint32_t *n_ctg, uint64_t *name_bytes);
/* the chromosomes (any pointer may be NULL): the id of chromosome c is names[name_off[c] .. name_off[c + 1]) (name_bytes
 * bytes, no NUL; name_off has n_chr + 1 entries), chr_len[c] its bases */
int gams_gen_chrs(gams_gpu_t *h, const gams_gen_t *g, char *names, uint64_t *name_off, uint32_t *chr_len);
/* the ctg table, n_ctg records */
int gams_gen_ctgs(gams_gpu_t *h, const gams_gen_t *g, gams_gen_ctg_t *ctgs);
/* The seqset, handed to the caller ONCE (a second call is GAMS_ESTATE); destroy it with gams_seqset_destroy.  An
 * ordinary seqset in the layout of gams_seqset_create with bytes and a valid plane, gaps zero: `wave`, `sw`, range_gc
 * and peak_text read it like an uploaded one, and gams_seqset_download brings a ctg's bases back for the store. */
int gams_gen_seqset(gams_gpu_t *h, gams_gen_t *g, gams_seqset_t **s);
/* frees the tables, and the seqset if it was not handed out */
void gams_gen_destroy(gams_gpu_t *h, gams_gen_t *g);

/* ---- gen: the `seq:{ctg}` values (gen.rs:153-156 -> redis.rs:137-154 insert_seq / encode_gz) ---- */
/* The value stored under seq:{ctg} is a gzip member of the ctg's bases.  The members made here are literal-only
 * deflate: one dynamic-Huffman block per GAMS_SEQ_GZ_BLOCK bases, no matches, which on DNA text is smaller than what
 * flate2 writes at Compression::fast().  Any RFC 1952 decoder inflates them to the bases (flate2, zlib, libdeflate,
 * this project's decode_gz); the bytes are not flate2's.  A ctg of length 0 is the fixed 30-byte empty member.  The
 * framing, the block structure and the code construction are described in gams_amd/csrc/seq_gz_code.hpp. */
#define GAMS_SEQ_GZ_BLOCK 32768u /* input bytes per deflate block */
#define GAMS_SEQ_GZ_MEMBERS 3    /* format, beside GAMS_LOADER_RESP: the members back to back */
/* Code lengths of a length-limited prefix code (host code, no device involved): len[s] in 1..limit for the symbols
 * with freq[s] != 0 among n_sym, 0 for the others; complete (Kraft sum exactly 1) for two or more used symbols, length
 * 1 for a single one.  Integer-only and a function of the histogram alone.  GAMS_EINVAL: n_sym 0 or above 288, limit 0
 * or above 15, more used symbols than 2^limit. */
int gams_deflate_lengths(const uint32_t *freq, uint32_t n_sym, uint32_t limit, uint8_t *len);
/* The member of n bases (any byte values), on the host: the very bytes gams_gpu_seq_gz writes for a slot that holds
 * them.  *n_out = the member's bytes; cap == 0 is the size query, a cap below *n_out is GAMS_EINVAL (nothing written). */
int gams_seq_gz_host(const uint8_t *seq, uint64_t n, uint8_t *out, uint64_t cap, uint64_t *n_out);
/* The members of slots first .. first + count of a resident seqset, deflated on the device; only the finished bytes
 * cross the link.  format GAMS_SEQ_GZ_MEMBERS: the members back to back (ctg_ids may be NULL).  GAMS_LOADER_RESP:
 * "*3\r\n$3\r\nSET\r\n${len}\r\nseq:{ctg_id}\r\n${len}\r\n{member}\r\n" per slot, ctg_ids entry i naming slot
 * first + i, the lengths in bytes as written, the member passing through as the binary it is.  The bytes of slot
 * first + i are out[out_off[i] .. out_off[i + 1]) (out_off has count + 1 entries, *out_bytes = out_off[count]).
 * *out is page-locked memory of this entry's own on the handle, valid until its next call; the texts of the other
 * entries stay valid across it.  Two calls return identical bytes.  The call waits for the uploads queued so far, as
 * gams_seqset_download does.  count == 0: GAMS_OK, no bytes.
 * GAMS_ESTATE: a seqset without the sequence bytes (plane-only).  GAMS_EINVAL: null arguments, a range outside the
 * set, a format other than the two, GAMS_LOADER_RESP without ctg_ids or with fewer than count of them.
 * GAMS_EUNSUPPORTED: more than 2^31 - 1 blocks in the range.
 * gams_gpu_last_stage_ms then reports five stages: hist (per block, the byte histogram and the raw CRC-32 from one
 * read of the bases), codes (per block, the code lengths, the codes and the header's bits), sizes (per ctg, the bit
 * offset of every block, the CRC-32 joined from its blocks' and the member's length), pack (the frames, headers and
 * trailers, then every block's bits), copy (the finished bytes to the host).  (GAMS_ESTATE for count == 0.) */
int gams_gpu_seq_gz(gams_gpu_t *h, gams_seqset_t *s, uint32_t first, uint32_t count, const gams_names_t *ctg_ids,
                    int format, const char **out, uint64_t *out_bytes, uint64_t *out_off);

/* ---- the `seq:{ctg}` values back into a seqset: indexed members, inflated on the device ---- */
/* GAMS_SEQ_GZ_INDEXED, ORed into `format` of gams_gpu_seq_gz (either format), writes the indexed form of the members:
 * FLG = 4 and, in the FEXTRA field (RFC 1952 2.3.1.1, which every gzip reader skips), one subfield 'G' 'I' holding
 * u32 block, u32 chunk and ceil(n / chunk) u32 bit offsets into the deflate body, all little-endian: entry j is the
 * BFINAL bit of the block that begins with base j * chunk where j * chunk is a multiple of `block`, the first bit of
 * that base's literal code everywhere else.  Body and trailer are the plain member's, bit for bit; without the flag
 * every byte is what it was.  The index costs 4 bytes per GAMS_SEQ_GZ_CHUNK bases.  A ctg whose index would not fit
 * XLEN <= 65535 (more than 16,380 chunks) gets the plain member: the indexed writers never fail for size.
 * (gams_amd/csrc/seq_gz_code.hpp has the layout.) */
#define GAMS_SEQ_GZ_INDEXED 0x100
#define GAMS_SEQ_GZ_CHUNK 1024u /* bases per index entry */
/* host twin of the indexed writer: the very bytes gams_gpu_seq_gz writes with GAMS_SEQ_GZ_INDEXED (sized like
 * gams_seq_gz_host) */
int gams_seq_gz_host_indexed(const uint8_t *seq, uint64_t n, uint8_t *out, uint64_t cap, uint64_t *n_out);
#define GAMS_SEQ_GZ_DONE 0    /* slot holds the bases and their plane */
#define GAMS_SEQ_GZ_FOREIGN 1 /* not taken: the host inflates this value and uploads it */
/* Host twin of the device inflater: the same decoder core, chunk by chunk on one core.  *status = GAMS_SEQ_GZ_DONE and
 * out[0, *n_out) the bases, or GAMS_SEQ_GZ_FOREIGN (*n_out = 0 where the header, subfield and trailer already disagree)
 * for anything that is not an intact indexed member; nothing in the member is trusted and no byte outside
 * [member, member + n_bytes) is read.  GAMS_EINVAL: null arguments, or a member that passed the O(1) checks and whose
 * ISIZE (then in *n_out) exceeds cap. */
int gams_seq_gunzip_host(const uint8_t *member, uint64_t n_bytes, uint8_t *out, uint64_t cap, uint64_t *n_out, int *status);
/* Slots first .. first + count of a seqset from their `seq:` values: members[i] / member_bytes[i] is the value of slot
 * first + i.  Indexed members with a chunk of 512, 1024, 2048 or 4096 and a block of 4096 .. 65,536 (a multiple of
 * 4096; larger blocks are refused: a block is staged in LDS) are uploaded as they are -- a third of the bases -- and
 * inflated on the device straight into their slots, bases and G/C plane; CRC-32 and ISIZE are verified.  status[i] is
 * GAMS_SEQ_GZ_DONE, or GAMS_SEQ_GZ_FOREIGN for a value the device does not take (*n_foreign counts them): plain or
 * foreign gzip (matches, stored blocks), anything damaged.  A value refused by the O(1) checks of its header,
 * subfield and trailer is not uploaded and its slot is not touched; one refused on the device (a chunk that does not
 * land on the next entry, a bad code, a CRC mismatch) leaves its slot's content unspecified.  No byte outside a taken
 * slot and its plane bytes is written.  The caller inflates FOREIGN values itself (gams_seqset_upload).
 * The call queues behind every pass already reading the seqset and returns when the statuses are known; later passes
 * wait for it like for an upload.  The plane stays valid if it was.
 * GAMS_EINVAL: null arguments, slots outside the set, or a member that passed the O(1) checks and whose ISIZE is not
 * its slot's length (nothing is written).  GAMS_ESTATE: a plane-only seqset.  count == 0: GAMS_OK.
 * gams_gpu_last_stage_ms then reports four stages: upload (the members and the block table), tables (per block, the
 * header into a decode table), decode (per block: chunks decoded by one lane each into LDS, then the bases, the plane
 * and the block's raw CRC-32), join (per ctg: the CRC-32 against the trailer, the status bytes back). */
int gams_seqset_upload_gz(gams_gpu_t *h, gams_seqset_t *s, uint32_t first, uint32_t count, const uint8_t *const *members,
                          const uint64_t *member_bytes, uint8_t *status, uint32_t *n_foreign);

#ifdef __cplusplus
}
#endif
#endif
