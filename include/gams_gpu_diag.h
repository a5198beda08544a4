/*
 * gams_gpu_diag.h -- measurement and tuning entries of libgams_gpu.so.
 *
 * Nothing here is needed to run the path (gams_gpu.h is the binding surface); these are what
 * bench.py, tools/ and the parity tests use to time kernels, name them for rocprofv3, look inside
 * a launch and move the knobs whose defaults were chosen from such measurements.  Results never
 * depend on any of them.
 */
#ifndef GAMS_GPU_DIAG_H
#define GAMS_GPU_DIAG_H

#include "gams_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* HIP-event stopwatch on the handle's compute stream (the stream the kernels of this library
 * are launched on; plans of depth > 1 also use auxiliary streams, which stop() queues the
 * compute stream behind before it records the closing event).  stop() synchronises and returns ms. */
int gams_gpu_timer_start(gams_gpu_t *h);
int gams_gpu_timer_stop(gams_gpu_t *h, float *ms);
/* Device time (HIP events around the kernel, excluding the host<->device copies) of the last
 * gams_gpu_sw / gams_gpu_count / gams_gpu_locate / gams_gpu_cover call on this handle; after a range loader call
 * (gams_gpu_read_range_text / gams_index_create_range_text) or gams_gpu_peak_text the sum of its stages. */
int gams_gpu_last_kernel_ms(gams_gpu_t *h, float *ms);

/* The stages of the last gams_gpu_read_range_text / gams_index_create_range_text call on this handle, in ms (HIP events
 * around each): lines (upload + line index), parse, locate, first, keep, offsets, order, gather, and for the index entry
 * build.  After gams_gpu_peak_text or gams_gpu_peak_records_text, its ten: lines, parse, locate, first, keep, offsets, order, gc (gather, checks and
 * range gc), rows (row lengths and their prefix), write.  After gams_gpu_sw_feature_text, its twelve: the loader's lines ..
 * order, then gather (with the middle check), geometry (rows per feature and their prefix), rows (sw_kernel), text lengths,
 * text write (seven when no line is kept).  After gams_gpu_sw_feature_summary, its ten: the same up to rows (the
 * summarising sw_kernel and the merge into the accumulator; no text stages).  After gams_gpu_gen_text (of an input that is not empty), its
 * five: upload, pack (mark, carry, count, offsets, compact), scan, table (the host's part), place.  After
 * gams_gpu_locate_seq_text (with a located line), its six: lines, parse, locate, lengths, offsets, copy.  Writes up to cap values; *n = the stages the call ran
 * (gams_gpu_last_kernel_ms is their sum).  GAMS_ESTATE when the last timed call was none of these (or its input had
 * no line; for the peak entry: no kept peak). */
int gams_gpu_last_stage_ms(gams_gpu_t *h, float *ms, uint32_t cap, uint32_t *n);
/* The chunk of gams_gpu_locate_seq_text's copy: the bytes of text one workgroup writes, a power of two and a multiple of
 * 16 (kSeqTextChunk, seq_text_plan.hpp).  Tests place rows on the seams between chunks with it. */
uint32_t gams_gpu_locate_seq_chunk(void);

/* Tapered launches.  A launch of the headline parameters (size 100, step 10, lag 100) over at least a
 * round and a half of workgroups ends in smaller tiles (the ctgs holding the last 17 % / 8 % of the
 * windows are cut into tiles of 2/3 and 1/3 the size), so that its last workgroups are short-lived and
 * the chip drains in ~3 instead of ~10 us; the small tiles cost 3-4 % more work.  mode -1 (default):
 * on for plans of depth 1; 0: off -- what a host wants that keeps several passes in flight (plans on
 * lanes, or depth > 1): their tails overlap anyway; 1: on.  Results are identical either way. */
int gams_wave_plan_set_taper(gams_gpu_t *h, gams_wave_plan_t *plan, int mode);
/* Size of the two tails of a tapered launch, in % of a round of workgroup slots (8 per CU): the ctgs
 * holding the last pct4 % of a round are cut into the smallest tiles, the pct8 % before them into the
 * middle ones; at most 8 % / 17 % of the batch.  0..100, default 25 / 50 (profiles/r02_taper_sweep.txt). */
int gams_wave_plan_set_taper_shape(gams_gpu_t *h, gams_wave_plan_t *plan, int pct4, int pct8);
/* The plan's tile table as the tile kernel reads it, for tests: three words per tile -- the ctg, the tile's first
 * window in it, and W (4, 8 or 12 windows per thread: a tile of 256 * W - lag - 1 windows) for a tapered table, 0
 * for every other table.  *n = the tiles of the table; the first min(cap, *n) tiles are written to out, which holds
 * room for cap of them (cap 0, out NULL: only the count).  Copied from the host's table, no device work; follows
 * the plan's current settings like gams_wave_plan_kernel_name. */
int gams_wave_plan_tiles(gams_gpu_t *h, gams_wave_plan_t *plan, uint32_t *out, uint64_t cap, uint64_t *n);
/* Host threads gams_wave_run_n queues a long batch of passes from (1..4, default one per way). */
int gams_wave_plan_set_queue_threads(gams_gpu_t *h, gams_wave_plan_t *plan, uint32_t n);
/* Name of the kernel that does the plan's work, spelled as rocprofv3 --kernel-trace prints the
 * instantiation (without the namespace), e.g. "wave_fast_taper_kernel<100, 10, 100, true>": lets a
 * benchmark line name the row of the profile its launch duration must agree with.  Follows the plan's
 * current settings (set_tile / set_taper / the seqset's size).  NUL-terminated, truncated to n. */
int gams_wave_plan_kernel_name(gams_gpu_t *h, gams_wave_plan_t *plan, char *buf, size_t n);
/* influence != 1: how the selected pass reached the reference's answer -- the sweeps of guess-and-iterate it took
 * (waits for them like every reader of the pass), and whether it was handed to the one-wavefront-per-ctg recurrence
 * instead (serial = 1).  influence == 1: 0 sweeps, serial = 0. */
int gams_wave_plan_settled(gams_gpu_t *h, gams_wave_plan_t *plan, uint32_t *sweeps, int *serial);

/* Tuning/diagnostics: windows per tile (0 = library default), and how many
 * windows of the last run took the exact-order f32 re-evaluation. */
int gams_wave_plan_set_tile(gams_gpu_t *h, gams_wave_plan_t *p, uint32_t tile_windows);
/* Threads per workgroup of the step-1 tile kernels (size 100, step 1, W = 28): 64, 128 or 256, 0 = the library's
 * choice.  A tile is then 64 / 128 / 256 threads x 28 windows; other plans ignore the request.  Rebuilds the tiling
 * like gams_wave_plan_set_tile. */
int gams_wave_plan_set_threads(gams_gpu_t *h, gams_wave_plan_t *p, uint32_t threads);
int gams_wave_exact_count(gams_gpu_t *h, gams_wave_plan_t *p, uint64_t *n_exact);
/* Diagnostics of the integer decision's guard band (stat.rs:36-38 is an f32 comparison; windows
 * whose integer margin is inside the band are re-evaluated in the reference's exact f32 order).
 * safety (default 1.5, >= 1) multiplies the derived error bound; all_exact != 0 sends every window
 * down the exact path.  Results are identical for every setting -- only the share of windows that
 * take the exact path changes -- which is what the tests check.  Applies to the next run. */
int gams_wave_plan_set_guard(gams_gpu_t *h, gams_wave_plan_t *p, float safety, int all_exact);
/* Diagnostics: with stamps on, thread 0 of every workgroup records the shader clock at the
 * kernel's phase boundaries.  mean_cycles[0..5] = mean duration of load+classify, chunk
 * prefix, window counts, z-score, exact re-evaluation, outputs; [6] = whole workgroup;
 * span_cycles = first workgroup start to last workgroup end. */
int gams_wave_plan_set_stamps(gams_gpu_t *h, gams_wave_plan_t *p, int enable);
int gams_wave_stamps(gams_gpu_t *h, gams_wave_plan_t *p, double *mean_cycles /* [8] */,
                     uint64_t *span_cycles);
/* the raw stamp words: 16 per workgroup (tile), see wave_stamp() in gams_amd/csrc/wave.hip */
int gams_wave_stamps_raw(gams_gpu_t *h, gams_wave_plan_t *p, uint64_t *out, uint64_t n_words);

/* What the tiled fast kernels of a plan read: the seqset's 1-bit G/C plane when it is valid at queueing time
 * (GAMS_WAVE_INPUT_AUTO, the default), always the bytes, or always the plane -- a forced input the seqset
 * cannot serve (stale plane, plane-only seqset, a plan outside the fast kernels asked for the plane) fails
 * the run with GAMS_ESTATE.  Results are identical; for tests and A/B runs. */
#define GAMS_WAVE_INPUT_AUTO 0
#define GAMS_WAVE_INPUT_BYTES 1
#define GAMS_WAVE_INPUT_PLANE 2
int gams_wave_plan_set_input(gams_gpu_t *h, gams_wave_plan_t *p, int mode);
/* the input the plan's most recently queued pass took: GAMS_WAVE_INPUT_BYTES or GAMS_WAVE_INPUT_PLANE */
int gams_wave_plan_last_input(gams_gpu_t *h, gams_wave_plan_t *p, int *input);
/* The body the plane-fed passes of a headline plan run (size 100, step 10, lag 100, peaks only, influence 1, the
 * library's own tile and thread count, no taper).  The tile of wave_fast_kernel<12, 100, 10, 100, NT, 256> -- 3,072
 * count slots -- is also 128 threads x 24 windows: GAMS_WAVE_BODY_NARROW launches wave_fast_narrow_kernel (that is the
 * name rocprofv3 --kernel-trace prints for it; it has no template arguments) over the same tile table, with workgroups
 * of two waves; GAMS_WAVE_BODY_WIDE keeps the 256-thread kernel; GAMS_WAVE_BODY_AUTO (the default) is the library's
 * choice.  gams_wave_plan_kernel_name names the list entry the plan selected either way.  A forced NARROW on a plan
 * without that body, or on a pass that reads the bytes (stale plane, forced bytes), fails the run with GAMS_ESTATE.
 * Results are identical; for tests and A/B runs. */
#define GAMS_WAVE_BODY_AUTO 0
#define GAMS_WAVE_BODY_WIDE 1
#define GAMS_WAVE_BODY_NARROW 2
int gams_wave_plan_set_body(gams_gpu_t *h, gams_wave_plan_t *p, int mode);
/* the body the plan's most recently queued pass ran: GAMS_WAVE_BODY_WIDE (every kernel but the narrow one) or _NARROW */
int gams_wave_plan_last_body(gams_gpu_t *h, gams_wave_plan_t *p, int *body);
/* The cut of the narrow body: its tile of 3,072 count slots as 128 threads x 24 windows (GAMS_WAVE_CUT_TWO_WAVES,
 * wave_fast_narrow_kernel) or as 64 threads x 48 windows, a workgroup of one wave (GAMS_WAVE_CUT_ONE_WAVE,
 * wave_fast_onewave_kernel), over the same tile table; GAMS_WAVE_CUT_AUTO (the default) is the library's choice.
 * gams_wave_plan_last_body says NARROW for both.  A forced ONE_WAVE on a pass the narrow body cannot take (a plan
 * without it, a pass that reads the bytes) fails the run with GAMS_ESTATE, as a forced NARROW does; a pass kept on the
 * wide kernel by GAMS_WAVE_BODY_WIDE has no cut.  Results are identical; for tests and A/B runs. */
#define GAMS_WAVE_CUT_AUTO 0
#define GAMS_WAVE_CUT_TWO_WAVES 1
#define GAMS_WAVE_CUT_ONE_WAVE 2
int gams_wave_plan_set_cut(gams_gpu_t *h, gams_wave_plan_t *p, int mode);
/* the cut of the plan's most recently queued pass: GAMS_WAVE_CUT_TWO_WAVES or _ONE_WAVE when it ran the narrow body,
 * GAMS_WAVE_CUT_AUTO (0) when it did not */
int gams_wave_plan_last_cut(gams_gpu_t *h, gams_wave_plan_t *p, int *cut);
/* gams_gc_plane with the body named: the AVX2 one (GAMS_EUNSUPPORTED on a CPU without it), the portable
 * 64-bit one, or the library's choice.  Every body writes the same bytes. */
#define GAMS_GC_BODY_AUTO 0
#define GAMS_GC_BODY_PORTABLE 1
#define GAMS_GC_BODY_AVX2 2
int gams_gc_plane_with(const uint8_t *seq, uint64_t n, uint8_t *plane, int body);
/* The block size of the `seq:` members, for measuring it: gams_seq_gz_host with the input bytes per deflate block
 * named, and the size gams_gpu_seq_gz uses on this handle from now on (GAMS_SEQ_GZ_BLOCK until set).  A block size is
 * a multiple of 4096 between 4096 and 2^24 (GAMS_EINVAL otherwise).  The device entry and the host twin agree byte
 * for byte at every size. */
int gams_seq_gz_host_block(const uint8_t *seq, uint64_t n, uint32_t block, uint8_t *out, uint64_t cap, uint64_t *n_out);
int gams_gpu_seq_gz_set_block(gams_gpu_t *h, uint32_t block);
/* The same for the indexed members: the host twin with the block size named (and GAMS_SEQ_GZ_CHUNK), with block size
 * and chunk named, and the chunk gams_gpu_seq_gz writes with GAMS_SEQ_GZ_INDEXED on this handle from now on.  A chunk
 * is 512, 1024, 2048 or 4096 (GAMS_EINVAL otherwise). */
int gams_seq_gz_host_indexed_block(const uint8_t *seq, uint64_t n, uint32_t block, uint8_t *out, uint64_t cap, uint64_t *n_out);
int gams_seq_gz_host_indexed_chunk(const uint8_t *seq, uint64_t n, uint32_t block, uint32_t chunk, uint8_t *out, uint64_t cap,
                                   uint64_t *n_out);
int gams_gpu_seq_gz_set_chunk(gams_gpu_t *h, uint32_t chunk);
/* The ΔG kernel (gams_gpu_range_dg_batch and the sw entries above it) walks a range in stages of this many bases' worth of
 * aligned 16-B pieces, staged as 2-bit codes in LDS: a range crosses a stage seam every GAMS_DG_STAGE_BASES bases counted
 * from the 16-B boundary at or below its first base.  For tests that place ranges on the seams. */
#define GAMS_DG_STAGE_BASES 512
/* Where the walk finds the sixteen dimer terms: in LDS (the default) or in a register per lane, read with ds_bpermute.
 * Both give the same bits; for measuring one against the other.  GAMS_EINVAL for another value. */
#define GAMS_DG_TABLE_LDS 0
#define GAMS_DG_TABLE_BPERMUTE 1
int gams_gpu_dg_set_table(gams_gpu_t *h, int placement);

#ifdef __cplusplus
}
#endif
#endif
