// gams_host.hpp -- C++17 host side of the hot path, above the C ABI (include/gams_gpu.h).
//
// The reference's host is Rust; no Rust toolchain exists in this image, so the host layer that
// a Rust build would keep is written in C++ against the same extern "C" boundary.  It mirrors
// the reference's seam fn(&Ctg, &ArgMatches) -> String (src/libs/utils.rs:216-220) for
//   wave::proc_ctg   src/cmd_gams/wave.rs:121-215  (+ merge_ints :217-252)
//   sw::proc_ctg     src/cmd_gams/sw.rs:108-194    (+ Sw Display, src/libs/data.rs:58-83)
//   locate loop      src/cmd_gams/locate.rs:111-141
//   anno loop        src/cmd_gams/anno.rs:95-142
// Everything numeric runs on the GPU through libgams_gpu.so; this layer only keeps the
// reference's bookkeeping: range grammar, peak merging, TSV text.
#pragma once

#include <cstdint>
#include <functional>
#include <map>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/gams_gpu.h"

namespace gams {

// src/libs/data.rs:5-14
struct Ctg {
    std::string id;      // "ctg:{chr}:{serial}"
    std::string range;   // "{chr}:{start}-{end}"
    std::string chr_id;
    int32_t chr_start = 0, chr_end = 0;
    std::string chr_strand = "+";
    int32_t length = 0;
};

// src/libs/data.rs:16-22 (only what sw needs)
struct Feature {
    std::string id;      // "feature:{ctg_id}:{serial}"
    int32_t start = 0, end = 0;
};

// intspan::Range (chr(strand):start-end)
struct Range {
    std::string name, chr, strand;
    int32_t start = 0, end = 0;
    bool valid = false;
    static Range from_str(const std::string &s);
    std::string to_string() const;
};

// Rust `{}` for f32: shortest round-trip digits, positional
std::string fmt_f32(float v);
// IntSpan::runlist of one span
std::string runlist(int64_t s, int64_t e);

struct WaveArgs {          // defaults of src/cmd_gams/wave.rs:23-99
    int32_t size = 100, step = 10;
    uint32_t lag = 100;
    float threshold = 3.0f, influence = 1.0f, coverage = 0.2f;
    bool signal = false;
};

struct SwArgs {            // defaults of src/cmd_gams/sw.rs:9-85
    int32_t size = 100, max = 20, resize = 500;
    uint32_t actions = GAMS_SW_GC;   // --action (sw.rs:28-32): GAMS_SW_GC | GAMS_SW_COUNT
};

class Error : public std::runtime_error {
public:
    int code;
    Error(int c, const std::string &m) : std::runtime_error(m), code(c) {}
};

// Where the time of one wave_proc_ctgs* call went, in ms (added to, so a caller may sum several calls).  With
// `sync` set the device is drained at every stage boundary, so each interval belongs to the stage just
// queued (a breakdown run: slower than the pipelined call, whose only host waits are in peaks); without it
// the slots hold host time between checkpoints and only total_ms means much.
struct WaveStages {
    bool sync = false;
    unsigned threads = 0;          // inflate workers used (gz form)
    uint64_t peaks = 0;            // signalled windows fetched
    bool plane_input = false;      // the pass read the seqset's 1-bit G/C plane, not its bytes (gams_wave_plan_last_input)
    bool device_text = false;      // the rows came as text from the device (gams_wave_rows_* / gams_wave_signal_text)
    double inflate_upload_ms = 0;  // gz form: seq: values -> bases in a page-locked image -> HBM (overlapped)
    double upload_ms = 0;          // buffer form: host buffers -> HBM (gams_seqset_upload_all)
    double plan_ms = 0, kernel_ms = 0, peaks_ms = 0, format_ms = 0, total_ms = 0;
};

// wave.rs:121-215 for a batch of ctgs in ONE device pass; returns one String per ctg.  Parameters of the library's
// tiled fast kernels (every BASELINE configuration): the workers classify the buffers into the 1-bit G/C plane and
// only the plane is uploaded; a plan that needs the bytes after all gets them (gams_seqset_upload_all), as before.
std::vector<std::string> wave_proc_ctgs(gams_gpu_t *h, const std::vector<Ctg> &ctgs,
                                        const std::vector<const uint8_t *> &seqs, const WaveArgs &a,
                                        WaveStages *stages = nullptr);
// The same from the `seq:{ctg}` values as the store holds them (gzip members, redis.rs:149-161):
// blobs[i] / blob_len[i] = the value of ctgs[i], which must inflate to exactly ctgs[i].length bases.
// `threads` workers inflate one ctg at a time each (the reference gunzips inside its --parallel workers,
// wave.rs:288-299 -> redis.rs:142-161) straight into a page-locked image of the device buffer, and the
// finished stretches go to the DMA engine while the rest still inflates.  threads == 0: 16.  With parameters of
// the tiled fast kernels each worker also classifies the ctg it has just inflated, and the stretches that go to
// the device are the G/C plane's, not the bytes'.
std::vector<std::string> wave_proc_ctgs_gz(gams_gpu_t *h, const std::vector<Ctg> &ctgs,
                                           const std::vector<const uint8_t *> &blobs, const std::vector<uint64_t> &blob_len,
                                           const WaveArgs &a, unsigned threads = 0, WaveStages *stages = nullptr);
// The same values through the device inflater: the seqset is filled by seqset_upload_gz (below) -- indexed members are
// uploaded as they are and inflated on the device, anything else is inflated here on `threads` threads and uploaded --
// and the pass runs over the resident seqset.  inflate_upload_ms covers the filling.
std::vector<std::string> wave_proc_ctgs_gz_device(gams_gpu_t *h, const std::vector<Ctg> &ctgs,
                                                  const std::vector<const uint8_t *> &blobs, const std::vector<uint64_t> &blob_len,
                                                  const WaveArgs &a, unsigned threads = 0, WaveStages *stages = nullptr);
std::string wave_proc_ctg(gams_gpu_t *h, const Ctg &ctg, const uint8_t *seq, const WaveArgs &a);
// The multi-GPU form: ctgs are split over the handles by longest-
// processing-time-first on their window counts, one host thread per handle, each thread walks
// its share in batches of at most `batch_bytes` bases (upload of batch k+1 overlaps the kernel
// of batch k).  No device talks to another; the per-ctg Strings come back in ctg order.
std::vector<std::string> wave_proc_ctgs_multi(const std::vector<gams_gpu_t *> &handles, const std::vector<Ctg> &ctgs,
                                              const std::vector<const uint8_t *> &seqs, const WaveArgs &a,
                                              uint64_t batch_bytes = 1ull << 30);
// longest-processing-time-first assignment (weights -> owner per item); ties by index
std::vector<uint32_t> lpt_assign(const std::vector<uint64_t> &weights, uint32_t n_owners);
// merge_ints (wave.rs:217-252) over the ascending window indices of one sign of one ctg: the merged
// component's chromosome span per window, and whether the window has any edge (is printed as "(+)").
void merge_windows(const uint32_t *w, size_t n, int32_t chr_start, int32_t size, int32_t step, float coverage,
                   int64_t *cmin, int64_t *cmax, char *in_graph);

// `locate --count` / `anno` over several devices: the groups (ctgs, or chromosomes of
// the runlist set) are split over the handles by longest-processing-time-first on their interval
// counts, every query is routed to the device that owns its group (a counting sort on the host:
// the only "exchange step" of the path), one host thread per handle runs its share, and the
// results scatter back to the query order.  Same arguments as gams_gpu_count / gams_gpu_cover with
// the index given as arrays; queries of unknown groups (>= n_groups) get 0.
void count_multi(const std::vector<gams_gpu_t *> &handles, uint32_t n_groups, const uint64_t *group_off,
                 const uint32_t *starts, const uint32_t *stops, const uint32_t *q_group, const uint32_t *qs,
                 const uint32_t *qe, uint64_t nq, int32_t *count);
void cover_multi(const std::vector<gams_gpu_t *> &handles, uint32_t n_groups, const uint64_t *group_off,
                 const int32_t *lo, const int32_t *hi, const uint32_t *q_group, const int32_t *clip_lo,
                 const int32_t *clip_hi, const int32_t *qs, const int32_t *qe, uint64_t nq, float *prop);

// the bytes of one input file of a load that takes several (`gams rg f1 f2 ...`): not NUL-terminated
using FileBytes = std::pair<const char *, size_t>;

// sw.rs:108-194.  With GAMS_SW_COUNT in a.actions, `rgs` (what read_range returns: the rg ranges of each ctg id) is
// the idx:rg: source; each call builds the device index of its own ctgs once.  A ctg without an entry in `rgs` counts
// 0 and is reported once on stderr ("{ctg} not found in idx", utils.rs:30 -- the reference says it once per window).
// Instead of `rgs` the three operators take the bytes of ONE rg file (rg_bytes != NULL, rg_n bytes): a Locator over the
// call's ctgs loads it on the device (Locator::set_rg_index_text), and a ctg with features and no bucket in the file is
// reported the same way.  Giving both sources is GAMS_EINVAL.  The file is located among the ctgs of the CALL: sw_proc_ctg
// sees one ctg, so a range that spans a ctg boundary, which the whole table gives to the ctg in front, lands in this
// ctg's bucket (and may be the line drop-first swallows); a host whose ranges can cross ctgs calls sw_proc_ctgs /
// sw_proc_ctgs_multi with every ctg, or keeps `rgs` from a read_range over the whole table.
// Several rg files loaded one after another (`gams rg f1 f2 ...`) are given as rg_files, a third form of the same source
// (Locator::set_rg_index_text over several files), for these operators and for sw_text.
std::string sw_proc_ctg(gams_gpu_t *h, const Ctg &ctg, const uint8_t *seq, const std::vector<Feature> &features,
                        const SwArgs &a, const std::map<std::string, std::vector<Range>> *rgs = nullptr,
                        const char *rg_bytes = nullptr, size_t rg_n = 0, const std::vector<FileBytes> *rg_files = nullptr);
// several ctgs on one handle: one seqset, one gams_gpu_sw_batch call and one readback per batch of
// <= batch_bytes bases; rows returned per ctg in the order given ("" for a ctg without features).
// index_ms (may be NULL) receives the ms of the rg index build (-a count).
std::vector<std::string> sw_proc_ctgs(gams_gpu_t *h, const std::vector<Ctg> &ctgs, const std::vector<const uint8_t *> &seqs,
                                      const std::vector<std::vector<Feature>> &features, const SwArgs &a,
                                      uint64_t batch_bytes = 256ull << 20,
                                      const std::map<std::string, std::vector<Range>> *rgs = nullptr,
                                      double *index_ms = nullptr, const char *rg_bytes = nullptr, size_t rg_n = 0,
                                      const std::vector<FileBytes> *rg_files = nullptr);
// `gams sw --parallel` over several devices: ctgs split over the handles by LPT on their feature
// counts, one host thread per handle, rows returned per ctg in the order given.  Each handle indexes the rgs of the
// ctgs it was given; index_ms = the longest of those builds.  With rg_bytes every handle loads the file against ALL ctgs
// of the call (a range is located among all of them, whichever handle owns its ctg).
std::vector<std::string> sw_proc_ctgs_multi(const std::vector<gams_gpu_t *> &handles, const std::vector<Ctg> &ctgs,
                                            const std::vector<const uint8_t *> &seqs,
                                            const std::vector<std::vector<Feature>> &features, const SwArgs &a,
                                            const std::map<std::string, std::vector<Range>> *rgs = nullptr,
                                            double *index_ms = nullptr, const char *rg_bytes = nullptr, size_t rg_n = 0,
                                            const std::vector<FileBytes> *rg_files = nullptr);

// sw_proc_ctgs with the nearest-neighbour ΔG (delta_g.rs) of every window as a tenth field, `{:.4}` and empty for None
// (DESIGN.md 3.3e): gams_gpu_sw_text_dg over the same batching, on one handle.  The column is this project's own: upstream
// declares `--action gibbs` and never fills it.  table: the terms (gams_dg_table).  resident, where given, is a seqset
// that holds the ctgs' bases already -- ctg i in slot slots[i] (NULL: slot i) -- and `seqs` is not read; every ctg then
// goes in one batch.  Where the device text refuses (GAMS_EUNSUPPORTED) the rows are formatted here, the column from
// gams_gpu_sw_dg_batch.
struct SwGibbs {
    const gams_dg_table_t *table = nullptr;
    gams_seqset_t *resident = nullptr;
    const uint32_t *slots = nullptr;
};
std::vector<std::string> sw_gibbs_proc_ctgs(gams_gpu_t *h, const std::vector<Ctg> &ctgs, const std::vector<const uint8_t *> &seqs,
                                            const std::vector<std::vector<Feature>> &features, const SwArgs &a,
                                            const SwGibbs &gb, uint64_t batch_bytes = 256ull << 20,
                                            const std::map<std::string, std::vector<Range>> *rgs = nullptr,
                                            const char *rg_bytes = nullptr, size_t rg_n = 0);
inline std::string sw_gibbs_header() {
    return "id\trange\ttype\tdistance\tgc_content\tgc_mean\tgc_stddev\tgc_cv\trg_count\tgibbs\n";
}
// the ΔG column's text: `{:.4}` of an f32 below 2^20 in size (gams_fmt_dg4); "" for anything else
std::string fmt_dg4(float v);

// what read_range_text returns: the buckets of read_range as arrays.  Bucket k belongs to ctg ids[k] (ctg-id order, the
// order of the reference's BTreeMap; a ctg with one located line has a bucket, and it is empty) and holds
// start/end/line[off[k] .. off[k+1]) in file order; line = the 0-based line number of the range in the file.
struct RangeBuckets {
    std::vector<std::string> ids;
    std::vector<uint64_t> off;            // ids.size() + 1
    std::vector<int32_t> start, end;
    std::vector<uint32_t> line;
};

struct LoaderText;

// idx:ctg: / idx:rg: on the device (redis.rs:236-324) + the locate loop (locate.rs:111-141)
class Locator {
public:
    Locator(gams_gpu_t *h, const std::vector<Ctg> &ctgs);
    ~Locator();
    // idx:rg:{ctg}: ranges already bucketed per ctg (rg loader, utils.rs:39-67)
    void set_rg_index(const std::map<std::string, std::vector<Range>> &rg_of_ctg);
    // idx:rg: from the bytes of ONE rg file, made on the device (gams_index_create_range_text): what
    // set_rg_index(read_range(*this, text_lines(bytes, n))) builds, which is also what runs where the device refuses
    // (GAMS_EUNSUPPORTED); *device (may be NULL) says which path built the index.  Only ctgs with a located line get a
    // group, as in the reference's map.
    void set_rg_index_text(const char *bytes, size_t n, bool *device = nullptr);
    // ... from several rg files loaded one after another, as `gams rg f1 f2 ...` loads them (rg.rs:40): drop-first is per
    // file, a ctg's ranges from all files share its group (gams_index_create_range_files).  Where the device refuses,
    // read_range runs per file and the buckets are appended.
    void set_rg_index_text(const std::vector<FileBytes> &files, bool *device = nullptr);
    // the rg index (NULL before one is set; owned by the Locator) and the group of a ctg id in it (UINT32_MAX: none)
    gams_index_t *rg_index() const { return rg_ix_; }
    uint32_t rg_group_of(const std::string &ctg_id) const;
    // find_one_idx for every range; "" when not located (utils.rs:7-22)
    std::vector<std::string> find(const std::vector<Range> &rgs);
    // locate output: "{rg}\t{ctg_id}\n" or with count "{rg}\t{count}\n" (locate.rs:135-140)
    std::string locate(const std::vector<std::string> &rgs, bool is_count);
    // locate -f / --count over the bytes of the input file (locate.rs:84-141): the same text as locate() of the
    // lines' first fields, made on the device (gams_gpu_locate_text / gams_gpu_count_text).  Where the device
    // refuses (GAMS_EUNSUPPORTED) the bytes are split into lines (text_lines) and locate() runs; *device (may be
    // NULL) says which path made the rows.
    std::string locate_text(const char *bytes, size_t n, bool is_count, bool *device = nullptr);
    // the device name tables of locate_text (chromosome -> group, ctg slot -> id), built once; locate_text calls it
    void text_tables();
    // locate --seq (locate.rs:124-134): ">{rg}\n{bases}\n"; seq_of maps ctg id -> gunzipped seq
    std::string locate_seq(const std::vector<std::string> &rgs, const std::map<std::string, std::string> &seq_of);
    // locate --seq over the bytes of a range file and a resident seqset (a host that has the ctgs from gen_text, or has
    // just run `wave` from these bases): the text of locate_seq() of the lines' first fields, copied on the device
    // (gams_gpu_locate_seq_text); the sequence bytes are not interpreted.  slots[i] = the seqset slot that holds the
    // i-th ctg given to the constructor, UINT32_MAX if none does (a line located to such a ctg is an error).  Where the
    // device refuses (GAMS_EUNSUPPORTED) the lines are cut at their first tab as locate_text cuts them, the ctgs they
    // are located to come back through gams_seqset_download and locate_seq() runs (that path checks a slot's index, not
    // its length, which the host cannot see); *device as in locate_text.
    std::string locate_seq_text(const char *bytes, size_t n, gams_seqset_t *seqset, const std::vector<uint32_t> &slots,
                                bool *device = nullptr);
    // ... seqs[i] = the bases of the i-th ctg given to the constructor: one seqset is built and uploaded for the call
    std::string locate_seq_text(const char *bytes, size_t n, const std::vector<const uint8_t *> &seqs, bool *device = nullptr);
    const Ctg *ctg(const std::string &id) const;
    friend RangeBuckets read_range_text(Locator &loc, const char *bytes, size_t n, bool *device);
    friend LoaderText loader_text(gams_gpu_t *h, const std::vector<Ctg> &ctgs, const std::vector<FileBytes> &files, int kind,
                                  const std::string &tag, int format, const std::map<std::string, int32_t> &serial_base,
                                  bool *device);
    friend struct PeakSetup;                      // what peak_text and peak_records_text set up once (gams_host.cpp)
    friend struct SwSetup;                       // what sw_text and sw_summary set up once (gams_host.cpp)
    friend std::string sw_text(gams_gpu_t *h, const std::vector<Ctg> &ctgs, gams_seqset_t *seqset,
                               const std::vector<uint32_t> &slots, const char *bytes, size_t n, const SwArgs &a,
                               const std::map<std::string, std::vector<Range>> *rgs, const char *rg_bytes, size_t rg_n,
                               bool *device, const std::function<char *(size_t)> *sink, const std::vector<FileBytes> *rg_files);

private:
    gams_gpu_t *h_;
    std::vector<Ctg> ctgs_;                       // in index order
    std::map<std::string, uint32_t> chr_group_;   // chr -> group of the ctg index
    std::map<std::string, uint32_t> ctg_slot_;    // ctg id -> position in ctgs_
    std::vector<uint32_t> given_;                 // the i-th ctg given to the constructor -> position in ctgs_
    gams_index_t *ctg_ix_ = nullptr;
    gams_index_t *rg_ix_ = nullptr;
    std::map<std::string, uint32_t> rg_group_;    // ctg id -> group of the rg index
    gams_names_t *chr_names_ = nullptr;           // chr_group_ as a device table
    gams_names_t *ctg_ids_ = nullptr;             // ctgs_[i].id
};

class Locator;

// src/libs/redis.rs:149-161: the `seq:` values are gzip members (flate2, Compression::fast)
std::string decode_gz(const uint8_t *bytes, size_t n);
// ... into caller memory (at most cap bytes; more is an error); returns the bytes written
size_t decode_gz_into(const uint8_t *bytes, size_t n, uint8_t *dst, size_t cap);
// a batch of values on `threads` host threads (0: 16), one value per worker at a time
std::vector<std::string> decode_gz_many(const std::vector<const uint8_t *> &blobs, const std::vector<uint64_t> &blob_len,
                                        unsigned threads = 0);
std::string encode_gz(const uint8_t *bytes, size_t n);
// the same value as a literal-only member (gams_seq_gz_host): what the device writes for these bases, for hosts that
// hold them; any gzip reader, decode_gz included, inflates it
// (indexed: the member with its chunk index in the FEXTRA field, gams_seq_gz_host_indexed, which the device inflates)
std::string encode_gz_fast(const uint8_t *bytes, size_t n, bool indexed = false);
// an indexed member inflated by the host twin of the device inflater (gams_seq_gunzip_host); anything else is an Error
std::string decode_gz_indexed(const uint8_t *bytes, size_t n);
// Slots first .. first + blobs.size() of a seqset from their `seq:` values: the device first (gams_seqset_upload_gz);
// every value it leaves FOREIGN is inflated here (decode_gz_into, `threads` threads, 0: 16) and uploaded
// (gams_seqset_upload); slot_len[i] is the length of slot first + i.  A value the host's inflate refuses too, or that
// does not hold its slot's bases, is the Error.
struct UploadGz {
    uint32_t device = 0, host = 0;   // how many went each way
};
UploadGz seqset_upload_gz(gams_gpu_t *h, gams_seqset_t *seqset, uint32_t first, const std::vector<const uint8_t *> &blobs,
                          const std::vector<uint64_t> &blob_len, const std::vector<uint32_t> &slot_len, unsigned threads = 0);
// The `seq:` values of slots first .. first + count of a resident seqset, deflated on the device (gams_gpu_seq_gz): the
// members back to back, or with ctg_ids (one per slot) the `SET seq:{id} {member}` stream of redis.rs:137-140; the bytes
// of slot first + i are bytes[off[i] .. off[i + 1]).
struct SeqGz {
    std::string bytes;
    std::vector<uint64_t> off;
};
// (indexed: GAMS_SEQ_GZ_INDEXED)
SeqGz seq_gz(gams_gpu_t *h, gams_seqset_t *seqset, uint32_t first, uint32_t count,
             const std::vector<std::string> *ctg_ids = nullptr, bool indexed = false);

// src/libs/utils.rs:39-67 read_range: locate every valid range and bucket it by ctg, INCLUDING
// the reference's quirk: `.entry(k).and_modify(push).or_default()` only creates the bucket for
// the first range of a ctg, so that range is dropped (tests/cli.rs:250,301: 79 lines -> 69).
std::map<std::string, std::vector<Range>> read_range(Locator &loc, const std::vector<std::string> &lines);
// the same over the bytes of the file, bucketed on the device (gams_gpu_read_range_text), for hosts that need the
// records themselves; where the device refuses, the lines are parsed and bucketed here.  *device as in locate_text.
RangeBuckets read_range_text(Locator &loc, const char *bytes, size_t n, bool *device = nullptr);

// src/libs/data.rs:30-43
struct Peak {
    std::string id, range, signal;
    int32_t length = 0;
    float gc = 0.0f;
    int32_t left_wave_length = 0, right_wave_length = 0;
    float left_amplitude = 0.0f, right_amplitude = 0.0f;
    std::string left_signal, right_signal;
};
// src/libs/utils.rs:83-116 read_peak: rows of a wave TSV (range \t gc \t signal) bucketed by ctg,
// strand stripped, with the same drop-first-per-ctg quirk as read_range; header / invalid rows skipped.
std::map<std::string, std::vector<std::pair<Range, std::string>>> read_peak(Locator &loc,
                                                                          const std::vector<std::string> &lines);
// src/cmd_gams/peak.rs:47-158 for one ctg: gc of every peak range (device), then the left /
// right wavelength, amplitude and neighbour signal.  Serials start at 1 (a fresh cnt:peak:).
std::vector<Peak> peak_records(gams_gpu_t *h, const Ctg &ctg, const uint8_t *seq,
                               const std::vector<std::pair<Range, std::string>> &peaks);
// the same for several ctgs on one handle: one seqset and ONE gams_gpu_range_gc_batch call per batch of
// <= batch_bytes bases; out[c] = the Peak records of ctgs[c]
std::vector<std::vector<Peak>> peak_records_batch(gams_gpu_t *h, const std::vector<Ctg> &ctgs,
                                                  const std::vector<const uint8_t *> &seqs,
                                                  const std::vector<std::vector<std::pair<Range, std::string>>> &peaks,
                                                  uint64_t batch_bytes = 256ull << 20);

// the TSV rows `gams peak` prints for these records: the eleven fields of Peak, tab-separated, floats as `{}`
std::string peak_rows(const std::vector<Peak> &recs);
// `gams peak` over the bytes of one wave TSV (utils.rs:83-116, peak.rs:41-160): the rows of every ctg, the ctgs in id
// order (the reference's BTreeMap), made on the device (gams_gpu_peak_text) from the bytes to the text.  Unlike
// read_peak + peak_records_batch, which take the bucket order as given, the kept peaks of a ctg are sorted by start
// (stably) before they are numbered, as peak.rs:49 does.  seqs[i] = the bases of ctgs[i]: one seqset is built and
// uploaded for the call.  Where the device refuses (GAMS_EUNSUPPORTED) the lines go through read_peak, the same
// sort, the gc of the ranges (gams_gpu_range_gc_batch) and peak_rows; *device as in Locator::locate_text.
std::string peak_text(gams_gpu_t *h, const std::vector<Ctg> &ctgs, const std::vector<const uint8_t *> &seqs,
                      const char *bytes, size_t n, bool *device = nullptr);
// ... on a resident seqset (a host that has just run `wave` from these bases): slots[i] = the seqset slot that holds
// ctgs[i], UINT32_MAX if none does (peaks in such a ctg are an error)
std::string peak_text(gams_gpu_t *h, const std::vector<Ctg> &ctgs, gams_seqset_t *seqset,
                      const std::vector<uint32_t> &slots, const char *bytes, size_t n, bool *device = nullptr);

// What `gams peak` stores, not prints (peak.rs:68-78,163-171: SET peak:{ctg_id}:{serial} serde_json(Peak)): the records of
// every ctg as text in `format` (GAMS_LOADER_TSV: the rows of peak_text; GAMS_LOADER_RECORDS: "{id}\t{json}\n";
// GAMS_LOADER_RESP: wire::resp_command({"SET", id, json})), the ctgs in id order, made on the device
// (gams_gpu_peak_records_text).  serial_base[ctg id] is cnt:peak:{ctg} before the load (absent: 0): the k-th kept peak of
// a ctg in sorted order gets base + k; serial_next holds the counter of every ctg of the call afterwards.  Where the
// device refuses (GAMS_EUNSUPPORTED: a control byte in a name or signal) the host's passes of peak_text run and
// peak_records_rows formats; *device says which.  seqs / (seqset, slots) as for peak_text.
struct PeakRecords {
    std::string text;
    std::map<std::string, int32_t> serial_next;
};
PeakRecords peak_records_text(gams_gpu_t *h, const std::vector<Ctg> &ctgs, const std::vector<const uint8_t *> &seqs,
                              const char *bytes, size_t n, int format, const std::map<std::string, int32_t> &serial_base = {},
                              bool *device = nullptr);
PeakRecords peak_records_text(gams_gpu_t *h, const std::vector<Ctg> &ctgs, gams_seqset_t *seqset,
                              const std::vector<uint32_t> &slots, const char *bytes, size_t n, int format,
                              const std::map<std::string, int32_t> &serial_base = {}, bool *device = nullptr);
// the host formatter of that route: the records as they stand (ids and all) in `format`
std::string peak_records_rows(const std::vector<Peak> &recs, int format);
// serde_json::to_string of one Peak (data.rs:30-43): field order, no spaces, strings through json_escape_serde, floats
// through fmt_f32_json
std::string peak_json(const Peak &p);
// a JSON string's contents as serde_json writes them: '"' and '\' behind a backslash, \b \t \n \f \r, every other byte
// below 0x20 as \u00xx in lower-case hex
std::string json_escape_serde(const std::string &v);

// `gams feature` + `gams sw` over the bytes of one range file (feature.rs:50-54 read_range, feature.rs:74-86 ids,
// sw.rs:132-191 rows): the rows of every ctg, the ctgs in id order (sw.rs:97), made on the device from the bytes to the
// text (gams_gpu_sw_feature_text).  The features are those feature_records would store: the kept lines of a ctg in file
// order, "feature:{ctg_id}:{k}" from 1.  seqs[i] = the bases of ctgs[i]: one seqset is built and uploaded for the call
// (nothing goes up without GAMS_SW_GC in a.actions).  The idx:rg: source of GAMS_SW_COUNT is `rgs` or the bytes of one rg
// file, as for sw_proc_ctgs (located among the ctgs of the call; both is GAMS_EINVAL).  Where the device refuses
// (GAMS_EUNSUPPORTED) the lines go through read_range, the ids are made here and gams_gpu_sw_text_actions runs on the
// same seqset: the text is the same; *device as in Locator::locate_text.
// With `sink` the rows go to the memory (*sink)(n) hands out -- it is called once, with the bytes of all rows -- and the
// string returned is empty: the device path copies the slices there with a few threads, each touching its own pages first
// (313 MB of rows into one fresh std::string cost one thread more than everything else in the call).
using TextSink = std::function<char *(size_t)>;
std::string sw_text(gams_gpu_t *h, const std::vector<Ctg> &ctgs, const std::vector<const uint8_t *> &seqs, const char *bytes,
                    size_t n, const SwArgs &a, const std::map<std::string, std::vector<Range>> *rgs = nullptr,
                    const char *rg_bytes = nullptr, size_t rg_n = 0, bool *device = nullptr, const TextSink *sink = nullptr,
                    const std::vector<FileBytes> *rg_files = nullptr);
// ... on a resident seqset (a host that holds the seqset of gen_text): slots[i] = the seqset slot that holds ctgs[i],
// UINT32_MAX if none does (features in such a ctg are an error under GAMS_SW_GC).  Without GAMS_SW_GC seqset may be NULL
// (slots is then not looked at).
std::string sw_text(gams_gpu_t *h, const std::vector<Ctg> &ctgs, gams_seqset_t *seqset, const std::vector<uint32_t> &slots,
                    const char *bytes, size_t n, const SwArgs &a, const std::map<std::string, std::vector<Range>> *rgs = nullptr,
                    const char *rg_bytes = nullptr, size_t rg_n = 0, bool *device = nullptr, const TextSink *sink = nullptr,
                    const std::vector<FileBytes> *rg_files = nullptr);

// The table the sw rows are loaded for (templates/dql/fsw-distance.tera.sql, fsw-distance-tag.tera.sql):
// per distance -- per (tag, distance) with tags -- the average of the four statistics, of rg_count, and the rows, kept as
// the exact integers of GAMS_SW_SUMMARY_WORDS (include/gams_gpu.h): group (t, d) at words[(t * (max + 1) + d) * 10 ..).
struct SwSummaryTable {
    int32_t max = 0;
    uint32_t actions = 0;
    std::vector<std::string> tags;        // the distinct tags in byte order, one slot each; empty: no tags, one slot
    std::vector<uint64_t> words;
    // the Prop columns (AVG_{prefix}Prop, one per span set, in the order given): prop[(t * (max + 1) + d) * n + a] = P_a,
    // the sum over the group's rows of the q that `gams anno` prints as q / 10^4 for set a; both empty without sets
    std::vector<std::string> prefixes;
    std::vector<uint64_t> prop;
    // the header and one line per group with COUNT > 0, ordered by tag bytes, then distance; an average is S / COUNT to
    // the nearest integer, ties to even, printed as q / 10^4 without trailing zeros; `nan` where a row's statistic was NaN.
    // The Prop columns stand behind AVG_gc_cv (the SQL's order), in front of AVG_rg_count and COUNT.
    std::string text() const;
};
std::string sw_summary_header(uint32_t actions, bool tagged, const std::vector<std::string> &prefixes = {});
// the q of a prop in [0, 1]: `{:.4}` prints q / 10^4 (csrc/text_fmt.hpp); GAMS_EINVAL outside
uint32_t prop4_units(float p);
// n rows (and, under GAMS_SW_COUNT, their counts) added into `table`, (max + 1) groups: the host's summariser, which runs
// where the device refuses.  A statistic of 1000 or more adds the integer nearest to v * 10^4; GAMS_EINVAL for a distance
// outside [0, max], GAMS_EUNSUPPORTED for a negative or infinite statistic.
// With n_props columns of Prop units (props[a][r] = q of row r against set a, at most 10000) they are added into
// prop_table, (max + 1) x n_props words, group-major.
void sw_summarise_rows(const gams_sw_row_t *rows, const int32_t *counts, uint64_t n, int32_t max, uint32_t actions,
                       uint64_t *table, uint32_t n_props = 0, const uint32_t *const *props = nullptr,
                       uint64_t *prop_table = nullptr);
// `gams feature` + `gams sw` + the summary over the bytes of one or several range files, files[f] under (*tags)[f] (tags
// NULL: no tag column): per file gams_gpu_sw_feature_summary into one accumulator on the device -- no row leaves it -- and
// one read-back of the integers.  Drop-first is per file.  seqs, seqset, slots, rgs, rg_files as for sw_text.  Where the
// device refuses a file (GAMS_EUNSUPPORTED) its lines go through read_range and, with GAMS_SW_GC, the rows of
// gams_gpu_sw_batch through sw_summarise_rows (without it through gams_gpu_sw_summary_batch); *device (may be NULL):
// every file took the device's route.
// anno (may be NULL): the span sets of the Prop columns, each under the prefix of its column (upstream: the file stem of the
// runlist JSON up to its first '.'), at most GAMS_SW_SUMMARY_MAX_ANNO; a set is built once (AnnoSet, either route) and shared
// by the calls.  The join is made on the device with the rows (gams_gpu_sw_feature_summary_anno); where the device refuses
// a file, the rows of gams_gpu_sw_batch go through gams_gpu_cover once per set and prop4_units here.  With sets, a ctg id
// that `gams anno` would not find whole in a row's id (utils.rs:118-129: ctg:[A-Za-z0-9_]+:\d+) is GAMS_EINVAL: upstream
// drops such rows from the table, which is not emulated.
class AnnoSet;
struct SwAnnoCol {
    std::string prefix;
    const AnnoSet *set;
};
SwSummaryTable sw_summary(gams_gpu_t *h, const std::vector<Ctg> &ctgs, const std::vector<const uint8_t *> &seqs,
                          const std::vector<FileBytes> &files, const std::vector<std::string> *tags, const SwArgs &a,
                          const std::map<std::string, std::vector<Range>> *rgs = nullptr,
                          const std::vector<FileBytes> *rg_files = nullptr, bool *device = nullptr,
                          const std::vector<SwAnnoCol> *anno = nullptr);
SwSummaryTable sw_summary(gams_gpu_t *h, const std::vector<Ctg> &ctgs, gams_seqset_t *seqset, const std::vector<uint32_t> &slots,
                          const std::vector<FileBytes> &files, const std::vector<std::string> *tags, const SwArgs &a,
                          const std::map<std::string, std::vector<Range>> *rgs = nullptr,
                          const std::vector<FileBytes> *rg_files = nullptr, bool *device = nullptr,
                          const std::vector<SwAnnoCol> *anno = nullptr);

// src/cmd_gams/rg.rs:41-77 / feature.rs:47-95: the records the loaders SET, as (key, JSON) pairs in
// the reference's order (ctg id order, then file order), serials from 1 per ctg (a fresh cnt:).
// JSON text as serde_json writes the structs of src/libs/data.rs:16-28 (field order, no spaces).
struct Record {
    std::string key, json;
};
// serde_json text of a Ctg as `gen` stores it under its id (redis.rs:127-130, data.rs:5-14) and the
// reverse (redis.rs:132-135); field order and number formats as serde_json writes them.
std::string ctg_json(const Ctg &c);
Ctg ctg_from_json(const std::string &json);

// header lines the commands print in front of the per-ctg rows (wave.rs:263-266, sw.rs:204-216)
inline const char *wave_header() { return "#range\tgc_content\tsignal\n"; }
inline const char *sw_header() { return "id\trange\ttype\tdistance\tgc_content\tgc_mean\tgc_stddev\tgc_cv\trg_count\n"; }

// src/cmd_gams/tsv.rs:31-71: `gams tsv -s "ctg:*"` = a header of the struct's field names
// (data.rs:5-14, serde order) and one tab-separated row per record; ctgs in the order given.
std::string tsv_ctgs(const std::vector<Ctg> &ctgs);
// the same for "feature:*" / "rg:*" records: the JSON objects' values in field order
std::string tsv_records(const std::vector<Record> &records, bool features);
std::vector<Record> rg_records(Locator &loc, const std::vector<std::string> &lines);
std::vector<Record> feature_records(Locator &loc, const std::vector<std::string> &lines, const std::string &tag);
// ... on a store that already holds records: cnt[ctg id] is cnt:rg:{ctg} / cnt:feature:{ctg} (absent: 0); the serials of
// a ctg continue behind it and cnt is left at the counter after the load (incr_sn_n, rg.rs:63-75), ready for the next file
std::vector<Record> rg_records(Locator &loc, const std::vector<std::string> &lines, std::map<std::string, int32_t> &cnt);
std::vector<Record> feature_records(Locator &loc, const std::vector<std::string> &lines, const std::string &tag,
                                    std::map<std::string, int32_t> &cnt);

// `gams rg f1 f2 ...` (kind GAMS_LOADER_RG) / `gams feature --tag T f1 f2 ...` (GAMS_LOADER_FEATURE) over the bytes of the
// files: the records the loader would SET, as text in `format` (GAMS_LOADER_RECORDS: "{key}\t{json}\n"; GAMS_LOADER_TSV: the
// rows of tsv_records without the header; GAMS_LOADER_RESP: wire::resp_command({"SET", key, json}) of every record), in
// the reference's order: file by file, the ctgs by id, file order inside a ctg.  serial_base[ctg id] is the ctg's counter
// before the load (absent: 0).  Made on the device (gams_gpu_loader_text); where it refuses (GAMS_EUNSUPPORTED) the
// lines of every file go through rg_records / feature_records with the counters carried on; *device says which.
struct LoaderText {
    std::string text;
    std::map<std::string, int32_t> serial_next;   // the counter of every ctg of the call after the load
    std::vector<uint64_t> n_in_file;              // records per file ("There are N rgs in this file")
};
LoaderText loader_text(gams_gpu_t *h, const std::vector<Ctg> &ctgs, const std::vector<FileBytes> &files, int kind,
                       const std::string &tag, int format, const std::map<std::string, int32_t> &serial_base = {},
                       bool *device = nullptr);

// gen.rs:81-157 for one chromosome: ambiguous-base scan (device), fill, excise, --piece split;
// ctg ids "ctg:{chr}:{serial}" with serial from 1 (gen.rs:133-134).  `seq` is the whole chromosome.
struct GenArgs {            // defaults of src/cmd_gams/gen.rs:26-49
    int32_t piece = 500000, fill = 50, min = 5000;
};
std::vector<Ctg> gen_ctgs(gams_gpu_t *h, const std::string &chr_id, const uint8_t *seq, uint64_t len,
                          const GenArgs &a);

// bio::io::fasta::Reader as gen.rs:67-78 uses it, over the bytes of a file: lines split on '\n' (a last line without
// one counts); a line that begins with '>' starts a record whose id is what follows up to the first ASCII white space;
// every other line is trimmed of trailing ASCII white space and appended to the record's sequence.  No bytes: no
// records; a first byte other than '>' is GAMS_EINVAL (the reference panics: "Expected > at record start").
struct FastaRecord {
    std::string id, seq;
};
std::vector<FastaRecord> read_fasta(const char *bytes, size_t n);

// `gams gen` over the bytes of one FASTA file: the ctgs (chromosomes in file order, then serial), the chromosome
// lengths, and the resident seqset of the ctgs' bases with its G/C plane (slot k = ctgs[k]; the caller destroys it).
// Made on the device from one upload of the bytes (gams_gpu_gen_text).  Where the device refuses (GAMS_EUNSUPPORTED) the
// host passes run: read_fasta, gen_ctgs per record, gams_seqset_upload_all; a duplicate id then continues its serial
// counter and keeps its last length, as cnt:ctg:{chr} and len_of do (gen.rs:78, :133).  *device as in locate_text.
struct GenText {
    std::vector<Ctg> ctgs;
    std::vector<std::pair<std::string, uint64_t>> chr_len;   // in order of first appearance
    gams_seqset_t *seqset = nullptr;
};
GenText gen_text(gams_gpu_t *h, const char *bytes, size_t n, const GenArgs &a, bool *device = nullptr);

// anno.rs:95-142; `sets` = runlists per chr (sorted disjoint spans)
struct Runlist {
    std::vector<int32_t> lo, hi;
};
std::string anno(gams_gpu_t *h, const std::map<std::string, Runlist> &sets, const std::vector<Ctg> &ctgs,
                 const std::vector<std::string> &lines, bool header, const std::string &prefix, size_t idx_id,
                 size_t idx_range);

// anno.rs:95-142 over the bytes of one input file: the same text as anno() of its lines, made on the device
// (gams_gpu_anno_text); where the device refuses, the bytes are split into lines and anno() runs.  *device as in
// Locator::locate_text.
std::string anno_text(gams_gpu_t *h, const std::map<std::string, Runlist> &sets, const std::vector<Ctg> &ctgs,
                      const char *bytes, size_t n, bool header, const std::string &prefix, size_t idx_id,
                      size_t idx_range, bool *device = nullptr);

// The runlist JSON file `anno` loads first (anno.rs:84-87), read on the host (gams_runlist.cpp): the complete reader --
// escapes, any white space, a key that comes twice keeps its first place and its last value -- and the fallback
// behind gams_spans_create_runlist_text.  chr[g] names sets[g], in file order; every set is normalised (sorted,
// overlapping and adjacent spans joined).  GAMS_EINVAL where the reference panics: not an object, a value that is no
// string, a runlist character that is no digit / '-' / ',', a > b, a number outside i32 (and any malformed document).
struct RunlistJson {
    std::vector<std::string> chr;
    std::vector<Runlist> sets;
};
RunlistJson read_runlist_json(const char *bytes, size_t n);
// one runlist string: what the device accepts, negative numbers (-5--1) and empty tokens next to a comma
Runlist parse_runlist(const std::string &text);

// The span set of an anno run, built once from the bytes of the runlist JSON file and shared by every input file
// (anno.rs:84-87 in front of the loop at anno.rs:95): gams_spans_create_runlist_text first; where the device refuses
// (GAMS_EUNSUPPORTED), read_runlist_json and gams_spans_create.  Owns the span set and the chr name table.
class AnnoSet {
public:
    AnnoSet(gams_gpu_t *h, const char *bytes, size_t n);
    AnnoSet(gams_gpu_t *h, const std::map<std::string, Runlist> &sets);   // one group per chr, in the map's order
    ~AnnoSet();
    AnnoSet(const AnnoSet &) = delete;
    AnnoSet &operator=(const AnnoSet &) = delete;
    bool device() const { return device_; }                // the device built it from the bytes
    gams_spans_t *spans() const { return sp_; }
    const gams_names_t *chr_names() const { return names_; }
    const std::vector<std::string> &chrs() const { return chr_; }   // chrs()[g] names group g
    uint64_t n_spans() const { return n_spans_; }

private:
    void from_arrays(const std::vector<std::string> &chr, const std::vector<const Runlist *> &sets);
    gams_gpu_t *h_;
    gams_spans_t *sp_ = nullptr;
    gams_names_t *names_ = nullptr;
    std::vector<std::string> chr_;
    uint64_t n_spans_ = 0;
    bool device_ = false;
};
// anno() / anno_text() over a set built once
std::string anno(gams_gpu_t *h, const AnnoSet &set, const std::vector<Ctg> &ctgs, const std::vector<std::string> &lines,
                 bool header, const std::string &prefix, size_t idx_id, size_t idx_range);
std::string anno_text(gams_gpu_t *h, const AnnoSet &set, const std::vector<Ctg> &ctgs, const char *bytes, size_t n,
                      bool header, const std::string &prefix, size_t idx_id, size_t idx_range, bool *device = nullptr);

// BufRead::lines() of the bytes: split on '\n', one '\r' before a '\n' dropped, a last line without '\n' kept
std::vector<std::string> text_lines(const char *bytes, size_t n);
// `{:.4}` of an anno prop in [0, 1] as the device prints it (integer arithmetic, csrc/text_fmt.hpp); "" outside
std::string fmt_prop4(float p);
// `{}` of an f32 in [0, 1] as the device prints a peak amplitude (csrc/text_fmt.hpp); "" where it refuses
std::string fmt_f32_short(float v);
// an f32 as serde_json prints it (ryu: shortest round trip, always a decimal point) where that is positional: for +0 and
// for [1e-5, 1] the text of fmt_f32_short, with ".0" behind one without a point.  Anything else throws (the exponent
// form is not implemented; parity with serde_json is its documented behaviour, not pinned: DESIGN.md)
std::string fmt_f32_json(float v);

// ---- wire formats either side of the path (gams_wire.cpp; SURVEY 8 f-3, parity unpinned) ----------
namespace wire {
// bundle:ctg:{chr}: bincode 1.3.3 of BTreeMap<String, Ctg> (redis.rs:216-233)
std::string bincode_ctg_bundle(const std::vector<Ctg> &ctgs);
std::vector<Ctg> bincode_ctg_bundle_decode(const uint8_t *bytes, size_t n);
// idx:ctg:{chr} / idx:rg:{ctg}: bincode of rust-lapper's Lapper<u32, String> (redis.rs:236-324)
struct LapperIv {
    uint32_t start = 0, stop = 0;   // half-open, stop = end + 1 (redis.rs:245-248, 291-294)
    std::string val;                // ctg id for idx:ctg, "" for idx:rg
};
struct LapperBlob {
    std::vector<LapperIv> intervals;      // sorted by (start, stop)
    std::vector<uint32_t> starts, stops;  // each sorted on its own
    uint32_t max_len = 0, cov = 0;
    bool has_cov = false, overlaps_merged = false;
};
std::string bincode_lapper(const std::vector<LapperIv> &intervals);   // Lapper::new + serialize
LapperBlob bincode_lapper_decode(const uint8_t *bytes, size_t n);
// device index over decoded idx: blobs, one group per blob (caller destroys it with gams_index_destroy)
gams_index_t *index_from_lappers(gams_gpu_t *h, const std::vector<LapperBlob> &blobs);
// RESP2
struct RespValue {
    enum Type { Simple, Error, Integer, Bulk, Null, Array } type = Null;
    std::string str;
    int64_t integer = 0;
    std::vector<RespValue> array;
};
std::string resp_command(const std::vector<std::string> &args);
std::string resp_pipeline_set(const std::vector<std::pair<std::string, std::string>> &kv);
std::string resp_eval(const std::string &script, const std::vector<std::string> &keys,
                      const std::vector<std::string> &argv);
const char *scan_values_script();
// one reply from the front of `bytes`: returns the bytes consumed, 0 if the reply is not complete yet
size_t resp_parse(const char *bytes, size_t n, RespValue &out);
std::string resp_dump(const RespValue &v);
}  // namespace wire

}  // namespace gams
