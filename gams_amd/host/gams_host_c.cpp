// gams_host_c.cpp -- flat C entry points of the host layer, for tests (ctypes) and for a
// non-C++ host.  Strings returned are malloc'd: release with gams_host_free.  On error the
// functions return NULL and gams_host_last_error() has the message.
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <sstream>
#include <thread>

#include "gams_host.hpp"

namespace {
thread_local std::string g_err;
thread_local int g_code = 0;

// malloc'd copy of s with a NUL behind it; *out_len (if asked for) = its length without the NUL
char *dup(const std::string &s, uint64_t *out_len = nullptr) {
    if (out_len) *out_len = s.size();
    char *p = (char *)std::malloc(s.size() + 1);
    if (p) {
        std::memcpy(p, s.data(), s.size());
        p[s.size()] = 0;
    }
    return p;
}

// f() under the error contract of this file: the thread's last error cleared, then f's result; an exception
// leaves its message and code behind and `fail` is returned
template <typename R, typename F>
R guard(R fail, F &&f) {
    try {
        g_err.clear();
        g_code = 0;
        return f();
    } catch (const gams::Error &e) {
        g_err = e.what();
        g_code = e.code;
    } catch (const std::exception &e) {
        g_err = e.what();
        g_code = -1;
    }
    return fail;
}
// the string f() makes, as a malloc'd copy (NULL on error)
template <typename F>
char *guarded(uint64_t *out_len, F &&f) {
    return guard((char *)nullptr, [&] { return dup(f(), out_len); });
}
template <typename F>
char *guarded(F &&f) {
    return guarded(nullptr, f);
}

std::vector<gams::Ctg> make_ctgs(uint32_t n, const char *const *ids, const char *const *chrs, const int32_t *starts,
                                 const int32_t *ends) {
    std::vector<gams::Ctg> v(n);
    for (uint32_t i = 0; i < n; ++i) {
        v[i].id = ids[i];
        v[i].chr_id = chrs[i];
        v[i].chr_start = starts[i];
        v[i].chr_end = ends[i];
        v[i].length = ends[i] - starts[i] + 1;
        v[i].range = v[i].chr_id + ":" + gams::runlist(starts[i], ends[i]);
    }
    return v;
}

std::vector<std::string> split_lines(const char *text) {
    std::vector<std::string> lines;
    std::istringstream is(text ? text : "");
    std::string ln;
    while (std::getline(is, ln)) lines.push_back(ln);
    return lines;
}

gams::WaveArgs wave_args(int32_t size, int32_t step, uint32_t lag, float threshold, float influence, float coverage,
                         bool signal) {
    gams::WaveArgs a;
    a.size = size;
    a.step = step;
    a.lag = lag;
    a.threshold = threshold;
    a.influence = influence;
    a.coverage = coverage;
    a.signal = signal;
    return a;
}

// the per-ctg Strings of an operator, concatenated in ctg order
std::string join(const std::vector<std::string> &rows) {
    size_t total = 0;
    for (auto &s : rows) total += s.size();
    std::string out;
    out.reserve(total);
    for (auto &s : rows) out += s;
    return out;
}

// the first TSV column of every line
std::vector<std::string> first_cols(const char *lines) {
    std::vector<std::string> v;
    for (const std::string &ln : split_lines(lines)) v.push_back(ln.substr(0, ln.find('\t')));
    return v;
}

std::map<std::string, std::vector<gams::Range>> rg_index_of(uint32_t n, const char *const *ids, const char *rg_lines) {
    std::map<std::string, std::vector<gams::Range>> rg_of;
    for (uint32_t i = 0; i < n; ++i) rg_of[ids[i]];  // build_idx_rg visits every ctg (redis.rs:279-302)
    for (const std::string &ln : split_lines(rg_lines)) {
        size_t tab = ln.find('\t');
        if (tab == std::string::npos) continue;
        gams::Range r = gams::Range::from_str(ln.substr(tab + 1));
        if (r.valid) rg_of[ln.substr(0, tab)].push_back(r);
    }
    return rg_of;
}

// several files given as arrays of pointers and lengths (a NULL pointer with length 0 is an empty file)
std::vector<gams::FileBytes> files_of(uint32_t n, const char *const *data, const uint64_t *len) {
    std::vector<gams::FileBytes> v(n);
    for (uint32_t i = 0; i < n; ++i) v[i] = gams::FileBytes(data[i] ? data[i] : "", (size_t)len[i]);
    return v;
}

std::map<std::string, gams::Runlist> runlists_of(const char *runlists) {
    std::map<std::string, gams::Runlist> sets;
    for (const std::string &ln : split_lines(runlists)) {
        size_t tab = ln.find('\t');
        if (tab == std::string::npos) continue;
        gams::Runlist &rl = sets[ln.substr(0, tab)];
        std::istringstream is(ln.substr(tab + 1));
        std::string part;
        while (std::getline(is, part, ',')) {
            if (part.empty() || part == "-") continue;
            size_t dash = part.find('-', 1);
            int32_t lo = std::atoi(part.substr(0, dash).c_str());
            int32_t hi = dash == std::string::npos ? lo : std::atoi(part.substr(dash + 1).c_str());
            rl.lo.push_back(lo);
            rl.hi.push_back(hi);
        }
    }
    return sets;
}

gams::SwArgs sw_args(int32_t size, int32_t max, int32_t resize, uint32_t actions) {
    gams::SwArgs a;
    a.size = size;
    a.max = max;
    a.resize = resize;
    a.actions = actions;
    return a;
}
std::vector<std::vector<gams::Feature>> sw_feature_rows(uint32_t n, const char *features) {
    std::vector<std::vector<gams::Feature>> f(n);
    for (const std::string &ln : split_lines(features)) {
        std::istringstream is(ln);
        std::string ci, id, s0, s1;
        std::getline(is, ci, '\t');
        std::getline(is, id, '\t');
        std::getline(is, s0, '\t');
        std::getline(is, s1, '\t');
        f.at((size_t)std::stoul(ci)).push_back(gams::Feature{id, std::stoi(s0), std::stoi(s1)});
    }
    return f;
}
thread_local double g_sw_index_ms = 0.0;
}  // namespace

// 1 if the rows of the last gams_host_wave* / gams_host_locate_text / gams_host_anno_text of this thread came as text
// from the device, 0 if the device refused the input and the host made them
static thread_local int g_operator_device = 0;

extern "C" {

const char *gams_host_last_error() { return g_err.c_str(); }
int gams_host_last_code() { return g_code; }
void gams_host_free(void *p) { std::free(p); }

// wave.rs:121-215 over n ctgs in one device pass; the per-ctg Strings are concatenated in ctg order
char *gams_host_wave(gams_gpu_t *h, uint32_t n, const char *const *ids, const char *const *chrs,
                     const int32_t *starts, const int32_t *ends, const uint8_t *const *seqs, int32_t size,
                     int32_t step, uint32_t lag, float threshold, float influence, float coverage, int is_signal) {
    return guarded([&] {
        const gams::WaveArgs a = wave_args(size, step, lag, threshold, influence, coverage, is_signal != 0);
        std::vector<const uint8_t *> sp(seqs, seqs + n);
        gams::WaveStages st;
        std::vector<std::string> rows = gams::wave_proc_ctgs(h, make_ctgs(n, ids, chrs, starts, ends), sp, a, &st);
        g_operator_device = st.device_text ? 1 : 0;
        return join(rows);
    });
}

namespace {
// stages[0..9] = inflate_upload, upload, plan, kernel, peaks, format, total ms, threads, peaks fetched, 1 if the pass
// read the G/C plane
void put_stages(const gams::WaveStages &st, double *stages) {
    if (!stages) return;
    stages[0] = st.inflate_upload_ms;
    stages[1] = st.upload_ms;
    stages[2] = st.plan_ms;
    stages[3] = st.kernel_ms;
    stages[4] = st.peaks_ms;
    stages[5] = st.format_ms;
    stages[6] = st.total_ms;
    stages[7] = (double)st.threads;
    stages[8] = (double)st.peaks;
    stages[9] = st.plane_input ? 1.0 : 0.0;
}
}  // namespace

// gams_host_wave with the stage clock of gams::WaveStages (sync bit 0: the device is drained at every stage
// boundary; bit 1: `--signal`, a row for every window); *out_len receives the length of the text
char *gams_host_wave_timed(gams_gpu_t *h, uint32_t n, const char *const *ids, const char *const *chrs,
                           const int32_t *starts, const int32_t *ends, const uint8_t *const *seqs, int32_t size,
                           int32_t step, uint32_t lag, float threshold, float influence, float coverage, int sync,
                           double *stages, uint64_t *out_len) {
    return guarded(out_len, [&] {
        const gams::WaveArgs a = wave_args(size, step, lag, threshold, influence, coverage, (sync & 2) != 0);
        gams::WaveStages st;
        st.sync = (sync & 1) != 0;
        std::vector<const uint8_t *> sp(seqs, seqs + n);
        std::vector<std::string> rows = gams::wave_proc_ctgs(h, make_ctgs(n, ids, chrs, starts, ends), sp, a, &st);
        g_operator_device = st.device_text ? 1 : 0;
        put_stages(st, stages);
        return join(rows);
    });
}

// the same from the gzip'd `seq:` values (gams::wave_proc_ctgs_gz): blobs[i] / blob_len[i] = value of ctg i
char *gams_host_wave_gz(gams_gpu_t *h, uint32_t n, const char *const *ids, const char *const *chrs,
                        const int32_t *starts, const int32_t *ends, const uint8_t *const *blobs,
                        const uint64_t *blob_len, int32_t size, int32_t step, uint32_t lag, float threshold,
                        float influence, float coverage, uint32_t threads, int sync, double *stages, uint64_t *out_len) {
    return guarded(out_len, [&] {
        const gams::WaveArgs a = wave_args(size, step, lag, threshold, influence, coverage, false);
        gams::WaveStages st;
        st.sync = sync != 0;
        std::vector<const uint8_t *> bp(blobs, blobs + n);
        std::vector<uint64_t> bl(blob_len, blob_len + n);
        std::vector<std::string> rows =
            gams::wave_proc_ctgs_gz(h, make_ctgs(n, ids, chrs, starts, ends), bp, bl, a, threads, &st);
        g_operator_device = st.device_text ? 1 : 0;
        put_stages(st, stages);
        return join(rows);
    });
}

// ... through the device inflater (gams::wave_proc_ctgs_gz_device)
char *gams_host_wave_gz_device(gams_gpu_t *h, uint32_t n, const char *const *ids, const char *const *chrs,
                               const int32_t *starts, const int32_t *ends, const uint8_t *const *blobs,
                               const uint64_t *blob_len, int32_t size, int32_t step, uint32_t lag, float threshold,
                               float influence, float coverage, uint32_t threads, int sync, double *stages, uint64_t *out_len) {
    return guarded(out_len, [&] {
        const gams::WaveArgs a = wave_args(size, step, lag, threshold, influence, coverage, false);
        gams::WaveStages st;
        st.sync = sync != 0;
        std::vector<const uint8_t *> bp(blobs, blobs + n);
        std::vector<uint64_t> bl(blob_len, blob_len + n);
        std::vector<std::string> rows =
            gams::wave_proc_ctgs_gz_device(h, make_ctgs(n, ids, chrs, starts, ends), bp, bl, a, threads, &st);
        g_operator_device = st.device_text ? 1 : 0;
        put_stages(st, stages);
        return join(rows);
    });
}

// gams::seqset_upload_gz: slots first .. first + n from their `seq:` values; went[0] / went[1] receive how many the device
// and the host inflated.  Returns 0, or -1 with the message in gams_host_last_error().
int gams_host_seqset_upload_gz(gams_gpu_t *h, gams_seqset_t *seqset, uint32_t first, uint32_t n, const uint8_t *const *blobs,
                               const uint64_t *blob_len, const uint32_t *slot_len, uint32_t threads, uint32_t *went) {
    return guard(-1, [&] {
        std::vector<const uint8_t *> bp(blobs, blobs + n);
        std::vector<uint64_t> bl(blob_len, blob_len + n);
        std::vector<uint32_t> sl(slot_len, slot_len + n);
        const gams::UploadGz w = gams::seqset_upload_gz(h, seqset, first, bp, bl, sl, threads);
        if (went) went[0] = w.device, went[1] = w.host;
        return 0;
    });
}

// decode_gz of n values on `threads` host threads into caller buffers: dst[i] has room for dst_cap[i] bytes,
// got[i] receives the bytes written.  Returns 0, or -1 with the message in gams_host_last_error().
int gams_host_decode_gz_many(uint32_t n, const uint8_t *const *blobs, const uint64_t *blob_len, uint8_t *const *dst,
                             const uint64_t *dst_cap, uint64_t *got, uint32_t threads) {
    return guard(-1, [&] {
        std::vector<const uint8_t *> bp(blobs, blobs + n);
        std::vector<uint64_t> bl(blob_len, blob_len + n);
        std::vector<std::string> out = gams::decode_gz_many(bp, bl, threads);
        for (uint32_t i = 0; i < n; ++i) {
            if (out[i].size() > dst_cap[i]) throw gams::Error(GAMS_EINVAL, "decode_gz_many: value " + std::to_string(i) + " does not fit");
            std::memcpy(dst[i], out[i].data(), out[i].size());
            got[i] = out[i].size();
        }
        return 0;
    });
}

// the same over several handles (one per device; tests pass two handles of one device)
char *gams_host_wave_multi(gams_gpu_t *const *handles, uint32_t n_handles, uint32_t n, const char *const *ids,
                           const char *const *chrs, const int32_t *starts, const int32_t *ends,
                           const uint8_t *const *seqs, int32_t size, int32_t step, uint32_t lag, float threshold,
                           float influence, float coverage, int is_signal, uint64_t batch_bytes) {
    return guarded([&] {
        const gams::WaveArgs a = wave_args(size, step, lag, threshold, influence, coverage, is_signal != 0);
        std::vector<gams_gpu_t *> hs(handles, handles + n_handles);
        std::vector<const uint8_t *> sp(seqs, seqs + n);
        return join(gams::wave_proc_ctgs_multi(hs, make_ctgs(n, ids, chrs, starts, ends), sp, a, batch_bytes));
    });
}

// locate.rs:111-141.  rgs: newline-separated ranges (first TSV column already cut).
// rg_lines (for --count): newline-separated "ctg_id\trange" rows = the rg: records per ctg.
static thread_local double g_operator_ms = 0.0;

char *gams_host_locate(gams_gpu_t *h, uint32_t n, const char *const *ids, const char *const *chrs,
                       const int32_t *starts, const int32_t *ends, const char *rgs, int is_count,
                       const char *rg_lines) {
    return guarded([&] {
        gams::Locator loc(h, make_ctgs(n, ids, chrs, starts, ends));
        if (is_count) loc.set_rg_index(rg_index_of(n, ids, rg_lines));
        const std::vector<std::string> lines = split_lines(rgs);
        const auto t0 = std::chrono::steady_clock::now();
        std::string out = loc.locate(lines, is_count != 0);
        g_operator_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        return out;
    });
}

// milliseconds the last gams_host_locate / gams_host_anno / gams_host_locate_text / gams_host_anno_text of this
// thread spent inside the operator itself (Locator::locate, gams::anno: parsing of the range strings, device lookups,
// row text; the text forms: from the input bytes in host memory to the finished string) -- without this wrapper's
// splitting of its arguments into lines and, for locate, the build of the ctg / rg index and its name tables, which
// are the caller's
double gams_host_last_operator_ms(void) { return g_operator_ms; }

int gams_host_last_operator_device(void) { return g_operator_device; }

// sw with an action set (GAMS_SW_GC | GAMS_SW_COUNT, sw.rs:28-32) and, for GAMS_SW_COUNT, the rg: records as
// "ctg_id\trange" lines (as gams_host_locate takes them; every ctg of the call gets a group, empty or not).
// sw.rs:108-194 for one ctg
char *gams_host_sw_actions(gams_gpu_t *h, const char *ctg_id, const char *chr, int32_t chr_start, int32_t chr_end,
                           const uint8_t *seq, uint32_t nf, const char *const *feature_ids, const int32_t *fs,
                           const int32_t *fe, int32_t size, int32_t max, int32_t resize, uint32_t actions,
                           const char *rg_lines) {
    return guarded([&] {
        const char *ids[1] = {ctg_id}, *chrs[1] = {chr};
        gams::Ctg c = make_ctgs(1, ids, chrs, &chr_start, &chr_end)[0];
        std::vector<gams::Feature> f(nf);
        for (uint32_t i = 0; i < nf; ++i) f[i] = gams::Feature{feature_ids[i], fs[i], fe[i]};
        const std::map<std::string, std::vector<gams::Range>> rg_of = rg_index_of(1, ids, rg_lines);
        return gams::sw_proc_ctg(h, c, seq, f, sw_args(size, max, resize, actions), &rg_of);
    });
}

// `gams sw` over several handles.  features: rows "ctg_index\tfeature_id\tstart\tend"
char *gams_host_sw_multi_actions(gams_gpu_t *const *handles, uint32_t n_handles, uint32_t n, const char *const *ids,
                                 const char *const *chrs, const int32_t *starts, const int32_t *ends,
                                 const uint8_t *const *seqs, const char *features, int32_t size, int32_t max,
                                 int32_t resize, uint32_t actions, const char *rg_lines) {
    return guarded([&] {
        const std::map<std::string, std::vector<gams::Range>> rg_of = rg_index_of(n, ids, rg_lines);
        return join(gams::sw_proc_ctgs_multi(std::vector<gams_gpu_t *>(handles, handles + n_handles),
                                             make_ctgs(n, ids, chrs, starts, ends),
                                             std::vector<const uint8_t *>(seqs, seqs + n), sw_feature_rows(n, features),
                                             sw_args(size, max, resize, actions), &rg_of));
    });
}

// the same, also reporting the milliseconds of the operator itself (gams::sw_proc_ctgs_multi: upload, kernels, text;
// without the parsing of `features` in front and the concatenation behind, which belong to this wrapper).  operator_ms
// includes the build of the rg index, which gams_host_last_sw_index_ms then reports on its own
char *gams_host_sw_multi_actions_timed(gams_gpu_t *const *handles, uint32_t n_handles, uint32_t n, const char *const *ids,
                                       const char *const *chrs, const int32_t *starts, const int32_t *ends,
                                       const uint8_t *const *seqs, const char *features, int32_t size, int32_t max,
                                       int32_t resize, uint32_t actions, const char *rg_lines, double *operator_ms,
                                       uint64_t *out_len) {
    return guarded(out_len, [&] {
        const std::vector<std::vector<gams::Feature>> f = sw_feature_rows(n, features);
        const std::map<std::string, std::vector<gams::Range>> rg_of = rg_index_of(n, ids, rg_lines);
        const std::vector<gams::Ctg> cv = make_ctgs(n, ids, chrs, starts, ends);
        const std::vector<const uint8_t *> sv(seqs, seqs + n);
        const std::vector<gams_gpu_t *> hv(handles, handles + n_handles);
        g_sw_index_ms = 0.0;
        const auto t0 = std::chrono::steady_clock::now();
        std::vector<std::string> rows =
            gams::sw_proc_ctgs_multi(hv, cv, sv, f, sw_args(size, max, resize, actions), &rg_of, &g_sw_index_ms);
        if (operator_ms) *operator_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        return join(rows);
    });
}

// ms the last gams_host_sw_multi_actions_timed of this thread spent building the rg index (the longest handle's)
double gams_host_last_sw_index_ms(void) { return g_sw_index_ms; }

// the three entries without an action set: those above with GAMS_SW_GC and no rg lines (no rg range is read)
char *gams_host_sw(gams_gpu_t *h, const char *ctg_id, const char *chr, int32_t chr_start, int32_t chr_end,
                   const uint8_t *seq, uint32_t nf, const char *const *feature_ids, const int32_t *fs,
                   const int32_t *fe, int32_t size, int32_t max, int32_t resize) {
    return gams_host_sw_actions(h, ctg_id, chr, chr_start, chr_end, seq, nf, feature_ids, fs, fe, size, max, resize,
                                GAMS_SW_GC, nullptr);
}
char *gams_host_sw_multi(gams_gpu_t *const *handles, uint32_t n_handles, uint32_t n, const char *const *ids,
                         const char *const *chrs, const int32_t *starts, const int32_t *ends,
                         const uint8_t *const *seqs, const char *features, int32_t size, int32_t max, int32_t resize) {
    return gams_host_sw_multi_actions(handles, n_handles, n, ids, chrs, starts, ends, seqs, features, size, max, resize,
                                      GAMS_SW_GC, nullptr);
}
char *gams_host_sw_multi_timed(gams_gpu_t *const *handles, uint32_t n_handles, uint32_t n, const char *const *ids,
                               const char *const *chrs, const int32_t *starts, const int32_t *ends,
                               const uint8_t *const *seqs, const char *features, int32_t size, int32_t max, int32_t resize,
                               double *operator_ms, uint64_t *out_len) {
    return gams_host_sw_multi_actions_timed(handles, n_handles, n, ids, chrs, starts, ends, seqs, features, size, max,
                                            resize, GAMS_SW_GC, nullptr, operator_ms, out_len);
}

// locate -f / --count over the bytes of the input file (bytes, n_bytes: not NUL-terminated); rg_lines as for
// gams_host_locate.  *out_len receives the text's length.
char *gams_host_locate_text(gams_gpu_t *h, uint32_t n, const char *const *ids, const char *const *chrs,
                            const int32_t *starts, const int32_t *ends, const char *bytes, uint64_t n_bytes,
                            int is_count, const char *rg_lines, uint64_t *out_len) {
    return guarded(out_len, [&] {
        gams::Locator loc(h, make_ctgs(n, ids, chrs, starts, ends));
        if (is_count) loc.set_rg_index(rg_index_of(n, ids, rg_lines));
        loc.text_tables();
        bool dev = false;
        const auto t0 = std::chrono::steady_clock::now();
        std::string out = loc.locate_text(bytes, (size_t)n_bytes, is_count != 0, &dev);
        g_operator_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        g_operator_device = dev ? 1 : 0;
        return out;
    });
}

// ---- the rg index from the bytes of an rg file (rg_data, rg_n: not NUL-terminated; Locator::set_rg_index_text) ----
// gams_host_locate with the rg index loaded from the file's bytes instead of rg_lines
char *gams_host_locate_rg(gams_gpu_t *h, uint32_t n, const char *const *ids, const char *const *chrs,
                          const int32_t *starts, const int32_t *ends, const char *rgs, int is_count, const char *rg_data,
                          uint64_t rg_n) {
    return guarded([&] {
        gams::Locator loc(h, make_ctgs(n, ids, chrs, starts, ends));
        if (is_count) loc.set_rg_index_text(rg_data ? rg_data : "", (size_t)rg_n);
        const std::vector<std::string> lines = split_lines(rgs);
        const auto t0 = std::chrono::steady_clock::now();
        std::string out = loc.locate(lines, is_count != 0);
        g_operator_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        return out;
    });
}

// gams_host_locate_text likewise
char *gams_host_locate_text_rg(gams_gpu_t *h, uint32_t n, const char *const *ids, const char *const *chrs,
                               const int32_t *starts, const int32_t *ends, const char *bytes, uint64_t n_bytes,
                               int is_count, const char *rg_data, uint64_t rg_n, uint64_t *out_len) {
    return guarded(out_len, [&] {
        gams::Locator loc(h, make_ctgs(n, ids, chrs, starts, ends));
        if (is_count) loc.set_rg_index_text(rg_data ? rg_data : "", (size_t)rg_n);
        loc.text_tables();
        bool dev = false;
        const auto t0 = std::chrono::steady_clock::now();
        std::string out = loc.locate_text(bytes, (size_t)n_bytes, is_count != 0, &dev);
        g_operator_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        g_operator_device = dev ? 1 : 0;
        return out;
    });
}

// ... and with several rg files loaded one after another (`gams rg f1 f2 ...`): n_rg files, rg_data[f] of rg_n[f] bytes
char *gams_host_locate_rgs(gams_gpu_t *h, uint32_t n, const char *const *ids, const char *const *chrs, const int32_t *starts,
                           const int32_t *ends, const char *rgs, int is_count, uint32_t n_rg, const char *const *rg_data,
                           const uint64_t *rg_n) {
    return guarded([&] {
        gams::Locator loc(h, make_ctgs(n, ids, chrs, starts, ends));
        if (is_count) loc.set_rg_index_text(files_of(n_rg, rg_data, rg_n));
        const std::vector<std::string> lines = split_lines(rgs);
        const auto t0 = std::chrono::steady_clock::now();
        std::string out = loc.locate(lines, is_count != 0);
        g_operator_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        return out;
    });
}
char *gams_host_locate_text_rgs(gams_gpu_t *h, uint32_t n, const char *const *ids, const char *const *chrs,
                                const int32_t *starts, const int32_t *ends, const char *bytes, uint64_t n_bytes, int is_count,
                                uint32_t n_rg, const char *const *rg_data, const uint64_t *rg_n, uint64_t *out_len) {
    return guarded(out_len, [&] {
        gams::Locator loc(h, make_ctgs(n, ids, chrs, starts, ends));
        if (is_count) loc.set_rg_index_text(files_of(n_rg, rg_data, rg_n));
        loc.text_tables();
        bool dev = false;
        const auto t0 = std::chrono::steady_clock::now();
        std::string out = loc.locate_text(bytes, (size_t)n_bytes, is_count != 0, &dev);
        g_operator_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        g_operator_device = dev ? 1 : 0;
        return out;
    });
}

// Loads the rg index of a file over the ctg table and reports the ms of the load itself in gams_host_last_operator_ms:
// text_path != 0 through Locator::set_rg_index_text (from the bytes in host memory to the finished index), else through
// set_rg_index(read_range(text_lines(bytes))), the passes over strings.  gams_host_last_operator_device says which path
// built it.  Returns the number of ctgs with a group, -1 on error.
int64_t gams_host_rg_load(gams_gpu_t *h, uint32_t n, const char *const *ids, const char *const *chrs, const int32_t *starts,
                          const int32_t *ends, const char *rg_data, uint64_t rg_n, int text_path) {
    return guard((int64_t)-1, [&]() -> int64_t {
        const std::vector<gams::Ctg> cv = make_ctgs(n, ids, chrs, starts, ends);
        gams::Locator loc(h, cv);
        loc.text_tables();
        bool dev = false;
        const char *data = rg_data ? rg_data : "";
        const auto t0 = std::chrono::steady_clock::now();
        if (text_path)
            loc.set_rg_index_text(data, (size_t)rg_n, &dev);
        else
            loc.set_rg_index(gams::read_range(loc, gams::text_lines(data, (size_t)rg_n)));
        g_operator_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        g_operator_device = dev ? 1 : 0;
        int64_t groups = 0;
        for (const gams::Ctg &c : cv) groups += loc.rg_group_of(c.id) != UINT32_MAX;
        return groups;
    });
}

// gams::read_range_text over the ctg table: the call keeps the buckets (per thread) and reports their sizes,
// gams_host_read_range_text_get copies them out: bucket_ctg[k] = the position in ids[] of bucket k's ctg, bucket_off
// n_buckets + 1 offsets, start / end / line n_kept entries each.  Returns 0, or -1 with the message in
// gams_host_last_error().
namespace {
thread_local gams::RangeBuckets g_buckets;
thread_local std::vector<uint32_t> g_bucket_ctg;
}  // namespace
int gams_host_read_range_text(gams_gpu_t *h, uint32_t n, const char *const *ids, const char *const *chrs,
                              const int32_t *starts, const int32_t *ends, const char *data, uint64_t n_bytes,
                              uint64_t *n_buckets, uint64_t *n_kept) {
    return guard(-1, [&] {
        gams::Locator loc(h, make_ctgs(n, ids, chrs, starts, ends));
        bool dev = false;
        g_buckets = gams::read_range_text(loc, data ? data : "", (size_t)n_bytes, &dev);
        g_operator_device = dev ? 1 : 0;
        std::map<std::string, uint32_t> pos;
        for (uint32_t i = 0; i < n; ++i) pos[ids[i]] = i;
        g_bucket_ctg.clear();
        for (const std::string &id : g_buckets.ids) g_bucket_ctg.push_back(pos.at(id));
        *n_buckets = g_buckets.ids.size();
        *n_kept = g_buckets.start.size();
        return 0;
    });
}
void gams_host_read_range_text_get(uint32_t *bucket_ctg, uint64_t *bucket_off, int32_t *start, int32_t *end, uint32_t *line) {
    std::copy(g_bucket_ctg.begin(), g_bucket_ctg.end(), bucket_ctg);
    std::copy(g_buckets.off.begin(), g_buckets.off.end(), bucket_off);
    std::copy(g_buckets.start.begin(), g_buckets.start.end(), start);
    std::copy(g_buckets.end.begin(), g_buckets.end.end(), end);
    std::copy(g_buckets.line.begin(), g_buckets.line.end(), line);
}

// gams_host_sw_actions / gams_host_sw_multi_actions with the bytes of an rg file as the idx:rg: source
char *gams_host_sw_actions_rg(gams_gpu_t *h, const char *ctg_id, const char *chr, int32_t chr_start, int32_t chr_end,
                              const uint8_t *seq, uint32_t nf, const char *const *feature_ids, const int32_t *fs,
                              const int32_t *fe, int32_t size, int32_t max, int32_t resize, uint32_t actions,
                              const char *rg_data, uint64_t rg_n) {
    return guarded([&] {
        const char *ids[1] = {ctg_id}, *chrs[1] = {chr};
        gams::Ctg c = make_ctgs(1, ids, chrs, &chr_start, &chr_end)[0];
        std::vector<gams::Feature> f(nf);
        for (uint32_t i = 0; i < nf; ++i) f[i] = gams::Feature{feature_ids[i], fs[i], fe[i]};
        return gams::sw_proc_ctg(h, c, seq, f, sw_args(size, max, resize, actions), nullptr, rg_data ? rg_data : "",
                                 (size_t)rg_n);
    });
}
char *gams_host_sw_multi_actions_rg(gams_gpu_t *const *handles, uint32_t n_handles, uint32_t n, const char *const *ids,
                                    const char *const *chrs, const int32_t *starts, const int32_t *ends,
                                    const uint8_t *const *seqs, const char *features, int32_t size, int32_t max,
                                    int32_t resize, uint32_t actions, const char *rg_data, uint64_t rg_n) {
    return guarded([&] {
        return join(gams::sw_proc_ctgs_multi(std::vector<gams_gpu_t *>(handles, handles + n_handles),
                                             make_ctgs(n, ids, chrs, starts, ends),
                                             std::vector<const uint8_t *>(seqs, seqs + n), sw_feature_rows(n, features),
                                             sw_args(size, max, resize, actions), nullptr, nullptr, rg_data ? rg_data : "",
                                             (size_t)rg_n));
    });
}

// gams::sw_gibbs_proc_ctgs on one handle: the rows of gams_host_sw_multi_actions with the ΔG of every window as a tenth
// field.  table: the 21 terms (gams_dg_table_t); the idx:rg: source of GAMS_SW_COUNT: the rg_n bytes of an rg file
// (rg_data == NULL: no rg range, every count is 0); seqset != NULL: the bases are resident, ctg i in slot slots[i]
// (NULL: i), and seqs is not read.
char *gams_host_sw_gibbs(gams_gpu_t *h, uint32_t n, const char *const *ids, const char *const *chrs, const int32_t *starts,
                         const int32_t *ends, const uint8_t *const *seqs, const char *features, int32_t size, int32_t max,
                         int32_t resize, uint32_t actions, const char *rg_data, uint64_t rg_n,
                         const gams_dg_table_t *table, gams_seqset_t *seqset, const uint32_t *slots) {
    return guarded([&] {
        const std::map<std::string, std::vector<gams::Range>> rg_of = rg_index_of(n, ids, nullptr);   // every ctg an empty group
        gams::SwGibbs gb;
        gb.table = table;
        gb.resident = seqset;
        gb.slots = slots;
        return join(gams::sw_gibbs_proc_ctgs(h, make_ctgs(n, ids, chrs, starts, ends),
                                             seqset ? std::vector<const uint8_t *>() : std::vector<const uint8_t *>(seqs, seqs + n),
                                             sw_feature_rows(n, features), sw_args(size, max, resize, actions), gb, 256ull << 20,
                                             rg_data ? nullptr : &rg_of, rg_data, (size_t)rg_n));
    });
}

// ... with several rg files (as gams_host_locate_rgs takes them)
char *gams_host_sw_actions_rgs(gams_gpu_t *h, const char *ctg_id, const char *chr, int32_t chr_start, int32_t chr_end,
                               const uint8_t *seq, uint32_t nf, const char *const *feature_ids, const int32_t *fs,
                               const int32_t *fe, int32_t size, int32_t max, int32_t resize, uint32_t actions, uint32_t n_rg,
                               const char *const *rg_data, const uint64_t *rg_n) {
    return guarded([&] {
        const char *ids[1] = {ctg_id}, *chrs[1] = {chr};
        gams::Ctg c = make_ctgs(1, ids, chrs, &chr_start, &chr_end)[0];
        std::vector<gams::Feature> f(nf);
        for (uint32_t i = 0; i < nf; ++i) f[i] = gams::Feature{feature_ids[i], fs[i], fe[i]};
        const std::vector<gams::FileBytes> files = files_of(n_rg, rg_data, rg_n);
        return gams::sw_proc_ctg(h, c, seq, f, sw_args(size, max, resize, actions), nullptr, nullptr, 0, &files);
    });
}
char *gams_host_sw_multi_actions_rgs(gams_gpu_t *const *handles, uint32_t n_handles, uint32_t n, const char *const *ids,
                                     const char *const *chrs, const int32_t *starts, const int32_t *ends,
                                     const uint8_t *const *seqs, const char *features, int32_t size, int32_t max,
                                     int32_t resize, uint32_t actions, uint32_t n_rg, const char *const *rg_data,
                                     const uint64_t *rg_n) {
    return guarded([&] {
        const std::vector<gams::FileBytes> files = files_of(n_rg, rg_data, rg_n);
        return join(gams::sw_proc_ctgs_multi(std::vector<gams_gpu_t *>(handles, handles + n_handles),
                                             make_ctgs(n, ids, chrs, starts, ends),
                                             std::vector<const uint8_t *>(seqs, seqs + n), sw_feature_rows(n, features),
                                             sw_args(size, max, resize, actions), nullptr, nullptr, nullptr, 0, &files));
    });
}

// anno over the bytes of one input file; runlists as for gams_host_anno
char *gams_host_anno_text(gams_gpu_t *h, uint32_t n, const char *const *ids, const char *const *chrs,
                          const int32_t *starts, const int32_t *ends, const char *runlists, const char *bytes,
                          uint64_t n_bytes, int header, const char *prefix, uint32_t idx_id, uint32_t idx_range,
                          uint64_t *out_len) {
    return guarded(out_len, [&] {
        const std::map<std::string, gams::Runlist> sets = runlists_of(runlists);
        const std::vector<gams::Ctg> cv = make_ctgs(n, ids, chrs, starts, ends);
        bool dev = false;
        const auto t0 = std::chrono::steady_clock::now();
        std::string out = gams::anno_text(h, sets, cv, bytes, (size_t)n_bytes, header != 0, prefix ? prefix : "", idx_id,
                                          idx_range, &dev);
        g_operator_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        g_operator_device = dev ? 1 : 0;
        return out;
    });
}

// ---- the span set of an anno run, built once from the bytes of the runlist JSON file (gams::AnnoSet) ----
// NULL on error (GAMS_EINVAL in gams_host_last_code where the host reader refuses the file).
// gams_host_last_operator_ms has the ms from the bytes to the usable set, gams_host_last_operator_device the route.
void *gams_host_anno_set_create(gams_gpu_t *h, const char *data, uint64_t n_bytes) {
    return guard((void *)nullptr, [&]() -> void * {
        const auto t0 = std::chrono::steady_clock::now();
        gams::AnnoSet *set = new gams::AnnoSet(h, data ? data : "", (size_t)n_bytes);
        g_operator_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        g_operator_device = set->device() ? 1 : 0;
        return set;
    });
}
void gams_host_anno_set_destroy(void *set) { delete static_cast<gams::AnnoSet *>(set); }
// 1 if the device built the set from the bytes, 0 if the host reader did
int gams_host_anno_set_device(const void *set) { return static_cast<const gams::AnnoSet *>(set)->device() ? 1 : 0; }
// the set's span set (owned by the set; for gams_spans_read and gams_gpu_cover) and its sizes
gams_spans_t *gams_host_anno_set_spans(const void *set, uint32_t *n_groups, uint64_t *n_spans) {
    const gams::AnnoSet *s = static_cast<const gams::AnnoSet *>(set);
    if (n_groups) *n_groups = (uint32_t)s->chrs().size();
    if (n_spans) *n_spans = s->n_spans();
    return s->spans();
}
// the chr names of the groups, in group order, each followed by a NUL; *out_len = the bytes of all of them
char *gams_host_anno_set_names(const void *set, uint64_t *out_len) {
    return guarded(out_len, [&] {
        std::string flat;
        for (const std::string &c : static_cast<const gams::AnnoSet *>(set)->chrs()) flat += c + '\0';
        return flat;
    });
}

// anno over the bytes of one input file, against a set built once (anno.rs:95: one set, several input files)
char *gams_host_anno_text_set(gams_gpu_t *h, uint32_t n, const char *const *ids, const char *const *chrs,
                              const int32_t *starts, const int32_t *ends, const void *set, const char *bytes,
                              uint64_t n_bytes, int header, const char *prefix, uint32_t idx_id, uint32_t idx_range,
                              uint64_t *out_len) {
    return guarded(out_len, [&] {
        const std::vector<gams::Ctg> cv = make_ctgs(n, ids, chrs, starts, ends);
        bool dev = false;
        const auto t0 = std::chrono::steady_clock::now();
        std::string out = gams::anno_text(h, *static_cast<const gams::AnnoSet *>(set), cv, bytes, (size_t)n_bytes, header != 0,
                                          prefix ? prefix : "", idx_id, idx_range, &dev);
        g_operator_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        g_operator_device = dev ? 1 : 0;
        return out;
    });
}
// ... and over lines, as gams_host_anno
char *gams_host_anno_set(gams_gpu_t *h, uint32_t n, const char *const *ids, const char *const *chrs, const int32_t *starts,
                         const int32_t *ends, const void *set, const char *lines, int header, const char *prefix,
                         uint32_t idx_id, uint32_t idx_range) {
    return guarded([&] {
        return gams::anno(h, *static_cast<const gams::AnnoSet *>(set), make_ctgs(n, ids, chrs, starts, ends), split_lines(lines),
                          header != 0, prefix ? prefix : "", idx_id, idx_range);
    });
}

// gams::read_runlist_json: the call keeps the set (per thread) and reports its sizes, gams_host_read_runlist_json_get
// copies it out: names = the keys back to back, name_off n_groups + 1 offsets into them, group_off n_groups + 1
// offsets into lo / hi.  Returns 0, or -1 with the message in gams_host_last_error() (code GAMS_EINVAL).
namespace {
thread_local gams::RunlistJson g_runlists;
}  // namespace
int gams_host_read_runlist_json(const char *data, uint64_t n_bytes, uint32_t *n_groups, uint64_t *n_spans,
                                uint64_t *name_bytes) {
    return guard(-1, [&] {
        g_runlists = gams::read_runlist_json(data ? data : "", (size_t)n_bytes);
        *n_groups = (uint32_t)g_runlists.chr.size();
        *n_spans = 0;
        *name_bytes = 0;
        for (size_t g = 0; g < g_runlists.chr.size(); ++g) {
            *n_spans += g_runlists.sets[g].lo.size();
            *name_bytes += g_runlists.chr[g].size();
        }
        return 0;
    });
}
void gams_host_read_runlist_json_get(char *names, uint64_t *name_off, uint64_t *group_off, int32_t *lo, int32_t *hi) {
    uint64_t nb = 0, ns = 0;
    for (size_t g = 0; g < g_runlists.chr.size(); ++g) {
        const std::string &c = g_runlists.chr[g];
        const gams::Runlist &r = g_runlists.sets[g];
        name_off[g] = nb;
        group_off[g] = ns;
        std::memcpy(names + nb, c.data(), c.size());
        if (!r.lo.empty()) {
            std::memcpy(lo + ns, r.lo.data(), r.lo.size() * sizeof(int32_t));
            std::memcpy(hi + ns, r.hi.data(), r.hi.size() * sizeof(int32_t));
        }
        nb += c.size();
        ns += r.lo.size();
    }
    name_off[g_runlists.chr.size()] = nb;
    group_off[g_runlists.chr.size()] = ns;
}

// Loads the span set of a runlist JSON file and drops it, reporting the ms of the load itself in
// gams_host_last_operator_ms: device_route != 0 through gams::AnnoSet (the device entry; the host reader where it
// refuses), else the host reader and gams_spans_create.  gams_host_last_operator_device says which route built it.
// Returns the spans of the set, -1 on error.
int64_t gams_host_runlist_load(gams_gpu_t *h, const char *data, uint64_t n_bytes, int device_route) {
    return guard((int64_t)-1, [&]() -> int64_t {
        const char *bytes = data ? data : "";
        const auto t0 = std::chrono::steady_clock::now();
        uint64_t spans = 0;
        bool dev = false;
        if (device_route) {
            const gams::AnnoSet set(h, bytes, (size_t)n_bytes);
            spans = set.n_spans();
            dev = set.device();
            g_operator_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        } else {
            gams::RunlistJson js = gams::read_runlist_json(bytes, (size_t)n_bytes);
            std::map<std::string, gams::Runlist> sets;
            for (size_t g = 0; g < js.chr.size(); ++g) sets[js.chr[g]] = std::move(js.sets[g]);
            const gams::AnnoSet set(h, sets);
            spans = set.n_spans();
            g_operator_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        }
        g_operator_device = dev ? 1 : 0;
        return (int64_t)spans;
    });
}

// `{:.4}` of an anno prop as the device formats it ("" outside [0, 1])
char *gams_host_fmt_prop4(float p) { return dup(gams::fmt_prop4(p)); }
char *gams_host_fmt_dg4(float v) { return dup(gams::fmt_dg4(v)); }
// For measurement only, like the _timed entries of this file; no operator calls it.  gams_dg_polymer_host over n ranges on
// `threads` host threads, what a host without the device would run (tools/bench_dg.py measures the device entries
// against it through host.dg_ranges_host): dg[q] of the len[q] bytes at seqs[which[q]] + off[q]
int gams_host_dg_ranges(const gams_dg_table_t *table, const uint8_t *const *seqs, const uint32_t *which, const uint64_t *off,
                        const uint32_t *len, uint64_t n, uint32_t threads, float *dg) {
    if (!table || !dg || (n && (!seqs || !which || !off || !len))) return GAMS_EINVAL;
    const uint32_t T = threads ? threads : 1u;
    std::vector<std::thread> pool;
    for (uint32_t t = 0; t < T; ++t)
        pool.emplace_back([=] {
            for (uint64_t q = n * t / T; q < n * (t + 1) / T; ++q)
                (void)gams_dg_polymer_host(table, seqs[which[q]] + off[q], len[q], &dg[q]);
        });
    for (std::thread &th : pool) th.join();
    return GAMS_OK;
}
// `{}` of an f32 in [0, 1] as the device formats a peak amplitude ("" where it refuses)
char *gams_host_fmt_f32_short(float v) { return dup(gams::fmt_f32_short(v)); }

// locate --seq (locate.rs:124-134).  seq_lines: "ctg_id\tbases" rows.
char *gams_host_locate_seq(gams_gpu_t *h, uint32_t n, const char *const *ids, const char *const *chrs,
                           const int32_t *starts, const int32_t *ends, const char *rgs, const char *seq_lines) {
    return guarded([&] {
        gams::Locator loc(h, make_ctgs(n, ids, chrs, starts, ends));
        std::map<std::string, std::string> seq_of;
        for (const std::string &ln : split_lines(seq_lines)) {
            size_t tab = ln.find('\t');
            if (tab != std::string::npos) seq_of[ln.substr(0, tab)] = ln.substr(tab + 1);
        }
        return loc.locate_seq(split_lines(rgs), seq_of);
    });
}

// locate --seq over the bytes of a range file (bytes, n_bytes: not NUL-terminated; Locator::locate_seq_text): the FASTA
// records of the located lines, copied on the device.  seqset == NULL: seqs[i] = the bases of ctg i, uploaded for the call;
// else the resident seqset and slots[i] = its slot of ctg i (UINT32_MAX: none), seqs unused.
char *gams_host_locate_seq_text(gams_gpu_t *h, uint32_t n, const char *const *ids, const char *const *chrs,
                                const int32_t *starts, const int32_t *ends, const uint8_t *const *seqs, gams_seqset_t *seqset,
                                const uint32_t *slots, const char *bytes, uint64_t n_bytes, uint64_t *out_len) {
    return guarded(out_len, [&] {
        gams::Locator loc(h, make_ctgs(n, ids, chrs, starts, ends));
        loc.text_tables();
        bool dev = false;
        std::string out;
        const auto t0 = std::chrono::steady_clock::now();
        if (seqset)
            out = loc.locate_seq_text(bytes, (size_t)n_bytes, seqset, std::vector<uint32_t>(slots, slots + n), &dev);
        else
            out = loc.locate_seq_text(bytes, (size_t)n_bytes, std::vector<const uint8_t *>(seqs, seqs + n), &dev);
        g_operator_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        g_operator_device = dev ? 1 : 0;
        return out;
    });
}

// utils.rs:39-67 read_range with the drop-first quirk: rows "ctg_id\trange" in bucket order
char *gams_host_read_range(gams_gpu_t *h, uint32_t n, const char *const *ids, const char *const *chrs,
                           const int32_t *starts, const int32_t *ends, const char *lines) {
    return guarded([&] {
        gams::Locator loc(h, make_ctgs(n, ids, chrs, starts, ends));
        const std::vector<std::string> cols = first_cols(lines);
        std::string out;
        for (auto &kv : gams::read_range(loc, cols))
            for (const gams::Range &r : kv.second) out += kv.first + "\t" + r.to_string() + "\n";
        return out;
    });
}

// `gams peak` (peak.rs:24-177) for a set of ctgs: `lines` = rows of a wave TSV.  Output rows, per ctg in
// id order: id, range, length, gc, signal, left_wave_length, left_amplitude, left_signal,
// right_wave_length, right_amplitude, right_signal (the fields of gams::Peak, data.rs:30-43).
char *gams_host_peak(gams_gpu_t *h, uint32_t n, const char *const *ids, const char *const *chrs,
                     const int32_t *starts, const int32_t *ends, const uint8_t *const *seqs, const char *lines) {
    return guarded([&] {
        std::vector<gams::Ctg> ctgs = make_ctgs(n, ids, chrs, starts, ends);
        gams::Locator loc(h, ctgs);
        auto peaks_of = gams::read_peak(loc, split_lines(lines));
        std::string out;
        // ctgs in id order (the map's), all of their merged ranges through one batched call
        std::vector<gams::Ctg> pc;
        std::vector<const uint8_t *> ps;
        std::vector<std::vector<std::pair<gams::Range, std::string>>> pp;
        for (auto &kv : peaks_of) {
            uint32_t slot = 0;
            while (slot < n && ctgs[slot].id != kv.first) ++slot;
            pc.push_back(ctgs[slot]);
            ps.push_back(seqs[slot]);
            pp.push_back(kv.second);
        }
        for (const std::vector<gams::Peak> &recs : gams::peak_records_batch(h, pc, ps, pp)) out += gams::peak_rows(recs);
        return out;
    });
}

// `gams peak` over the bytes of a wave TSV (bytes, n_bytes: not NUL-terminated; gams::peak_text): the rows of
// gams_host_peak with every ctg's peaks sorted by start, made on the device.  seqset == NULL: seqs[i] = the bases of
// ctg i, uploaded for the call; else the resident seqset and slots[i] = its slot of ctg i (UINT32_MAX: none), seqs unused.
char *gams_host_peak_text(gams_gpu_t *h, uint32_t n, const char *const *ids, const char *const *chrs, const int32_t *starts,
                          const int32_t *ends, const uint8_t *const *seqs, gams_seqset_t *seqset, const uint32_t *slots,
                          const char *bytes, uint64_t n_bytes, uint64_t *out_len) {
    return guarded(out_len, [&] {
        const std::vector<gams::Ctg> cv = make_ctgs(n, ids, chrs, starts, ends);
        bool dev = false;
        std::string out;
        const auto t0 = std::chrono::steady_clock::now();
        if (seqset)
            out = gams::peak_text(h, cv, seqset, std::vector<uint32_t>(slots, slots + n), bytes, (size_t)n_bytes, &dev);
        else
            out = gams::peak_text(h, cv, std::vector<const uint8_t *>(seqs, seqs + n), bytes, (size_t)n_bytes, &dev);
        g_operator_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        g_operator_device = dev ? 1 : 0;
        return out;
    });
}

// What `gams peak` stores (gams::peak_records_text): the records of every ctg in id order as text in `format`
// (GAMS_LOADER_RECORDS / _TSV / _RESP), made on the device.  seqs / seqset / slots as for gams_host_peak_text; serial_base[i]
// (NULL: all 0) = cnt:peak:{ctg i} before the load, serial_next[i] (may be NULL) receives the counter after it.
char *gams_host_peak_records_text(gams_gpu_t *h, uint32_t n, const char *const *ids, const char *const *chrs, const int32_t *starts,
                                  const int32_t *ends, const uint8_t *const *seqs, gams_seqset_t *seqset, const uint32_t *slots,
                                  const char *bytes, uint64_t n_bytes, int format, const int32_t *serial_base, int32_t *serial_next,
                                  uint64_t *out_len) {
    return guarded(out_len, [&] {
        const std::vector<gams::Ctg> cv = make_ctgs(n, ids, chrs, starts, ends);
        std::map<std::string, int32_t> base;
        for (uint32_t i = 0; i < n && serial_base; ++i) base[ids[i]] = serial_base[i];
        bool dev = false;
        gams::PeakRecords r;
        const auto t0 = std::chrono::steady_clock::now();
        if (seqset)
            r = gams::peak_records_text(h, cv, seqset, std::vector<uint32_t>(slots, slots + n), bytes, (size_t)n_bytes, format, base, &dev);
        else
            r = gams::peak_records_text(h, cv, std::vector<const uint8_t *>(seqs, seqs + n), bytes, (size_t)n_bytes, format, base, &dev);
        g_operator_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        g_operator_device = dev ? 1 : 0;
        for (uint32_t i = 0; i < n && serial_next; ++i) serial_next[i] = r.serial_next.at(ids[i]);
        return std::move(r.text);
    });
}

// The host formatter of that operator's host route over rows `gams peak` printed (the eleven tab-separated fields of
// gams_host_peak_text, ids as they stand): gams::peak_records_rows of them in `format`.
char *gams_host_peak_rows_records(const char *rows, uint64_t n_bytes, int format, uint64_t *out_len) {
    return guarded(out_len, [&] {
        std::vector<gams::Peak> recs;
        const std::string all(rows ? rows : "", (size_t)n_bytes);
        for (size_t lb = 0, le; lb < all.size(); lb = le + 1) {         // rows end at '\n' and nowhere else (a signal may end in '\r')
            le = std::min(all.find('\n', lb), all.size());
            const std::string ln = all.substr(lb, le - lb);
            std::vector<std::string> f;
            size_t b = 0;
            for (size_t t; (t = ln.find('\t', b)) != std::string::npos; b = t + 1) f.push_back(ln.substr(b, t - b));
            f.push_back(ln.substr(b));
            if (f.size() != 11) throw gams::Error(GAMS_EINVAL, "peak_rows_records: a row without eleven fields");
            gams::Peak p;
            p.id = f[0];
            p.range = f[1];
            p.length = (int32_t)std::stol(f[2]);
            p.gc = std::stof(f[3]);
            p.signal = f[4];
            p.left_wave_length = (int32_t)std::stol(f[5]);
            p.left_amplitude = std::stof(f[6]);
            p.left_signal = f[7];
            p.right_wave_length = (int32_t)std::stol(f[8]);
            p.right_amplitude = std::stof(f[9]);
            p.right_signal = f[10];
            recs.push_back(std::move(p));
        }
        return gams::peak_records_rows(recs, format);
    });
}

// an f32 as serde_json prints it, for +0 and [1e-5, 1] (gams::fmt_f32_json); NULL with the error set elsewhere
char *gams_host_fmt_f32_json(float v) {
    return guarded([&] { return gams::fmt_f32_json(v); });
}

// `gams sw` over the bytes of a feature file (bytes, n_bytes: not NUL-terminated; gams::sw_text): the rows of every ctg
// in id order, made on the device.  seqset == NULL: seqs[i] = the bases of ctg i, uploaded for the call (seqs may be NULL
// without GAMS_SW_GC); else the resident seqset and slots[i] = its slot of ctg i (UINT32_MAX: none), seqs unused.  The
// idx:rg: source of GAMS_SW_COUNT: rg_lines ("ctg_id\trange" rows, as gams_host_sw_multi_actions takes them; NULL: none)
// or rg_data (the rg_n bytes of an rg file; NULL: none); both is GAMS_EINVAL.
namespace {
char *host_sw_text(gams_gpu_t *h, uint32_t n, const char *const *ids, const char *const *chrs, const int32_t *starts,
                   const int32_t *ends, const uint8_t *const *seqs, gams_seqset_t *seqset, const uint32_t *slots,
                   const char *bytes, uint64_t n_bytes, int32_t size, int32_t max, int32_t resize, uint32_t actions,
                   const char *rg_lines, const char *rg_data, uint64_t rg_n, const std::vector<gams::FileBytes> *rg_files,
                   uint64_t *out_len) {
    // the rows go straight into the buffer this call returns (gams::TextSink): no string in between
    struct Out {
        char *p = nullptr;
        size_t n = 0;
        ~Out() { std::free(p); }
    };
    return guard((char *)nullptr, [&] {
        const std::vector<gams::Ctg> cv = make_ctgs(n, ids, chrs, starts, ends);
        std::map<std::string, std::vector<gams::Range>> rg_of;
        if (rg_lines) rg_of = rg_index_of(n, ids, rg_lines);
        const gams::SwArgs a = sw_args(size, max, resize, actions);
        const char *data = bytes ? bytes : "";
        bool dev = false;
        Out out;
        const gams::TextSink sink = [&](size_t len) {
            std::free(out.p);
            out.p = static_cast<char *>(std::malloc(len + 1));
            if (!out.p) throw std::bad_alloc();
            out.p[len] = 0;
            out.n = len;
            return out.p;
        };
        const auto t0 = std::chrono::steady_clock::now();
        if (seqset || !seqs)
            gams::sw_text(h, cv, seqset, seqset ? std::vector<uint32_t>(slots, slots + n) : std::vector<uint32_t>(), data,
                          (size_t)n_bytes, a, rg_lines ? &rg_of : nullptr, rg_data, (size_t)rg_n, &dev, &sink, rg_files);
        else
            gams::sw_text(h, cv, std::vector<const uint8_t *>(seqs, seqs + n), data, (size_t)n_bytes, a,
                          rg_lines ? &rg_of : nullptr, rg_data, (size_t)rg_n, &dev, &sink, rg_files);
        g_operator_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        g_operator_device = dev ? 1 : 0;
        if (!out.p) (void)sink(0);
        if (out_len) *out_len = out.n;
        char *const p = out.p;
        out.p = nullptr;
        return p;
    });
}
}  // namespace
char *gams_host_sw_text(gams_gpu_t *h, uint32_t n, const char *const *ids, const char *const *chrs, const int32_t *starts,
                        const int32_t *ends, const uint8_t *const *seqs, gams_seqset_t *seqset, const uint32_t *slots,
                        const char *bytes, uint64_t n_bytes, int32_t size, int32_t max, int32_t resize, uint32_t actions,
                        const char *rg_lines, const char *rg_data, uint64_t rg_n, uint64_t *out_len) {
    return host_sw_text(h, n, ids, chrs, starts, ends, seqs, seqset, slots, bytes, n_bytes, size, max, resize, actions, rg_lines,
                        rg_data, rg_n, nullptr, out_len);
}
// ... with several rg files as the idx:rg: source (as gams_host_locate_rgs takes them)
char *gams_host_sw_text_rgs(gams_gpu_t *h, uint32_t n, const char *const *ids, const char *const *chrs, const int32_t *starts,
                            const int32_t *ends, const uint8_t *const *seqs, gams_seqset_t *seqset, const uint32_t *slots,
                            const char *bytes, uint64_t n_bytes, int32_t size, int32_t max, int32_t resize, uint32_t actions,
                            uint32_t n_rg, const char *const *rg_data, const uint64_t *rg_n, uint64_t *out_len) {
    const std::vector<gams::FileBytes> files = files_of(n_rg, rg_data, rg_n);
    return host_sw_text(h, n, ids, chrs, starts, ends, seqs, seqset, slots, bytes, n_bytes, size, max, resize, actions, nullptr,
                        nullptr, 0, &files, out_len);
}

// The per-distance summary of the sw rows over the bytes of n_files feature files (gams::sw_summary), reduced on the
// device: the table's text (header, then one line per tag and distance with rows).  ctgs, seqs / seqset / slots, actions
// and rg_lines as for gams_host_sw_text; tags: NULL, or one NUL-terminated tag per file; the rg files (n_rg, rg_data,
// rg_n; n_rg 0: none) as for gams_host_sw_text_rgs.  table (may be NULL) receives the raw integers, n_slots * (max + 1)
// groups of GAMS_SW_SUMMARY_WORDS words, n_slots = the distinct tags (1 without tags), in byte order.
// ... with the Prop columns: n_anno span sets (gams_host_anno_set_create), each under the NUL-terminated prefix of its
// column; prop_table (may be NULL) receives n_slots * (max + 1) * n_anno words, group-major.  n_anno 0: the entry below.
char *gams_host_sw_summary_anno(gams_gpu_t *h, uint32_t n, const char *const *ids, const char *const *chrs, const int32_t *starts,
                                const int32_t *ends, const uint8_t *const *seqs, gams_seqset_t *seqset, const uint32_t *slots,
                                uint32_t n_files, const char *const *data, const uint64_t *n_bytes, const char *const *tags,
                                int32_t size, int32_t max, int32_t resize, uint32_t actions, const char *rg_lines, uint32_t n_rg,
                                const char *const *rg_data, const uint64_t *rg_n, uint32_t n_anno, const char *const *prefixes,
                                const void *const *sets, uint64_t *table, uint64_t *prop_table, uint64_t *out_len) {
    return guarded(out_len, [&] {
        std::vector<gams::SwAnnoCol> anno;
        for (uint32_t k = 0; k < n_anno; ++k)
            anno.push_back(gams::SwAnnoCol{prefixes[k] ? prefixes[k] : "", static_cast<const gams::AnnoSet *>(sets[k])});
        const std::vector<gams::Ctg> cv = make_ctgs(n, ids, chrs, starts, ends);
        std::map<std::string, std::vector<gams::Range>> rg_of;
        if (rg_lines) rg_of = rg_index_of(n, ids, rg_lines);
        const gams::SwArgs a = sw_args(size, max, resize, actions);
        const std::vector<gams::FileBytes> files = files_of(n_files, data, n_bytes), rg_files = files_of(n_rg, rg_data, rg_n);
        std::vector<std::string> tv;
        if (tags) tv.assign(tags, tags + n_files);
        bool dev = false;
        const auto t0 = std::chrono::steady_clock::now();
        const gams::SwSummaryTable T =
            (seqset || !seqs) ? gams::sw_summary(h, cv, seqset, seqset ? std::vector<uint32_t>(slots, slots + n) : std::vector<uint32_t>(),
                                                 files, tags ? &tv : nullptr, a, rg_lines ? &rg_of : nullptr, n_rg ? &rg_files : nullptr, &dev,
                                                 n_anno ? &anno : nullptr)
                              : gams::sw_summary(h, cv, std::vector<const uint8_t *>(seqs, seqs + n), files, tags ? &tv : nullptr, a,
                                                 rg_lines ? &rg_of : nullptr, n_rg ? &rg_files : nullptr, &dev, n_anno ? &anno : nullptr);
        std::string out = T.text();
        g_operator_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        g_operator_device = dev ? 1 : 0;
        if (table) std::memcpy(table, T.words.data(), T.words.size() * 8);
        if (prop_table && !T.prop.empty()) std::memcpy(prop_table, T.prop.data(), T.prop.size() * 8);
        return out;
    });
}
char *gams_host_sw_summary(gams_gpu_t *h, uint32_t n, const char *const *ids, const char *const *chrs, const int32_t *starts,
                           const int32_t *ends, const uint8_t *const *seqs, gams_seqset_t *seqset, const uint32_t *slots,
                           uint32_t n_files, const char *const *data, const uint64_t *n_bytes, const char *const *tags,
                           int32_t size, int32_t max, int32_t resize, uint32_t actions, const char *rg_lines, uint32_t n_rg,
                           const char *const *rg_data, const uint64_t *rg_n, uint64_t *table, uint64_t *out_len) {
    return gams_host_sw_summary_anno(h, n, ids, chrs, starts, ends, seqs, seqset, slots, n_files, data, n_bytes, tags, size, max,
                                     resize, actions, rg_lines, n_rg, rg_data, rg_n, 0, nullptr, nullptr, table, nullptr, out_len);
}
// The host's summariser on its own (gams::sw_summarise_rows): n rows of gams_gpu_sw_batch and, under GAMS_SW_COUNT, their
// counts, added into table ((max + 1) groups of GAMS_SW_SUMMARY_WORDS words, which the caller zeroes).  0, or -1 with the
// thread's last error set.
int gams_host_sw_summarise_rows(const gams_sw_row_t *rows, const int32_t *counts, uint64_t n, int32_t max, uint32_t actions,
                                uint64_t *table) {
    return guard(-1, [&] {
        gams::sw_summarise_rows(rows, counts, n, max, actions, table);
        return 0;
    });
}
// ... with n_props columns of Prop units (props[a][r]) into prop_table, (max + 1) * n_props words the caller zeroes
int gams_host_sw_summarise_rows_props(const gams_sw_row_t *rows, const int32_t *counts, uint64_t n, int32_t max, uint32_t actions,
                                      uint64_t *table, uint32_t n_props, const uint32_t *const *props, uint64_t *prop_table) {
    return guard(-1, [&] {
        gams::sw_summarise_rows(rows, counts, n, max, actions, table, n_props, props, prop_table);
        return 0;
    });
}
// The text of a table of n_slots * (max + 1) groups; tags: NULL (n_slots = 1, no tag column) or the n_slots tags in byte order;
// n_props Prop columns under `prefixes` with their sums in prop_table (n_props 0: none).
char *gams_host_sw_summary_text_props(const uint64_t *table, uint32_t n_slots, const char *const *tags, int32_t max,
                                      uint32_t actions, uint32_t n_props, const char *const *prefixes, const uint64_t *prop_table,
                                      uint64_t *out_len) {
    return guarded(out_len, [&] {
        gams::SwSummaryTable T;
        T.max = max;
        T.actions = actions;
        if (tags) T.tags.assign(tags, tags + n_slots);
        const size_t groups = (size_t)(tags ? n_slots : 1) * ((size_t)max + 1);
        T.words.assign(table, table + groups * GAMS_SW_SUMMARY_WORDS);
        for (uint32_t k = 0; k < n_props; ++k) T.prefixes.push_back(prefixes[k] ? prefixes[k] : "");
        if (n_props) T.prop.assign(prop_table, prop_table + groups * n_props);
        return T.text();
    });
}
char *gams_host_sw_summary_text(const uint64_t *table, uint32_t n_slots, const char *const *tags, int32_t max, uint32_t actions,
                                uint64_t *out_len) {
    return gams_host_sw_summary_text_props(table, n_slots, tags, max, actions, 0, nullptr, nullptr, out_len);
}
// the q of a prop in [0, 1] (`{:.4}` prints q / 10^4), as the device computes it; -1 outside
int32_t gams_host_prop4_units(float p) {
    return guard((int32_t)-1, [&] { return (int32_t)gams::prop4_units(p); });
}

// `gams rg f1 f2 ...` (kind 0) / `gams feature --tag T f1 f2 ...` (kind 1) over the bytes of the files (gams::loader_text):
// the records as text in `format` (GAMS_LOADER_RECORDS / _TSV / _RESP), in the reference's SET order.  serial_base[i] (NULL:
// all 0) = the counter of ctg i before the load; serial_next[i] and n_in_file[f] (either may be NULL) receive the counters
// after it and the records of every file.
char *gams_host_loader_text(gams_gpu_t *h, uint32_t n, const char *const *ids, const char *const *chrs, const int32_t *starts,
                            const int32_t *ends, uint32_t n_files, const char *const *data, const uint64_t *n_bytes, int kind,
                            const char *tag, int format, const int32_t *serial_base, int32_t *serial_next, uint64_t *n_in_file,
                            uint64_t *out_len) {
    return guarded(out_len, [&] {
        std::map<std::string, int32_t> base;
        for (uint32_t i = 0; i < n && serial_base; ++i) base[ids[i]] = serial_base[i];
        bool dev = false;
        const auto t0 = std::chrono::steady_clock::now();
        gams::LoaderText r = gams::loader_text(h, make_ctgs(n, ids, chrs, starts, ends), files_of(n_files, data, n_bytes), kind,
                                               tag ? tag : "", format, base, &dev);
        g_operator_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        g_operator_device = dev ? 1 : 0;
        for (uint32_t i = 0; i < n && serial_next; ++i) serial_next[i] = r.serial_next.at(ids[i]);
        for (uint32_t f = 0; f < n_files && n_in_file; ++f) n_in_file[f] = r.n_in_file[f];
        return std::move(r.text);
    });
}

// rg.rs:41-77 / feature.rs:47-95: rows "key\tjson" of the records the loaders SET (tag == NULL: rg)
char *gams_host_loader_records(gams_gpu_t *h, uint32_t n, const char *const *ids, const char *const *chrs,
                               const int32_t *starts, const int32_t *ends, const char *lines, const char *tag) {
    return guarded([&] {
        gams::Locator loc(h, make_ctgs(n, ids, chrs, starts, ends));
        const std::vector<std::string> cols = first_cols(lines);
        std::string out;
        for (const gams::Record &r : tag ? gams::feature_records(loc, cols, tag) : gams::rg_records(loc, cols))
            out += r.key + "\t" + r.json + "\n";
        return out;
    });
}

// tsv.rs for "rg:*" (tag == NULL) / "feature:*" records of the loaders above
char *gams_host_loader_tsv(gams_gpu_t *h, uint32_t n, const char *const *ids, const char *const *chrs,
                           const int32_t *starts, const int32_t *ends, const char *lines, const char *tag) {
    return guarded([&] {
        gams::Locator loc(h, make_ctgs(n, ids, chrs, starts, ends));
        const std::vector<std::string> cols = first_cols(lines);
        return gams::tsv_records(tag ? gams::feature_records(loc, cols, tag) : gams::rg_records(loc, cols),
                                 tag != nullptr);
    });
}

// gzip framing of seq: values (redis.rs:149-161); *out_len receives the length
char *gams_host_decode_gz(const uint8_t *bytes, uint64_t n, uint64_t *out_len) {
    return guarded(out_len, [&] { return gams::decode_gz(bytes, n); });
}
char *gams_host_encode_gz(const uint8_t *bytes, uint64_t n, uint64_t *out_len) {
    try {
        std::string s = gams::encode_gz(bytes, n);
        if (out_len) *out_len = s.size();
        char *p = (char *)std::malloc(s.size() + 1);
        if (p) std::memcpy(p, s.data(), s.size());
        return p;
    } catch (const std::exception &e) {
        g_err = e.what();
        return nullptr;
    }
}

char *gams_host_encode_gz_fast(const uint8_t *bytes, uint64_t n, uint64_t *out_len) {
    return guarded(out_len, [&] { return gams::encode_gz_fast(bytes, n); });
}
// ... with the chunk index (gams_seq_gz_host_indexed), and the host twin of the device inflater for such a member
char *gams_host_encode_gz_indexed(const uint8_t *bytes, uint64_t n, uint64_t *out_len) {
    return guarded(out_len, [&] { return gams::encode_gz_fast(bytes, n, true); });
}
char *gams_host_decode_gz_indexed(const uint8_t *bytes, uint64_t n, uint64_t *out_len) {
    return guarded(out_len, [&] { return gams::decode_gz_indexed(bytes, n); });
}
// gams::seq_gz: the members of slots first .. first + count (ids == NULL) or their SET stream; off receives count + 1
// offsets into the returned bytes
char *gams_host_seq_gz(gams_gpu_t *h, gams_seqset_t *seqset, uint32_t first, uint32_t count, const char *const *ids,
                       uint64_t *off, uint64_t *out_len) {
    return guarded(out_len, [&] {
        std::vector<std::string> v;
        if (ids) v.assign(ids, ids + count);
        gams::SeqGz g = gams::seq_gz(h, seqset, first, count, ids ? &v : nullptr);
        std::copy(g.off.begin(), g.off.end(), off);
        return g.bytes;
    });
}
// ... the indexed form of either (GAMS_SEQ_GZ_INDEXED)
char *gams_host_seq_gz_indexed(gams_gpu_t *h, gams_seqset_t *seqset, uint32_t first, uint32_t count, const char *const *ids,
                               uint64_t *off, uint64_t *out_len) {
    return guarded(out_len, [&] {
        std::vector<std::string> v;
        if (ids) v.assign(ids, ids + count);
        gams::SeqGz g = gams::seq_gz(h, seqset, first, count, ids ? &v : nullptr, true);
        std::copy(g.off.begin(), g.off.end(), off);
        return g.bytes;
    });
}

// utils.rs:7-22 for many ranges: one ctg id (or empty) per line
char *gams_host_find(gams_gpu_t *h, uint32_t n, const char *const *ids, const char *const *chrs,
                     const int32_t *starts, const int32_t *ends, const char *rgs) {
    return guarded([&] {
        gams::Locator loc(h, make_ctgs(n, ids, chrs, starts, ends));
        std::vector<gams::Range> v;
        for (const std::string &ln : split_lines(rgs)) {
            gams::Range r = gams::Range::from_str(ln);
            r.strand.clear();
            if (!r.valid) r.chr = "\x01invalid";  // never located
            v.push_back(r);
        }
        std::string out;
        for (const std::string &id : loc.find(v)) out += id + "\n";
        return out;
    });
}

// anno.rs:95-142.  runlists: newline-separated "chr\trunlist" rows of the JSON set.
char *gams_host_anno(gams_gpu_t *h, uint32_t n, const char *const *ids, const char *const *chrs,
                     const int32_t *starts, const int32_t *ends, const char *runlists, const char *lines,
                     int header, const char *prefix, uint32_t idx_id, uint32_t idx_range) {
    return guarded([&] {
        const std::map<std::string, gams::Runlist> sets = runlists_of(runlists);
        const std::vector<gams::Ctg> cv = make_ctgs(n, ids, chrs, starts, ends);
        const std::vector<std::string> lv = split_lines(lines);
        const auto t0 = std::chrono::steady_clock::now();
        std::string out = gams::anno(h, sets, cv, lv, header != 0, prefix ? prefix : "", idx_id, idx_range);
        g_operator_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        return out;
    });
}

// gen.rs:81-157 for one chromosome; rows "id\trange\tchr_id\tchr_start\tchr_end\tchr_strand\tlength"
// (the columns of `gams tsv -s "ctg:*"`, tests/S288c/ctg.tsv)
char *gams_host_gen(gams_gpu_t *h, const char *chr_id, const uint8_t *seq, uint64_t len, int32_t piece,
                    int32_t fill, int32_t min_len) {
    return guarded([&] {
        gams::GenArgs a;
        a.piece = piece;
        a.fill = fill;
        a.min = min_len;
        std::string out;
        for (const gams::Ctg &c : gams::gen_ctgs(h, chr_id, seq, len, a))
            out += c.id + "\t" + c.range + "\t" + c.chr_id + "\t" + std::to_string(c.chr_start) + "\t" +
                   std::to_string(c.chr_end) + "\t" + c.chr_strand + "\t" + std::to_string(c.length) + "\n";
        return out;
    });
}

// gams::read_fasta over the bytes of a file (no device work): a "{id}\t{length}\n" row per record, an empty line, then
// the records' sequences one behind the other (a sequence may hold any byte but '\n', so it is given by length)
char *gams_host_read_fasta(const char *bytes, uint64_t n_bytes, uint64_t *out_len) {
    return guarded(out_len, [&] {
        const std::vector<gams::FastaRecord> recs = gams::read_fasta(bytes, (size_t)n_bytes);
        std::string out;
        for (const gams::FastaRecord &r : recs) out += r.id + "\t" + std::to_string(r.seq.size()) + "\n";
        out += "\n";
        for (const gams::FastaRecord &r : recs) out += r.seq;
        return out;
    });
}

// `gams gen` over the bytes of one FASTA file (gams::gen_text): "chr\t{id}\t{length}\n" per chromosome, then
// "ctg\t{id}\t{chr_id}\t{chr_start}\t{chr_end}\n" per ctg; *seqset receives the resident seqset (slot k = ctg k; the
// caller destroys it with gams_seqset_destroy).  gams_host_last_operator_device says which path ran.
char *gams_host_gen_text(gams_gpu_t *h, const char *bytes, uint64_t n_bytes, int32_t piece, int32_t fill, int32_t min_len,
                         gams_seqset_t **seqset, uint64_t *out_len) {
    return guarded(out_len, [&] {
        gams::GenArgs a;
        a.piece = piece;
        a.fill = fill;
        a.min = min_len;
        bool dev = false;
        const auto t0 = std::chrono::steady_clock::now();
        gams::GenText g = gams::gen_text(h, bytes, (size_t)n_bytes, a, &dev);
        g_operator_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        g_operator_device = dev ? 1 : 0;
        *seqset = g.seqset;
        std::string out;
        for (auto &c : g.chr_len) out += "chr\t" + c.first + "\t" + std::to_string(c.second) + "\n";
        for (const gams::Ctg &c : g.ctgs)
            out += "ctg\t" + c.id + "\t" + c.chr_id + "\t" + std::to_string(c.chr_start) + "\t" + std::to_string(c.chr_end) + "\n";
        return out;
    });
}

// tsv.rs:31-71 for "ctg:*" (no device work)
char *gams_host_tsv_ctgs(uint32_t n, const char *const *ids, const char *const *chrs, const int32_t *starts,
                         const int32_t *ends) {
    return guarded([&] { return gams::tsv_ctgs(make_ctgs(n, ids, chrs, starts, ends)); });
}

// header lines of `gams wave` (which == 0) and `gams sw` (which == 1)
char *gams_host_header(int which) {   // 0 wave, 1 sw, 2 sw with the ΔG column
    if (which == 2) return dup(gams::sw_gibbs_header());
    return dup(which == 0 ? gams::wave_header() : gams::sw_header());
}

// locate --count / anno coverage over several handles (one per GPU)
int gams_host_count_multi(gams_gpu_t *const *handles, uint32_t n_handles, uint32_t n_groups, const uint64_t *group_off,
                          const uint32_t *starts, const uint32_t *stops, const uint32_t *q_group, const uint32_t *qs,
                          const uint32_t *qe, uint64_t nq, int32_t *count) {
    char *r = guarded([&] {
        gams::count_multi(std::vector<gams_gpu_t *>(handles, handles + n_handles), n_groups, group_off, starts, stops,
                          q_group, qs, qe, nq, count);
        return std::string();
    });
    if (!r) return g_code ? g_code : -1;
    free(r);
    return 0;
}

int gams_host_cover_multi(gams_gpu_t *const *handles, uint32_t n_handles, uint32_t n_groups, const uint64_t *group_off,
                          const int32_t *lo, const int32_t *hi, const uint32_t *q_group, const int32_t *clip_lo,
                          const int32_t *clip_hi, const int32_t *qs, const int32_t *qe, uint64_t nq, float *prop) {
    char *r = guarded([&] {
        gams::cover_multi(std::vector<gams_gpu_t *>(handles, handles + n_handles), n_groups, group_off, lo, hi, q_group,
                          clip_lo, clip_hi, qs, qe, nq, prop);
        return std::string();
    });
    if (!r) return g_code ? g_code : -1;
    free(r);
    return 0;
}

// merge_ints of wave.rs:217-252, for CPU-only tests of the host logic
void gams_host_merge_windows(const uint32_t *w, uint64_t n, int32_t chr_start, int32_t size, int32_t step,
                             float coverage, int64_t *cmin, int64_t *cmax, char *in_graph) {
    gams::merge_windows(w, (size_t)n, chr_start, size, step, coverage, cmin, cmax, in_graph);
}

// serde_json round trip of a ctg: record (redis.rs:127-135); returns the JSON re-serialised from the parse
char *gams_host_ctg_json_roundtrip(const char *json) {
    return guarded([&] { return gams::ctg_json(gams::ctg_from_json(json)); });
}

// formatting helpers exposed for CPU-only tests
char *gams_host_fmt_f32(float v) { return dup(gams::fmt_f32(v)); }
char *gams_host_range_roundtrip(const char *s) {
    gams::Range r = gams::Range::from_str(s);
    return dup(r.valid ? r.to_string() : std::string("<invalid>"));
}


// ---- wire formats (gams_wire.cpp): byte strings out, *out_len = their length ------------------------
char *gams_host_bincode_ctg_bundle(uint32_t n, const char *const *ids, const char *const *chrs, const int32_t *starts,
                                   const int32_t *ends, uint64_t *out_len) {
    return guarded(out_len, [&] { return gams::wire::bincode_ctg_bundle(make_ctgs(n, ids, chrs, starts, ends)); });
}
// decoded bundle as the ctg.tsv text of `gams tsv` (one line per ctg, key order)
char *gams_host_bincode_ctg_bundle_decode(const uint8_t *bytes, uint64_t n) {
    return guarded([&] { return gams::tsv_ctgs(gams::wire::bincode_ctg_bundle_decode(bytes, n)); });
}
// intervals as parallel arrays; vals: n NUL-terminated strings (NULL = all empty, the idx:rg case)
char *gams_host_bincode_lapper(uint64_t n, const uint32_t *starts, const uint32_t *stops, const char *const *vals,
                               uint64_t *out_len) {
    return guarded(out_len, [&] {
        std::vector<gams::wire::LapperIv> ivs(n);
        for (uint64_t i = 0; i < n; ++i) {
            ivs[i].start = starts[i];
            ivs[i].stop = stops[i];
            if (vals && vals[i]) ivs[i].val = vals[i];
        }
        return gams::wire::bincode_lapper(ivs);
    });
}
// decoded Lapper as text: "start\tstop\tval" per interval, then "#starts ...", "#stops ...", "#max_len N cov C merged B"
char *gams_host_bincode_lapper_decode(const uint8_t *bytes, uint64_t n) {
    return guarded([&] {
        const gams::wire::LapperBlob b = gams::wire::bincode_lapper_decode(bytes, n);
        std::string o;
        for (const auto &v : b.intervals) o += std::to_string(v.start) + "\t" + std::to_string(v.stop) + "\t" + v.val + "\n";
        o += "#starts";
        for (uint32_t x : b.starts) o += " " + std::to_string(x);
        o += "\n#stops";
        for (uint32_t x : b.stops) o += " " + std::to_string(x);
        o += "\n#max_len " + std::to_string(b.max_len) + " cov " + (b.has_cov ? std::to_string(b.cov) : std::string("None")) +
             " merged " + (b.overlaps_merged ? "true" : "false") + "\n";
        return o;
    });
}
// args: n byte strings (arg_len[i] bytes each)
char *gams_host_resp_command(uint32_t n, const char *const *args, const uint64_t *arg_len, uint64_t *out_len) {
    return guarded(out_len, [&] {
        std::vector<std::string> a(n);
        for (uint32_t i = 0; i < n; ++i) a[i].assign(args[i], (size_t)arg_len[i]);
        return gams::wire::resp_command(a);
    });
}
char *gams_host_resp_scan_values(const char *pattern, uint64_t *out_len) {
    return guarded(out_len, [&] {
        return gams::wire::resp_eval(gams::wire::scan_values_script(), {}, {pattern ? pattern : "", "1000"});
    });
}
// parses one reply; returns its flat text form (resp_dump), *consumed = bytes used (0: incomplete, "" returned)
char *gams_host_resp_parse(const char *bytes, uint64_t n, uint64_t *consumed) {
    return guarded([&] {
        gams::wire::RespValue v;
        const size_t used = gams::wire::resp_parse(bytes, n, v);
        if (consumed) *consumed = used;
        return used ? gams::wire::resp_dump(v) : std::string();
    });
}

// idx: blobs (n of them, blob i = blob_len[i] bytes) -> device index, one group per blob; NULL on error
void *gams_host_index_from_lappers(void *h, uint32_t n, const uint8_t *const *blobs, const uint64_t *blob_len) {
    return guard((void *)nullptr, [&]() -> void * {
        std::vector<gams::wire::LapperBlob> dec;
        for (uint32_t i = 0; i < n; ++i) dec.push_back(gams::wire::bincode_lapper_decode(blobs[i], (size_t)blob_len[i]));
        return gams::wire::index_from_lappers(static_cast<gams_gpu_t *>(h), dec);
    });
}
}  // extern "C"
