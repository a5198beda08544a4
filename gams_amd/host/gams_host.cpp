// gams_host.cpp -- see gams_host.hpp.  Citations are file:line under the reference.
#include "gams_host.hpp"
#include "../../include/gams_gpu_diag.h"   // the stage clock reports which input a pass read
#include "../csrc/gen_split.hpp"
#include "../csrc/text_fmt.hpp"

#include <algorithm>
#include <atomic>
#include <mutex>
#include <charconv>
#include <string_view>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <memory>
#include <numeric>
#include <queue>
#include <set>
#include <thread>

#include <dlfcn.h>
#include <zlib.h>
#include <chrono>

namespace gams {

namespace {

void check(gams_gpu_t *h, int rc) {
    if (rc != GAMS_OK) throw Error(rc, gams_gpu_last_error(h));
}

bool is_word(char c) {
    return (c >= '0' && c <= '9') || (c >= 'a' && c <= 'z') || (c >= 'A' && c <= 'Z') || c == '_';
}

struct SeqSetGuard {
    gams_gpu_t *h;
    gams_seqset_t *s = nullptr;
    ~SeqSetGuard() {
        if (s) gams_seqset_destroy(h, s);
    }
};
struct PlanGuard {
    gams_gpu_t *h;
    gams_wave_plan_t *p = nullptr;
    ~PlanGuard() {
        if (p) gams_wave_plan_destroy(h, p);
    }
};

}  // namespace

// ---------------------------------------------------------------------------
// formatting
// ---------------------------------------------------------------------------
std::string fmt_f32(float v) {
    if (std::isnan(v)) return "NaN";
    if (std::isinf(v)) return v < 0 ? "-inf" : "inf";
    if (v == 0.0f) return std::signbit(v) ? "-0" : "0";
    // shortest round-trip digits (Ryu-style, like Rust), then positional notation
    char buf[64];
    auto r = std::to_chars(buf, buf + sizeof buf, v, std::chars_format::scientific);
    std::string sci(buf, r.ptr);           // [-]d[.ddd]e[+-]XX
    std::string out;
    size_t i = 0;
    if (sci[0] == '-') {
        out += '-';
        i = 1;
    }
    std::string digits;
    for (; i < sci.size() && sci[i] != 'e'; ++i)
        if (sci[i] != '.') digits += sci[i];
    const int ex = std::atoi(sci.c_str() + i + 1);
    const int nd = (int)digits.size();
    if (ex >= 0) {
        for (int k = 0; k <= ex; ++k) out += k < nd ? digits[k] : '0';
        if (nd > ex + 1) {
            out += '.';
            out.append(digits, ex + 1, std::string::npos);
        }
    } else {
        out += "0.";
        out.append((size_t)(-ex - 1), '0');
        out += digits;
    }
    return out;
}

std::string runlist(int64_t s, int64_t e) {
    std::string o = std::to_string(s);
    if (e != s) {
        o += '-';
        o += std::to_string(e);
    }
    return o;
}

// intspan::Range::from_str: [name.]chr[(strand)]:start[-end]
Range Range::from_str(const std::string &in) {
    // (views into `in` until the end: the text paths call this once per line, 10^6-10^8 times)
    Range r;
    std::string_view s(in);
    while (!s.empty() && (s.back() == '\r' || s.back() == '\n' || s.back() == ' ')) s.remove_suffix(1);
    const size_t colon = s.rfind(':');
    if (colon == std::string_view::npos || colon == 0 || colon + 1 >= s.size()) return r;
    std::string_view head = s.substr(0, colon);
    const std::string_view tail = s.substr(colon + 1);
    auto number = [](std::string_view d) {             // <= 10 digits: no overflow of long long
        long long v = 0;
        for (char c : d) v = v * 10 + (c - '0');
        return v;
    };
    // start[-_]end
    size_t i = 0;
    while (i < tail.size() && tail[i] >= '0' && tail[i] <= '9') ++i;
    if (i == 0 || i > 10) return r;
    long long st = number(tail.substr(0, i)), en = st;
    if (i < tail.size()) {
        size_t j = i;
        while (j < tail.size() && (tail[j] == '-' || tail[j] == '_')) ++j;
        if (j == i) return r;
        size_t k = j;
        while (k < tail.size() && tail[k] >= '0' && tail[k] <= '9') ++k;
        if (k == j || k != tail.size() || k - j > 10) return r;
        en = number(tail.substr(j, k - j));
    }
    if (st > INT32_MAX || en > INT32_MAX) return r;
    // head: [name.]chr[(strand)]
    std::string_view strand, name;
    if (!head.empty() && head.back() == ')') {
        const size_t open = head.rfind('(');
        if (open == std::string_view::npos) return r;
        strand = head.substr(open + 1, head.size() - open - 2);
        head = head.substr(0, open);
    }
    const size_t dot = head.find('.');
    if (dot != std::string_view::npos) {
        name = head.substr(0, dot);
        head = head.substr(dot + 1);
    }
    if (head.empty()) return r;
    for (char c : head)
        if (!(is_word(c) || c == '-' || c == '/')) return r;
    r.strand.assign(strand);
    r.name.assign(name);
    r.chr.assign(head);
    r.start = (int32_t)st;
    r.end = (int32_t)en;
    r.valid = true;
    return r;
}

std::string Range::to_string() const {
    std::string o;
    if (!name.empty()) o += name + ".";
    o += chr;
    if (!strand.empty()) o += "(" + strand + ")";
    o += ":" + runlist(start, end);
    return o;
}

// ---------------------------------------------------------------------------
// wave
// ---------------------------------------------------------------------------
namespace {

// merge_ints (wave.rs:217-252) for the peaks of one sign.  All windows have the
// same size and start at chr_start + k*step, so the intersection of windows k_i
// < k_j has size - (k_j-k_i)*step bases and the edge test (:229-231) depends on
// d = k_j - k_i alone: d in [dmin, dmax].  Components by union-find.
struct Merge {
    std::vector<int64_t> cmin, cmax;
    std::vector<char> in_graph;
};

Merge merge_ints(const std::vector<uint32_t> &w, int32_t chr_start, int32_t size, int32_t step, float coverage) {
    const size_t p = w.size();
    Merge m;
    m.cmin.resize(p);
    m.cmax.resize(p);
    m.in_graph.assign(p, 0);
    std::vector<size_t> par(p);
    std::iota(par.begin(), par.end(), (size_t)0);
    auto find = [&](size_t x) {
        while (par[x] != x) {
            par[x] = par[par[x]];
            x = par[x];
        }
        return x;
    };
    // d range with a non-empty intersection that passes both coverage tests
    const int64_t dmax = ((int64_t)size + step - 1) / step - 1;  // largest d with d*step < size
    int64_t dmin = dmax + 1;
    for (int64_t d = 1; d <= dmax; ++d) {
        const float inter = (float)(int32_t)(size - d * step);
        const float cov = (float)size / inter;                   // cov_i == cov_j (:229-230)
        if (cov >= coverage) {                                   // monotone in d
            dmin = d;
            break;
        }
    }
    if (dmin == 1) {
        // every overlap links (coverage <= 1, the usual case): components are the maximal runs whose
        // consecutive windows are at most dmax apart -- one sweep instead of p*dmax pair tests
        // (step 1: dmax = 99 and tens of thousands of peaks per ctg)
        for (size_t i = 1; i < p; ++i) {
            if ((int64_t)w[i] - (int64_t)w[i - 1] <= dmax) {
                par[i] = find(i - 1);
                m.in_graph[i] = m.in_graph[i - 1] = 1;
            }
        }
    } else {
        for (size_t i = 0; i < p; ++i) {
            for (size_t j = i + 1; j < p; ++j) {
                const int64_t d = (int64_t)w[j] - (int64_t)w[i];
                if (d > dmax) break;
                if (d >= dmin) {
                    size_t a = find(i), b = find(j);
                    if (a != b) par[b] = a;
                    m.in_graph[i] = m.in_graph[j] = 1;
                }
            }
        }
    }
    std::vector<int64_t> mn(p, INT64_MAX), mx(p, INT64_MIN);
    for (size_t i = 0; i < p; ++i) {
        const size_t r = find(i);
        const int64_t s = (int64_t)chr_start + (int64_t)w[i] * step, e = s + size - 1;
        mn[r] = std::min(mn[r], s);
        mx[r] = std::max(mx[r], e);
    }
    for (size_t i = 0; i < p; ++i) {
        const size_t r = find(i);
        m.cmin[i] = mn[r];
        m.cmax[i] = mx[r];
    }
    return m;
}

}  // namespace

void merge_windows(const uint32_t *w, size_t n, int32_t chr_start, int32_t size, int32_t step, float coverage,
                   int64_t *cmin, int64_t *cmax, char *in_graph) {
    const Merge m = merge_ints(std::vector<uint32_t>(w, w + n), chr_start, size, step, coverage);
    for (size_t i = 0; i < n; ++i) {
        cmin[i] = m.cmin[i];
        cmax[i] = m.cmax[i];
        in_graph[i] = m.in_graph[i];
    }
}

namespace {

// One batch of ctgs in flight on one handle: start() queues the uploads (copy stream) and the
// kernels (compute stream, behind the upload event) and returns; finish() waits, fetches and
// formats.  Starting batch k+1 before finishing batch k overlaps its upload with k's kernel and
// k's host-side merge/formatting with k+1's kernel.
// fn(i) for i in [0,n) on `threads` host threads, the caller one of them; the first exception is rethrown on the caller
template <typename F>
void parallel_for(uint32_t n, unsigned threads, F fn) {
    if (threads <= 1) {
        for (uint32_t i = 0; i < n; ++i) fn(i);
        return;
    }
    std::atomic<uint32_t> next{0};
    std::exception_ptr err;
    std::mutex mu;
    auto work = [&] {
        try {
            for (uint32_t i = next.fetch_add(1); i < n; i = next.fetch_add(1)) fn(i);
        } catch (...) {
            std::lock_guard<std::mutex> lk(mu);
            if (!err) err = std::current_exception();
            next.store(n);
        }
    };
    std::vector<std::thread> pool;
    for (unsigned t = 1; t < threads; ++t) pool.emplace_back(work);
    work();
    for (auto &th : pool) th.join();
    if (err) std::rethrow_exception(err);
}
// threads for the per-ctg formatting of a wave batch: up to 8, one for every 4 ctgs
unsigned ctg_threads(uint32_t n) { return std::max(1u, std::min({8u, std::thread::hardware_concurrency(), n / 4u})); }

double now_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

struct WaveJob {
    gams_gpu_t *h;
    std::vector<Ctg> ctgs;
    WaveArgs a;
    SeqSetGuard sg;
    PlanGuard pg;
    uint8_t *image = nullptr;      // start_gz: page-locked image of the seqset the workers inflate into
    uint8_t *plane = nullptr;      // page-locked image of the seqset's G/C plane the workers classify into (plane-only upload)
    uint64_t image_end = 0;        // end of the last ctg in the device layout
    const std::vector<const uint8_t *> *seqs_held = nullptr;   // start(): the caller's buffers, should the bytes be wanted after all
    WaveStages *st = nullptr;      // optional stage clock (wave_proc_ctgs*, see gams_host.hpp)
    double t_mark = 0;
    WaveJob(gams_gpu_t *h_, std::vector<Ctg> c, const WaveArgs &a_) : h(h_), ctgs(std::move(c)), a(a_), sg{h_}, pg{h_} {}
    ~WaveJob() {
        // a DMA may still be reading them -- unless finish() has fetched the pass's results: the pass waited for its uploads
        if ((image || plane) && !consumed) (void)gams_gpu_sync(h);
        if (image) gams_gpu_host_free(h, image);
        if (plane) gams_gpu_host_free(h, plane);
    }
    // Parameters the library runs through its tiled fast kernels (wave.hip: wave_build_geometry), which read the 1-bit
    // G/C plane: the upload then sends the plane alone, an eighth of the bytes.  A guess that errs is harmless: a plan
    // that needs the bytes refuses a plane-only seqset (GAMS_ESTATE) and plan_and_run brings them.
    bool plane_params() const {
        return a.size >= 1 && a.size <= 255 && a.step >= 1 && a.step <= 32 && a.lag >= 2 &&
               (uint64_t)a.lag * (uint64_t)a.size <= 65535 && (uint64_t)a.lag * (uint64_t)a.size * (uint64_t)a.size < (1ull << 24) &&
               (uint64_t)(a.lag + 1) * (uint64_t)a.step + (uint64_t)a.size + 32 + 1024ull * (uint64_t)a.step <= 65520;
    }
    void bring_bytes();
    void start(const std::vector<const uint8_t *> &seqs);
    void start_gz(const std::vector<const uint8_t *> &blobs, const std::vector<uint64_t> &blob_len, unsigned threads);
    void start_gz_device(const std::vector<const uint8_t *> &blobs, const std::vector<uint64_t> &blob_len, unsigned threads);
    std::vector<std::string> finish() {
        std::vector<std::string> out = finish_rows();
        consumed = true;
        return out;
    }
    std::vector<std::string> finish_rows();
    bool consumed = false;         // the pass has finished (its results were read), and with it every DMA out of image / plane
    // stage clock: with st->sync the device is drained first, so the interval belongs to the stage just queued
    void mark(double WaveStages::*slot) {
        if (!st) return;
        if (st->sync) check(h, gams_gpu_sync(h));
        const double t = now_ms();
        st->*slot += t - t_mark;
        t_mark = t;
    }
    void plan_and_run();
    bool device_rows = false;      // the rows come as text from the device (gams_wave_rows_*): coverage links every overlap
};

void WaveJob::plan_and_run() {
    gams_wave_params_t prm{a.size, a.step, a.lag, a.threshold, a.influence};
    check(h, gams_wave_plan_create(h, sg.s, &prm, a.signal ? GAMS_WAVE_DENSE : GAMS_WAVE_PEAKS, &pg.p));
    check(h, gams_wave_plan_set_pipelined(h, pg.p, 1));   // finish() waits for this job, not the stream
    if (!a.signal) {
        // merged rows on the device when --coverage links every overlap (every value up to 1; the default is 0.2);
        // otherwise the peaks come back and merge_ints runs here
        std::vector<const char *> chr(ctgs.size());
        std::vector<int32_t> cs(ctgs.size());
        for (size_t c = 0; c < ctgs.size(); ++c) {
            chr[c] = ctgs[c].chr_id.c_str();
            cs[c] = ctgs[c].chr_start;
        }
        const int rc = gams_wave_rows_setup(h, pg.p, chr.data(), cs.data(), a.coverage);
        if (rc == GAMS_OK)
            device_rows = true;
        else if (rc != GAMS_EUNSUPPORTED)
            check(h, rc);
    }
    mark(&WaveStages::plan_ms);
    {
        int rc = gams_wave_run(h, pg.p);
        if (rc == GAMS_ESTATE && plane) {      // the plan reads bytes: today's path
            bring_bytes();
            rc = gams_wave_run(h, pg.p);
        }
        check(h, rc);
    }
    if (st) {
        int input = GAMS_WAVE_INPUT_BYTES;
        if (gams_wave_plan_last_input(h, pg.p, &input) == GAMS_OK) st->plane_input = input == GAMS_WAVE_INPUT_PLANE;
    }
    if (device_rows) check(h, gams_wave_rows_begin(h, pg.p));   // packing, merging, formatting and the copy queue behind the pass
    mark(&WaveStages::kernel_ms);
}

// the bytes of a plane-only seqset, for a plan that turned out to need them
void WaveJob::bring_bytes() {
    if (seqs_held)
        check(h, gams_seqset_upload_all(h, sg.s, seqs_held->data()));
    else
        check(h, gams_seqset_upload_ranges(h, sg.s, image, plane, 0, image_end));
}

void WaveJob::start(const std::vector<const uint8_t *> &seqs) {
    const uint32_t n = (uint32_t)ctgs.size();
    if (n == 0) return;
    t_mark = now_ms();
    std::vector<uint32_t> lens(n);
    for (uint32_t c = 0; c < n; ++c) lens[c] = (uint32_t)(ctgs[c].chr_end - ctgs[c].chr_start + 1);
    check(h, gams_seqset_create(h, n, lens.data(), &sg.s));
    if (!plane_params()) {
        check(h, gams_seqset_upload_all(h, sg.s, seqs.data()));
        mark(&WaveStages::upload_ms);
        plan_and_run();
        return;
    }
    // Plane-only upload: the workers classify the caller's buffers straight into a page-locked image of the plane
    // (no copy of the bases is made), pieces of at most 4 Mb so that a few long ctgs still spread over all of them;
    // the calling thread follows and hands every finished stretch of >= 1 MiB to the DMA engine.
    seqs_held = &seqs;
    std::vector<uint64_t> off(n);
    uint64_t bytes = 0;
    check(h, gams_seqset_layout(h, sg.s, off.data(), &bytes));
    image_end = off[n - 1] + lens[n - 1];
    void *blk = nullptr;
    check(h, gams_gpu_host_alloc(h, bytes / 8 + 8, &blk));
    plane = static_cast<uint8_t *>(blk);
    struct Piece {
        uint32_t ctg;
        uint64_t lo, hi;       // bases [lo, hi) of the ctg; lo a multiple of 8
        uint64_t stop;         // device-layout byte up to which the plane is complete once this piece is (gap included)
    };
    constexpr uint64_t kPieceBases = 4ull << 20;
    std::vector<Piece> pieces;
    for (uint32_t i = 0; i < n; ++i) {
        const uint64_t next = i + 1 < n ? off[i + 1] : ((image_end + 7) & ~7ull);
        uint64_t lo = 0;
        do {
            const uint64_t hi = std::min<uint64_t>(lens[i], lo + kPieceBases);
            pieces.push_back(Piece{i, lo, hi, hi == lens[i] ? next : off[i] + hi});
            lo = hi;
        } while (lo < lens[i]);
    }
    const uint32_t np = (uint32_t)pieces.size();
    const unsigned T = std::max(1u, std::min(std::min(16u, std::max(1u, std::thread::hardware_concurrency())), np));
    std::vector<std::atomic<uint8_t>> done(np);
    for (auto &d : done) d.store(0, std::memory_order_relaxed);
    std::atomic<uint32_t> next_piece{0};
    auto work = [&] {
        for (uint32_t k = next_piece.fetch_add(1); k < np; k = next_piece.fetch_add(1)) {
            const Piece &pc = pieces[k];
            uint8_t *dst = plane + ((off[pc.ctg] + pc.lo) >> 3);
            if (pc.hi > pc.lo) (void)gams_gc_plane(seqs[pc.ctg] + pc.lo, pc.hi - pc.lo, dst);
            // the alignment gap behind the ctg's last piece: bits zero
            const uint64_t filled = (off[pc.ctg] + pc.hi + 7) >> 3, want = (pc.stop + 7) >> 3;
            if (want > filled) std::memset(plane + filled, 0, want - filled);
            done[k].store(1, std::memory_order_release);
        }
    };
    std::vector<std::thread> pool;
    for (unsigned t = 0; t < T; ++t) pool.emplace_back(work);
    constexpr uint64_t kStretch = 8ull << 20;      // bases: 1 MiB of plane
    uint64_t lo = 0;
    int rc = GAMS_OK;
    for (uint32_t k = 0; k < np && rc == GAMS_OK; ++k) {
        while (!done[k].load(std::memory_order_acquire)) std::this_thread::yield();
        const uint64_t hi = k + 1 == np ? image_end : pieces[k].stop;
        if (hi - lo >= kStretch || k + 1 == np) {
            rc = gams_seqset_upload_ranges(h, sg.s, nullptr, plane, lo, hi);
            lo = hi & ~7ull;
        }
    }
    for (auto &th : pool) th.join();
    check(h, rc);
    mark(&WaveStages::upload_ms);
    plan_and_run();
    seqs_held = nullptr;       // the caller's vector is only promised for the length of this call
}

// The `seq:` values as the store holds them (gzip members, redis.rs:149-161): `threads` workers take the
// ctgs in order -- one ctg per worker at a time, like the reference's --parallel workers (wave.rs:288-299
// call get_seq -> decode_gz inside the worker) -- and inflate each one straight into a page-locked image
// of the device buffer; the calling thread follows them and hands every finished stretch of >= 8 MiB to
// the DMA engine (gams_seqset_upload_image): no staging copy, and the upload hides behind the inflate.
void WaveJob::start_gz(const std::vector<const uint8_t *> &blobs, const std::vector<uint64_t> &blob_len,
                       unsigned threads) {
    const uint32_t n = (uint32_t)ctgs.size();
    if (n == 0) return;
    t_mark = now_ms();
    std::vector<uint32_t> lens(n);
    for (uint32_t c = 0; c < n; ++c) lens[c] = (uint32_t)(ctgs[c].chr_end - ctgs[c].chr_start + 1);
    check(h, gams_seqset_create(h, n, lens.data(), &sg.s));
    std::vector<uint64_t> off(n);
    uint64_t bytes = 0;
    check(h, gams_seqset_layout(h, sg.s, off.data(), &bytes));
    void *blk = nullptr;
    check(h, gams_gpu_host_alloc(h, bytes, &blk));
    image = static_cast<uint8_t *>(blk);
    image_end = off[n - 1] + lens[n - 1];
    // parameters of the tiled fast kernels: every worker also classifies its ctg while the bases are in its cache, and
    // the plane goes to the device INSTEAD of the bytes (an eighth of the DMA; the image stays, should a plan want it)
    const bool send_plane = plane_params();
    if (send_plane) {
        void *pblk = nullptr;
        check(h, gams_gpu_host_alloc(h, bytes / 8 + 8, &pblk));
        plane = static_cast<uint8_t *>(pblk);
    }
    const unsigned T = std::max(1u, std::min(threads ? threads : 16u, n));
    if (st) st->threads = T;
    std::vector<std::atomic<uint8_t>> done(n);
    for (auto &d : done) d.store(0, std::memory_order_relaxed);
    std::atomic<uint32_t> next{0};
    std::atomic<bool> failed{false};
    std::exception_ptr err;
    std::mutex mu;
    auto work = [&] {
        try {
            for (uint32_t i = next.fetch_add(1); i < n && !failed.load(); i = next.fetch_add(1)) {
                const size_t got = decode_gz_into(blobs[i], (size_t)blob_len[i], image + off[i], lens[i]);
                if (got != lens[i])
                    throw Error(GAMS_EINVAL, "seq:" + ctgs[i].id + " inflates to " + std::to_string(got) +
                                                 " bases, the ctg record says " + std::to_string(lens[i]));
                // the alignment gap behind the ctg (never counted; kept defined)
                const uint64_t end = off[i] + lens[i], stop = i + 1 < n ? off[i + 1] : end;
                if (stop > end) std::memset(image + end, 0, stop - end);
                if (send_plane) {
                    (void)gams_gc_plane(image + off[i], lens[i], plane + (off[i] >> 3));
                    const uint64_t filled = (end + 7) >> 3, want = (stop + 7) >> 3;
                    if (want > filled) std::memset(plane + filled, 0, want - filled);
                }
                done[i].store(1, std::memory_order_release);
            }
        } catch (...) {
            std::lock_guard<std::mutex> lk(mu);
            if (!err) err = std::current_exception();
            failed.store(true);
        }
    };
    std::vector<std::thread> pool;
    for (unsigned t = 0; t < T; ++t) pool.emplace_back(work);
    // follow the workers: ctgs are taken in order, so they also finish roughly in order
    constexpr uint64_t kPiece = 8ull << 20;
    uint64_t lo = 0;
    int rc = GAMS_OK;
    for (uint32_t i = 0; i < n && rc == GAMS_OK; ++i) {
        while (!done[i].load(std::memory_order_acquire) && !failed.load()) std::this_thread::yield();
        if (failed.load()) break;
        const uint64_t hi = i + 1 < n ? off[i + 1] : off[i] + lens[i];
        if (hi - lo >= kPiece || i + 1 == n) {
            rc = send_plane ? gams_seqset_upload_ranges(h, sg.s, nullptr, plane, lo, hi)
                            : gams_seqset_upload_image(h, sg.s, image, lo, hi);
            lo = hi;
        }
    }
    for (auto &th : pool) th.join();
    if (err) std::rethrow_exception(err);
    check(h, rc);
    mark(&WaveStages::inflate_upload_ms);
    plan_and_run();
}

// The same values through the device inflater (seqset_upload_gz): bytes and plane are resident when it returns.
void WaveJob::start_gz_device(const std::vector<const uint8_t *> &blobs, const std::vector<uint64_t> &blob_len,
                              unsigned threads) {
    const uint32_t n = (uint32_t)ctgs.size();
    if (n == 0) return;
    t_mark = now_ms();
    std::vector<uint32_t> lens(n);
    for (uint32_t c = 0; c < n; ++c) lens[c] = (uint32_t)(ctgs[c].chr_end - ctgs[c].chr_start + 1);
    check(h, gams_seqset_create(h, n, lens.data(), &sg.s));
    const UploadGz went = seqset_upload_gz(h, sg.s, 0, blobs, blob_len, lens, threads);
    if (st) st->threads = went.host ? std::max(1u, std::min(threads ? threads : 16u, went.host)) : 0;
    mark(&WaveStages::inflate_upload_ms);
    plan_and_run();
}

std::vector<std::string> WaveJob::finish_rows() {
    const uint32_t n = (uint32_t)ctgs.size();
    std::vector<std::string> out(n);
    if (n == 0) return out;
    const float fsize = (float)a.size;
    if (a.signal) {                                                     // wave.rs:158-168
        // the rows as text from the device (gams_wave_signal_text); what it does not cover goes the host way below
        {
            std::vector<const char *> chr(n);
            std::vector<int32_t> cst(n);
            for (uint32_t c = 0; c < n; ++c) {
                chr[c] = ctgs[c].chr_id.c_str();
                cst[c] = ctgs[c].chr_start;
            }
            const char *text = nullptr;
            uint64_t bytes = 0;
            const uint64_t *off = nullptr;
            const int rc = gams_wave_signal_text(h, pg.p, chr.data(), cst.data(), &text, &bytes, &off);
            if (rc == GAMS_OK) {
                if (st) st->device_text = true;
                mark(&WaveStages::peaks_ms);
                const unsigned T = (unsigned)std::max<uint64_t>(
                    1, std::min<uint64_t>({16, std::thread::hardware_concurrency(), (uint64_t)n, bytes / (4u << 20) + 1}));
                std::atomic<uint32_t> next{0};
                std::vector<std::exception_ptr> errs(T);
                auto work = [&](unsigned t) {
                    try {
                        for (uint32_t c = next.fetch_add(1); c < n; c = next.fetch_add(1)) out[c].assign(text + off[c], text + off[c + 1]);
                    } catch (...) {
                        errs[t] = std::current_exception();
                    }
                };
                std::vector<std::thread> pool;
                for (unsigned t = 1; t < T; ++t) pool.emplace_back(work, t);
                work(0);
                for (auto &th : pool) th.join();
                for (auto &er : errs)
                    if (er) std::rethrow_exception(er);
                if (st) st->peaks = bytes;
                mark(&WaveStages::format_ms);
                return out;
            }
            if (rc != GAMS_EUNSUPPORTED && rc != GAMS_EINVAL) check(h, rc);
        }
        // fetch the dense rows on this thread (the handle's), format the ctgs on several
        std::vector<std::vector<uint32_t>> cnts(n);
        std::vector<std::vector<int8_t>> sigs(n);
        for (uint32_t c = 0; c < n; ++c) {
            const uint32_t nw = gams_wave_ctg_windows(pg.p, c);
            cnts[c].resize(nw ? nw : 1);
            sigs[c].resize(nw ? nw : 1);
            check(h, gams_wave_dense(h, pg.p, c, cnts[c].data(), sigs[c].data()));
        }
        parallel_for(n, ctg_threads(n), [&](uint32_t c) {
            const uint32_t nw = gams_wave_ctg_windows(pg.p, c);
            const std::vector<uint32_t> &cnt = cnts[c];
            const std::vector<int8_t> &sig = sigs[c];
            std::string &o = out[c];
            o.reserve((size_t)nw * 24);
            for (uint32_t i = 0; i < nw; ++i) {
                const int64_t s = (int64_t)ctgs[c].chr_start + (int64_t)i * a.step;
                o += ctgs[c].chr_id;
                o += ':';
                o += runlist(s, s + a.size - 1);
                o += '\t';
                o += fmt_f32((float)cnt[i] / fsize);                    // gc_content: count as f32 / len as f32
                o += '\t';
                o += std::to_string((int)sig[i]);
                o += '\n';
            }
        });
        return out;
    }
    if (device_rows) {
        const char *text = nullptr;
        uint64_t bytes = 0;
        const uint64_t *off = nullptr;
        check(h, gams_wave_rows_end(h, pg.p, &text, &bytes, &off));
        if (st) st->device_text = true;
        mark(&WaveStages::peaks_ms);
        for (uint32_t c = 0; c < n; ++c) out[c].assign(text + off[c], text + off[c + 1]);
        if (st) st->peaks = bytes;          // (text bytes fetched: the peak records stay on the device)
        mark(&WaveStages::format_ms);
        return out;
    }
    const gams_peak_t *pk = nullptr;
    uint64_t np = 0;
    check(h, gams_wave_peaks(h, pg.p, &pk, &np));
    mark(&WaveStages::peaks_ms);
    if (st) st->peaks = np;
    // peaks arrive ordered by (ctg, window): slice per ctg, then merge + format the ctgs on a few
    // host threads (the rows of one ctg depend on nothing else)
    std::vector<uint64_t> first(n + 1, np);
    {
        uint64_t q = 0;
        for (uint32_t c = 0; c < n; ++c) {
            first[c] = q;
            while (q < np && pk[q].ctg == c) ++q;
        }
        first[n] = q;
    }
    parallel_for(n, ctg_threads(n), [&](uint32_t c) {                                   // wave.rs:169-211
        const uint64_t q = first[c], q1 = first[c + 1];
        // crests and troughs separately (:172-186)
        std::vector<uint32_t> w[2];
        std::vector<uint64_t> src[2];
        for (uint64_t i = q; i < q1; ++i) {
            const int s = pk[i].signal == 1 ? 0 : 1;
            w[s].push_back(pk[i].window);
            src[s].push_back(i);
        }
        std::vector<int64_t> cmin(q1 - q), cmax(q1 - q);
        std::vector<char> merged(q1 - q, 0);
        for (int s = 0; s < 2; ++s) {
            Merge m = merge_ints(w[s], ctgs[c].chr_start, a.size, a.step, a.coverage);
            for (size_t k = 0; k < w[s].size(); ++k) {
                cmin[src[s][k] - q] = m.cmin[k];
                cmax[src[s][k] - q] = m.cmax[k];
                merged[src[s][k] - q] = m.in_graph[k];
            }
        }
        std::string &o = out[c];
        o.reserve((size_t)(q1 - q) * 24);
        for (uint64_t i = q; i < q1; ++i) {                             // window order (:191)
            const int64_t s = (int64_t)ctgs[c].chr_start + (int64_t)pk[i].window * a.step, e = s + a.size - 1;
            if (merged[i - q]) {
                // printed once, at the first member of the component (:201-206)
                if (s != cmin[i - q]) continue;
                o += ctgs[c].chr_id;
                o += "(+):";
                o += runlist(cmin[i - q], cmax[i - q]);
            } else {
                o += ctgs[c].chr_id;
                o += ':';
                o += runlist(s, e);
            }
            o += '\t';
            o += fmt_f32((float)pk[i].gc_count / fsize);
            o += '\t';
            o += std::to_string(pk[i].signal);
            o += '\n';
        }
    });
    mark(&WaveStages::format_ms);
    return out;
}

}  // namespace

std::vector<std::string> wave_proc_ctgs(gams_gpu_t *h, const std::vector<Ctg> &ctgs,
                                        const std::vector<const uint8_t *> &seqs, const WaveArgs &a, WaveStages *stages) {
    if (ctgs.size() != seqs.size()) throw Error(GAMS_EINVAL, "wave_proc_ctgs: ctgs/seqs size mismatch");
    const double t0 = now_ms();
    WaveJob job(h, ctgs, a);
    job.st = stages;
    job.start(seqs);
    std::vector<std::string> out = job.finish();
    if (stages) stages->total_ms += now_ms() - t0;
    return out;
}

std::vector<std::string> wave_proc_ctgs_gz(gams_gpu_t *h, const std::vector<Ctg> &ctgs,
                                           const std::vector<const uint8_t *> &blobs, const std::vector<uint64_t> &blob_len,
                                           const WaveArgs &a, unsigned threads, WaveStages *stages) {
    if (ctgs.size() != blobs.size() || ctgs.size() != blob_len.size())
        throw Error(GAMS_EINVAL, "wave_proc_ctgs_gz: ctgs/blobs size mismatch");
    const double t0 = now_ms();
    WaveJob job(h, ctgs, a);
    job.st = stages;
    job.start_gz(blobs, blob_len, threads);
    std::vector<std::string> out = job.finish();
    if (stages) stages->total_ms += now_ms() - t0;
    return out;
}

std::vector<std::string> wave_proc_ctgs_gz_device(gams_gpu_t *h, const std::vector<Ctg> &ctgs,
                                                  const std::vector<const uint8_t *> &blobs, const std::vector<uint64_t> &blob_len,
                                                  const WaveArgs &a, unsigned threads, WaveStages *stages) {
    if (ctgs.size() != blobs.size() || ctgs.size() != blob_len.size())
        throw Error(GAMS_EINVAL, "wave_proc_ctgs_gz_device: ctgs/blobs size mismatch");
    const double t0 = now_ms();
    WaveJob job(h, ctgs, a);
    job.st = stages;
    job.start_gz_device(blobs, blob_len, threads);
    std::vector<std::string> out = job.finish();
    if (stages) stages->total_ms += now_ms() - t0;
    return out;
}

std::string wave_proc_ctg(gams_gpu_t *h, const Ctg &ctg, const uint8_t *seq, const WaveArgs &a) {
    return wave_proc_ctgs(h, {ctg}, {seq}, a)[0];
}

std::vector<uint32_t> lpt_assign(const std::vector<uint64_t> &weights, uint32_t n_owners) {
    std::vector<size_t> order(weights.size());
    std::iota(order.begin(), order.end(), (size_t)0);
    std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return weights[a] > weights[b]; });
    using Load = std::pair<uint64_t, uint32_t>;  // (load, owner): smallest load first, then smallest owner
    std::priority_queue<Load, std::vector<Load>, std::greater<Load>> heap;
    for (uint32_t o = 0; o < n_owners; ++o) heap.push({0, o});
    std::vector<uint32_t> owner(weights.size(), 0);
    for (size_t i : order) {
        Load l = heap.top();
        heap.pop();
        owner[i] = l.second;
        heap.push({l.first + weights[i], l.second});
    }
    return owner;
}

namespace {

// what one device owns of a sharded interval problem: its groups (renumbered 0..), its queries
struct IntervalShare {
    std::vector<uint32_t> groups;       // global group ids, ascending
    std::vector<uint64_t> off;          // local group_off
    std::vector<uint64_t> q;            // global query indices, in query order
};

// groups -> owners by LPT on their sizes; queries follow their group
std::vector<IntervalShare> shard_intervals(uint32_t n_owners, uint32_t n_groups, const uint64_t *group_off,
                                           const uint32_t *q_group, uint64_t nq, std::vector<uint32_t> &local_id) {
    std::vector<uint64_t> weight(n_groups);
    for (uint32_t g = 0; g < n_groups; ++g) weight[g] = group_off[g + 1] - group_off[g] + 1;
    const std::vector<uint32_t> owner = lpt_assign(weight, n_owners);
    std::vector<IntervalShare> sh(n_owners);
    local_id.assign(n_groups, 0);
    for (uint32_t g = 0; g < n_groups; ++g) {
        IntervalShare &s = sh[owner[g]];
        local_id[g] = (uint32_t)s.groups.size();
        if (s.off.empty()) s.off.push_back(0);
        s.groups.push_back(g);
        s.off.push_back(s.off.back() + (group_off[g + 1] - group_off[g]));
    }
    for (auto &s : sh)
        if (s.off.empty()) s.off.push_back(0);
    for (uint64_t i = 0; i < nq; ++i)
        if (q_group[i] < n_groups) sh[owner[q_group[i]]].q.push_back(i);
    return sh;
}

template <typename F>
void run_shares(uint32_t n, F fn) {
    std::vector<std::exception_ptr> errs(n);
    std::vector<std::thread> pool;
    for (uint32_t g = 0; g < n; ++g)
        pool.emplace_back([&, g] {
            try {
                fn(g);
            } catch (...) {
                errs[g] = std::current_exception();
            }
        });
    for (auto &t : pool) t.join();
    for (auto &e : errs)
        if (e) std::rethrow_exception(e);
}

}  // namespace

// sw_proc_ctgs with the ctg table an rg file is located in given apart from the ctgs to process (NULL: those)
static std::vector<std::string> sw_proc_ctgs_located(gams_gpu_t *h, const std::vector<Ctg> &ctgs, const std::vector<const uint8_t *> &seqs,
                                              const std::vector<std::vector<Feature>> &features, const SwArgs &a,
                                              uint64_t batch_bytes, const std::map<std::string, std::vector<Range>> *rgs,
                                              double *index_ms, const char *rg_bytes, size_t rg_n,
                                              const std::vector<Ctg> *located_in, const std::vector<FileBytes> *rg_files,
                                              const SwGibbs *gb = nullptr);

// the rows of one ctg with the ΔG of every window as a tenth field, where the host formats them: dg[r] for row r, `{:.4}`
// (what "%.4f" of the widened value prints, whatever its size), nothing for NaN
static std::string sw_append_dg(const std::string &rows, const float *dg) {
    std::string out;
    out.reserve(rows.size() + rows.size() / 6);
    size_t at = 0, r = 0;
    while (at < rows.size()) {
        const size_t nl = rows.find('\n', at);
        out.append(rows, at, nl - at);
        out += '\t';
        if (dg[r] == dg[r]) {
            char buf[64];
            out.append(buf, (size_t)snprintf(buf, sizeof buf, "%.4f", (double)dg[r]));
        }
        out += '\n';
        at = nl + 1;
        ++r;
    }
    return out;
}

std::vector<std::string> sw_gibbs_proc_ctgs(gams_gpu_t *h, const std::vector<Ctg> &ctgs, const std::vector<const uint8_t *> &seqs,
                                            const std::vector<std::vector<Feature>> &features, const SwArgs &a,
                                            const SwGibbs &gb, uint64_t batch_bytes,
                                            const std::map<std::string, std::vector<Range>> *rgs, const char *rg_bytes,
                                            size_t rg_n) {
    if (!gb.table) throw Error(GAMS_EINVAL, "sw_gibbs: null table");
    return sw_proc_ctgs_located(h, ctgs, seqs, features, a, batch_bytes, rgs, nullptr, rg_bytes, rg_n, nullptr, nullptr, &gb);
}

std::string fmt_dg4(float v) {
    char buf[kGamsDg4MaxLen];
    return std::string(buf, gams_fmt_dg4(v, buf));
}

std::vector<std::string> sw_proc_ctgs_multi(const std::vector<gams_gpu_t *> &handles, const std::vector<Ctg> &ctgs,
                                            const std::vector<const uint8_t *> &seqs,
                                            const std::vector<std::vector<Feature>> &features, const SwArgs &a,
                                            const std::map<std::string, std::vector<Range>> *rgs, double *index_ms,
                                            const char *rg_bytes, size_t rg_n, const std::vector<FileBytes> *rg_files) {
    if (handles.empty()) throw Error(GAMS_EINVAL, "sw_proc_ctgs_multi: no handles");
    if (rgs && (rg_bytes || rg_files)) throw Error(GAMS_EINVAL, "sw: both the rg ranges and the bytes of an rg file were given");
    if (ctgs.size() != seqs.size() || ctgs.size() != features.size())
        throw Error(GAMS_EINVAL, "sw_proc_ctgs_multi: ctgs / seqs / features size mismatch");
    std::vector<uint64_t> weight(ctgs.size());
    for (size_t c = 0; c < ctgs.size(); ++c) weight[c] = features[c].size() + 1;
    const std::vector<uint32_t> owner = lpt_assign(weight, (uint32_t)handles.size());
    std::vector<std::string> out(ctgs.size());
    std::vector<double> ix_ms(handles.size(), 0.0);
    run_shares((uint32_t)handles.size(), [&](uint32_t d) {
        std::vector<Ctg> dc;
        std::vector<const uint8_t *> ds;
        std::vector<std::vector<Feature>> df;
        std::vector<size_t> where;
        for (size_t c = 0; c < ctgs.size(); ++c)
            if (owner[c] == d && !features[c].empty()) {
                dc.push_back(ctgs[c]);
                ds.push_back(seqs[c]);
                df.push_back(features[c]);
                where.push_back(c);
            }
        std::vector<std::string> rows =
            sw_proc_ctgs_located(handles[d], dc, ds, df, a, 256ull << 20, rgs, &ix_ms[d], rg_bytes, rg_n, &ctgs, rg_files);
        for (size_t k = 0; k < where.size(); ++k) out[where[k]] = std::move(rows[k]);
    });
    if (index_ms) *index_ms = *std::max_element(ix_ms.begin(), ix_ms.end());
    return out;
}

void count_multi(const std::vector<gams_gpu_t *> &handles, uint32_t n_groups, const uint64_t *group_off,
                 const uint32_t *starts, const uint32_t *stops, const uint32_t *q_group, const uint32_t *qs,
                 const uint32_t *qe, uint64_t nq, int32_t *count) {
    if (handles.empty()) throw Error(GAMS_EINVAL, "count_multi: no handles");
    std::vector<uint32_t> local_id;
    const std::vector<IntervalShare> sh = shard_intervals((uint32_t)handles.size(), n_groups, group_off, q_group, nq, local_id);
    for (uint64_t i = 0; i < nq; ++i)
        if (q_group[i] >= n_groups) count[i] = 0;                        // utils.rs:29-32: ctg without an index
    run_shares((uint32_t)handles.size(), [&](uint32_t d) {
        const IntervalShare &s = sh[d];
        if (s.q.empty()) return;
        gams_gpu_t *h = handles[d];
        std::vector<uint32_t> st, sp;
        for (uint32_t g : s.groups) {
            st.insert(st.end(), starts + group_off[g], starts + group_off[g + 1]);
            sp.insert(sp.end(), stops + group_off[g], stops + group_off[g + 1]);
        }
        gams_index_t *ix = nullptr;
        check(h, gams_index_create(h, (uint32_t)s.groups.size(), s.off.data(), st.data(), sp.data(), &ix));
        std::vector<uint32_t> g(s.q.size()), a(s.q.size()), b(s.q.size());
        for (size_t k = 0; k < s.q.size(); ++k) {
            g[k] = local_id[q_group[s.q[k]]];
            a[k] = qs[s.q[k]];
            b[k] = qe[s.q[k]];
        }
        std::vector<int32_t> out(s.q.size());
        const int rc = gams_gpu_count(h, ix, g.data(), a.data(), b.data(), s.q.size(), out.data());
        gams_index_destroy(h, ix);
        check(h, rc);
        for (size_t k = 0; k < s.q.size(); ++k) count[s.q[k]] = out[k];
    });
}

void cover_multi(const std::vector<gams_gpu_t *> &handles, uint32_t n_groups, const uint64_t *group_off,
                 const int32_t *lo, const int32_t *hi, const uint32_t *q_group, const int32_t *clip_lo,
                 const int32_t *clip_hi, const int32_t *qs, const int32_t *qe, uint64_t nq, float *prop) {
    if (handles.empty()) throw Error(GAMS_EINVAL, "cover_multi: no handles");
    std::vector<uint32_t> local_id;
    const std::vector<IntervalShare> sh = shard_intervals((uint32_t)handles.size(), n_groups, group_off, q_group, nq, local_id);
    for (uint64_t i = 0; i < nq; ++i)
        if (q_group[i] >= n_groups) prop[i] = 0.0f;                      // anno.rs:128: chr absent from the set
    run_shares((uint32_t)handles.size(), [&](uint32_t d) {
        const IntervalShare &s = sh[d];
        if (s.q.empty()) return;
        gams_gpu_t *h = handles[d];
        std::vector<int32_t> l, u;
        for (uint32_t g : s.groups) {
            l.insert(l.end(), lo + group_off[g], lo + group_off[g + 1]);
            u.insert(u.end(), hi + group_off[g], hi + group_off[g + 1]);
        }
        gams_spans_t *sp = nullptr;
        check(h, gams_spans_create(h, (uint32_t)s.groups.size(), s.off.data(), l.data(), u.data(), &sp));
        const size_t m = s.q.size();
        std::vector<uint32_t> g(m);
        std::vector<int32_t> cl(m), ch(m), a(m), b(m);
        for (size_t k = 0; k < m; ++k) {
            const uint64_t i = s.q[k];
            g[k] = local_id[q_group[i]];
            cl[k] = clip_lo[i];
            ch[k] = clip_hi[i];
            a[k] = qs[i];
            b[k] = qe[i];
        }
        std::vector<float> out(m);
        const int rc = gams_gpu_cover(h, sp, g.data(), cl.data(), ch.data(), a.data(), b.data(), m, out.data());
        gams_spans_destroy(h, sp);
        check(h, rc);
        for (size_t k = 0; k < m; ++k) prop[s.q[k]] = out[k];
    });
}

std::vector<std::string> wave_proc_ctgs_multi(const std::vector<gams_gpu_t *> &handles, const std::vector<Ctg> &ctgs,
                                              const std::vector<const uint8_t *> &seqs, const WaveArgs &a,
                                              uint64_t batch_bytes) {
    if (handles.empty()) throw Error(GAMS_EINVAL, "wave_proc_ctgs_multi: no handles");
    if (ctgs.size() != seqs.size()) throw Error(GAMS_EINVAL, "wave_proc_ctgs_multi: ctgs/seqs size mismatch");
    const uint32_t G = (uint32_t)handles.size();
    std::vector<uint64_t> weight(ctgs.size());
    for (size_t c = 0; c < ctgs.size(); ++c) {
        const int64_t n = gams_window_count((int64_t)ctgs[c].chr_end - ctgs[c].chr_start + 1, a.size, a.step);
        weight[c] = n > 0 ? (uint64_t)n : 0;
    }
    const std::vector<uint32_t> owner = lpt_assign(weight, G);
    std::vector<std::string> out(ctgs.size());
    std::vector<std::exception_ptr> errs(G);
    auto work = [&](uint32_t g) {
        try {
            // this device's ctgs, in ctg order, cut into batches of <= batch_bytes bases
            std::vector<size_t> mine;
            for (size_t c = 0; c < ctgs.size(); ++c)
                if (owner[c] == g) mine.push_back(c);
            // cut this device's share into batches, keep two jobs in flight
            std::vector<std::pair<size_t, size_t>> batches;   // [b, e) into `mine`
            for (size_t b = 0; b < mine.size();) {
                uint64_t bytes = 0;
                size_t e = b;
                while (e < mine.size()) {
                    const uint64_t len = (uint64_t)(ctgs[mine[e]].chr_end - ctgs[mine[e]].chr_start + 1);
                    if (e > b && bytes + len > batch_bytes) break;
                    bytes += len;
                    ++e;
                }
                batches.emplace_back(b, e);
                b = e;
            }
            auto make_job = [&](size_t k) {
                std::vector<Ctg> bc;
                std::vector<const uint8_t *> bs;
                for (size_t i = batches[k].first; i < batches[k].second; ++i) {
                    bc.push_back(ctgs[mine[i]]);
                    bs.push_back(seqs[mine[i]]);
                }
                std::unique_ptr<WaveJob> job(new WaveJob(handles[g], std::move(bc), a));
                job->start(bs);
                return job;
            };
            std::unique_ptr<WaveJob> cur, next;
            if (!batches.empty()) cur = make_job(0);
            for (size_t k = 0; k < batches.size(); ++k) {
                if (k + 1 < batches.size()) next = make_job(k + 1);     // queued behind batch k on the device
                std::vector<std::string> rows = cur->finish();
                for (size_t i = batches[k].first; i < batches[k].second; ++i)
                    out[mine[i]] = std::move(rows[i - batches[k].first]);
                cur = std::move(next);
            }
        } catch (...) {
            errs[g] = std::current_exception();
        }
    };
    std::vector<std::thread> threads;
    for (uint32_t g = 1; g < G; ++g) threads.emplace_back(work, g);
    work(0);
    for (auto &t : threads) t.join();
    for (auto &e : errs)
        if (e) std::rethrow_exception(e);
    return out;
}

// ---------------------------------------------------------------------------
// sw
// ---------------------------------------------------------------------------
namespace {
// TSV text of the rows of ONE ctg (sw.rs:152-190), `rows` in the device's order (feature, then M, L1.., R1..);
// the statistics when `actions` has GAMS_SW_GC, rg_count from cnt[] (one per row) when cnt is given
std::string sw_format_rows(const gams_sw_row_t *rows, uint64_t nrows, const Ctg &ctg, const std::vector<Feature> &features,
                           unsigned max_threads, uint32_t actions = GAMS_SW_GC, const int32_t *cnt = nullptr) {
    static const char *TYPES[3] = {"M", "L", "R"};
    // text of rows [r0, r1), r0 on a feature boundary (the serial number restarts per feature)
    auto format = [&](uint64_t r0, uint64_t r1, std::string &o) {
        o.reserve((r1 - r0) * 80);
        uint32_t cur = UINT32_MAX, sn = 0;
        for (uint64_t r = r0; r < r1; ++r) {                            // sw.rs:152-190
            const gams_sw_row_t &w = rows[r];
            if (w.feature != cur) {
                cur = w.feature;
                sn = 1;                                                 // sw.rs:148
            }
            o += "sw:";                                                 // sw.rs:153
            o += features[w.feature].id;
            o += ':';
            o += std::to_string(sn++);
            o += '\t';
            o += ctg.chr_id;                                            // sw.rs:157 Range::from(chr, min, max)
            o += ':';
            o += runlist(w.start, w.end);
            o += '\t';
            o += TYPES[w.type];
            o += '\t';
            o += std::to_string(w.distance);
            o += '\t';
            if (actions & GAMS_SW_GC) {
                o += fmt_f32(w.gc_content);                             // data.rs:61-67
                o += '\t';
                o += fmt_f32(w.gc_mean);
                o += '\t';
                o += fmt_f32(w.gc_stddev);
                o += '\t';
                o += fmt_f32(w.gc_cv);
            } else {
                o += "\t\t\t";                                          // data.rs:68-70: empty fields
            }
            o += '\t';
            if (cnt) o += std::to_string(cnt[r]);                       // data.rs:71-75 (else empty)
            o += '\n';
        }
    };
    std::string out;
    // a few host threads, each a run of whole features
    const unsigned T = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>({max_threads, std::thread::hardware_concurrency(), nrows / 20000}));
    if (T <= 1) {
        format(0, nrows, out);
        return out;
    }
    std::vector<uint64_t> cut(T + 1, nrows);
    cut[0] = 0;
    for (unsigned t = 1; t < T; ++t) {
        uint64_t b = std::max(cut[t - 1], nrows * t / T);
        while (b < nrows && b > 0 && rows[b].feature == rows[b - 1].feature) ++b;
        cut[t] = b;
    }
    std::vector<std::string> part(T);
    std::vector<std::thread> pool;
    for (unsigned t = 1; t < T; ++t) pool.emplace_back([&, t] { format(cut[t], cut[t + 1], part[t]); });
    format(cut[0], cut[1], part[0]);
    for (auto &th : pool) th.join();
    size_t total = 0;
    for (auto &x : part) total += x.size();
    out.reserve(total);
    for (auto &x : part) out += x;
    return out;
}

// idx:rg: (redis.rs:288-299) for the ctgs of one sw call that have features: one group per distinct ctg id that `rgs`
// has an entry for; group[c] = the group of ctgs[c], UINT32_MAX (count 0) for a ctg `rgs` lacks, which is reported once
// ("{ctg} not found in idx", utils.rs:30).  Intervals as Locator::set_rg_index stores them: [start, end + 1).
// From the bytes of an rg file instead (rg_bytes): the index and the groups are those of a Locator over `located_in`
// that loaded the file (Locator::set_rg_index_text); the Locator owns the index.
struct RgIndex {
    gams_gpu_t *h;
    gams_index_t *ix = nullptr;
    std::unique_ptr<Locator> loc;
    std::vector<uint32_t> group;
    explicit RgIndex(gams_gpu_t *hh) : h(hh) {}
    ~RgIndex() {
        if (ix && !loc) gams_index_destroy(h, ix);
    }
};
void sw_rg_index(RgIndex &out, const std::vector<Ctg> &ctgs, const std::vector<std::vector<Feature>> &features,
                 const std::map<std::string, std::vector<Range>> *rgs, double *index_ms, const char *rg_bytes = nullptr,
                 size_t rg_n = 0, const std::vector<Ctg> *located_in = nullptr, const std::vector<FileBytes> *rg_files = nullptr) {
    if (!rgs && !rg_bytes && !rg_files) throw Error(GAMS_EINVAL, "sw: --action count needs the rg ranges");
    const auto t0 = std::chrono::steady_clock::now();
    out.group.assign(ctgs.size(), UINT32_MAX);
    if (rg_bytes || rg_files) {
        std::vector<Ctg> table;                                          // a ctg given twice is one ctg of the table
        std::set<std::string> ids;
        for (const Ctg &c : located_in ? *located_in : ctgs)
            if (ids.insert(c.id).second) table.push_back(c);
        out.loc.reset(new Locator(out.h, table));
        if (rg_files)
            out.loc->set_rg_index_text(*rg_files);
        else
            out.loc->set_rg_index_text(rg_bytes, rg_n);
        out.ix = out.loc->rg_index();
        std::set<std::string> told;
        for (size_t c = 0; c < ctgs.size(); ++c) {
            if (features[c].empty()) continue;
            out.group[c] = out.loc->rg_group_of(ctgs[c].id);
            if (out.group[c] == UINT32_MAX && told.insert(ctgs[c].id).second)
                fprintf(stderr, "%s not found in idx\n", ctgs[c].id.c_str());
        }
        if (index_ms) *index_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        return;
    }
    std::map<std::string, uint32_t> seen;
    std::vector<uint64_t> off{0};
    std::vector<uint32_t> st, sp;
    uint32_t g = 0;
    for (size_t c = 0; c < ctgs.size(); ++c) {
        if (features[c].empty()) continue;
        auto was = seen.find(ctgs[c].id);
        if (was != seen.end()) {
            out.group[c] = was->second;
            continue;
        }
        auto it = rgs->find(ctgs[c].id);
        if (it == rgs->end()) {
            fprintf(stderr, "%s not found in idx\n", ctgs[c].id.c_str());
            seen[ctgs[c].id] = UINT32_MAX;
            continue;
        }
        for (const Range &r : it->second) {
            st.push_back((uint32_t)r.start);
            sp.push_back((uint32_t)r.end + 1u);
        }
        off.push_back(st.size());
        seen[ctgs[c].id] = out.group[c] = g++;
    }
    check(out.h, gams_index_create(out.h, g, off.data(), st.data(), sp.data(), &out.ix));
    if (index_ms) *index_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}
}  // namespace

std::string sw_proc_ctg(gams_gpu_t *h, const Ctg &ctg, const uint8_t *seq, const std::vector<Feature> &features,
                        const SwArgs &a, const std::map<std::string, std::vector<Range>> *rgs, const char *rg_bytes,
                        size_t rg_n, const std::vector<FileBytes> *rg_files) {
    if (rgs && (rg_bytes || rg_files)) throw Error(GAMS_EINVAL, "sw: both the rg ranges and the bytes of an rg file were given");
    const uint32_t nf = (uint32_t)features.size();
    if (nf == 0) return std::string();
    uint32_t len = (uint32_t)(ctg.chr_end - ctg.chr_start + 1);
    SeqSetGuard sg{h};
    check(h, gams_seqset_create(h, 1, &len, &sg.s));
    check(h, gams_seqset_upload(h, sg.s, 0, seq));
    std::vector<int32_t> fs(nf), fe(nf);
    for (uint32_t f = 0; f < nf; ++f) {
        fs[f] = features[f].start;
        fe[f] = features[f].end;
    }
    uint64_t nrows = 0;
    check(h, gams_gpu_sw(h, sg.s, 0, ctg.chr_start, fs.data(), fe.data(), nf, a.size, a.max, a.resize, nullptr, 0,
                         &nrows));
    std::vector<gams_sw_row_t> rows(nrows ? nrows : 1);
    check(h, gams_gpu_sw(h, sg.s, 0, ctg.chr_start, fs.data(), fe.data(), nf, a.size, a.max, a.resize,
                         rows.data(), nrows, &nrows));
    if (!(a.actions & GAMS_SW_COUNT)) return sw_format_rows(rows.data(), nrows, ctg, features, 8, a.actions);
    // rg_count through the array entry (and this host formatter), the path sw_proc_ctgs falls back to
    RgIndex rx(h);
    sw_rg_index(rx, std::vector<Ctg>{ctg}, std::vector<std::vector<Feature>>{features}, rgs, nullptr, rg_bytes, rg_n, nullptr, rg_files);
    const uint32_t zero = 0;
    const uint64_t feat_off[2] = {0, nf};
    std::vector<int32_t> cnt(nrows ? nrows : 1);
    check(h, gams_gpu_sw_count_batch(h, sg.s, 1, &zero, &ctg.chr_start, feat_off, fs.data(), fe.data(), a.size, a.max,
                                     rx.ix, rx.group.data(), cnt.data(), nrows, nullptr, &nrows));
    return sw_format_rows(rows.data(), nrows, ctg, features, 8, a.actions, cnt.data());
}

// Several ctgs on one handle: their sequences go into one seqset per batch of <= batch_bytes bases, all
// features of a batch through ONE gams_gpu_sw_batch call (one upload, one gc index, one launch, one readback
// into page-locked memory), and the rows of the batch's ctgs are formatted on host threads, a ctg each.
std::vector<std::string> sw_proc_ctgs(gams_gpu_t *h, const std::vector<Ctg> &ctgs, const std::vector<const uint8_t *> &seqs,
                                      const std::vector<std::vector<Feature>> &features, const SwArgs &a,
                                      uint64_t batch_bytes, const std::map<std::string, std::vector<Range>> *rgs,
                                      double *index_ms, const char *rg_bytes, size_t rg_n, const std::vector<FileBytes> *rg_files) {
    return sw_proc_ctgs_located(h, ctgs, seqs, features, a, batch_bytes, rgs, index_ms, rg_bytes, rg_n, nullptr, rg_files);
}

static std::vector<std::string> sw_proc_ctgs_located(gams_gpu_t *h, const std::vector<Ctg> &ctgs, const std::vector<const uint8_t *> &seqs,
                                              const std::vector<std::vector<Feature>> &features, const SwArgs &a,
                                              uint64_t batch_bytes, const std::map<std::string, std::vector<Range>> *rgs,
                                              double *index_ms, const char *rg_bytes, size_t rg_n,
                                              const std::vector<Ctg> *located_in, const std::vector<FileBytes> *rg_files,
                                              const SwGibbs *gb) {
    if (rgs && (rg_bytes || rg_files)) throw Error(GAMS_EINVAL, "sw: both the rg ranges and the bytes of an rg file were given");
    gams_seqset_t *const resident = gb ? gb->resident : nullptr;   // sw_gibbs_proc_ctgs: the bases may be on the device already
    if ((!resident && ctgs.size() != seqs.size()) || ctgs.size() != features.size())
        throw Error(GAMS_EINVAL, "sw_proc_ctgs: ctgs / seqs / features size mismatch");
    std::vector<std::string> out(ctgs.size());
    std::vector<size_t> todo;                                           // ctgs with features, in ctg order
    for (size_t c = 0; c < ctgs.size(); ++c)
        if (!features[c].empty()) todo.push_back(c);
    const bool do_count = (a.actions & GAMS_SW_COUNT) != 0;
    RgIndex rx(h);                                                      // -a count: the rgs of this call's ctgs, once
    if (do_count && !todo.empty()) sw_rg_index(rx, ctgs, features, rgs, index_ms, rg_bytes, rg_n, located_in, rg_files);
    for (size_t b = 0; b < todo.size();) {
        uint64_t bytes = 0;
        size_t e = b;
        while (e < todo.size()) {
            const uint64_t len = (uint64_t)(ctgs[todo[e]].chr_end - ctgs[todo[e]].chr_start + 1);
            if (!resident && e > b && bytes + len > batch_bytes) break;   // (a resident seqset: one batch)
            bytes += len;
            ++e;
        }
        const uint32_t n = (uint32_t)(e - b);
        std::vector<uint32_t> lens(n), index(n);
        std::vector<const uint8_t *> ptrs(n);
        std::vector<int32_t> chr_start(n);
        std::vector<uint64_t> feat_off(n + 1, 0);
        for (uint32_t k = 0; k < n; ++k) {
            const Ctg &c = ctgs[todo[b + k]];
            lens[k] = (uint32_t)(c.chr_end - c.chr_start + 1);
            ptrs[k] = resident ? nullptr : seqs[todo[b + k]];
            index[k] = resident ? (gb->slots ? gb->slots[todo[b + k]] : (uint32_t)todo[b + k]) : k;
            chr_start[k] = c.chr_start;
            feat_off[k + 1] = feat_off[k] + features[todo[b + k]].size();
        }
        std::vector<int32_t> fs(feat_off[n]), fe(feat_off[n]);
        for (uint32_t k = 0; k < n; ++k) {
            const std::vector<Feature> &fv = features[todo[b + k]];
            for (size_t f = 0; f < fv.size(); ++f) {
                fs[feat_off[k] + f] = fv[f].start;
                fe[feat_off[k] + f] = fv[f].end;
            }
        }
        std::vector<uint32_t> rg_group(do_count ? n : 0);
        for (uint32_t k = 0; k < rg_group.size(); ++k) rg_group[k] = rx.group[todo[b + k]];
        SeqSetGuard sg{h};
        if (!resident) check(h, gams_seqset_create(h, n, lens.data(), &sg.s));
        gams_seqset_t *const set = resident ? resident : sg.s;
        // -a count alone reads no sequence byte on the device path: the bases go up only when a gc, the ΔG column or the
        // rows of the fallback below need them
        bool uploaded = resident != nullptr;
        auto upload = [&]() {
            if (!uploaded) check(h, gams_seqset_upload_all(h, set, ptrs.data()));
            uploaded = true;
        };
        if ((a.actions & GAMS_SW_GC) || gb) upload();
        std::vector<uint64_t> row_off(n + 1, 0);
        uint64_t nrows = 0;
        {
            // the rows' text straight from the device (gams_gpu_sw_text); values it does not cover send the batch
            // down the host formatter below
            std::vector<const char *> chr(n), ids(feat_off[n]);
            for (uint32_t k = 0; k < n; ++k) {
                chr[k] = ctgs[todo[b + k]].chr_id.c_str();
                const std::vector<Feature> &fv = features[todo[b + k]];
                for (size_t f = 0; f < fv.size(); ++f) ids[feat_off[k] + f] = fv[f].id.c_str();
            }
            const char *text = nullptr;
            uint64_t tbytes = 0;
            const uint64_t *toff = nullptr;
            const int rc = gb ? gams_gpu_sw_text_dg(h, set, n, index.data(), chr.data(), chr_start.data(), feat_off.data(),
                                                    fs.data(), fe.data(), ids.data(), a.size, a.max, a.resize, a.actions,
                                                    rx.ix, rg_group.data(), gb->table, &text, &tbytes, &toff, &nrows)
                              : gams_gpu_sw_text_actions(h, set, n, index.data(), chr.data(), chr_start.data(), feat_off.data(),
                                                         fs.data(), fe.data(), ids.data(), a.size, a.max, a.resize, a.actions,
                                                         rx.ix, rg_group.data(), &text, &tbytes, &toff, &nrows);
            if (rc == GAMS_OK) {
                // proc_ctg's Strings: slices of the page-locked text, copied by a few host threads (one thread moves
                // ~10 GB/s; 313 MB for the 4.1 M rows of a 30-Mb chromosome)
                const unsigned T = (unsigned)std::max<uint64_t>(
                    1, std::min<uint64_t>({16, std::thread::hardware_concurrency(), (uint64_t)n, tbytes / (4u << 20) + 1}));
                parallel_for(n, T, [&](uint32_t k) { out[todo[b + k]].assign(text + toff[k], text + toff[k + 1]); });
                b = e;
                continue;
            }
            if (rc != GAMS_EUNSUPPORTED) check(h, rc);
        }
        upload();
        check(h, gams_gpu_sw_batch(h, set, n, index.data(), chr_start.data(), feat_off.data(), fs.data(), fe.data(),
                                   a.size, a.max, a.resize, nullptr, 0, row_off.data(), &nrows));
        // rows land in page-locked memory: the readback runs at the rate of the link
        struct Pinned {
            gams_gpu_t *h;
            void *p = nullptr;
            ~Pinned() { if (p) gams_gpu_host_free(h, p); }
        } pin{h};
        check(h, gams_gpu_host_alloc(h, std::max<uint64_t>(nrows, 1) * sizeof(gams_sw_row_t), &pin.p));
        gams_sw_row_t *rows = static_cast<gams_sw_row_t *>(pin.p);
        check(h, gams_gpu_sw_batch(h, set, n, index.data(), chr_start.data(), feat_off.data(), fs.data(), fe.data(),
                                   a.size, a.max, a.resize, rows, nrows, row_off.data(), &nrows));
        std::vector<int32_t> cnt(do_count ? std::max<uint64_t>(nrows, 1) : 0);
        if (do_count)
            check(h, gams_gpu_sw_count_batch(h, set, n, index.data(), chr_start.data(), feat_off.data(), fs.data(), fe.data(),
                                             a.size, a.max, rx.ix, rg_group.data(), cnt.data(), nrows, nullptr, &nrows));
        std::vector<float> dg(gb ? std::max<uint64_t>(nrows, 1) : 0);
        if (gb)
            check(h, gams_gpu_sw_dg_batch(h, set, n, index.data(), chr_start.data(), feat_off.data(), fs.data(), fe.data(),
                                          a.size, a.max, gb->table, dg.data(), nrows, nullptr, &nrows));
        // format: ctgs of the batch dealt to a few host threads
        const unsigned T = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>({16, std::thread::hardware_concurrency(), (uint64_t)n}));
        parallel_for(n, T, [&](uint32_t k) {
            out[todo[b + k]] = sw_format_rows(rows + row_off[k], row_off[k + 1] - row_off[k], ctgs[todo[b + k]],
                                              features[todo[b + k]], T > 1 ? 1 : 8, a.actions,
                                              do_count ? cnt.data() + row_off[k] : nullptr);
            if (gb) out[todo[b + k]] = sw_append_dg(out[todo[b + k]], dg.data() + row_off[k]);
        });
        b = e;
    }
    return out;
}

// ---------------------------------------------------------------------------
// locate
// ---------------------------------------------------------------------------
Locator::Locator(gams_gpu_t *h, const std::vector<Ctg> &ctgs) : h_(h), ctgs_(ctgs) {
    // redis.rs:236-258: per chr a Lapper of (chr_start, chr_end + 1, ctg_id)
    std::map<std::string, std::vector<uint32_t>> by_chr;
    for (uint32_t i = 0; i < ctgs_.size(); ++i) {
        by_chr[ctgs_[i].chr_id].push_back(i);
        ctg_slot_[ctgs_[i].id] = i;
    }
    std::vector<uint64_t> off{0};
    std::vector<uint32_t> st, sp;
    std::vector<Ctg> ordered;
    uint32_t g = 0;
    for (auto &kv : by_chr) {
        chr_group_[kv.first] = g++;
        for (uint32_t i : kv.second) {
            st.push_back((uint32_t)ctgs_[i].chr_start);
            sp.push_back((uint32_t)ctgs_[i].chr_end + 1u);
            ordered.push_back(ctgs_[i]);
        }
        off.push_back(st.size());
    }
    ctgs_ = ordered;  // hit indices refer to this order
    ctg_slot_.clear();
    for (uint32_t i = 0; i < ctgs_.size(); ++i) ctg_slot_[ctgs_[i].id] = i;
    for (const Ctg &c : ctgs) given_.push_back(ctg_slot_.at(c.id));
    check(h_, gams_index_create(h_, g, off.data(), st.data(), sp.data(), &ctg_ix_));
}

Locator::~Locator() {
    if (ctg_ix_) gams_index_destroy(h_, ctg_ix_);
    if (rg_ix_) gams_index_destroy(h_, rg_ix_);
    if (chr_names_) gams_names_destroy(h_, chr_names_);
    if (ctg_ids_) gams_names_destroy(h_, ctg_ids_);
}

const Ctg *Locator::ctg(const std::string &id) const {
    auto it = ctg_slot_.find(id);
    return it == ctg_slot_.end() ? nullptr : &ctgs_[it->second];
}

void Locator::set_rg_index(const std::map<std::string, std::vector<Range>> &rg_of_ctg) {
    if (rg_ix_) {
        gams_index_destroy(h_, rg_ix_);
        rg_ix_ = nullptr;
    }
    rg_group_.clear();
    std::vector<uint64_t> off{0};
    std::vector<uint32_t> st, sp;
    uint32_t g = 0;
    for (auto &kv : rg_of_ctg) {                                        // redis.rs:288-299
        rg_group_[kv.first] = g++;
        for (const Range &r : kv.second) {
            st.push_back((uint32_t)r.start);
            sp.push_back((uint32_t)r.end + 1u);
        }
        off.push_back(st.size());
    }
    check(h_, gams_index_create(h_, g, off.data(), st.data(), sp.data(), &rg_ix_));
}

uint32_t Locator::rg_group_of(const std::string &ctg_id) const {
    auto it = rg_group_.find(ctg_id);
    return it == rg_group_.end() ? UINT32_MAX : it->second;
}

void Locator::set_rg_index_text(const char *bytes, size_t n, bool *device) {
    if (device) *device = false;
    text_tables();
    gams_index_t *ix = nullptr;
    std::vector<uint32_t> group(std::max<size_t>(ctgs_.size(), 1), UINT32_MAX);
    uint64_t kept = 0;
    const int rc = gams_index_create_range_text(h_, ctg_ix_, chr_names_, bytes, n, &ix, group.data(), &kept);
    if (rc == GAMS_EUNSUPPORTED) {                                       // the host passes over the lines
        set_rg_index(read_range(*this, text_lines(bytes, n)));
        return;
    }
    check(h_, rc);
    if (rg_ix_) gams_index_destroy(h_, rg_ix_);
    rg_ix_ = ix;
    rg_group_.clear();
    for (size_t i = 0; i < ctgs_.size(); ++i)
        if (group[i] != UINT32_MAX) rg_group_[ctgs_[i].id] = group[i];
    if (device) *device = true;
}

void Locator::set_rg_index_text(const std::vector<FileBytes> &files, bool *device) {
    if (device) *device = false;
    text_tables();
    std::vector<const char *> fb;
    std::vector<uint64_t> fn;
    for (const FileBytes &f : files) {
        fb.push_back(f.first);
        fn.push_back(f.second);
    }
    gams_index_t *ix = nullptr;
    std::vector<uint32_t> group(std::max<size_t>(ctgs_.size(), 1), UINT32_MAX);
    uint64_t kept = 0;
    const int rc = gams_index_create_range_files(h_, ctg_ix_, chr_names_, (uint32_t)files.size(), fb.data(), fn.data(), &ix,
                                                 group.data(), &kept);
    if (rc == GAMS_EUNSUPPORTED) {                                       // read_range per file, the buckets appended
        std::map<std::string, std::vector<Range>> all;
        for (const FileBytes &f : files)
            for (auto &kv : read_range(*this, text_lines(f.first, f.second))) {
                std::vector<Range> &b = all[kv.first];
                b.insert(b.end(), kv.second.begin(), kv.second.end());
            }
        set_rg_index(all);
        return;
    }
    check(h_, rc);
    if (rg_ix_) gams_index_destroy(h_, rg_ix_);
    rg_ix_ = ix;
    rg_group_.clear();
    for (size_t i = 0; i < ctgs_.size(); ++i)
        if (group[i] != UINT32_MAX) rg_group_[ctgs_[i].id] = group[i];
    if (device) *device = true;
}

std::vector<std::string> Locator::find(const std::vector<Range> &rgs) {
    const uint64_t nq = rgs.size();
    std::vector<uint32_t> grp(nq), qs(nq), qe(nq);
    for (uint64_t i = 0; i < nq; ++i) {
        auto it = chr_group_.find(rgs[i].chr);                          // utils.rs:11-13
        grp[i] = it == chr_group_.end() ? UINT32_MAX : it->second;
        qs[i] = (uint32_t)rgs[i].start;                                 // utils.rs:16: find(start, end)
        qe[i] = (uint32_t)rgs[i].end;
    }
    std::vector<int64_t> hit(nq ? nq : 1);
    check(h_, gams_gpu_locate(h_, ctg_ix_, grp.data(), qs.data(), qe.data(), nq, hit.data()));
    std::vector<std::string> out(nq);
    for (uint64_t i = 0; i < nq; ++i)
        if (hit[i] >= 0) out[i] = ctgs_[(size_t)hit[i]].id;
    return out;
}

std::string Locator::locate(const std::vector<std::string> &rgs, bool is_count) {
    // Range strings are parsed and rows are formatted on several host threads (contiguous shares of the lines, joined
    // in order); the lookups in between are one device call each.  Nothing string-valued is kept per line between the
    // stages: a share keeps (chromosome group, start, end, line number) of its valid ranges, the ctg of a hit is an index
    // into the ctg table, and the rg group of a ctg is a table by that index (1e6 lines: 169 -> ~40 ms, most of it
    // Range::from_str).
    const unsigned T = (unsigned)std::max<size_t>(1, std::min<size_t>({16, std::thread::hardware_concurrency(), rgs.size() / 20000}));
    auto cut = [&](size_t n, unsigned t) { return n * t / T; };
    struct Share {
        std::vector<uint32_t> grp, qs, qe;
        std::vector<size_t> src;
        size_t first = 0;               // position of the share's first valid range in the joined arrays
        std::string out;
    };
    std::vector<Share> sh(T);
    run_shares(T, [&](uint32_t t) {
        Share &m = sh[t];
        const std::string *last_chr = nullptr;
        uint32_t last_grp = UINT32_MAX;
        std::string keep;
        for (size_t i = cut(rgs.size(), t); i < cut(rgs.size(), t + 1); ++i) {   // locate.rs:111-116
            const Range r = Range::from_str(rgs[i]);
            if (!r.valid) continue;
            if (!last_chr || r.chr != keep) {                                   // utils.rs:11-13 (runs of one chromosome are the rule)
                auto it = chr_group_.find(r.chr);
                last_grp = it == chr_group_.end() ? UINT32_MAX : it->second;
                keep = r.chr;
                last_chr = &keep;
            }
            m.grp.push_back(last_grp);
            m.qs.push_back((uint32_t)r.start);                                  // utils.rs:16: find(start, end)
            m.qe.push_back((uint32_t)r.end);
            m.src.push_back(i);
        }
    });
    size_t nq = 0;
    for (Share &m : sh) {
        m.first = nq;
        nq += m.src.size();
    }
    std::vector<uint32_t> grp(nq), qs(nq), qe(nq);
    run_shares(T, [&](uint32_t t) {
        const Share &m = sh[t];
        std::copy(m.grp.begin(), m.grp.end(), grp.begin() + m.first);
        std::copy(m.qs.begin(), m.qs.end(), qs.begin() + m.first);
        std::copy(m.qe.begin(), m.qe.end(), qe.begin() + m.first);
    });
    std::vector<int64_t> hit(nq ? nq : 1);
    check(h_, gams_gpu_locate(h_, ctg_ix_, grp.data(), qs.data(), qe.data(), nq, hit.data()));
    auto join = [&] {
        std::string out;
        size_t bytes = 0;
        for (auto &m : sh) bytes += m.out.size();
        out.reserve(bytes);
        for (auto &m : sh) out += m.out;
        return out;
    };
    if (!is_count) {
        run_shares(T, [&](uint32_t t) {
            Share &m = sh[t];
            for (size_t j = 0; j < m.src.size(); ++j) {
                const int64_t c = hit[m.first + j];
                if (c < 0) continue;                                            // locate.rs:120-122
                m.out += rgs[m.src[j]];
                m.out += '\t';
                m.out += ctgs_[(size_t)c].id;                                   // locate.rs:139
                m.out += '\n';
            }
        });
        return join();
    }
    if (!rg_ix_) throw Error(GAMS_ESTATE, "locate --count: no rg index loaded");
    // rg group of every ctg of the table (UINT32_MAX: the ctg has no entry in the index)
    std::vector<uint32_t> group_of(ctgs_.size(), UINT32_MAX);
    for (size_t c = 0; c < ctgs_.size(); ++c) {
        auto it = rg_group_.find(ctgs_[c].id);
        if (it != rg_group_.end()) group_of[c] = it->second;
    }
    // the located ranges, in line order: the reference counts only those (locate.rs:120-122, :135-137)
    std::vector<size_t> kept(T + 1, 0);
    for (unsigned t = 0; t < T; ++t) {
        size_t n = 0;
        for (size_t j = 0; j < sh[t].src.size(); ++j) n += hit[sh[t].first + j] >= 0;
        kept[t + 1] = kept[t] + n;
    }
    const size_t nk = kept[T];
    std::vector<uint32_t> cg(nk), cs(nk), ce(nk);
    run_shares(T, [&](uint32_t t) {
        const Share &m = sh[t];
        size_t o = kept[t];
        for (size_t j = 0; j < m.src.size(); ++j) {
            const int64_t c = hit[m.first + j];
            if (c < 0) continue;
            cg[o] = group_of[(size_t)c];
            cs[o] = qs[m.first + j];
            ce[o] = qe[m.first + j];
            ++o;
        }
    });
    for (size_t o = 0; o < nk; ++o)                                             // utils.rs:30 (rare: serial is fine)
        if (cg[o] == UINT32_MAX) {
            // (which ctg: recomputed only on this path)
            size_t seen = 0;
            for (unsigned t = 0; t < T && seen <= o; ++t)
                for (size_t j = 0; j < sh[t].src.size(); ++j) {
                    const int64_t c = hit[sh[t].first + j];
                    if (c < 0) continue;
                    if (seen++ == o) fprintf(stderr, "%s not found in idx\n", ctgs_[(size_t)c].id.c_str());
                }
        }
    std::vector<int32_t> cnt(nk ? nk : 1);
    check(h_, gams_gpu_count(h_, rg_ix_, cg.data(), cs.data(), ce.data(), nk, cnt.data()));
    run_shares(T, [&](uint32_t t) {
        Share &m = sh[t];
        size_t o = kept[t];
        char num[16];
        for (size_t j = 0; j < m.src.size(); ++j) {
            if (hit[m.first + j] < 0) continue;
            m.out += rgs[m.src[j]];
            m.out += '\t';
            auto r = std::to_chars(num, num + sizeof num, cnt[o++]);                // locate.rs:137
            m.out.append(num, r.ptr);
            m.out += '\n';
        }
    });
    return join();
}

void Locator::text_tables() {
    if (chr_names_) return;
    std::vector<const char *> chr(chr_group_.size()), ids(ctgs_.size());
    for (auto &kv : chr_group_) chr[kv.second] = kv.first.c_str();
    for (size_t i = 0; i < ctgs_.size(); ++i) ids[i] = ctgs_[i].id.c_str();
    check(h_, gams_names_create(h_, (uint32_t)chr.size(), chr.data(), &chr_names_));
    check(h_, gams_names_create(h_, (uint32_t)ids.size(), ids.data(), &ctg_ids_));
}

std::string Locator::locate_text(const char *bytes, size_t n, bool is_count, bool *device) {
    if (device) *device = false;
    if (is_count && !rg_ix_) throw Error(GAMS_ESTATE, "locate --count: no rg index loaded");
    text_tables();
    const char *text = nullptr;
    uint64_t text_bytes = 0, rows = 0;
    int rc;
    if (is_count) {
        std::vector<uint32_t> group_of(ctgs_.size(), UINT32_MAX);    // rg group of every ctg of the table
        for (size_t c = 0; c < ctgs_.size(); ++c) {
            auto it = rg_group_.find(ctgs_[c].id);
            if (it != rg_group_.end()) group_of[c] = it->second;
        }
        rc = gams_gpu_count_text(h_, ctg_ix_, chr_names_, rg_ix_, group_of.data(), bytes, n, &text, &text_bytes, &rows);
    } else {
        rc = gams_gpu_locate_text(h_, ctg_ix_, chr_names_, ctg_ids_, bytes, n, &text, &text_bytes, &rows);
    }
    if (rc == GAMS_EUNSUPPORTED) {                                       // the array path, from the lines' first fields
        std::vector<std::string> rgs = text_lines(bytes, n);
        for (std::string &s : rgs) {
            const size_t tab = s.find('\t');                             // locate.rs:89-91
            if (tab != std::string::npos) s.resize(tab);
        }
        return locate(rgs, is_count);
    }
    check(h_, rc);
    if (device) *device = true;
    return std::string(text, (size_t)text_bytes);
}

std::string Locator::locate_seq(const std::vector<std::string> &rgs,
                                const std::map<std::string, std::string> &seq_of) {
    std::vector<Range> valid;
    std::vector<size_t> src;
    for (size_t i = 0; i < rgs.size(); ++i) {
        Range r = Range::from_str(rgs[i]);
        if (!r.valid) continue;
        r.strand.clear();
        valid.push_back(r);
        src.push_back(i);
    }
    std::vector<std::string> ctg_ids = find(valid);
    std::string out;
    for (size_t k = 0; k < valid.size(); ++k) {
        if (ctg_ids[k].empty()) continue;
        const Ctg *c = ctg(ctg_ids[k]);
        auto it = seq_of.find(ctg_ids[k]);
        if (!c || it == seq_of.end()) throw Error(GAMS_EINVAL, "locate --seq: no sequence for " + ctg_ids[k]);
        const int64_t from = (int64_t)valid[k].start - c->chr_start + 1;   // locate.rs:128-129
        const int64_t to = (int64_t)valid[k].end - c->chr_start + 1;
        if (from < 1 || to > (int64_t)it->second.size() || to < from)
            throw Error(GAMS_EINVAL, "locate --seq: range outside " + ctg_ids[k] +
                                         " (the reference panics, locate.rs:133)");
        out += ">" + rgs[src[k]] + "\n" + it->second.substr((size_t)from - 1, (size_t)(to - from + 1)) + "\n";
    }
    return out;
}

std::string Locator::locate_seq_text(const char *bytes, size_t n, gams_seqset_t *seqset, const std::vector<uint32_t> &slots,
                                     bool *device) {
    if (device) *device = false;
    if (!seqset || slots.size() != given_.size()) throw Error(GAMS_EINVAL, "locate_seq_text: one seqset slot per ctg");
    text_tables();
    // per interval of the ctg index (ctgs_' order): seqset slot, chr_start, chr_end
    const size_t n_ctg = ctgs_.size();
    std::vector<uint32_t> slot(std::max<size_t>(n_ctg, 1), UINT32_MAX);
    std::vector<int32_t> cs(std::max<size_t>(n_ctg, 1), 0), ce(std::max<size_t>(n_ctg, 1), 0);
    for (size_t i = 0; i < given_.size(); ++i) slot[given_[i]] = slots[i];
    for (size_t c = 0; c < n_ctg; ++c) {
        cs[c] = ctgs_[c].chr_start;
        ce[c] = ctgs_[c].chr_end;
    }
    const char *text = nullptr;
    uint64_t text_bytes = 0, rows = 0;
    const int rc = gams_gpu_locate_seq_text(h_, seqset, ctg_ix_, chr_names_, slot.data(), cs.data(), ce.data(), bytes, n, &text,
                                            &text_bytes, &rows);
    if (rc != GAMS_EUNSUPPORTED) {
        check(h_, rc);
        if (device) *device = true;
        return std::string(text, (size_t)text_bytes);
    }
    // the host's passes: the lines' first fields (locate.rs:89-91) through locate_seq, over the sequences of the ctgs
    // they are located to, brought back from the seqset
    std::vector<std::string> rgs = text_lines(bytes, n);
    std::vector<Range> valid;
    for (std::string &s : rgs) {
        const size_t tab = s.find('\t');
        if (tab != std::string::npos) s.resize(tab);
        Range r = Range::from_str(s);
        if (!r.valid) continue;
        r.strand.clear();
        valid.push_back(r);
    }
    std::map<std::string, std::string> seq_of;
    // (a slot's length is not the host's to see: any slot fits a buffer of the whole seqset, and the ctg's bases are its head)
    uint64_t set_bytes = 0;
    check(h_, gams_seqset_layout(h_, seqset, nullptr, &set_bytes));
    std::vector<uint8_t> whole;
    for (const std::string &id : find(valid)) {
        if (id.empty() || seq_of.count(id)) continue;
        const uint32_t c = ctg_slot_.at(id);
        if (slot[c] == UINT32_MAX) continue;                             // locate_seq reports it
        whole.resize((size_t)set_bytes + 1);
        check(h_, gams_seqset_download(h_, seqset, slot[c], whole.data(), nullptr));
        seq_of[id].assign(reinterpret_cast<const char *>(whole.data()), (size_t)((int64_t)ce[c] - cs[c] + 1));
    }
    return locate_seq(rgs, seq_of);
}

std::string Locator::locate_seq_text(const char *bytes, size_t n, const std::vector<const uint8_t *> &seqs, bool *device) {
    if (seqs.size() != given_.size()) throw Error(GAMS_EINVAL, "locate_seq_text: ctgs / seqs size mismatch");
    std::vector<uint32_t> lens(std::max<size_t>(given_.size(), 1), 0), slots(given_.size());
    for (size_t i = 0; i < given_.size(); ++i) {
        lens[i] = (uint32_t)(ctgs_[given_[i]].chr_end - ctgs_[given_[i]].chr_start + 1);
        slots[i] = (uint32_t)i;
    }
    SeqSetGuard sg{h_};
    check(h_, gams_seqset_create(h_, (uint32_t)given_.size(), lens.data(), &sg.s));
    check(h_, gams_seqset_upload_all(h_, sg.s, seqs.data()));
    return locate_seq_text(bytes, n, sg.s, slots, device);
}

// ---------------------------------------------------------------------------
// loaders' bucketing (utils.rs:39-67) and the gzip framing of `seq:` (redis.rs:149-161)
// ---------------------------------------------------------------------------
std::map<std::string, std::vector<Range>> read_range(Locator &loc, const std::vector<std::string> &lines) {
    std::vector<Range> valid;
    for (const std::string &ln : lines) {
        Range r = Range::from_str(ln);                                  // utils.rs:50-53
        if (r.valid) valid.push_back(r);
    }
    std::vector<std::string> ids = loc.find(valid);                     // utils.rs:55 (strand is not used by the lookup)
    std::map<std::string, std::vector<Range>> ranges_of;
    for (size_t k = 0; k < valid.size(); ++k) {
        if (ids[k].empty()) continue;                                   // utils.rs:56-58
        auto it = ranges_of.find(ids[k]);
        if (it == ranges_of.end())
            ranges_of[ids[k]];                                          // or_default(): the first range is dropped
        else
            it->second.push_back(valid[k]);                             // and_modify(push)
    }
    return ranges_of;
}

RangeBuckets read_range_text(Locator &loc, const char *bytes, size_t n, bool *device) {
    if (device) *device = false;
    loc.text_tables();
    const size_t n_ctg = loc.ctgs_.size();
    std::vector<uint64_t> off(n_ctg + 1, 0);
    std::vector<uint8_t> seen(std::max<size_t>(n_ctg, 1), 0);
    std::vector<int32_t> st, en;
    std::vector<uint32_t> ln;
    // one call: the file's lines bound the kept ranges, so the columns are sized by the newlines
    uint64_t kept = 0;
    const size_t cap = (size_t)std::count(bytes, bytes + n, '\n') + 1;
    st.resize(cap);
    en.resize(cap);
    ln.resize(cap);
    const int rc = gams_gpu_read_range_text(loc.h_, loc.ctg_ix_, loc.chr_names_, bytes, n, off.data(), seen.data(), st.data(),
                                            en.data(), ln.data(), cap, &kept);
    if (rc == GAMS_OK) {
        st.resize(kept);
        en.resize(kept);
        ln.resize(kept);
    }
    if (rc == GAMS_EUNSUPPORTED) {
        // utils.rs:39-67 on the host, by ctg slot: the lines whole, located, the first of every ctg dropped
        const std::vector<std::string> lines = text_lines(bytes, n);
        std::vector<Range> valid;
        std::vector<uint32_t> src;
        for (size_t i = 0; i < lines.size(); ++i) {
            Range r = Range::from_str(lines[i]);
            if (!r.valid) continue;
            valid.push_back(r);
            src.push_back((uint32_t)i);
        }
        const std::vector<std::string> ids = loc.find(valid);
        std::vector<std::vector<size_t>> of(n_ctg);
        std::fill(seen.begin(), seen.end(), 0);
        for (size_t k = 0; k < valid.size(); ++k) {
            if (ids[k].empty()) continue;
            const uint32_t c = loc.ctg_slot_.at(ids[k]);
            if (seen[c]) of[c].push_back(k);
            seen[c] = 1;
        }
        st.clear(), en.clear(), ln.clear();
        for (size_t c = 0; c < n_ctg; ++c) {
            for (size_t k : of[c]) {
                st.push_back(valid[k].start);
                en.push_back(valid[k].end);
                ln.push_back(src[k]);
            }
            off[c + 1] = st.size();
        }
    } else {
        check(loc.h_, rc);
        if (device) *device = true;
    }
    // the buckets in ctg-id order (BTreeMap<String, _>), empty ones included
    RangeBuckets out;
    out.off.push_back(0);
    for (auto &kv : loc.ctg_slot_) {
        const uint32_t c = kv.second;
        if (!seen[c]) continue;
        out.ids.push_back(kv.first);
        out.start.insert(out.start.end(), st.begin() + off[c], st.begin() + off[c + 1]);
        out.end.insert(out.end.end(), en.begin() + off[c], en.begin() + off[c + 1]);
        out.line.insert(out.line.end(), ln.begin() + off[c], ln.begin() + off[c + 1]);
        out.off.push_back(out.start.size());
    }
    return out;
}

std::map<std::string, std::vector<std::pair<Range, std::string>>> read_peak(Locator &loc,
                                                                          const std::vector<std::string> &lines) {
    std::vector<Range> valid;
    std::vector<std::string> sig;
    for (const std::string &ln : lines) {
        std::vector<std::string> parts;
        size_t b = 0;
        for (;;) {
            size_t e = ln.find('\t', b);
            parts.push_back(ln.substr(b, e == std::string::npos ? std::string::npos : e - b));
            if (e == std::string::npos) break;
            b = e + 1;
        }
        Range r = Range::from_str(parts[0]);                            // utils.rs:96-99
        if (!r.valid) continue;
        if (parts.size() < 3) throw Error(GAMS_EINVAL, "read_peak: a row has no signal column (the reference panics, utils.rs:102)");
        r.strand.clear();                                               // utils.rs:100
        valid.push_back(r);
        sig.push_back(parts[2]);
    }
    std::vector<std::string> ids = loc.find(valid);
    std::map<std::string, std::vector<std::pair<Range, std::string>>> peaks_of;
    for (size_t k = 0; k < valid.size(); ++k) {
        if (ids[k].empty()) continue;
        auto it = peaks_of.find(ids[k]);
        if (it == peaks_of.end())
            peaks_of[ids[k]];                                           // utils.rs:109-112: first one dropped
        else
            it->second.emplace_back(valid[k], sig[k]);
    }
    return peaks_of;
}

namespace {
void peak_check_inside(const Ctg &ctg, const std::vector<std::pair<Range, std::string>> &peaks) {
    for (const auto &pk : peaks)
        if (pk.first.start < ctg.chr_start || pk.first.end > ctg.chr_end || pk.first.end < pk.first.start)
            throw Error(GAMS_EINVAL, "peak: " + pk.first.to_string() + " is not inside " + ctg.id +
                                         " (the reference panics on the slice, utils.rs:155)");
}

// the Peak records of one ctg from its merged ranges and their gc (peak.rs:65-158)
std::vector<Peak> peak_fill(const Ctg &ctg, const std::vector<std::pair<Range, std::string>> &peaks, const float *gc) {
    std::vector<Peak> out(peaks.size());
    if (peaks.empty()) return out;
    for (size_t i = 0; i < peaks.size(); ++i) {                         // peak.rs:65-95
        Peak &p = out[i];
        p.id = "peak:" + ctg.id + ":" + std::to_string(i + 1);
        p.range = peaks[i].first.to_string();
        p.length = peaks[i].first.end - peaks[i].first.start + 1;
        p.signal = peaks[i].second;
        p.gc = gc[i];
    }
    // left (peak.rs:112-133)
    std::string prev_signal = out.front().signal;
    float prev_gc = out.front().gc;
    int32_t prev_end = ctg.chr_start;
    for (size_t i = 0; i < out.size(); ++i) {
        out[i].left_wave_length = peaks[i].first.start - prev_end + 1;
        out[i].left_amplitude = std::fabs(out[i].gc - prev_gc);
        out[i].left_signal = prev_signal;
        prev_signal = out[i].signal;
        prev_end = peaks[i].first.end;
        prev_gc = out[i].gc;
    }
    // right (peak.rs:135-157)
    std::string next_signal = out.back().signal;
    float next_gc = out.back().gc;
    int32_t next_start = ctg.chr_end;
    for (size_t i = out.size(); i-- > 0;) {
        out[i].right_wave_length = next_start - peaks[i].first.end + 1;
        out[i].right_amplitude = std::fabs(out[i].gc - next_gc);
        out[i].right_signal = next_signal;
        next_signal = out[i].signal;
        next_start = peaks[i].first.start;
        next_gc = out[i].gc;
    }
    return out;
}
}  // namespace

std::vector<Peak> peak_records(gams_gpu_t *h, const Ctg &ctg, const uint8_t *seq,
                               const std::vector<std::pair<Range, std::string>> &peaks) {
    if (peaks.empty()) return {};
    peak_check_inside(ctg, peaks);
    uint32_t len = (uint32_t)(ctg.chr_end - ctg.chr_start + 1);
    SeqSetGuard sg{h};
    check(h, gams_seqset_create(h, 1, &len, &sg.s));
    check(h, gams_seqset_upload(h, sg.s, 0, seq));
    std::vector<int32_t> rs(peaks.size()), re(peaks.size());
    for (size_t i = 0; i < peaks.size(); ++i) {
        rs[i] = peaks[i].first.start;
        re[i] = peaks[i].first.end;
    }
    std::vector<float> gc(peaks.size());
    check(h, gams_gpu_range_gc(h, sg.s, 0, ctg.chr_start, rs.data(), re.data(), (uint32_t)peaks.size(), gc.data()));
    return peak_fill(ctg, peaks, gc.data());
}

// several ctgs: one seqset per batch of <= batch_bytes bases, the merged ranges of all of its ctgs through ONE
// gams_gpu_range_gc_batch call (a ctg's few hundred ranges are one or two workgroups)
std::vector<std::vector<Peak>> peak_records_batch(gams_gpu_t *h, const std::vector<Ctg> &ctgs,
                                                  const std::vector<const uint8_t *> &seqs,
                                                  const std::vector<std::vector<std::pair<Range, std::string>>> &peaks,
                                                  uint64_t batch_bytes) {
    if (ctgs.size() != seqs.size() || ctgs.size() != peaks.size())
        throw Error(GAMS_EINVAL, "peak_records_batch: ctgs / seqs / peaks size mismatch");
    std::vector<std::vector<Peak>> out(ctgs.size());
    std::vector<size_t> todo;
    for (size_t c = 0; c < ctgs.size(); ++c)
        if (!peaks[c].empty()) {
            peak_check_inside(ctgs[c], peaks[c]);
            todo.push_back(c);
        }
    for (size_t b = 0; b < todo.size();) {
        uint64_t bytes = 0;
        size_t e = b;
        while (e < todo.size()) {
            const uint64_t len = (uint64_t)(ctgs[todo[e]].chr_end - ctgs[todo[e]].chr_start + 1);
            if (e > b && bytes + len > batch_bytes) break;
            bytes += len;
            ++e;
        }
        const uint32_t n = (uint32_t)(e - b);
        std::vector<uint32_t> lens(n), index(n);
        std::vector<const uint8_t *> ptrs(n);
        std::vector<int32_t> chr_start(n);
        std::vector<uint64_t> off(n + 1, 0);
        for (uint32_t k = 0; k < n; ++k) {
            const Ctg &c = ctgs[todo[b + k]];
            lens[k] = (uint32_t)(c.chr_end - c.chr_start + 1);
            ptrs[k] = seqs[todo[b + k]];
            index[k] = k;
            chr_start[k] = c.chr_start;
            off[k + 1] = off[k] + peaks[todo[b + k]].size();
        }
        std::vector<int32_t> rs(off[n]), re(off[n]);
        for (uint32_t k = 0; k < n; ++k) {
            const auto &pv = peaks[todo[b + k]];
            for (size_t i = 0; i < pv.size(); ++i) {
                rs[off[k] + i] = pv[i].first.start;
                re[off[k] + i] = pv[i].first.end;
            }
        }
        SeqSetGuard sg{h};
        check(h, gams_seqset_create(h, n, lens.data(), &sg.s));
        check(h, gams_seqset_upload_all(h, sg.s, ptrs.data()));
        std::vector<float> gc(off[n]);
        check(h, gams_gpu_range_gc_batch(h, sg.s, n, index.data(), chr_start.data(), off.data(), rs.data(), re.data(),
                                         gc.data()));
        for (uint32_t k = 0; k < n; ++k) out[todo[b + k]] = peak_fill(ctgs[todo[b + k]], peaks[todo[b + k]], gc.data() + off[k]);
        b = e;
    }
    return out;
}

std::string peak_rows(const std::vector<Peak> &recs) {
    std::string out;
    for (const Peak &p : recs)
        out += p.id + "\t" + p.range + "\t" + std::to_string(p.length) + "\t" + fmt_f32(p.gc) + "\t" + p.signal + "\t" +
               std::to_string(p.left_wave_length) + "\t" + fmt_f32(p.left_amplitude) + "\t" + p.left_signal + "\t" +
               std::to_string(p.right_wave_length) + "\t" + fmt_f32(p.right_amplitude) + "\t" + p.right_signal + "\n";
    return out;
}

// What peak_text and peak_records_text set up once for a call: the Locator with its text tables and, per interval of the
// ctg index (the Locator's order), the seqset slot, chr_start and chr_end; and the host's passes both fall back on
struct PeakSetup {
    gams_gpu_t *h;
    gams_seqset_t *seqset;
    Locator loc;
    size_t n_ctg;
    std::vector<uint32_t> slot;
    std::vector<int32_t> cs, ce;
    PeakSetup(gams_gpu_t *h_, const std::vector<Ctg> &ctgs, gams_seqset_t *seqset_, const std::vector<uint32_t> &slots,
              const std::string &who)
        : h(h_), seqset(seqset_), loc(h_, ctgs) {
        if (!seqset || slots.size() != ctgs.size()) throw Error(GAMS_EINVAL, who + ": one seqset slot per ctg");
        loc.text_tables();
        n_ctg = loc.ctgs_.size();
        slot.assign(std::max<size_t>(n_ctg, 1), UINT32_MAX);
        cs.assign(std::max<size_t>(n_ctg, 1), 0);
        ce.assign(std::max<size_t>(n_ctg, 1), 0);
        for (size_t i = 0; i < ctgs.size(); ++i) slot[loc.ctg_slot_.at(ctgs[i].id)] = slots[i];
        for (size_t c = 0; c < n_ctg; ++c) {
            cs[c] = loc.ctgs_[c].chr_start;
            ce[c] = loc.ctgs_[c].chr_end;
        }
    }
    gams_index_t *ctg_ix() const { return loc.ctg_ix_; }
    gams_names_t *chr_names() const { return loc.chr_names_; }
    gams_names_t *ctg_ids() const { return loc.ctg_ids_; }
    const Ctg &ctg(size_t c) const { return loc.ctgs_[c]; }
    // the text of a device call (rows grouped by interval, off per interval and the end) with the ctgs in id order
    std::string by_id(const char *text, uint64_t text_bytes, const std::vector<uint64_t> &off) const {
        std::string out;
        out.reserve((size_t)text_bytes);
        for (auto &kv : loc.ctg_slot_) out.append(text + off[kv.second], (size_t)(off[kv.second + 1] - off[kv.second]));
        return out;
    }
    // the host's passes: read_peak, every bucket sorted by start (peak.rs:49), the gc of all ranges in one call -> the
    // Peak records (serials from 1) of every ctg with kept peaks and its interval, the ctgs in id order
    std::vector<std::pair<uint32_t, std::vector<Peak>>> host_peaks(const char *bytes, size_t n, const std::string &who) {
        auto peaks_of = read_peak(loc, text_lines(bytes, n));
        std::vector<uint32_t> sel, index;
        std::vector<int32_t> sel_start, rs, re;
        std::vector<uint64_t> roff{0};
        for (auto &kv : peaks_of) {
            auto &pv = kv.second;
            if (pv.empty()) continue;
            std::stable_sort(pv.begin(), pv.end(), [](const auto &a, const auto &b) { return a.first.start < b.first.start; });
            const uint32_t c = loc.ctg_slot_.at(kv.first);
            peak_check_inside(loc.ctgs_[c], pv);
            if (slot[c] == UINT32_MAX) throw Error(GAMS_EINVAL, who + ": no sequence for " + kv.first);
            sel.push_back(c);
            index.push_back(slot[c]);
            sel_start.push_back(cs[c]);
            for (const auto &pk : pv) {
                rs.push_back(pk.first.start);
                re.push_back(pk.first.end);
            }
            roff.push_back(rs.size());
        }
        std::vector<float> gc(std::max<size_t>(rs.size(), 1));
        check(h, gams_gpu_range_gc_batch(h, seqset, (uint32_t)sel.size(), index.data(), sel_start.data(), roff.data(), rs.data(),
                                         re.data(), gc.data()));
        std::vector<std::pair<uint32_t, std::vector<Peak>>> out;
        for (size_t k = 0; k < sel.size(); ++k)                              // (peaks_of, hence sel, is in ctg-id order)
            out.emplace_back(sel[k], peak_fill(loc.ctgs_[sel[k]], peaks_of[loc.ctgs_[sel[k]].id], gc.data() + roff[k]));
        return out;
    }
};

// one seqset of the ctgs' bases, uploaded for a call: slot i holds ctgs[i]
static std::vector<uint32_t> peak_upload(gams_gpu_t *h, const std::vector<Ctg> &ctgs, const std::vector<const uint8_t *> &seqs,
                                         SeqSetGuard &sg, const std::string &who) {
    if (ctgs.size() != seqs.size()) throw Error(GAMS_EINVAL, who + ": ctgs / seqs size mismatch");
    std::vector<uint32_t> lens(std::max<size_t>(ctgs.size(), 1), 0), slots(ctgs.size());
    for (size_t i = 0; i < ctgs.size(); ++i) {
        lens[i] = (uint32_t)(ctgs[i].chr_end - ctgs[i].chr_start + 1);
        slots[i] = (uint32_t)i;
    }
    check(h, gams_seqset_create(h, (uint32_t)ctgs.size(), lens.data(), &sg.s));
    check(h, gams_seqset_upload_all(h, sg.s, seqs.data()));
    return slots;
}

std::string peak_text(gams_gpu_t *h, const std::vector<Ctg> &ctgs, gams_seqset_t *seqset, const std::vector<uint32_t> &slots,
                      const char *bytes, size_t n, bool *device) {
    if (device) *device = false;
    PeakSetup S(h, ctgs, seqset, slots, "peak_text");
    std::vector<uint64_t> off(S.n_ctg + 1, 0);
    const char *text = nullptr;
    uint64_t text_bytes = 0, rows = 0;
    const int rc = gams_gpu_peak_text(h, seqset, S.ctg_ix(), S.chr_names(), S.ctg_ids(), S.slot.data(), S.cs.data(),
                                      S.ce.data(), bytes, n, &text, &text_bytes, off.data(), &rows);
    if (rc != GAMS_EUNSUPPORTED) {
        check(h, rc);
        if (device) *device = true;
        return S.by_id(text, text_bytes, off);
    }
    std::string out;
    for (const auto &cp : S.host_peaks(bytes, n, "peak_text")) out += peak_rows(cp.second);
    return out;
}

std::string peak_text(gams_gpu_t *h, const std::vector<Ctg> &ctgs, const std::vector<const uint8_t *> &seqs, const char *bytes,
                      size_t n, bool *device) {
    SeqSetGuard sg{h};
    const std::vector<uint32_t> slots = peak_upload(h, ctgs, seqs, sg, "peak_text");
    return peak_text(h, ctgs, sg.s, slots, bytes, n, device);
}

std::string fmt_f32_json(float v) {
    if (!((v == 0.0f && !std::signbit(v)) || (v >= 1e-5f && v <= 1.0f)))
        throw Error(GAMS_EUNSUPPORTED, "fmt_f32_json: " + fmt_f32(v) + " is not 0 or in [1e-5, 1] (serde_json's exponent form is not implemented)");
    std::string t = fmt_f32_short(v);
    if (t.find('.') == std::string::npos) t += ".0";
    return t;
}

std::string json_escape_serde(const std::string &v) {
    static const char hex[] = "0123456789abcdef";
    std::string o;
    o.reserve(v.size());
    for (const char ch : v) {
        const unsigned char c = (unsigned char)ch;
        switch (c) {
        case '"': o += "\\\""; break;
        case '\\': o += "\\\\"; break;
        case '\b': o += "\\b"; break;
        case '\t': o += "\\t"; break;
        case '\n': o += "\\n"; break;
        case '\f': o += "\\f"; break;
        case '\r': o += "\\r"; break;
        default:
            if (c < 0x20) {
                o += "\\u00";
                o += hex[c >> 4];
                o += hex[c & 15];
            } else {
                o += ch;
            }
        }
    }
    return o;
}

std::string peak_json(const Peak &p) {                                   // data.rs:30-43, serde's field order
    return "{\"id\":\"" + json_escape_serde(p.id) + "\",\"range\":\"" + json_escape_serde(p.range) + "\",\"length\":" +
           std::to_string(p.length) + ",\"gc\":" + fmt_f32_json(p.gc) + ",\"signal\":\"" + json_escape_serde(p.signal) +
           "\",\"left_wave_length\":" + std::to_string(p.left_wave_length) + ",\"left_amplitude\":" +
           fmt_f32_json(p.left_amplitude) + ",\"left_signal\":\"" + json_escape_serde(p.left_signal) +
           "\",\"right_wave_length\":" + std::to_string(p.right_wave_length) + ",\"right_amplitude\":" +
           fmt_f32_json(p.right_amplitude) + ",\"right_signal\":\"" + json_escape_serde(p.right_signal) + "\"}";
}

std::string peak_records_rows(const std::vector<Peak> &recs, int format) {
    if (format == GAMS_LOADER_TSV) return peak_rows(recs);
    if (format != GAMS_LOADER_RECORDS && format != GAMS_LOADER_RESP) throw Error(GAMS_EINVAL, "peak_records_rows: unknown format");
    std::string out;
    for (const Peak &p : recs)
        out += format == GAMS_LOADER_RESP ? wire::resp_command({"SET", p.id, peak_json(p)}) : p.id + "\t" + peak_json(p) + "\n";
    return out;
}

PeakRecords peak_records_text(gams_gpu_t *h, const std::vector<Ctg> &ctgs, gams_seqset_t *seqset, const std::vector<uint32_t> &slots,
                              const char *bytes, size_t n, int format, const std::map<std::string, int32_t> &serial_base,
                              bool *device) {
    if (device) *device = false;
    if (format != GAMS_LOADER_RECORDS && format != GAMS_LOADER_TSV && format != GAMS_LOADER_RESP)
        throw Error(GAMS_EINVAL, "peak_records_text: unknown format");
    PeakSetup S(h, ctgs, seqset, slots, "peak_records_text");
    std::vector<int32_t> base(std::max<size_t>(S.n_ctg, 1), 0), next(std::max<size_t>(S.n_ctg, 1), 0);
    for (size_t i = 0; i < S.n_ctg; ++i) {
        auto it = serial_base.find(S.ctg(i).id);
        if (it != serial_base.end()) base[i] = it->second;
        if (base[i] < 0) throw Error(GAMS_EINVAL, "peak_records_text: a negative serial_base");
    }
    PeakRecords out;
    std::vector<uint64_t> off(S.n_ctg + 1, 0);
    const char *text = nullptr;
    uint64_t text_bytes = 0, rows = 0;
    const int rc = gams_gpu_peak_records_text(h, seqset, S.ctg_ix(), S.chr_names(), S.ctg_ids(), S.slot.data(),
                                              S.cs.data(), S.ce.data(), bytes, n, format, base.data(), &text, &text_bytes,
                                              off.data(), next.data(), &rows);
    if (rc != GAMS_EUNSUPPORTED) {
        check(h, rc);
        if (device) *device = true;
        out.text = S.by_id(text, text_bytes, off);
        for (size_t i = 0; i < S.n_ctg; ++i) out.serial_next[S.ctg(i).id] = next[i];
        return out;
    }
    // the host's passes, renumbered behind the counters
    for (size_t i = 0; i < S.n_ctg; ++i) out.serial_next[S.ctg(i).id] = base[i];
    for (auto &cp : S.host_peaks(bytes, n, "peak_records_text")) {
        const Ctg &ctg = S.ctg(cp.first);
        int64_t serial = base[cp.first];
        for (Peak &p : cp.second) {
            if (++serial > INT32_MAX) throw Error(GAMS_EINVAL, "peak_records_text: a serial beyond INT32_MAX");
            p.id = "peak:" + ctg.id + ":" + std::to_string(serial);      // peak.rs:71-77
        }
        out.serial_next[ctg.id] = (int32_t)serial;
        out.text += peak_records_rows(cp.second, format);
    }
    return out;
}

PeakRecords peak_records_text(gams_gpu_t *h, const std::vector<Ctg> &ctgs, const std::vector<const uint8_t *> &seqs,
                              const char *bytes, size_t n, int format, const std::map<std::string, int32_t> &serial_base,
                              bool *device) {
    SeqSetGuard sg{h};
    const std::vector<uint32_t> slots = peak_upload(h, ctgs, seqs, sg, "peak_records_text");
    return peak_records_text(h, ctgs, sg.s, slots, bytes, n, format, serial_base, device);
}

// What sw_text and sw_summary set up once for a call: the Locator with its text tables and, under GAMS_SW_COUNT, its rg
// index, and per interval of the ctg index (the Locator's order) the seqset slot, chr_start, chr_end and the rg group
struct SwSetup {
    Locator loc;
    size_t n_ctg;
    std::vector<uint32_t> slot, rg_group;
    std::vector<int32_t> cs, ce;
    SwSetup(gams_gpu_t *h, const std::vector<Ctg> &ctgs, gams_seqset_t *seqset, const std::vector<uint32_t> &slots, bool do_count,
            const std::map<std::string, std::vector<Range>> *rgs, const char *rg_bytes, size_t rg_n,
            const std::vector<FileBytes> *rg_files)
        : loc(h, ctgs) {
        loc.text_tables();
        n_ctg = loc.ctgs_.size();
        slot.assign(std::max<size_t>(n_ctg, 1), UINT32_MAX);
        rg_group.assign(std::max<size_t>(n_ctg, 1), UINT32_MAX);
        cs.assign(std::max<size_t>(n_ctg, 1), 0);
        ce.assign(std::max<size_t>(n_ctg, 1), 0);
        if (seqset)
            for (size_t i = 0; i < ctgs.size(); ++i) slot[loc.ctg_slot_.at(ctgs[i].id)] = slots[i];
        if (do_count) {                                                  // idx:rg: on the call's ctg table, once
            if (rg_files)
                loc.set_rg_index_text(*rg_files);
            else if (rg_bytes)
                loc.set_rg_index_text(rg_bytes, rg_n);
            else
                loc.set_rg_index(*rgs);
        }
        for (size_t c = 0; c < n_ctg; ++c) {
            cs[c] = loc.ctgs_[c].chr_start;
            ce[c] = loc.ctgs_[c].chr_end;
            if (do_count) rg_group[c] = loc.rg_group_of(loc.ctgs_[c].id);
        }
    }
    gams_index_t *ctg_ix() const { return loc.ctg_ix_; }
    const gams_names_t *chr_names() const { return loc.chr_names_; }
    const gams_names_t *ctg_ids() const { return loc.ctg_ids_; }
    const std::string &chr_of(size_t c) const { return loc.ctgs_[c].chr_id; }   // the chromosome of interval c
    // the host's passes over one feature file: read_range over the lines and the ids of feature_records, as the arrays
    // the batch entries take -- the ctgs with kept features in id order (BTreeMap order)
    struct Arrays {
        std::vector<uint32_t> sel, index, lens, group;
        std::vector<int32_t> sel_start, fs, fe;
        std::vector<uint64_t> feat_off{0};
        std::vector<std::string> ids;
        std::vector<std::vector<Feature>> feat_of;
    };
    Arrays arrays(const char *bytes, size_t n, bool do_gc, const char *who) {
        Arrays A;
        const auto ranges_of = read_range(loc, text_lines(bytes, n));
        for (auto &kv : ranges_of) {
            if (kv.second.empty()) continue;
            const uint32_t c = loc.ctg_slot_.at(kv.first);
            if (do_gc && slot[c] == UINT32_MAX) throw Error(GAMS_EINVAL, std::string(who) + ": no sequence for " + kv.first);
            A.index.push_back(do_gc ? slot[c] : (uint32_t)A.sel.size());
            A.sel.push_back(c);
            A.lens.push_back((uint32_t)(ce[c] - cs[c] + 1));
            A.sel_start.push_back(cs[c]);
            A.group.push_back(rg_group[c]);
            A.feat_of.emplace_back();
            int32_t serial = 0;
            for (const Range &r : kv.second) {
                A.ids.push_back("feature:" + kv.first + ":" + std::to_string(++serial));   // feature.rs:81-83
                A.fs.push_back(r.start);
                A.fe.push_back(r.end);
                A.feat_of.back().push_back(Feature{A.ids.back(), r.start, r.end});
            }
            A.feat_off.push_back(A.fs.size());
        }
        return A;
    }
};

std::string sw_text(gams_gpu_t *h, const std::vector<Ctg> &ctgs, gams_seqset_t *seqset, const std::vector<uint32_t> &slots,
                    const char *bytes, size_t n, const SwArgs &a, const std::map<std::string, std::vector<Range>> *rgs,
                    const char *rg_bytes, size_t rg_n, bool *device, const TextSink *sink, const std::vector<FileBytes> *rg_files) {
    if (device) *device = false;
    if (rgs && (rg_bytes || rg_files)) throw Error(GAMS_EINVAL, "sw: both the rg ranges and the bytes of an rg file were given");
    const bool do_gc = (a.actions & GAMS_SW_GC) != 0, do_count = (a.actions & GAMS_SW_COUNT) != 0;
    auto done = [&](std::string &&rows) {                                // a finished string: into the sink, if there is one
        if (!sink) return std::move(rows);
        char *dst = (*sink)(rows.size());
        if (!rows.empty()) std::memcpy(dst, rows.data(), rows.size());
        return std::string();
    };
    if (do_gc && !seqset) throw Error(GAMS_EINVAL, "sw_text: --action gc needs a seqset");
    if (seqset && slots.size() != ctgs.size()) throw Error(GAMS_EINVAL, "sw_text: one seqset slot per ctg");
    if (do_count && !rgs && !rg_bytes && !rg_files) throw Error(GAMS_EINVAL, "sw: --action count needs the rg ranges");
    SwSetup U(h, ctgs, seqset, slots, do_count, rgs, rg_bytes, rg_n, rg_files);
    Locator &loc = U.loc;
    const size_t n_ctg = U.n_ctg;
    const std::vector<uint32_t> &slot = U.slot, &rg_group = U.rg_group;
    const std::vector<int32_t> &cs = U.cs, &ce = U.ce;
    std::vector<uint64_t> off(n_ctg + 1, 0);
    const char *text = nullptr;
    uint64_t text_bytes = 0, feats = 0, rows = 0;
    const int rc = gams_gpu_sw_feature_text(h, do_gc ? seqset : nullptr, loc.ctg_ix_, loc.chr_names_, loc.ctg_ids_, slot.data(),
                                            cs.data(), ce.data(), bytes, n, a.size, a.max, a.resize, a.actions, loc.rg_index(),
                                            rg_group.data(), &text, &text_bytes, off.data(), &feats, &rows);
    std::string out;
    if (rc != GAMS_EUNSUPPORTED) {
        check(h, rc);
        if (device) *device = true;
        if (!sink) {
            out.reserve((size_t)text_bytes);
            for (auto &kv : loc.ctg_slot_)                               // ctg-id order (sw.rs:97)
                out.append(text + off[kv.second], (size_t)(off[kv.second + 1] - off[kv.second]));
            return out;
        }
        // ... by a few host threads, a ctg at a time (one thread moves ~10 GB/s and pays every page fault of the target)
        char *const dst = (*sink)((size_t)text_bytes);
        std::vector<std::pair<uint32_t, uint64_t>> part;                 // (interval, where its slice goes)
        uint64_t at = 0;
        for (auto &kv : loc.ctg_slot_) {
            part.emplace_back(kv.second, at);
            at += off[kv.second + 1] - off[kv.second];
        }
        const unsigned T = (unsigned)std::max<uint64_t>(
            1, std::min<uint64_t>({16, std::thread::hardware_concurrency(), (uint64_t)part.size(), text_bytes / (4u << 20) + 1}));
        parallel_for((uint32_t)part.size(), T, [&](uint32_t k) {
            const uint32_t c = part[k].first;
            if (off[c + 1] > off[c]) std::memcpy(dst + part[k].second, text + off[c], (size_t)(off[c + 1] - off[c]));
        });
        return out;
    }
    // the host's passes: read_range over the lines, the ids of feature_records, the existing text entry on the same
    // seqset (without gc no sequence is read: a seqset of the lengths alone stands in)
    const SwSetup::Arrays A = U.arrays(bytes, n, do_gc, "sw_text");
    const std::vector<uint32_t> &sel = A.sel, &index = A.index, &lens = A.lens, &group = A.group;
    const std::vector<int32_t> &sel_start = A.sel_start, &fs = A.fs, &fe = A.fe;
    const std::vector<uint64_t> &feat_off = A.feat_off;
    const std::vector<std::string> &ids = A.ids;
    const std::vector<std::vector<Feature>> &feat_of = A.feat_of;
    const uint32_t n_sel = (uint32_t)sel.size();
    if (n_sel == 0) return done(std::move(out));
    SeqSetGuard sg{h};
    gams_seqset_t *s = seqset;
    if (!do_gc) {
        check(h, gams_seqset_create(h, n_sel, lens.data(), &sg.s));
        s = sg.s;
    }
    std::vector<const char *> chr(n_sel), idp(ids.size());
    for (uint32_t k = 0; k < n_sel; ++k) chr[k] = loc.ctgs_[sel[k]].chr_id.c_str();
    for (size_t f = 0; f < ids.size(); ++f) idp[f] = ids[f].c_str();
    const uint64_t *toff = nullptr;
    const int rt = gams_gpu_sw_text_actions(h, s, n_sel, index.data(), chr.data(), sel_start.data(), feat_off.data(), fs.data(),
                                            fe.data(), idp.data(), a.size, a.max, a.resize, a.actions, loc.rg_index(),
                                            group.data(), &text, &text_bytes, &toff, &rows);
    if (rt != GAMS_EUNSUPPORTED) {
        check(h, rt);
        return done(std::string(text, (size_t)text_bytes));              // (the selected ctgs are in id order)
    }
    // a value the device formatter does not cover: the rows (and counts) as arrays, formatted here.  Without gc the only
    // such value is a negative coordinate, and the array entry needs the bases this call never had
    if (!do_gc) check(h, rt);
    std::vector<uint64_t> row_off(n_sel + 1, 0);
    check(h, gams_gpu_sw_batch(h, s, n_sel, index.data(), sel_start.data(), feat_off.data(), fs.data(), fe.data(), a.size,
                               a.max, a.resize, nullptr, 0, row_off.data(), &rows));
    std::vector<gams_sw_row_t> rv(std::max<uint64_t>(rows, 1));
    std::vector<int32_t> cnt(do_count ? std::max<uint64_t>(rows, 1) : 0);
    check(h, gams_gpu_sw_batch(h, s, n_sel, index.data(), sel_start.data(), feat_off.data(), fs.data(), fe.data(), a.size,
                               a.max, a.resize, rv.data(), rows, row_off.data(), &rows));
    if (do_count)
        check(h, gams_gpu_sw_count_batch(h, s, n_sel, index.data(), sel_start.data(), feat_off.data(), fs.data(), fe.data(),
                                         a.size, a.max, loc.rg_index(), group.data(), cnt.data(), rows, nullptr, &rows));
    for (uint32_t k = 0; k < n_sel; ++k)
        out += sw_format_rows(rv.data() + row_off[k], row_off[k + 1] - row_off[k], loc.ctgs_[sel[k]], feat_of[k], 8, a.actions,
                              do_count ? cnt.data() + row_off[k] : nullptr);
    return done(std::move(out));
}

std::string sw_text(gams_gpu_t *h, const std::vector<Ctg> &ctgs, const std::vector<const uint8_t *> &seqs, const char *bytes,
                    size_t n, const SwArgs &a, const std::map<std::string, std::vector<Range>> *rgs, const char *rg_bytes,
                    size_t rg_n, bool *device, const TextSink *sink, const std::vector<FileBytes> *rg_files) {
    if (ctgs.size() != seqs.size()) throw Error(GAMS_EINVAL, "sw_text: ctgs / seqs size mismatch");
    if (!(a.actions & GAMS_SW_GC))                                       // nothing reads a base: nothing goes up
        return sw_text(h, ctgs, static_cast<gams_seqset_t *>(nullptr), std::vector<uint32_t>(), bytes, n, a, rgs, rg_bytes, rg_n,
                       device, sink, rg_files);
    std::vector<uint32_t> lens(std::max<size_t>(ctgs.size(), 1), 0), slots(ctgs.size());
    for (size_t i = 0; i < ctgs.size(); ++i) {
        lens[i] = (uint32_t)(ctgs[i].chr_end - ctgs[i].chr_start + 1);
        slots[i] = (uint32_t)i;
    }
    SeqSetGuard sg{h};
    check(h, gams_seqset_create(h, (uint32_t)ctgs.size(), lens.data(), &sg.s));
    check(h, gams_seqset_upload_all(h, sg.s, seqs.data()));
    return sw_text(h, ctgs, sg.s, slots, bytes, n, a, rgs, rg_bytes, rg_n, device, sink, rg_files);
}

// ---- the per-distance summary of the sw rows ---------------------------------------------------------
// (the summariser itself -- sw_summarise_rows, the header and SwSummaryTable::text -- is gams_sw_summary.cpp: no device call)
namespace {
bool extract_ctg_id(const std::string &s, std::string &id);            // (with anno's helpers, below)
}  // namespace

SwSummaryTable sw_summary(gams_gpu_t *h, const std::vector<Ctg> &ctgs, gams_seqset_t *seqset, const std::vector<uint32_t> &slots,
                          const std::vector<FileBytes> &files, const std::vector<std::string> *tags, const SwArgs &a,
                          const std::map<std::string, std::vector<Range>> *rgs, const std::vector<FileBytes> *rg_files,
                          bool *device, const std::vector<SwAnnoCol> *anno) {
    if (device) *device = false;
    if (rgs && rg_files) throw Error(GAMS_EINVAL, "sw: both the rg ranges and the bytes of an rg file were given");
    const uint32_t n_anno = anno ? (uint32_t)anno->size() : 0u;
    if (anno && anno->size() > GAMS_SW_SUMMARY_MAX_ANNO) throw Error(GAMS_EINVAL, "sw_summary: more than GAMS_SW_SUMMARY_MAX_ANNO span sets");
    for (uint32_t a = 0; a < n_anno; ++a)
        if (!(*anno)[a].set) throw Error(GAMS_EINVAL, "sw_summary: a null span set");
    if (n_anno)   // utils.rs:118-129 on "sw:feature:{ctg_id}:{k}:{sn}" must give the ctg id back whole
        for (const Ctg &c : ctgs) {
            std::string got;
            if (!extract_ctg_id(c.id, got) || got != c.id)
                throw Error(GAMS_EINVAL, "sw_summary: `gams anno` would not find the ctg id " + c.id + " in its rows (ctg:[A-Za-z0-9_]+:\\d+)");
        }
    const bool do_gc = (a.actions & GAMS_SW_GC) != 0, do_count = (a.actions & GAMS_SW_COUNT) != 0;
    if (do_gc && !seqset) throw Error(GAMS_EINVAL, "sw_summary: --action gc needs a seqset");
    if (seqset && slots.size() != ctgs.size()) throw Error(GAMS_EINVAL, "sw_summary: one seqset slot per ctg");
    if (do_count && !rgs && !rg_files) throw Error(GAMS_EINVAL, "sw: --action count needs the rg ranges");
    if (tags && tags->size() != files.size()) throw Error(GAMS_EINVAL, "sw_summary: one tag per file");
    if (a.max < 0) throw Error(GAMS_EINVAL, "sw_summary: max >= 0");
    SwSummaryTable T;
    T.max = a.max;
    T.actions = a.actions;
    if (tags) {                                                          // the slots: the distinct tags in byte order
        T.tags = *tags;
        std::sort(T.tags.begin(), T.tags.end());
        T.tags.erase(std::unique(T.tags.begin(), T.tags.end()), T.tags.end());
    }
    const uint32_t n_tags = (uint32_t)std::max<size_t>(T.tags.size(), 1);
    const size_t group_words = ((size_t)a.max + 1) * GAMS_SW_SUMMARY_WORDS;
    T.words.assign(group_words * n_tags, 0);                             // what the host's passes add; the device's joins below
    const size_t group_props = ((size_t)a.max + 1) * n_anno;
    T.prop.assign(group_props * n_tags, 0);
    SwSetup U(h, ctgs, seqset, slots, do_count, rgs, nullptr, 0, rg_files);
    // per set: the group of every interval's chromosome in it (UINT32_MAX: the set does not hold the chromosome)
    std::vector<std::vector<uint32_t>> set_group(n_anno, std::vector<uint32_t>(std::max<size_t>(U.n_ctg, 1), UINT32_MAX));
    std::vector<gams_spans_t *> sets(n_anno);
    std::vector<const uint32_t *> set_group_p(n_anno);
    for (uint32_t s = 0; s < n_anno; ++s) {
        const AnnoSet &as = *(*anno)[s].set;
        T.prefixes.push_back((*anno)[s].prefix);
        std::map<std::string, uint32_t> group_of;
        for (uint32_t g = 0; g < as.chrs().size(); ++g) group_of.emplace(as.chrs()[g], g);
        for (size_t c = 0; c < U.n_ctg; ++c) {
            const auto it = group_of.find(U.chr_of(c));
            if (it != group_of.end()) set_group[s][c] = it->second;
        }
        sets[s] = as.spans();
        set_group_p[s] = set_group[s].data();
    }
    struct Acc {
        gams_gpu_t *h;
        gams_sw_summary_t *p = nullptr;
        ~Acc() { gams_sw_summary_destroy(h, p); }
    } acc{h};
    check(h, gams_sw_summary_create_anno(h, a.max, n_tags, a.actions, a.size, a.resize, n_anno, &acc.p));
    bool all_device = true;
    for (size_t f = 0; f < files.size(); ++f) {
        const uint32_t tag = tags ? (uint32_t)(std::lower_bound(T.tags.begin(), T.tags.end(), (*tags)[f]) - T.tags.begin()) : 0u;
        const char *bytes = files[f].first ? files[f].first : "";
        uint64_t feats = 0, rows = 0;
        const int rc = gams_gpu_sw_feature_summary_anno(h, do_gc ? seqset : nullptr, U.ctg_ix(), U.chr_names(), U.ctg_ids(),
                                                        U.slot.data(), U.cs.data(), U.ce.data(), bytes, files[f].second, a.size,
                                                        a.max, a.resize, a.actions, U.loc.rg_index(), U.rg_group.data(), acc.p, tag,
                                                        n_anno, sets.data(), set_group_p.data(), &feats, &rows);
        if (rc != GAMS_EUNSUPPORTED) {
            check(h, rc);
            continue;
        }
        // the host's passes for this file: read_range and the arrays; with gc the rows of gams_gpu_sw_batch (and their
        // counts) summarised here, without it -- no statistic, nothing to refuse -- the array entry of the device
        all_device = false;
        const SwSetup::Arrays A = U.arrays(bytes, files[f].second, do_gc, "sw_summary");
        const uint32_t n_sel = (uint32_t)A.sel.size();
        if (n_sel == 0) continue;
        std::vector<std::vector<uint32_t>> sel_group(n_anno, std::vector<uint32_t>(n_sel));   // set_group of the selected ctgs
        std::vector<const uint32_t *> sel_group_p(n_anno);
        for (uint32_t s = 0; s < n_anno; ++s) {
            for (uint32_t k = 0; k < n_sel; ++k) sel_group[s][k] = set_group[s][A.sel[k]];
            sel_group_p[s] = sel_group[s].data();
        }
        if (!do_gc) {
            SeqSetGuard sg{h};
            check(h, gams_seqset_create(h, n_sel, A.lens.data(), &sg.s));
            check(h, gams_gpu_sw_summary_batch_anno(h, sg.s, n_sel, A.index.data(), A.sel_start.data(), A.feat_off.data(),
                                                    A.fs.data(), A.fe.data(), a.size, a.max, a.resize, a.actions, U.loc.rg_index(),
                                                    A.group.data(), acc.p, tag, n_anno, sets.data(), sel_group_p.data(), &rows));
            continue;
        }
        check(h, gams_gpu_sw_batch(h, seqset, n_sel, A.index.data(), A.sel_start.data(), A.feat_off.data(), A.fs.data(),
                                   A.fe.data(), a.size, a.max, a.resize, nullptr, 0, nullptr, &rows));
        std::vector<gams_sw_row_t> rv(std::max<uint64_t>(rows, 1));
        std::vector<int32_t> cnt(do_count ? std::max<uint64_t>(rows, 1) : 0);
        std::vector<uint64_t> row_off((size_t)n_sel + 1, 0);
        check(h, gams_gpu_sw_batch(h, seqset, n_sel, A.index.data(), A.sel_start.data(), A.feat_off.data(), A.fs.data(),
                                   A.fe.data(), a.size, a.max, a.resize, rv.data(), rows, row_off.data(), &rows));
        // the Prop units of the rows: gams_gpu_cover over their windows, once per set (the clip is the row's ctg)
        std::vector<std::vector<uint32_t>> units(n_anno, std::vector<uint32_t>(std::max<uint64_t>(rows, 1), 0u));
        std::vector<const uint32_t *> units_p(n_anno);
        if (n_anno) {
            const size_t nr = (size_t)std::max<uint64_t>(rows, 1);
            std::vector<uint32_t> grp(nr);
            std::vector<int32_t> cl(nr), ch(nr), qs(nr), qe(nr);
            std::vector<float> prop(nr);
            for (uint32_t k = 0; k < n_sel; ++k)
                for (uint64_t r = row_off[k]; r < row_off[k + 1]; ++r) {
                    cl[r] = U.cs[A.sel[k]];
                    ch[r] = U.ce[A.sel[k]];
                    qs[r] = rv[r].start;
                    qe[r] = rv[r].end;
                }
            for (uint32_t s = 0; s < n_anno; ++s) {
                for (uint32_t k = 0; k < n_sel; ++k)
                    std::fill(grp.begin() + row_off[k], grp.begin() + row_off[k + 1], sel_group[s][k]);
                check(h, gams_gpu_cover(h, sets[s], grp.data(), cl.data(), ch.data(), qs.data(), qe.data(), rows, prop.data()));
                for (uint64_t r = 0; r < rows; ++r) units[s][r] = prop4_units(prop[r]);
                units_p[s] = units[s].data();
            }
        }
        if (do_count)
            check(h, gams_gpu_sw_count_batch(h, seqset, n_sel, A.index.data(), A.sel_start.data(), A.feat_off.data(), A.fs.data(),
                                             A.fe.data(), a.size, a.max, U.loc.rg_index(), A.group.data(), cnt.data(), rows,
                                             nullptr, &rows));
        sw_summarise_rows(rv.data(), do_count ? cnt.data() : nullptr, rows, a.max, a.actions, T.words.data() + tag * group_words,
                          n_anno, units_p.data(), T.prop.data() + tag * group_props);
    }
    // one small read-back: the device's integers join the host's
    const size_t n = ((size_t)a.max + 1) * n_tags;
    std::vector<uint64_t> count(n), s(4 * n), nan(4 * n), c(n);
    check(h, gams_sw_summary_read(h, acc.p, count.data(), s.data(), nan.data(), c.data()));
    for (size_t g = 0; g < n; ++g) {
        uint64_t *w = T.words.data() + g * GAMS_SW_SUMMARY_WORDS;
        w[0] += count[g];
        w[9] += c[g];
        for (int k = 0; k < 4; ++k) {
            w[1 + k] += s[4 * g + k];
            w[5 + k] += nan[4 * g + k];
        }
    }
    if (n_anno) {
        std::vector<uint64_t> p(T.prop.size());
        check(h, gams_sw_summary_read_anno(h, acc.p, p.data()));
        for (size_t i = 0; i < p.size(); ++i) T.prop[i] += p[i];
    }
    if (device) *device = all_device;
    return T;
}

SwSummaryTable sw_summary(gams_gpu_t *h, const std::vector<Ctg> &ctgs, const std::vector<const uint8_t *> &seqs,
                          const std::vector<FileBytes> &files, const std::vector<std::string> *tags, const SwArgs &a,
                          const std::map<std::string, std::vector<Range>> *rgs, const std::vector<FileBytes> *rg_files,
                          bool *device, const std::vector<SwAnnoCol> *anno) {
    if (!(a.actions & GAMS_SW_GC))                                       // nothing reads a base: nothing goes up
        return sw_summary(h, ctgs, static_cast<gams_seqset_t *>(nullptr), std::vector<uint32_t>(), files, tags, a, rgs, rg_files,
                          device, anno);
    if (ctgs.size() != seqs.size()) throw Error(GAMS_EINVAL, "sw_summary: ctgs / seqs size mismatch");
    std::vector<uint32_t> lens(std::max<size_t>(ctgs.size(), 1), 0), slots(ctgs.size());
    for (size_t i = 0; i < ctgs.size(); ++i) {
        lens[i] = (uint32_t)(ctgs[i].chr_end - ctgs[i].chr_start + 1);
        slots[i] = (uint32_t)i;
    }
    SeqSetGuard sg{h};
    check(h, gams_seqset_create(h, (uint32_t)ctgs.size(), lens.data(), &sg.s));
    check(h, gams_seqset_upload_all(h, sg.s, seqs.data()));
    return sw_summary(h, ctgs, sg.s, slots, files, tags, a, rgs, rg_files, device, anno);
}

namespace {
std::string json_escape(const std::string &v) {
    std::string o;
    for (char c : v) {
        if (c == '"' || c == '\\') o += '\\';
        o += c;
    }
    return o;
}
}  // namespace

std::string ctg_json(const Ctg &c) {
    return "{\"id\":\"" + json_escape(c.id) + "\",\"range\":\"" + json_escape(c.range) + "\",\"chr_id\":\"" +
           json_escape(c.chr_id) + "\",\"chr_start\":" + std::to_string(c.chr_start) + ",\"chr_end\":" +
           std::to_string(c.chr_end) + ",\"chr_strand\":\"" + json_escape(c.chr_strand) + "\",\"length\":" +
           std::to_string(c.length) + "}";
}

Ctg ctg_from_json(const std::string &json) {
    // flat object of strings and integers, any field order, whitespace tolerated
    Ctg c;
    size_t pos = 0;
    auto skip = [&] {
        while (pos < json.size() && (json[pos] == ' ' || json[pos] == '\n' || json[pos] == '\t' || json[pos] == '\r')) ++pos;
    };
    auto str = [&]() {
        std::string v;
        if (pos >= json.size() || json[pos] != '"') throw Error(GAMS_EINVAL, "ctg_from_json: expected a string");
        for (++pos; pos < json.size() && json[pos] != '"'; ++pos) {
            if (json[pos] == '\\' && pos + 1 < json.size()) ++pos;
            v += json[pos];
        }
        if (pos >= json.size()) throw Error(GAMS_EINVAL, "ctg_from_json: unterminated string");
        ++pos;
        return v;
    };
    skip();
    if (pos >= json.size() || json[pos] != '{') throw Error(GAMS_EINVAL, "ctg_from_json: not an object");
    ++pos;
    for (;;) {
        skip();
        if (pos < json.size() && json[pos] == '}') break;
        const std::string key = str();
        skip();
        if (pos >= json.size() || json[pos] != ':') throw Error(GAMS_EINVAL, "ctg_from_json: expected ':'");
        ++pos;
        skip();
        if (pos < json.size() && json[pos] == '"') {
            const std::string v = str();
            if (key == "id") c.id = v;
            else if (key == "range") c.range = v;
            else if (key == "chr_id") c.chr_id = v;
            else if (key == "chr_strand") c.chr_strand = v;
        } else {
            size_t e = pos;
            while (e < json.size() && (json[e] == '-' || (json[e] >= '0' && json[e] <= '9'))) ++e;
            if (e == pos) throw Error(GAMS_EINVAL, "ctg_from_json: expected a number");
            const int32_t v = (int32_t)std::stol(json.substr(pos, e - pos));
            pos = e;
            if (key == "chr_start") c.chr_start = v;
            else if (key == "chr_end") c.chr_end = v;
            else if (key == "length") c.length = v;
        }
        skip();
        if (pos < json.size() && json[pos] == ',') ++pos;
    }
    if (c.id.empty() || c.chr_id.empty()) throw Error(GAMS_EINVAL, "ctg_from_json: id / chr_id missing");
    return c;
}

std::string tsv_ctgs(const std::vector<Ctg> &ctgs) {
    std::string out = "id\trange\tchr_id\tchr_start\tchr_end\tchr_strand\tlength\n";   // data.rs:5-14
    for (const Ctg &c : ctgs)
        out += c.id + "\t" + c.range + "\t" + c.chr_id + "\t" + std::to_string(c.chr_start) + "\t" +
               std::to_string(c.chr_end) + "\t" + c.chr_strand + "\t" + std::to_string(c.length) + "\n";
    return out;
}

std::string tsv_records(const std::vector<Record> &records, bool features) {
    std::string out = features ? "id\trange\tlength\ttag\n" : "id\trange\n";           // data.rs:16-28
    for (const Record &r : records) {
        // values of the flat JSON object this library wrote itself, in field order
        std::string row;
        size_t pos = 0;
        while ((pos = r.json.find("\":", pos)) != std::string::npos) {
            pos += 2;
            std::string v;
            if (r.json[pos] == '"') {
                for (++pos; pos < r.json.size() && r.json[pos] != '"'; ++pos) {
                    if (r.json[pos] == '\\' && pos + 1 < r.json.size()) ++pos;
                    v += r.json[pos];
                }
            } else {
                while (pos < r.json.size() && r.json[pos] != ',' && r.json[pos] != '}') v += r.json[pos++];
            }
            if (!row.empty()) row += '\t';
            row += v;
        }
        out += row + "\n";
    }
    return out;
}

namespace {
std::string rg_json(const std::string &id, const Range &r) {
    return "{\"id\":\"" + json_escape(id) + "\",\"range\":\"" + json_escape(r.to_string()) + "\"}";
}
std::string feature_json(const std::string &id, const Range &r, const std::string &tag) {            // feature.rs:85-92
    return "{\"id\":\"" + json_escape(id) + "\",\"range\":\"" + json_escape(r.to_string()) + "\",\"length\":" +
           std::to_string(r.end - r.start + 1) + ",\"tag\":\"" + json_escape(tag) + "\"}";
}
// the records of one file: the kept ranges of every ctg (BTreeMap order = ctg id order) numbered behind cnt[ctg]
template <typename Json>
std::vector<Record> loader_records(Locator &loc, const std::vector<std::string> &lines, const char *kind,
                                   std::map<std::string, int32_t> &cnt, Json json) {
    std::vector<Record> out;
    for (auto &kv : read_range(loc, lines)) {
        if (kv.second.empty()) continue;
        int64_t serial = cnt[kv.first];
        for (const Range &r : kv.second) {
            if (++serial > INT32_MAX) throw Error(GAMS_EINVAL, "loader: a serial beyond INT32_MAX");
            const std::string id = std::string(kind) + ":" + kv.first + ":" + std::to_string(serial);   // rg.rs:64-66, feature.rs:81-83
            out.push_back({id, json(id, r)});
        }
        cnt[kv.first] = (int32_t)serial;
    }
    return out;
}
}  // namespace

std::vector<Record> rg_records(Locator &loc, const std::vector<std::string> &lines, std::map<std::string, int32_t> &cnt) {
    return loader_records(loc, lines, "rg", cnt, [](const std::string &id, const Range &r) { return rg_json(id, r); });
}

std::vector<Record> feature_records(Locator &loc, const std::vector<std::string> &lines, const std::string &tag,
                                    std::map<std::string, int32_t> &cnt) {
    return loader_records(loc, lines, "feature", cnt, [&](const std::string &id, const Range &r) { return feature_json(id, r, tag); });
}

std::vector<Record> rg_records(Locator &loc, const std::vector<std::string> &lines) {
    std::map<std::string, int32_t> fresh;                               // serials from 1 (a fresh cnt:rg:)
    return rg_records(loc, lines, fresh);
}

std::vector<Record> feature_records(Locator &loc, const std::vector<std::string> &lines, const std::string &tag) {
    std::map<std::string, int32_t> fresh;
    return feature_records(loc, lines, tag, fresh);
}

LoaderText loader_text(gams_gpu_t *h, const std::vector<Ctg> &ctgs, const std::vector<FileBytes> &files, int kind,
                       const std::string &tag, int format, const std::map<std::string, int32_t> &serial_base, bool *device) {
    if (device) *device = false;
    if ((kind != GAMS_LOADER_RG && kind != GAMS_LOADER_FEATURE) ||
        (format != GAMS_LOADER_RECORDS && format != GAMS_LOADER_TSV && format != GAMS_LOADER_RESP))
        throw Error(GAMS_EINVAL, "loader_text: unknown kind or format");
    Locator loc(h, ctgs);
    loc.text_tables();
    const size_t n_ctg = loc.ctgs_.size(), n_files = files.size();
    LoaderText out;
    out.n_in_file.assign(n_files, 0);
    std::vector<int32_t> base(std::max<size_t>(n_ctg, 1), 0), next(std::max<size_t>(n_ctg, 1), 0);
    for (size_t i = 0; i < n_ctg; ++i) {
        auto it = serial_base.find(loc.ctgs_[i].id);
        if (it != serial_base.end()) base[i] = it->second;
        if (base[i] < 0) throw Error(GAMS_EINVAL, "loader_text: a negative serial_base");
    }
    std::vector<const char *> fb;
    std::vector<uint64_t> fn;
    for (const FileBytes &f : files) {
        fb.push_back(f.first);
        fn.push_back(f.second);
    }
    const char *text = nullptr;
    uint64_t tbytes = 0, rows = 0;
    std::vector<uint64_t> toff(n_files * n_ctg + 1, 0);
    const int rc = gams_gpu_loader_text(h, loc.ctg_ix_, loc.chr_names_, loc.ctg_ids_, (uint32_t)n_files, fb.data(), fn.data(), kind,
                                        tag.data(), tag.size(), format, base.data(), &text, &tbytes, toff.data(), next.data(),
                                        out.n_in_file.data(), &rows);
    if (rc == GAMS_OK) {
        // the reference's SET order: file by file, the ctgs by id
        out.text.reserve(tbytes);
        for (size_t f = 0; f < n_files; ++f)
            for (auto &kv : loc.ctg_slot_) {
                const size_t b = f * n_ctg + kv.second;
                out.text.append(text + toff[b], text + toff[b + 1]);
            }
        for (size_t i = 0; i < n_ctg; ++i) out.serial_next[loc.ctgs_[i].id] = next[i];
        if (device) *device = true;
        return out;
    }
    if (rc != GAMS_EUNSUPPORTED) check(h, rc);
    // the host's passes, file after file, the counters carried on
    std::map<std::string, int32_t> cnt;
    for (size_t i = 0; i < n_ctg; ++i) cnt[loc.ctgs_[i].id] = base[i];
    for (size_t f = 0; f < n_files; ++f) {
        const std::vector<std::string> lines = text_lines(files[f].first, files[f].second);
        const std::vector<Record> recs = kind == GAMS_LOADER_FEATURE ? feature_records(loc, lines, tag, cnt) : rg_records(loc, lines, cnt);
        out.n_in_file[f] = recs.size();
        if (format == GAMS_LOADER_TSV) {
            const std::string t = tsv_records(recs, kind == GAMS_LOADER_FEATURE);
            out.text.append(t, t.find('\n') + 1, std::string::npos);     // without the header
        } else {
            for (const Record &r : recs)
                out.text += format == GAMS_LOADER_RESP ? wire::resp_command({"SET", r.key, r.json}) : r.key + "\t" + r.json + "\n";
        }
    }
    out.serial_next = cnt;
    return out;
}

namespace {
// libdeflate (the runtime library ships with the image: libdeflate.so.0, no headers) inflates DNA text about
// three times as fast as zlib; bound by hand to its stable C API, zlib when it is absent.
struct LibDeflate {
    void *(*alloc)() = nullptr;
    int (*gunzip)(void *, const void *, size_t, void *, size_t, size_t *) = nullptr;
    void (*release)(void *) = nullptr;
    LibDeflate() {
        if (void *so = dlopen("libdeflate.so.0", RTLD_NOW | RTLD_LOCAL)) {
            alloc = reinterpret_cast<void *(*)()>(dlsym(so, "libdeflate_alloc_decompressor"));
            gunzip = reinterpret_cast<int (*)(void *, const void *, size_t, void *, size_t, size_t *)>(
                dlsym(so, "libdeflate_gzip_decompress"));
            release = reinterpret_cast<void (*)(void *)>(dlsym(so, "libdeflate_free_decompressor"));
            if (!alloc || !gunzip || !release) alloc = nullptr;
        }
    }
    bool ok() const { return alloc != nullptr; }
};
const LibDeflate &libdeflate() {
    static const LibDeflate L;
    return L;
}
struct Decompressor {   // one per thread, reused
    void *d = nullptr;
    ~Decompressor() {
        if (d) libdeflate().release(d);
    }
};

size_t zlib_gunzip_into(const uint8_t *bytes, size_t n, uint8_t *dst, size_t cap, bool *overflow) {
    z_stream zs{};
    if (inflateInit2(&zs, 15 + 16) != Z_OK) throw Error(GAMS_EINVAL, "decode_gz: inflateInit2 failed");
    zs.next_in = const_cast<Bytef *>(bytes);
    zs.avail_in = (uInt)n;
    size_t at = 0;
    int rc;
    do {
        zs.next_out = dst + at;
        zs.avail_out = (uInt)std::min<size_t>(cap - at, 1u << 30);
        const size_t room = zs.avail_out;
        rc = inflate(&zs, Z_NO_FLUSH);
        at += room - zs.avail_out;
        if (rc != Z_OK && rc != Z_STREAM_END) {
            inflateEnd(&zs);
            throw Error(GAMS_EINVAL, "decode_gz: corrupt gzip member");
        }
        if (rc == Z_OK && at == cap) {          // output full before the member ended
            inflateEnd(&zs);
            *overflow = true;
            return at;
        }
    } while (rc != Z_STREAM_END);
    inflateEnd(&zs);
    return at;
}
}  // namespace

// The first gzip member of `bytes` (flate2's GzDecoder reads one member, redis.rs:156-161) inflated into
// dst[0, cap); returns the bases written.  A member longer than cap is an error.
size_t decode_gz_into(const uint8_t *bytes, size_t n, uint8_t *dst, size_t cap) {
    if (n < 18) throw Error(GAMS_EINVAL, "decode_gz: corrupt gzip member");
    if (libdeflate().ok()) {
        static thread_local Decompressor dc;
        if (!dc.d) dc.d = libdeflate().alloc();
        if (dc.d) {
            size_t got = 0;
            const int rc = libdeflate().gunzip(dc.d, bytes, n, dst, cap, &got);
            if (rc == 0) return got;
            if (rc == 3) throw Error(GAMS_EINVAL, "decode_gz: the member inflates to more than " + std::to_string(cap) + " bytes");
            throw Error(GAMS_EINVAL, "decode_gz: corrupt gzip member");
        }
    }
    bool overflow = false;
    const size_t got = zlib_gunzip_into(bytes, n, dst, cap, &overflow);
    if (overflow) throw Error(GAMS_EINVAL, "decode_gz: the member inflates to more than " + std::to_string(cap) + " bytes");
    return got;
}

std::string decode_gz(const uint8_t *bytes, size_t n) {
    if (n < 18) throw Error(GAMS_EINVAL, "decode_gz: corrupt gzip member");
    // ISIZE (RFC 1952: uncompressed size mod 2^32 in the last four bytes) sizes the output in one piece for a
    // single-member value, which is what the reference stores; anything else grows the buffer
    uint32_t isize;
    std::memcpy(&isize, bytes + n - 4, 4);
    std::string out;
    // (deflate cannot expand beyond 1032:1, so a trailer claiming more is not believed)
    size_t cap = std::max<size_t>(std::min<uint64_t>(isize, (uint64_t)n * 1032u + 64u), 64);
    for (int attempt = 0; attempt < 40; ++attempt) {
        out.resize(cap);
        if (libdeflate().ok()) {
            static thread_local Decompressor dc;
            if (!dc.d) dc.d = libdeflate().alloc();
            if (dc.d) {
                size_t got = 0;
                const int rc = libdeflate().gunzip(dc.d, bytes, n, &out[0], cap, &got);
                if (rc == 0) {
                    out.resize(got);
                    return out;
                }
                if (rc != 3) throw Error(GAMS_EINVAL, "decode_gz: corrupt gzip member");
                cap *= 2;
                continue;
            }
        }
        bool overflow = false;
        const size_t got = zlib_gunzip_into(bytes, n, reinterpret_cast<uint8_t *>(&out[0]), cap, &overflow);
        if (!overflow) {
            out.resize(got);
            return out;
        }
        cap *= 2;
    }
    throw Error(GAMS_EINVAL, "decode_gz: output too large");
}

// get_seq + decode_gz for a batch of values on `threads` host threads, one ctg per worker at a time
// (redis.rs:142-161 inside the workers of wave.rs:288-299)
std::vector<std::string> decode_gz_many(const std::vector<const uint8_t *> &blobs, const std::vector<uint64_t> &blob_len,
                                        unsigned threads) {
    if (blobs.size() != blob_len.size()) throw Error(GAMS_EINVAL, "decode_gz_many: blobs/lengths size mismatch");
    const uint32_t n = (uint32_t)blobs.size();
    std::vector<std::string> out(n);
    const unsigned T = std::max(1u, std::min(threads ? threads : 16u, std::max(n, 1u)));
    std::atomic<uint32_t> next{0};
    std::exception_ptr err;
    std::mutex mu;
    auto work = [&] {
        try {
            for (uint32_t i = next.fetch_add(1); i < n; i = next.fetch_add(1))
                out[i] = decode_gz(blobs[i], (size_t)blob_len[i]);
        } catch (...) {
            std::lock_guard<std::mutex> lk(mu);
            if (!err) err = std::current_exception();
            next.store(n);
        }
    };
    std::vector<std::thread> pool;
    for (unsigned t = 1; t < T; ++t) pool.emplace_back(work);
    work();
    for (auto &th : pool) th.join();
    if (err) std::rethrow_exception(err);
    return out;
}

std::string encode_gz(const uint8_t *bytes, size_t n) {
    z_stream zs{};
    if (deflateInit2(&zs, Z_BEST_SPEED, Z_DEFLATED, 15 + 16, 8, Z_DEFAULT_STRATEGY) != Z_OK)
        throw Error(GAMS_EINVAL, "encode_gz: deflateInit2 failed");
    zs.next_in = const_cast<Bytef *>(bytes);
    zs.avail_in = (uInt)n;
    std::string out;
    char buf[1 << 16];
    int rc;
    do {
        zs.next_out = reinterpret_cast<Bytef *>(buf);
        zs.avail_out = sizeof buf;
        rc = deflate(&zs, Z_FINISH);
        out.append(buf, sizeof buf - zs.avail_out);
    } while (rc != Z_STREAM_END);
    deflateEnd(&zs);
    return out;
}

std::string encode_gz_fast(const uint8_t *bytes, size_t n, bool indexed) {
    const auto twin = indexed ? gams_seq_gz_host_indexed : gams_seq_gz_host;
    uint64_t need = 0;
    if (twin(bytes, n, nullptr, 0, &need) != GAMS_OK) throw Error(GAMS_EINVAL, "encode_gz_fast: bad argument");
    std::string out((size_t)need, '\0');
    if (twin(bytes, n, reinterpret_cast<uint8_t *>(&out[0]), need, &need) != GAMS_OK)
        throw Error(GAMS_EINVAL, "encode_gz_fast: bad argument");
    return out;
}

std::string decode_gz_indexed(const uint8_t *bytes, size_t n) {
    // no room first: the twin checks header, subfield and trailer against one another and says how many bases the member
    // holds (at most 16,380 chunks of 4096); only then is anything allocated
    uint64_t got = 0;
    int status = GAMS_SEQ_GZ_FOREIGN;
    uint8_t spare = 0;
    int rc = gams_seq_gunzip_host(bytes, n, &spare, 0, &got, &status);
    std::string out;
    if (rc == GAMS_EINVAL && bytes && got != 0) {
        out.resize((size_t)got);
        rc = gams_seq_gunzip_host(bytes, n, reinterpret_cast<uint8_t *>(&out[0]), out.size(), &got, &status);
    }
    if (rc != GAMS_OK || status != GAMS_SEQ_GZ_DONE) throw Error(GAMS_EINVAL, "decode_gz_indexed: not an intact indexed member");
    out.resize((size_t)got);
    return out;
}

UploadGz seqset_upload_gz(gams_gpu_t *h, gams_seqset_t *seqset, uint32_t first, const std::vector<const uint8_t *> &blobs,
                          const std::vector<uint64_t> &blob_len, const std::vector<uint32_t> &slot_len, unsigned threads) {
    if (blobs.size() != blob_len.size() || blobs.size() != slot_len.size()) throw Error(GAMS_EINVAL, "seqset_upload_gz: blobs/lengths size mismatch");
    const uint32_t n = (uint32_t)blobs.size();
    UploadGz went;
    if (n == 0) return went;
    std::vector<uint8_t> status(n, GAMS_SEQ_GZ_FOREIGN);
    uint32_t n_foreign = 0;
    check(h, gams_seqset_upload_gz(h, seqset, first, n, blobs.data(), blob_len.data(), status.data(), &n_foreign));
    went.device = n - n_foreign;
    went.host = n_foreign;
    if (n_foreign == 0) return went;
    // the host's way for what is left: inflate on the workers, upload from the calling thread as the values finish
    std::vector<uint32_t> todo;
    for (uint32_t i = 0; i < n; ++i)
        if (status[i] != GAMS_SEQ_GZ_DONE) todo.push_back(i);
    std::vector<std::string> bases(todo.size());
    const unsigned T = std::max(1u, std::min(threads ? threads : 16u, (unsigned)todo.size()));
    std::atomic<uint32_t> next{0};
    std::exception_ptr err;
    std::mutex mu;
    auto work = [&] {
        try {
            for (uint32_t k = next.fetch_add(1); k < todo.size(); k = next.fetch_add(1)) {
                const uint32_t i = todo[k];
                if (blob_len[i] < 18) throw Error(GAMS_EINVAL, "seqset_upload_gz: value " + std::to_string(i) + " is no gzip member");
                bases[k].resize(std::max<size_t>(slot_len[i], 1));   // (a longer value is decode_gz_into's error)
                const size_t got = decode_gz_into(blobs[i], (size_t)blob_len[i], reinterpret_cast<uint8_t *>(&bases[k][0]), slot_len[i]);
                bases[k].resize(got);
            }
        } catch (...) {
            std::lock_guard<std::mutex> lk(mu);
            if (!err) err = std::current_exception();
            next.store((uint32_t)todo.size());
        }
    };
    std::vector<std::thread> pool;
    for (unsigned t = 1; t < T; ++t) pool.emplace_back(work);
    work();
    for (auto &th : pool) th.join();
    if (err) std::rethrow_exception(err);
    for (size_t k = 0; k < todo.size(); ++k) {
        // (gams_seqset_upload reads the slot's length from the buffer: a value of another length is not sent)
        if (bases[k].size() != slot_len[todo[k]])
            throw Error(GAMS_EINVAL, "seqset_upload_gz: value " + std::to_string(todo[k]) + " inflates to " +
                                         std::to_string(bases[k].size()) + " bases, its slot holds " + std::to_string(slot_len[todo[k]]));
        if (!bases[k].empty())
            check(h, gams_seqset_upload(h, seqset, first + todo[k], reinterpret_cast<const uint8_t *>(bases[k].data())));
    }
    check(h, gams_gpu_sync(h));   // the uploads read `bases`
    return went;
}

SeqGz seq_gz(gams_gpu_t *h, gams_seqset_t *seqset, uint32_t first, uint32_t count, const std::vector<std::string> *ctg_ids,
             bool indexed) {
    struct Names {
        gams_gpu_t *h;
        gams_names_t *nm = nullptr;
        ~Names() { gams_names_destroy(h, nm); }
    } names{h};
    if (ctg_ids) {
        if (ctg_ids->size() != count) throw Error(GAMS_EINVAL, "seq_gz: one ctg id per slot");
        std::vector<const char *> p(std::max<size_t>(count, 1), "");
        for (uint32_t i = 0; i < count; ++i) p[i] = (*ctg_ids)[i].c_str();
        check(h, gams_names_create(h, count, p.data(), &names.nm));
    }
    SeqGz out;
    out.off.assign((size_t)count + 1, 0);
    const char *bytes = nullptr;
    uint64_t n = 0;
    check(h, gams_gpu_seq_gz(h, seqset, first, count, names.nm, (ctg_ids ? GAMS_LOADER_RESP : GAMS_SEQ_GZ_MEMBERS) | (indexed ? GAMS_SEQ_GZ_INDEXED : 0), &bytes, &n,
                             out.off.data()));
    out.bytes.assign(bytes, (size_t)n);
    return out;
}

// ---------------------------------------------------------------------------
// gen
// ---------------------------------------------------------------------------
namespace {
// gen.rs:131-150
Ctg make_ctg(const std::string &chr_id, int64_t serial, int32_t start, int32_t end) {
    Ctg c;
    c.id = "ctg:" + chr_id + ":" + std::to_string(serial);
    c.chr_id = chr_id;
    c.chr_start = start;
    c.chr_end = end;
    c.chr_strand = "+";
    c.length = end - start + 1;
    c.range = chr_id + ":" + runlist(start, end);
    return c;
}
}  // namespace

std::vector<Ctg> gen_ctgs(gams_gpu_t *h, const std::string &chr_id, const uint8_t *seq, uint64_t len,
                          const GenArgs &a) {
    // one scan of the chromosome; a second only if it has more valid regions than a generous first guess
    uint64_t n = 0;
    std::vector<int32_t> lo(4096), hi(4096);
    check(h, gams_gpu_valid_spans(h, seq, len, a.fill, a.min, lo.data(), hi.data(), lo.size(), &n));
    if (n > lo.size()) {
        lo.resize(n);
        hi.resize(n);
        check(h, gams_gpu_valid_spans(h, seq, len, a.fill, a.min, lo.data(), hi.data(), n, &n));
    }
    std::vector<Ctg> out;
    int32_t serial = 0;
    for (uint64_t i = 0; i < n; ++i) {                                 // gen.rs:108-126
        gams_piece_split(lo[i], hi[i], a.piece,
                         [&](int64_t s0, int64_t e0) { out.push_back(make_ctg(chr_id, ++serial, (int32_t)s0, (int32_t)e0)); });
    }
    return out;
}

std::vector<FastaRecord> read_fasta(const char *bytes, size_t n) {
    std::vector<FastaRecord> out;
    if (n == 0) return out;
    if (bytes[0] != '>') throw Error(GAMS_EINVAL, "read_fasta: Expected > at record start");
    for (size_t b = 0; b < n;) {
        const char *nl = (const char *)std::memchr(bytes + b, '\n', n - b);
        const size_t end = nl ? (size_t)(nl - bytes) : n;   // the line is bytes[b, end)
        if (bytes[b] == '>') {
            size_t e = b + 1;
            while (e < end && !gams_fasta_space((uint8_t)bytes[e])) ++e;
            out.push_back(FastaRecord{std::string(bytes + b + 1, bytes + e), std::string()});
        } else {
            size_t e = end;
            while (e > b && gams_fasta_space((uint8_t)bytes[e - 1])) --e;
            out.back().seq.append(bytes + b, bytes + e);
        }
        b = end + 1;
    }
    return out;
}

GenText gen_text(gams_gpu_t *h, const char *bytes, size_t n, const GenArgs &a, bool *device) {
    GenText out;
    SeqSetGuard guard{h};
    const gams_gen_params_t prm{a.piece, a.fill, a.min};
    gams_gen_t *g = nullptr;
    const int rc = gams_gpu_gen_text(h, bytes, n, &prm, &g);
    if (device) *device = rc == GAMS_OK;
    if (rc == GAMS_OK) {
        struct GenGuard {
            gams_gpu_t *h;
            gams_gen_t *g;
            ~GenGuard() { gams_gen_destroy(h, g); }
        } gg{h, g};
        uint32_t n_chr = 0, n_ctg = 0;
        uint64_t name_bytes = 0;
        check(h, gams_gen_counts(h, g, &n_chr, &n_ctg, &name_bytes));
        std::string names(name_bytes, '\0');
        std::vector<uint64_t> name_off((size_t)n_chr + 1);
        std::vector<uint32_t> len(n_chr);
        std::vector<gams_gen_ctg_t> tab(n_ctg);
        check(h, gams_gen_chrs(h, g, names.data(), name_off.data(), len.data()));
        check(h, gams_gen_ctgs(h, g, tab.data()));
        for (uint32_t c = 0; c < n_chr; ++c)
            out.chr_len.emplace_back(names.substr(name_off[c], name_off[c + 1] - name_off[c]), len[c]);
        out.ctgs.reserve(n_ctg);
        for (const gams_gen_ctg_t &t : tab) out.ctgs.push_back(make_ctg(out.chr_len[t.chr].first, t.serial, t.chr_start, t.chr_end));
        check(h, gams_gen_seqset(h, g, &out.seqset));
        return out;
    }
    if (rc != GAMS_EUNSUPPORTED) throw Error(rc, gams_gpu_last_error(h));
    // the host passes
    const std::vector<FastaRecord> recs = read_fasta(bytes, n);
    std::map<std::string, int64_t> serial;      // cnt:ctg:{chr}
    std::map<std::string, size_t> len_slot;     // len_of
    std::vector<const uint8_t *> seqs;
    std::vector<uint32_t> lengths;
    for (const FastaRecord &r : recs) {
        auto it = len_slot.find(r.id);
        if (it == len_slot.end()) {
            len_slot[r.id] = out.chr_len.size();
            out.chr_len.emplace_back(r.id, r.seq.size());
        } else {
            out.chr_len[it->second].second = r.seq.size();
        }
        if (r.seq.empty()) continue;
        if (r.seq.size() > 0x7fffffffull) throw Error(GAMS_EUNSUPPORTED, "gen_text: " + r.id + " has more than 2^31 - 1 bases");
        int64_t &sn = serial[r.id];
        for (const Ctg &c : gen_ctgs(h, r.id, (const uint8_t *)r.seq.data(), r.seq.size(), a)) {
            out.ctgs.push_back(make_ctg(r.id, ++sn, c.chr_start, c.chr_end));
            seqs.push_back((const uint8_t *)r.seq.data() + (c.chr_start - 1));
            lengths.push_back((uint32_t)c.length);
        }
    }
    check(h, gams_seqset_create(h, (uint32_t)lengths.size(), lengths.data(), &guard.s));
    check(h, gams_seqset_upload_all(h, guard.s, seqs.data()));   // (staged when it returns: `recs` may go)
    out.seqset = guard.s;
    guard.s = nullptr;
    return out;
}

// ---------------------------------------------------------------------------
// anno
// ---------------------------------------------------------------------------
namespace {

// utils.rs:118-129: first match of (?i)ctg:[\w_]+:\d+
bool extract_ctg_id(const std::string &s, std::string &id) {
    for (size_t i = 0; i + 4 <= s.size(); ++i) {
        if ((s[i] == 'c' || s[i] == 'C') && (s[i + 1] == 't' || s[i + 1] == 'T') &&
            (s[i + 2] == 'g' || s[i + 2] == 'G') && s[i + 3] == ':') {
            size_t j = i + 4;
            while (j < s.size() && is_word(s[j])) ++j;
            if (j == i + 4 || j >= s.size() || s[j] != ':') continue;
            size_t k = j + 1;
            while (k < s.size() && s[k] >= '0' && s[k] <= '9') ++k;
            if (k == j + 1) continue;
            id = s.substr(i, k - i);
            return true;
        }
    }
    return false;
}

}  // namespace

AnnoSet::AnnoSet(gams_gpu_t *h, const char *bytes, size_t n) : h_(h) {
    uint32_t n_groups = 0;
    const int rc = gams_spans_create_runlist_text(h, bytes, n, &sp_, &names_, &n_groups, &n_spans_);
    if (rc == GAMS_EUNSUPPORTED) {                    // the host reader judges the file; its set goes up as arrays
        const RunlistJson js = read_runlist_json(bytes, n);
        std::vector<const Runlist *> sets;
        for (const Runlist &r : js.sets) sets.push_back(&r);
        from_arrays(js.chr, sets);
        return;
    }
    check(h, rc);
    device_ = true;
    // the keys as the device read them, for the lines path of anno()
    uint64_t name_bytes = 0;
    int rc2 = gams_names_read(h, names_, &n_groups, &name_bytes, nullptr, nullptr);
    std::string flat((size_t)name_bytes, '\0');
    std::vector<uint64_t> off((size_t)n_groups + 1, 0);
    if (rc2 == GAMS_OK) rc2 = gams_names_read(h, names_, &n_groups, &name_bytes, &flat[0], off.data());
    if (rc2 != GAMS_OK) {
        gams_spans_destroy(h, sp_);
        gams_names_destroy(h, names_);
        check(h, rc2);
    }
    for (uint32_t g = 0; g < n_groups; ++g) chr_.push_back(flat.substr((size_t)off[g], (size_t)(off[g + 1] - off[g])));
}

AnnoSet::AnnoSet(gams_gpu_t *h, const std::map<std::string, Runlist> &sets) : h_(h) {
    std::vector<std::string> chr;
    std::vector<const Runlist *> rl;
    for (auto &kv : sets) {
        chr.push_back(kv.first);
        rl.push_back(&kv.second);
    }
    from_arrays(chr, rl);
}

void AnnoSet::from_arrays(const std::vector<std::string> &chr, const std::vector<const Runlist *> &sets) {
    std::vector<uint64_t> off{0};
    std::vector<int32_t> lo, hi;
    std::vector<const char *> names;
    for (size_t g = 0; g < chr.size(); ++g) {
        if (chr[g].find('\0') != std::string::npos) throw Error(GAMS_EUNSUPPORTED, "anno: a chr name holds a NUL");
        names.push_back(chr[g].c_str());
        lo.insert(lo.end(), sets[g]->lo.begin(), sets[g]->lo.end());
        hi.insert(hi.end(), sets[g]->hi.begin(), sets[g]->hi.end());
        off.push_back(lo.size());
    }
    check(h_, gams_spans_create(h_, (uint32_t)chr.size(), off.data(), lo.data(), hi.data(), &sp_));
    const int rc = gams_names_create(h_, (uint32_t)chr.size(), names.data(), &names_);
    if (rc != GAMS_OK) {
        gams_spans_destroy(h_, sp_);
        sp_ = nullptr;
        check(h_, rc);
    }
    chr_ = chr;
    n_spans_ = lo.size();
}

AnnoSet::~AnnoSet() {
    if (sp_) gams_spans_destroy(h_, sp_);
    if (names_) gams_names_destroy(h_, names_);
}

std::string anno(gams_gpu_t *h, const std::map<std::string, Runlist> &sets, const std::vector<Ctg> &ctgs,
                 const std::vector<std::string> &lines, bool header, const std::string &prefix, size_t idx_id,
                 size_t idx_range) {
    const AnnoSet set(h, sets);
    return anno(h, set, ctgs, lines, header, prefix, idx_id, idx_range);
}

std::string anno(gams_gpu_t *h, const AnnoSet &set, const std::vector<Ctg> &ctgs, const std::vector<std::string> &lines,
                 bool header, const std::string &prefix, size_t idx_id, size_t idx_range) {
    std::map<std::string, const Ctg *> ctg_of;
    for (const Ctg &c : ctgs) ctg_of[c.id] = &c;
    // the set's groups: one per chr
    std::map<std::string, uint32_t> group_of;
    for (uint32_t g = 0; g < set.chrs().size(); ++g) group_of[set.chrs()[g]] = g;
    gams_spans_t *const sp = set.spans();

    // parse the lines on several threads (each a contiguous run, results concatenated in order),
    // one device call, then format the rows the same way
    struct Part {
        std::vector<size_t> keep;  // lines that produce a row
        std::vector<uint32_t> grp;
        std::vector<int32_t> cl, ch, qs, qe;
        std::string out;
    };
    const size_t first = header ? 1 : 0;
    const size_t n_lines = lines.size() > first ? lines.size() - first : 0;
    const unsigned T = (unsigned)std::max<size_t>(1, std::min<size_t>({16, std::thread::hardware_concurrency(), n_lines / 20000}));
    std::vector<Part> part(T);
    run_shares(T, [&](uint32_t t) {
        Part &P = part[t];
        const size_t b0 = first + n_lines * t / T, b1 = first + n_lines * (t + 1) / T;
        for (size_t i = b0; i < b1; ++i) {                             // anno.rs:97
            // the two tab-separated fields the line is asked for (no vector of all its fields)
            const std::string &ln = lines[i];
            size_t n_fields = 0, fb = 0, id_b = 0, id_e = 0, rg_b = 0, rg_e = 0;
            for (;;) {
                const size_t fe = std::min(ln.find('\t', fb), ln.size());
                ++n_fields;
                if (n_fields == idx_id) id_b = fb, id_e = fe;
                if (n_fields == idx_range) rg_b = fb, rg_e = fe;
                if (fe == ln.size()) break;
                fb = fe + 1;
            }
            if (idx_id == 0 || idx_range == 0 || idx_id > n_fields || idx_range > n_fields)
                throw Error(GAMS_EINVAL, "anno: field index out of range (the reference panics, anno.rs:115)");
            std::string ctg_id;
            if (!extract_ctg_id(ln.substr(id_b, id_e - id_b), ctg_id)) continue;   // anno.rs:116-119
            Range r = Range::from_str(ln.substr(rg_b, rg_e - rg_b));
            if (!r.valid) continue;                                     // anno.rs:123-125
            auto gi = group_of.find(r.chr);
            uint32_t gq = UINT32_MAX;
            int32_t c0 = 0, c1 = 0;
            if (gi != group_of.end()) {                                 // anno.rs:129
                auto ci = ctg_of.find(ctg_id);
                if (ci == ctg_of.end())
                    throw Error(GAMS_EINVAL, "anno: unknown " + ctg_id + " (the reference panics, redis.rs:133-134)");
                gq = gi->second;
                c0 = ci->second->chr_start;
                c1 = ci->second->chr_end;
            }
            P.keep.push_back(i);
            P.grp.push_back(gq);
            P.cl.push_back(c0);
            P.ch.push_back(c1);
            P.qs.push_back(r.start);
            P.qe.push_back(r.end);
        }
    });
    std::vector<size_t> base(T + 1, 0);
    for (unsigned t = 0; t < T; ++t) base[t + 1] = base[t] + part[t].keep.size();
    const size_t nk = base[T];
    std::vector<uint32_t> grp(nk ? nk : 1);
    std::vector<int32_t> cl(nk ? nk : 1), ch(nk ? nk : 1), qs(nk ? nk : 1), qe(nk ? nk : 1);
    for (unsigned t = 0; t < T; ++t) {
        std::copy(part[t].grp.begin(), part[t].grp.end(), grp.begin() + base[t]);
        std::copy(part[t].cl.begin(), part[t].cl.end(), cl.begin() + base[t]);
        std::copy(part[t].ch.begin(), part[t].ch.end(), ch.begin() + base[t]);
        std::copy(part[t].qs.begin(), part[t].qs.end(), qs.begin() + base[t]);
        std::copy(part[t].qe.begin(), part[t].qe.end(), qe.begin() + base[t]);
    }
    std::vector<float> prop(nk ? nk : 1);
    check(h, gams_gpu_cover(h, sp, grp.data(), cl.data(), ch.data(), qs.data(), qe.data(), nk, prop.data()));
    run_shares(T, [&](uint32_t t) {
        Part &P = part[t];
        char buf[64];
        size_t bytes = 0;
        for (size_t i : P.keep) bytes += lines[i].size() + 9;
        P.out.reserve(bytes);
        for (size_t k = 0; k < P.keep.size(); ++k) {
            snprintf(buf, sizeof buf, "%.4f", (double)prop[base[t] + k]);   // anno.rs:140 {:.4}
            P.out += lines[P.keep[k]];
            P.out += '\t';
            P.out += buf;
            P.out += '\n';
        }
    });
    std::string out;
    if (header && !lines.empty()) out += lines[0] + "\t" + prefix + "Prop\n";  // anno.rs:108
    for (unsigned t = 0; t < T; ++t) out += part[t].out;
    return out;
}

std::vector<std::string> text_lines(const char *bytes, size_t n) {
    std::vector<std::string> lines;
    size_t b = 0;
    while (b < n) {
        const char *nl = static_cast<const char *>(std::memchr(bytes + b, '\n', n - b));
        if (!nl) {
            lines.emplace_back(bytes + b, n - b);                        // the last line keeps a '\r'
            break;
        }
        size_t e = (size_t)(nl - bytes);
        const size_t next = e + 1;
        if (e > b && bytes[e - 1] == '\r') --e;
        lines.emplace_back(bytes + b, e - b);
        b = next;
    }
    return lines;
}

std::string fmt_f32_short(float v) {
    char buf[40];
    return std::string(buf, gams_fmt_f32_short(v, buf));
}

std::string fmt_prop4(float p) {
    char buf[8];
    if (!gams_fmt_prop4(p, buf)) return std::string();
    return std::string(buf, 6);
}

std::string anno_text(gams_gpu_t *h, const std::map<std::string, Runlist> &sets, const std::vector<Ctg> &ctgs,
                      const char *bytes, size_t n, bool header, const std::string &prefix, size_t idx_id,
                      size_t idx_range, bool *device) {
    if (device) *device = false;
    // the device image of the runlists (one group per chr, in the set's order) and its name table, for this call
    const AnnoSet set(h, sets);
    return anno_text(h, set, ctgs, bytes, n, header, prefix, idx_id, idx_range, device);
}

std::string anno_text(gams_gpu_t *h, const AnnoSet &set, const std::vector<Ctg> &ctgs, const char *bytes, size_t n,
                      bool header, const std::string &prefix, size_t idx_id, size_t idx_range, bool *device) {
    if (device) *device = false;
    std::vector<const char *> ids(ctgs.size());
    std::vector<int32_t> cs(ctgs.size()), ce(ctgs.size());
    for (size_t i = 0; i < ctgs.size(); ++i) {
        ids[i] = ctgs[i].id.c_str();
        cs[i] = ctgs[i].chr_start;
        ce[i] = ctgs[i].chr_end;
    }
    struct Guard {
        gams_gpu_t *h;
        gams_names_t *ids = nullptr;
        ~Guard() {
            if (ids) gams_names_destroy(h, ids);
        }
    } g{h};
    check(h, gams_names_create(h, (uint32_t)ids.size(), ids.data(), &g.ids));
    if (idx_id > UINT32_MAX || idx_range > UINT32_MAX) throw Error(GAMS_EINVAL, "anno: field index out of range");
    const char *text = nullptr;
    uint64_t text_bytes = 0, rows = 0;
    const int rc = gams_gpu_anno_text(h, set.spans(), set.chr_names(), g.ids, cs.data(), ce.data(), bytes, n, header ? 1 : 0,
                                      prefix.c_str(), (uint32_t)idx_id, (uint32_t)idx_range, &text, &text_bytes, &rows);
    if (rc == GAMS_EUNSUPPORTED)
        return anno(h, set, ctgs, text_lines(bytes, n), header, prefix, idx_id, idx_range);
    check(h, rc);
    if (device) *device = true;
    return std::string(text, (size_t)text_bytes);
}

}  // namespace gams
