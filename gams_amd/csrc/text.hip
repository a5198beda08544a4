// text.hip -- text in, text out for the interval commands: the bytes of a `locate -f` / `locate --count` /
// `anno` input file go to the device once, and the finished TSV rows come back.
//
//   gams_gpu_locate_text   locate.rs:84-141 with utils.rs:7-22   "{rg}\t{ctg_id}\n"
//   gams_gpu_count_text    locate.rs:84-141 with utils.rs:24-36  "{rg}\t{count}\n"
//   gams_gpu_anno_text     anno.rs:95-142 (one input file)       "{line}\t{prop:.4}\n"
// and text in, index out for the rg loader (utils.rs:39-67 read_range, then redis.rs:288-299), behind the same
// upload and line index (the stages are listed in front of its kernels, below):
//   gams_gpu_read_range_text       the ranges of one .rg file bucketed per ctg, as arrays
//   gams_index_create_range_text   the rg index of the file and the ctg -> group table
// and, on the loader itself (rg_load, each with a spec and a consumer of its own, which takes the kept lines as an
// RgKept), `gams peak` (utils.rs:83-116 read_peak, then peak.rs:41-160), its rows through the keyed row writer:
//   gams_gpu_peak_text             the bytes of one wave TSV -> the Peak rows of every ctg
//   gams_gpu_peak_records_text     ... -> the records `gams peak` SETs: "{id}\t{json}" rows, TSV or RESP, serials behind a counter
// and `gams sw` from a feature file (feature.rs:50-86 read_range and ids, then sw.rs:132-191):
//   gams_gpu_sw_feature_text       the bytes of one range file -> the sw rows of its features (stages 2-5 in sw.hip)
// and several files in one load (rg.rs:40, feature.rs:47: one read_range per file), an RgInput of files:
//   gams_index_create_range_files  the rg index of `gams rg f1 f2 ...`
//   gams_gpu_loader_text           the records `gams rg` / `gams feature` SET, as "{id}\t{json}" rows, TSV or RESP
// and `locate --seq` (locate.rs:124-134), behind the front of locate_text, with a writer of its own (a row may be a whole ctg):
//   gams_gpu_locate_seq_text       the bytes of one range file -> ">{rg}\n{bases}\n" of every located line
//
// Pipeline (one handle, the compute stream):
//   1. one copy of the bytes into a cached device buffer, padded with spaces to 16 B and 16 B beyond;
//   2. line index: every lane takes 64 contiguous bytes as four 16-B loads, counts the '\n' bytes with an exact
//      zero-byte mask and flags bytes >= 0x80 or NUL; a one-workgroup scan of the block counts and a second pass
//      turn them into 64-bit line starts (BufRead::lines(): split on '\n', one '\r' before it dropped);
//   3. parse, one lane per line: the field(s), Range::from_str, the chromosome (and for anno the ctg id) looked up
//      in a device hash table of names (gams_names_t);
//   4. the existing lookup kernels (interval_kernels.hpp) on those device columns;
//   5. row lengths -> block scan -> rows written at their offsets, echoing the input bytes; one read-back into
//      page-locked memory owned by the handle.
// Three host waits per call: the line count (to size the per-line columns), the flags and the text size (to size
// the text), the text.

#include "interval_kernels.hpp"
#include "seq_text_plan.hpp"
#include "text_emit.hpp"
#include "text_fmt.hpp"

#include <rocprim/rocprim.hpp>   // the radix sort that orders the kept lines of the range loader

#include <algorithm>
#include <string>
#include <type_traits>
#include <unordered_set>
#include <vector>

// one slot of the open-addressing table: 64-bit hash of the name and its position (UINT32_MAX: empty)
struct NameSlot {
    unsigned long long hash;
    uint32_t idx;
    uint32_t pad;
};

struct NameTab {
    const NameSlot *slot;
    const unsigned long long *off;   // n + 1 byte offsets into bytes
    const char *bytes;
    uint32_t mask;                   // slots - 1 (slots a power of two >= 2n: load <= 0.5)
    uint32_t n;
};

struct gams_names {
    NameTab t{};
    uint8_t *arena = nullptr;
    size_t arena_bytes = 0;
    uint32_t max_len = 0;            // the longest name, in bytes (bounds a row that prints one)
};

// The entries that own a text: each keeps the page-locked text of its last call in a slot of its own (gams_gpu.h: valid
// until the next call of THAT entry; and a text of whole ctgs from locate --seq is not held by the others for good).
enum TextSlot : int { TEXT_LOCATE = 0, TEXT_COUNT, TEXT_ANNO, TEXT_PEAK, TEXT_RECORDS, TEXT_SEQ, TEXT_PEAK_RECORDS, TEXT_SLOTS };

// What the text entries keep on the handle: the device copy of the input (grows, cached) and the text slots.
struct gams_text_state {
    uint8_t *d_in = nullptr;
    size_t d_in_cap = 0;
    char *out[TEXT_SLOTS] = {};
    size_t out_cap[TEXT_SLOTS] = {};
};

void gams_text_free(gams_gpu_t *h) {
    gams_text_state *t = h->text;
    if (!t) return;
    gams_pool_free(h, false, t->d_in, t->d_in_cap);
    for (int k = 0; k < TEXT_SLOTS; ++k) gams_pool_free(h, true, t->out[k], t->out_cap[k]);
    delete t;
    h->text = nullptr;
}

void gams_names_view(const gams_names_t *nm, const unsigned long long **off, const char **bytes, uint32_t *n) {
    *off = nm->t.off;
    *bytes = nm->t.bytes;
    *n = nm->t.n;
}

hipError_t gams_text_input(gams_gpu_t *h, size_t bytes, uint8_t **d_in) {
    if (!h->text) h->text = new gams_text_state();
    gams_text_state *T = h->text;
    const hipError_t e = gams_pool_grow(h, false, &T->d_in, &T->d_in_cap, bytes, bytes);
    *d_in = T->d_in;
    return e;
}

namespace {

// FNV-1a, 64 bits, over the name's bytes (host and device)
__host__ __device__ inline unsigned long long name_hash(const char *s, uint64_t n) {
    unsigned long long x = 0xcbf29ce484222325ull;
    for (uint64_t i = 0; i < n; ++i) {
        x ^= (uint8_t)s[i];
        x *= 0x100000001b3ull;
    }
    return x;
}

// position of the name s[0..n) in the table, UINT32_MAX if absent (exact byte equality)
__device__ inline uint32_t name_find(const NameTab &t, const char *s, uint64_t n) {
    if (t.n == 0) return UINT32_MAX;
    const unsigned long long x = name_hash(s, n);
    for (uint32_t i = (uint32_t)x & t.mask;; i = (i + 1u) & t.mask) {
        const NameSlot sl = t.slot[i];
        if (sl.idx == UINT32_MAX) return UINT32_MAX;
        if (sl.hash != x) continue;
        const unsigned long long b = t.off[sl.idx];
        if (t.off[sl.idx + 1u] - b != n) continue;
        uint64_t k = 0;
        while (k < n && t.bytes[b + k] == s[k]) ++k;
        if (k == n) return sl.idx;
    }
}

enum : uint32_t {
    W_NL = 0,      // '\n' bytes of the input
    W_BAD = 1,     // a byte >= 0x80 or NUL
    W_EFIELD = 2,  // anno: a line without field idx_id or idx_range; peak: a valid range without a third field
    W_EID = 3,     // anno: a ctg id not in ctg_ids on a chromosome of the set; peak: a kept peak that leaves its ctg
    W_UNSUP = 4,   // count: a located ctg without an rg group; anno: a prop that is not finite in [0, 1]; peak: a float
                   // the formatters do not cover
    W_BYTES = 5,   // text bytes
    W_ROWS = 6,    // rows
    W_ENOSEQ = 7,  // peak: a kept peak in a ctg without a sequence
    W_COUNT = 8
};

// the words of the call in h->pin_scratch, once everything queued on the compute stream has run: one host wait
hipError_t read_words(gams_gpu_t *h, const unsigned long long *d_words) {
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(h->pin_scratch, d_words, W_COUNT * 8, hipMemcpyDeviceToHost, h->compute);
    return e == hipSuccess ? hipStreamSynchronize(h->compute) : e;
}

constexpr uint32_t kIdxBytes = 256u * 64u;   // bytes per workgroup of the line-index kernels

__device__ __forceinline__ uint32_t nl_mask(uint32_t w) { return zero_bytes(w ^ 0x0a0a0a0au); }
__device__ __forceinline__ uint32_t bad_mask(uint32_t w) { return (w & 0x80808080u) | zero_bytes(w); }

// pass 1: '\n' per workgroup of kIdxBytes, and the flag of refused bytes.  n16: the input rounded up to 16 B
// (the padding holds spaces).
__global__ __launch_bounds__(256) void text_nl_count_kernel(const uint8_t *in, uint64_t n16, uint32_t *blk_nl,
                                                            unsigned long long *words) {
    __shared__ uint32_t ws[4];
    const uint64_t p0 = ((uint64_t)blockIdx.x * 256u + threadIdx.x) * 64u;
    uint32_t c = 0, bad = 0;
#pragma unroll
    for (uint32_t u = 0; u < 4u; ++u) {
        const uint64_t p = p0 + 16u * u;
        if (p >= n16) break;
        const uint4 v = *reinterpret_cast<const uint4 *>(in + p);
        c += __popc(nl_mask(v.x)) + __popc(nl_mask(v.y)) + __popc(nl_mask(v.z)) + __popc(nl_mask(v.w));
        bad |= bad_mask(v.x) | bad_mask(v.y) | bad_mask(v.z) | bad_mask(v.w);
    }
    if (bad) words[W_BAD] = 1ull;
    uint32_t tot;
    (void)block_excl_scan_256<uint32_t>(c, ws, tot);
    if (threadIdx.x == 0) blk_nl[blockIdx.x] = tot;
}

// pass 2: starts[k + 1] = position after the k-th '\n'; starts[0] = 0 and starts[nl + 1] = n + 1, so that line i
// is [starts[i], starts[i + 1] - 1) before the '\r' rule
__global__ __launch_bounds__(256) void text_line_start_kernel(const uint8_t *in, uint64_t n, uint64_t n16,
                                                              const unsigned long long *blk_off, uint64_t nl,
                                                              unsigned long long *starts) {
    __shared__ uint32_t ws[4];
    const uint64_t p0 = ((uint64_t)blockIdx.x * 256u + threadIdx.x) * 64u;
    uint4 v[4];
    uint32_t c = 0;
#pragma unroll
    for (uint32_t u = 0; u < 4u; ++u) {
        const uint64_t p = p0 + 16u * u;
        v[u] = p < n16 ? *reinterpret_cast<const uint4 *>(in + p) : make_uint4(0u, 0u, 0u, 0u);
        c += __popc(nl_mask(v[u].x)) + __popc(nl_mask(v[u].y)) + __popc(nl_mask(v[u].z)) + __popc(nl_mask(v[u].w));
    }
    uint32_t tot;
    const uint32_t rel = block_excl_scan_256<uint32_t>(c, ws, tot);
    unsigned long long *dst = starts + 1u + blk_off[blockIdx.x] + rel;
#pragma unroll
    for (uint32_t u = 0; u < 4u; ++u) {
        const uint32_t w4[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
#pragma unroll
        for (uint32_t k = 0; k < 4u; ++k) {
            uint32_t m = nl_mask(w4[k]);
            while (m) {
                const uint32_t byte = (uint32_t)__builtin_ctz(m) >> 3;
                *dst++ = p0 + 16u * u + 4u * k + byte + 1u;
                m &= m - 1u;
            }
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        starts[0] = 0;
        starts[nl + 1u] = n + 1u;
    }
}

struct TextLines {
    const char *in;
    const unsigned long long *starts;
    uint64_t nl;
    uint32_t n_lines;
};

__device__ __forceinline__ void line_of(const TextLines &t, uint32_t i, uint64_t &b, uint64_t &e) {
    b = t.starts[i];
    e = t.starts[i + 1u] - 1u;
    if (i < t.nl && e > b && t.in[e - 1u] == '\r') --e;   // "\r\n" ends the line; a last line keeps its '\r'
}

__device__ __forceinline__ bool is_word_c(char c) {
    return (c >= '0' && c <= '9') || (c >= 'a' && c <= 'z') || (c >= 'A' && c <= 'Z') || c == '_';
}

// intspan Range::from_str over s[b, e) (gams_host.cpp Range::from_str, step for step): on success the chromosome
// is s[cb, ce) and the range start..end
struct RangeField {
    uint64_t cb, ce;      // the chromosome: s[cb, ce)
    uint32_t start, end;
    bool ok;
};

__device__ RangeField parse_range(const char *s, uint64_t b, uint64_t e) {
    RangeField r{0, 0, 0, 0, false};
    while (e > b && (s[e - 1u] == '\r' || s[e - 1u] == '\n' || s[e - 1u] == ' ')) --e;
    // rfind(':'): past the last colon only digits and separators can follow in a valid range
    uint64_t c = e;
    while (c > b) {
        const char x = s[c - 1u];
        if (x == ':') break;
        if (!(is_digit_c(x) || x == '-' || x == '_')) return r;
        --c;
    }
    if (c == b) return r;                 // no colon
    const uint64_t colon = c - 1u;
    if (colon == b || colon + 1u >= e) return r;
    uint64_t i = colon + 1u, k;
    const uint32_t st = digits(s, i, e);
    if (i == colon + 1u || i - colon - 1u > 10u) return r;
    uint32_t en = st;
    if (i < e) {
        uint64_t j = i;
        while (j < e && (s[j] == '-' || s[j] == '_')) ++j;
        if (j == i) return r;
        k = j;
        en = digits(s, k, e);
        if (k == j || k != e || k - j > 10u) return r;
    }
    if (st > 0x7fffffffu || en > 0x7fffffffu) return r;
    // head: [name.]chr[(strand)]
    uint64_t hb = b, he = colon;
    if (he > hb && s[he - 1u] == ')') {
        uint64_t o = he - 1u;
        while (o > hb && s[o - 1u] != '(') --o;
        if (o == hb) return r;            // no '('
        he = o - 1u;
    }
    for (uint64_t d = hb; d < he; ++d)
        if (s[d] == '.') {
            hb = d + 1u;
            break;
        }
    if (he == hb) return r;
    for (uint64_t d = hb; d < he; ++d) {
        const char x = s[d];
        if (!(is_word_c(x) || x == '-' || x == '/')) return r;
    }
    r.cb = hb;
    r.ce = he;
    r.start = st;
    r.end = en;
    r.ok = true;
    return r;
}

// locate / count: rg = the line up to its first tab (locate.rs:89-91); (group, start, end) and where rg ends
__global__ __launch_bounds__(256) void text_parse_rg_kernel(const TextLines t, const NameTab chr, uint32_t *grp,
                                                            uint32_t *qs, uint32_t *qe, unsigned long long *fend) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= t.n_lines) return;
    uint64_t b, e;
    line_of(t, i, b, e);
    uint64_t f = b;
    while (f < e && t.in[f] != '\t') ++f;
    const RangeField r = parse_range(t.in, b, f);
    grp[i] = r.ok ? name_find(chr, t.in + r.cb, r.ce - r.cb) : UINT32_MAX;
    qs[i] = r.start;
    qe[i] = r.end;
    fend[i] = f;
}

// count: rg group of the located ctg (UINT32_MAX for an unlocated line)
__global__ __launch_bounds__(256) void text_rg_group_kernel(uint32_t n_lines, const int64_t *hit, const uint32_t *rg_group,
                                                            uint32_t *cg, unsigned long long *words) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_lines) return;
    const int64_t c = hit[i];
    uint32_t g = UINT32_MAX;
    if (c >= 0) {
        g = rg_group[c];
        if (g == UINT32_MAX) words[W_UNSUP] = 1ull;   // the host path reports "not found in idx" (utils.rs:30)
    }
    cg[i] = g;
}

struct AnnoArgs {
    NameTab chr, ids;
    const int32_t *ctg_start, *ctg_end;
    uint32_t idx_id, idx_range;
    uint32_t first;   // 1 with a header line: line 0 is not parsed
};

// anno.rs:112-139 per line: field idx_id -> first (?i)ctg:[\w_]+:\d+ (utils.rs:118-129); field idx_range -> Range
__global__ __launch_bounds__(256) void text_parse_anno_kernel(const TextLines t, const AnnoArgs a, uint32_t *grp,
                                                              int32_t *cl, int32_t *ch, int32_t *qs, int32_t *qe,
                                                              uint8_t *keep, unsigned long long *words) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= t.n_lines) return;
    grp[i] = UINT32_MAX;
    keep[i] = 0;
    if (i < a.first) return;
    uint64_t b, e;
    line_of(t, i, b, e);
    const char *s = t.in;
    // the two fields, 1-based
    uint64_t ib = 0, ie = 0, rb = 0, re = 0, fb = b;
    uint32_t nf = 0, found = 0;
    for (;;) {
        uint64_t fe = fb;
        while (fe < e && s[fe] != '\t') ++fe;
        ++nf;
        if (nf == a.idx_id) ib = fb, ie = fe, found |= 1u;
        if (nf == a.idx_range) rb = fb, re = fe, found |= 2u;
        if (found == 3u || fe == e) break;
        fb = fe + 1u;
    }
    if (found != 3u) {
        words[W_EFIELD] = 1ull;                // the reference panics (anno.rs:115)
        return;
    }
    uint64_t xb = 0, xe = 0;
    bool has_id = false;
    for (uint64_t p = ib; p + 4u <= ie && !has_id; ++p) {
        if (!((s[p] == 'c' || s[p] == 'C') && (s[p + 1u] == 't' || s[p + 1u] == 'T') &&
              (s[p + 2u] == 'g' || s[p + 2u] == 'G') && s[p + 3u] == ':'))
            continue;
        uint64_t j = p + 4u;
        while (j < ie && is_word_c(s[j])) ++j;
        if (j == p + 4u || j >= ie || s[j] != ':') continue;
        uint64_t k = j + 1u;
        while (k < ie && is_digit_c(s[k])) ++k;
        if (k == j + 1u) continue;
        xb = p;
        xe = k;
        has_id = true;
    }
    if (!has_id) return;                       // anno.rs:116-119
    const RangeField r = parse_range(s, rb, re);
    if (!r.ok) return;                         // anno.rs:123-125
    const uint32_t g = name_find(a.chr, s + r.cb, r.ce - r.cb);
    int32_t c0 = 0, c1 = 0;
    if (g != UINT32_MAX) {                     // anno.rs:129
        const uint32_t slot = name_find(a.ids, s + xb, xe - xb);
        if (slot == UINT32_MAX) {
            words[W_EID] = 1ull;               // the reference panics (redis.rs:133-134)
            return;
        }
        c0 = a.ctg_start[slot];
        c1 = a.ctg_end[slot];
    }
    grp[i] = g;
    cl[i] = c0;
    ch[i] = c1;
    qs[i] = (int32_t)r.start;
    qe[i] = (int32_t)r.end;
    keep[i] = 1;
}

enum : int { K_LOCATE = TEXT_LOCATE, K_COUNT = TEXT_COUNT, K_ANNO = TEXT_ANNO };   // a kind of text_run is the slot of its text

struct RowArgs {
    TextLines t;
    int kind;
    const unsigned long long *fend;   // locate / count: end of the rg field
    const int64_t *hit;               // locate / count
    NameTab ids;                      // locate: ctg id text
    const int32_t *cnt;               // count
    const uint8_t *keep;              // anno
    const uint32_t *grp;              // anno: span group (UINT32_MAX: chromosome not in the set)
    const int32_t *qs, *qe;           // anno
    const float *prop;                // anno
    const char *prefix;               // anno header
    uint32_t prefix_len;
    uint32_t header;
    unsigned long long *blk_bytes;    // per workgroup of 256 rows
    const unsigned long long *blk_off;
    unsigned long long *words;
    char *text;
};

// The row of line i (none for a line that has none), counted or written; `bad`: the value has no text of the reference's
template <bool kWrite>
__device__ void text_row(const RowArgs &a, uint32_t i, RowOut<kWrite, uint64_t> &o, bool &bad) {
    uint64_t b, e;
    if (a.kind == K_ANNO) {
        const bool head = a.header && i == 0u;
        if (!head && !a.keep[i]) return;
        line_of(a.t, i, b, e);
        o.bytes(a.t.in + b, e - b);
        o.ch('\t');
        if (head) {                                     // "{line}\t{prefix}Prop\n"
            o.bytes(a.prefix, a.prefix_len);
            o.bytes("Prop\n", 5u);
            return;
        }
        const float p = a.prop[i];
        // a reversed range on a chromosome of the set: the reference's prop is 0/0
        if (a.grp[i] != UINT32_MAX && (a.qe[i] < a.qs[i] || !(p >= 0.0f && p <= 1.0f))) bad = true;
        o.prop4(p);                                     // anno.rs:140
        o.ch('\n');
        return;
    }
    const int64_t c = a.hit[i];
    if (c < 0) return;
    b = a.t.starts[i];
    o.bytes(a.t.in + b, a.fend[i] - b);
    o.ch('\t');
    if (a.kind == K_LOCATE) {
        const unsigned long long io = a.ids.off[c];
        o.bytes(a.ids.bytes + io, a.ids.off[c + 1] - io);   // locate.rs:139
    } else {
        o.i32(a.cnt[i]);                                    // locate.rs:137
    }
    o.ch('\n');
}

__device__ __forceinline__ uint64_t text_row_len(const RowArgs &a, uint32_t i, bool &bad) {
    RowOut<false, uint64_t> n;
    if (i < a.t.n_lines) text_row(a, i, n, bad);
    return n.n;
}

// behind a block's row lengths (l: this thread's, 0 = no row): the block's bytes, and its rows added to words[W_ROWS]
__device__ __forceinline__ void row_block_totals(uint64_t l, unsigned long long *blk_bytes, unsigned long long *words) {
    __shared__ uint64_t ws[4];
    uint64_t tot;
    (void)block_excl_scan_256<uint64_t>(l, ws, tot);
    __shared__ uint32_t rows[4];
    uint32_t r = __popcll(__ballot(l != 0ull));
    if ((threadIdx.x & 63u) == 0u) rows[threadIdx.x >> 6] = r;
    __syncthreads();
    if (threadIdx.x == 0) {
        blk_bytes[blockIdx.x] = tot;
        atomicAdd(words + W_ROWS, (unsigned long long)(rows[0] + rows[1] + rows[2] + rows[3]));
    }
}

__global__ __launch_bounds__(256) void text_row_len_kernel(const RowArgs a) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    bool bad = false;
    const uint64_t l = text_row_len(a, i, bad);
    if (bad) a.words[W_UNSUP] = 1ull;
    row_block_totals(l, a.blk_bytes, a.words);
}

__global__ __launch_bounds__(256) void text_row_write_kernel(const RowArgs a) {
    __shared__ uint64_t ws[4];
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    bool bad = false;                          // (the length pass flagged what has no text)
    const uint64_t l = text_row_len(a, i, bad);
    uint64_t tot;
    const uint64_t rel = block_excl_scan_256<uint64_t>(l, ws, tot);
    if (l == 0ull) return;
    RowOut<true, uint64_t> o{a.text + a.blk_off[blockIdx.x] + rel};
    text_row(a, i, o, bad);
}

struct TextJob {
    int kind;
    const gams_index_t *ctg_ix;
    const gams_index_t *rg_ix;
    const gams_names_t *chr, *ids;
    const uint32_t *rg_group;          // count: ctg_ix->m entries
    const gams_spans_t *sp;
    const int32_t *ctg_start, *ctg_end;
    int header;
    const char *prefix;
    uint32_t idx_id, idx_range;
};

const char *const kEntry[3] = {"gpu_locate_text", "gpu_count_text", "gpu_anno_text"};

// several input files of one load (the rg / feature loaders): n files, file f = bytes[f][0 .. n_bytes[f])
struct TextFiles {
    uint32_t n;
    const char *const *bytes;
    const uint64_t *n_bytes;
};

// What steps 1 and 2 (pass 1) of every text entry leave behind: the input in the handle's cached device buffer, the
// words, the '\n' count of every index block with its prefix, and the line count.  s0 is the pooled block behind the
// three small arrays.
struct TextFront {
    explicit TextFront(gams_gpu_t *h) : s0(h, false) {}
    PoolBlock s0;
    // set by the caller in front of text_front: the input is these files, uploaded back to back with a '\n' put behind
    // a file that lacks its last one and has a file behind it, so that no line runs across a seam and the line numbers
    // of the buffer rise with (file, line).  (The '\r' such a line keeps in the reference is dropped with the '\n' here;
    // Range::from_str trims it either way.)  text_front leaves where every file begins, and the end, in file_off.
    const TextFiles *files = nullptr;
    std::vector<uint64_t> file_off;
    uint64_t n_in = 0;       // bytes of the input as uploaded
    unsigned long long *d_words = nullptr;
    uint32_t *d_bnl = nullptr;
    unsigned long long *d_bnloff = nullptr;
    uint32_t nbi = 0;
    uint64_t n16 = 0, nl = 0;
    uint32_t L = 0;          // lines (BufRead::lines())
};

int text_front(gams_gpu_t *h, const std::string &who, const char *bytes, uint64_t n_bytes, TextFront &F) {
    if (!h->text) h->text = new gams_text_state();
    gams_text_state *T = h->text;
    bool last_nl = n_bytes && bytes[n_bytes - 1] == '\n';
    if (F.files) {
        const TextFiles &S = *F.files;
        F.file_off.assign((size_t)S.n + 1, 0);
        uint64_t at = 0;
        for (uint32_t f = 0; f < S.n; ++f) {
            F.file_off[f] = at;
            const uint64_t nb = S.n_bytes[f];
            if (nb == 0) continue;
            at += nb;
            last_nl = S.bytes[f][nb - 1] == '\n';
            if (!last_nl && f + 1u < S.n) {
                ++at;
                last_nl = true;
            }
        }
        F.file_off[S.n] = at;
        n_bytes = at;
    }
    F.n_in = n_bytes;
    const uint64_t n16 = (n_bytes + 15u) & ~15ull;
    F.n16 = n16;
    // 1. upload into the cached buffer; the 16-B tail is spaces (no '\n', nothing refused)
    const uint64_t n_pad = n16 + 16u;                 // the parse kernels may look 11 bytes past a field's end
    GAMS_TRY(h, who, gams_pool_grow(h, false, &T->d_in, &T->d_in_cap, n_pad, n_pad));
    hipStream_t st = h->compute;
    const uint32_t nbi = (uint32_t)std::max<uint64_t>(1, (n16 + kIdxBytes - 1) / kIdxBytes);
    F.nbi = nbi;
    auto front = [&](Carver &c) {         // words | '\n' per index block | their prefix
        F.d_words = c.take<unsigned long long>(W_COUNT);
        F.d_bnl = c.take<uint32_t>(nbi);
        F.d_bnloff = c.take<unsigned long long>((size_t)nbi + 1);
    };
    GAMS_TRY(h, who, F.s0.alloc(layout_bytes(front)));
    carve(F.s0.p, front);
    unsigned long long *const d_words = F.d_words;
    GAMS_TRY(h, who, hipEventRecord(h->k0, st));
    h->k_valid = false;
    h->kq_used = 0;
    GAMS_TRY(h, who, hipMemsetAsync(d_words, 0, W_COUNT * 8, st));
    if (F.files) {
        for (uint32_t f = 0; f < F.files->n; ++f) {
            const uint64_t nb = F.files->n_bytes[f], at = F.file_off[f];
            if (nb) GAMS_TRY(h, who, hipMemcpyAsync(T->d_in + at, F.files->bytes[f], nb, hipMemcpyHostToDevice, st));
            if (F.file_off[f + 1] - at > nb) GAMS_TRY(h, who, hipMemsetAsync(T->d_in + at + nb, '\n', 1, st));
        }
    } else if (n_bytes) {
        GAMS_TRY(h, who, hipMemcpyAsync(T->d_in, bytes, n_bytes, hipMemcpyHostToDevice, st));
    }
    GAMS_TRY(h, who, hipMemsetAsync(T->d_in + n_bytes, ' ', n_pad - n_bytes, st));
    // 2. line index, pass 1
    hipLaunchKernelGGL(text_nl_count_kernel, dim3(nbi), dim3(256), 0, st, T->d_in, n16, F.d_bnl, d_words);
    hipLaunchKernelGGL(blk_offsets_scan_kernel<uint32_t>, dim3(1), dim3(1024), 0, st, F.d_bnl, nbi, F.d_bnloff, d_words, (uint32_t)W_NL);
    GAMS_TRY(h, who, hipGetLastError());
    GAMS_TRY(h, who, hipMemcpyAsync(h->pin_scratch, d_words, 2 * 8, hipMemcpyDeviceToHost, st));
    GAMS_TRY(h, who, hipStreamSynchronize(st));
    F.nl = h->pin_scratch[W_NL];
    if (h->pin_scratch[W_BAD])
        return gams_fail(h, GAMS_EUNSUPPORTED, who + ": the input holds a byte >= 0x80 or a NUL (use the host path)");
    const uint64_t L64 = n_bytes == 0 ? 0 : F.nl + (last_nl ? 0u : 1u);
    if (L64 > 0xffffffffull) return gams_fail(h, GAMS_EUNSUPPORTED, who + ": more than 2^32 - 1 lines");
    F.L = (uint32_t)L64;
    return GAMS_OK;
}

int text_run(gams_gpu_t *h, const TextJob &J, const char *bytes, uint64_t n_bytes, const char **text,
             uint64_t *text_bytes, uint64_t *n_rows) {
    const std::string who = kEntry[J.kind];
    *text = nullptr;
    *text_bytes = 0;
    *n_rows = 0;
    GAMS_HIP(h, hipSetDevice(h->device));
    PoolBlock s1(h, false);
    TextFront F(h);
    const int rc_front = text_front(h, who, bytes, n_bytes, F);
    if (rc_front != GAMS_OK) return rc_front;
    gams_text_state *T = h->text;
    hipStream_t st = h->compute;
    const uint64_t n16 = F.n16, nl = F.nl;
    const uint32_t nbi = F.nbi, L = F.L;
    unsigned long long *d_words = F.d_words, *d_bnloff = F.d_bnloff;
    if (J.kind == K_ANNO && L > (uint32_t)(J.header ? 1 : 0) && (J.idx_id == 0 || J.idx_range == 0))
        return gams_fail(h, GAMS_EINVAL, who + ": field index 0 (the reference panics, anno.rs:115)");
    if (L == 0) {
        *text = "";
        return GAMS_OK;
    }
    // per-line columns
    const uint32_t nbr = (L + 255u) / 256u;
    const uint64_t m_ctg = J.kind == K_ANNO ? 0 : J.ctg_ix->m, n_ids = J.ids ? J.ids->t.n : 0;
    const size_t n_rgg = J.kind == K_COUNT ? std::max<uint64_t>(m_ctg, 1) : 0;
    const size_t n_cpos = J.kind == K_ANNO ? std::max<uint64_t>(n_ids, 1) : 0;
    const size_t prefix_len = J.kind == K_ANNO && J.header && J.prefix ? strlen(J.prefix) : 0;
    auto cols = [&](Carver &cv) { return text_cols_layout(cv, nl, L, nbr, n_rgg, n_cpos, prefix_len); };
    GAMS_TRY(h, who, s1.alloc(layout_bytes(cols)));
    const TextCols c = carve(s1.p, cols);
    if (n_rgg && m_ctg) GAMS_TRY(h, who, hipMemcpyAsync(c.rgg, J.rg_group, m_ctg * 4, hipMemcpyHostToDevice, st));
    if (n_cpos && n_ids) {
        GAMS_TRY(h, who, hipMemcpyAsync(c.cs, J.ctg_start, n_ids * 4, hipMemcpyHostToDevice, st));
        GAMS_TRY(h, who, hipMemcpyAsync(c.ce, J.ctg_end, n_ids * 4, hipMemcpyHostToDevice, st));
    }
    if (prefix_len) GAMS_TRY(h, who, hipMemcpyAsync(c.prefix, J.prefix, prefix_len, hipMemcpyHostToDevice, st));
    // 2. line index, pass 2
    hipLaunchKernelGGL(text_line_start_kernel, dim3(nbi), dim3(256), 0, st, T->d_in, n_bytes, n16, d_bnloff, nl, c.starts);
    const TextLines tl{reinterpret_cast<const char *>(T->d_in), c.starts, nl, L};
    RowArgs ra{};
    ra.t = tl;
    ra.kind = J.kind;
    ra.blk_bytes = c.blk_bytes;
    ra.blk_off = c.blk_off;
    ra.words = d_words;
    // 3. parse + 4. lookups
    if (J.kind == K_ANNO) {
        AnnoArgs aa{J.chr->t, J.ids->t, c.cs, c.ce, J.idx_id, J.idx_range, J.header ? 1u : 0u};
        int32_t *d_cl = reinterpret_cast<int32_t *>(c.cg), *d_ch = reinterpret_cast<int32_t *>(c.cnt);
        float *d_prop = reinterpret_cast<float *>(c.fend);
        hipLaunchKernelGGL(text_parse_anno_kernel, dim3(nbr), dim3(256), 0, st, tl, aa, c.grp, d_cl, d_ch,
                           reinterpret_cast<int32_t *>(c.qs), reinterpret_cast<int32_t *>(c.qe), c.keep, d_words);
        launch_span_cover(J.sp, c.grp, d_cl, d_ch, reinterpret_cast<const int32_t *>(c.qs),
                          reinterpret_cast<const int32_t *>(c.qe), L, d_prop, st);
        ra.keep = c.keep;
        ra.grp = c.grp;
        ra.qs = reinterpret_cast<const int32_t *>(c.qs);
        ra.qe = reinterpret_cast<const int32_t *>(c.qe);
        ra.prop = d_prop;
        ra.prefix = c.prefix;
        ra.prefix_len = (uint32_t)prefix_len;
        ra.header = J.header ? 1u : 0u;
    } else {
        hipLaunchKernelGGL(text_parse_rg_kernel, dim3(nbr), dim3(256), 0, st, tl, J.chr->t, c.grp, c.qs, c.qe, c.fend);
        launch_interval_locate(J.ctg_ix, c.grp, c.qs, c.qe, L, c.hit, st);
        if (J.kind == K_COUNT) {
            hipLaunchKernelGGL(text_rg_group_kernel, dim3(nbr), dim3(256), 0, st, L, c.hit, c.rgg, c.cg, d_words);
            launch_interval_count(J.rg_ix, c.cg, c.qs, c.qe, L, reinterpret_cast<int32_t *>(c.cnt), st);
        }
        ra.fend = c.fend;
        ra.hit = c.hit;
        ra.ids = J.kind == K_LOCATE ? J.ids->t : NameTab{};
        ra.cnt = reinterpret_cast<const int32_t *>(c.cnt);
    }
    // 5. row lengths and their offsets
    hipLaunchKernelGGL(text_row_len_kernel, dim3(nbr), dim3(256), 0, st, ra);
    hipLaunchKernelGGL(blk_offsets_scan_kernel<unsigned long long>, dim3(1), dim3(1024), 0, st, c.blk_bytes, nbr, c.blk_off, d_words,
                       (uint32_t)W_BYTES);
    GAMS_TRY(h, who, read_words(h, d_words));
    const unsigned long long *w = h->pin_scratch;
    if (w[W_EFIELD]) return gams_fail(h, GAMS_EINVAL, who + ": field index out of range (the reference panics, anno.rs:115)");
    if (w[W_EID])
        return gams_fail(h, GAMS_EINVAL, who + ": a ctg id not in ctg_ids on a chromosome of the set (the reference "
                                               "panics, redis.rs:133-134)");
    if (w[W_UNSUP])
        return gams_fail(h, GAMS_EUNSUPPORTED,
                         who + (J.kind == K_COUNT ? ": a located ctg has no rg group (use the host path)"
                                                  : ": a prop that is not a finite value in [0, 1] (use the host path)"));
    const uint64_t tb = w[W_BYTES], rows = w[W_ROWS];
    // the text: device buffer from the pool, read back into the entry's page-locked buffer
    char *&out = T->out[J.kind];
    size_t &out_cap = T->out_cap[J.kind];
    GAMS_TRY(h, who, gams_pool_grow(h, true, &out, &out_cap, std::max<uint64_t>(tb, 1), std::max<uint64_t>(tb, 1)));
    if (tb) {
        PoolBlock d_text(h, false);
        GAMS_TRY(h, who, d_text.alloc(tb));
        ra.text = reinterpret_cast<char *>(d_text.p);
        hipLaunchKernelGGL(text_row_write_kernel, dim3(nbr), dim3(256), 0, st, ra);
        GAMS_TRY(h, who, hipGetLastError());
        GAMS_TRY(h, who, hipMemcpyAsync(out, d_text.p, tb, hipMemcpyDeviceToHost, st));
        GAMS_TRY(h, who, hipEventRecord(h->k1, st));
        GAMS_TRY(h, who, hipStreamSynchronize(st));
    } else {
        GAMS_TRY(h, who, hipEventRecord(h->k1, st));
        GAMS_TRY(h, who, hipStreamSynchronize(st));
    }
    h->k_valid = true;
    *text = out;
    *text_bytes = tb;
    *n_rows = rows;
    return GAMS_OK;
}


// ---- read_range on the device (utils.rs:39-67): the bytes of a .rg file -> the ranges bucketed per ctg ----------
// Stages behind the line index (one lane per line unless said otherwise):
//   parse    the WHOLE line through Range::from_str (no cut at a tab) -> (chromosome group, start, end);
//   locate   interval_locate_kernel on those columns -> the ctg of every line (its interval of ctg_ix), or -1;
//   first    first[c] = the smallest line number located to ctg c: the line `.or_default()` swallows;
//   keep     keep = located and not first[c]; count[c] = kept lines of c; the sort key (c, line) of every line
//            (the peak entry puts the range's start between the two: (c, start, line));
//   offsets  exclusive scan of count -> bucket_off;
//   order    ONE radix sort of the 64-bit keys (c << line bits | line); dropped lines carry c = n_ctg and sort
//            behind every bucket.  The keys are unique, so the order is (ctg, line) whatever order lanes ran in;
//   gather   start / end (or the index builder's [start, end + 1) columns) through the sorted line numbers.
// first and keep issue one atomic per run of equal ctgs inside a wavefront: lanes are in line order, a range file is
// sorted by position, so a wavefront usually holds one run and its leader's line is the run's smallest.  The atomics
// are integer min and add: their result does not depend on arrival order.

// the ctg of lane - 1 (lane 0: none), for the run leaders: a lane leads when its predecessor's ctg differs
__device__ __forceinline__ bool run_leader(int64_t c) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t plo = __shfl_up((uint32_t)c, 1, 64), phi = __shfl_up((uint32_t)((uint64_t)c >> 32), 1, 64);
    const int64_t prev = (int64_t)(((uint64_t)phi << 32) | plo);
    return lane == 0u || prev != c;
}

__global__ __launch_bounds__(256) void rg_parse_kernel(const TextLines t, const NameTab chr, uint32_t *grp, uint32_t *qs,
                                                       uint32_t *qe) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= t.n_lines) return;
    uint64_t b, e;
    line_of(t, i, b, e);
    const RangeField r = parse_range(t.in, b, e);          // utils.rs:50: the line, not its first field
    grp[i] = r.ok ? name_find(chr, t.in + r.cb, r.ce - r.cb) : UINT32_MAX;
    qs[i] = r.start;
    qe[i] = r.end;
}

// ---- several files in one load (rg.rs:40, feature.rs:47: one read_range per file) ----
// The files lie back to back in the input buffer (TextFront::files), every file beginning at a line start, so the line
// numbers of the buffer rise with (file, line).  line0[f] = the first line of file f (n_files + 1 entries, the last one
// the line count): the position of the file's first byte among the line starts.  A line's file is the last one whose first
// line is not behind it (an empty file shares its first line with the next one and is never that).  Drop-first is per
// file: first[] is keyed by file * n_ctg + ctg, and a run of equal ctgs ends where the file changes.  The bucket a kept
// line is counted and sorted into is (file, ctg) for the records and the ctg alone for the index.
struct RgFileTab {
    const uint32_t *line0;
    uint32_t n_files, n_ctg;
};

__global__ __launch_bounds__(256) void rg_file_lines_kernel(const unsigned long long *starts, uint64_t nl,
                                                            const unsigned long long *file_off, uint32_t n_files, uint32_t *line0) {
    const uint32_t f = blockIdx.x * 256u + threadIdx.x;
    if (f > n_files) return;
    const unsigned long long at = file_off[f];
    uint64_t lo = 0, hi = nl + 2u;                    // lower bound over starts[0, nl + 2); starts[nl + 1] = n + 1 > at
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (starts[mid] < at)
            lo = mid + 1u;
        else
            hi = mid;
    }
    line0[f] = (uint32_t)lo;
}

__device__ __forceinline__ uint32_t rg_file_of(const RgFileTab &F, uint32_t i) {
    uint32_t lo = 0, hi = F.n_files;                  // line0[0] = 0 <= i
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (F.line0[mid] <= i)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

// The run key of line i, located to ctg c (-1: not located): what first[] is indexed by and where a run of equal lanes
// ends.  A load of one file (kFiles false) searches no file and reads nothing of F: the key is the ctg.
template <bool kFiles>
__device__ __forceinline__ int64_t rg_run_key(const RgFileTab &F, uint32_t i, int64_t c) {
    if constexpr (kFiles)
        return c >= 0 ? (int64_t)rg_file_of(F, i) * F.n_ctg + c : -1;
    else
        return c;
}

template <bool kFiles>
__global__ __launch_bounds__(256) void rg_first_kernel(uint32_t n_lines, const int64_t *hit, const RgFileTab F, uint32_t *first) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const int64_t b = rg_run_key<kFiles>(F, i, i < n_lines ? hit[i] : -1);
    if (run_leader(b) && b >= 0) atomicMin(first + b, i);
}

// by_file (several files): count[] and the key's bucket are by (file, ctg) like the runs, else by ctg.  qs (one file): the
// start of a kept line goes between bucket and line, mid_bits wide; the rg loader passes none.
template <bool kFiles>
__global__ __launch_bounds__(256) void rg_keep_kernel(uint32_t n_lines, uint32_t n_bkt, uint32_t line_bits, const int64_t *hit,
                                                      const RgFileTab F, uint32_t by_file, const uint32_t *first, uint32_t *count,
                                                      unsigned long long *key, const uint32_t *qs, uint32_t mid_bits) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    const int64_t c = i < n_lines ? hit[i] : -1;
    const int64_t b = rg_run_key<kFiles>(F, i, c);
    const bool keep = b >= 0 && first[b] != i;
    const bool lead = run_leader(b);
    const unsigned long long kept = __ballot(keep), leads = __ballot(lead);
    const uint32_t bucket = kFiles && by_file ? (uint32_t)b : (uint32_t)c;
    if (lead && b >= 0) {
        // the run is [lane, next leader): its kept lines, one add
        const unsigned long long above = lane == 63u ? 0ull : leads & (~0ull << (lane + 1u));
        const uint32_t end = above ? (uint32_t)__builtin_ctzll(above) : 64u;
        const unsigned long long run = (end == 64u ? ~0ull : (1ull << end) - 1ull) & (~0ull << lane);
        const uint32_t n = (uint32_t)__popcll(kept & run);
        if (n) atomicAdd(count + bucket, n);
    }
    const uint32_t mid = kFiles ? 0u : mid_bits;
    if (i < n_lines)
        key[i] = ((unsigned long long)(keep ? bucket : n_bkt) << (mid + line_bits)) |
                 ((unsigned long long)(!kFiles && qs && keep ? qs[i] : 0u) << line_bits) | i;
}

// The kept lines of a load in key order, as the loader hands them to its consumer's kernels.  A key is taken apart here
// and nowhere else.
struct RgKept {
    const unsigned long long *key;          // sorted: the first n_kept are the kept lines in (bucket[, start], line) order
    uint16_t line_bits, mid_bits;           // the key: bucket << (mid_bits + line_bits) | start << line_bits | line
    uint32_t n_kept;
    const uint32_t *qs, *qe;                // per line
    const unsigned long long *bucket_off;   // device, one per bucket and the end
    __device__ __forceinline__ uint32_t line(uint32_t k) const { return (uint32_t)(key[k] & ((1ull << line_bits) - 1ull)); }
    __device__ __forceinline__ uint32_t bucket(uint32_t k) const { return (uint32_t)(key[k] >> (mid_bits + line_bits)); }
};

struct RgGather {
    RgKept v;
    uint32_t *start, *end, *line;        // end = the range's end + end_plus; line may be NULL
    uint32_t end_plus;
    uint32_t *off32;                     // not NULL: v.bucket_off, n_off of them, narrowed for the index builder
    uint64_t n_off;
};

__global__ __launch_bounds__(256) void rg_gather_kernel(const RgGather a) {
    const uint64_t k = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (k < a.v.n_kept) {
        const uint32_t i = a.v.line((uint32_t)k);
        a.start[k] = a.v.qs[i];
        a.end[k] = a.v.qe[i] + a.end_plus;
        if (a.line) a.line[k] = i;
    }
    if (a.off32 && k < a.n_off) a.off32[k] = (uint32_t)a.v.bucket_off[k];
}

// what the loader hands its consumer while the scratch is alive
struct RgCols {
    uint64_t n_ctg, n_kept;
    // a load of one file: one bucket and one entry of first[] per ctg.  Of several files (RgInput::files): first[] has one
    // entry per (file, ctg), file-major, and the buckets are the (file, ctg) pairs or the ctgs (RgInput::by_file)
    uint64_t n_files, n_bkt, n_first;
    const unsigned long long *bucket_off;   // host, n_bkt + 1
    const uint32_t *first;                  // host, n_first: UINT32_MAX = no located line
    bool seen(uint64_t ctg) const {         // a located line in any file
        for (uint64_t f = 0; f < n_files; ++f)
            if (first[f * n_ctg + ctg] != UINT32_MAX) return true;
        return false;
    }
    RgKept v;                               // the kept lines on the device; n_kept == 0: nothing there, all zero
    TextLines t;                            // the line index (device), with lines
    unsigned long long *words;              // device: the W_* words of the call
    bool ran;                               // the input had lines: the stages up to RG_OFFSETS (with `order` RG_ORDER) were queued and timed
};

enum : int { RG_LINES = 0, RG_PARSE, RG_LOCATE, RG_FIRST, RG_KEEP, RG_OFFSETS, RG_ORDER, RG_GATHER, RG_BUILD, RG_STAGES };

// What the range entries ask of the loader: the whole line is the range, nothing else is kept of it, key (ctg, line).
// A caller's own spec (PeakLoad, below) has the same members:
//   mid_bits  31: the start of a kept line is the key's middle field, (ctg, start, line); 0: none
//   efield    the message for a line its parse kernel flags W_EFIELD: the words are read back with the offsets and
//             the call is refused there, in front of every later check (nullptr: no such flag, no read-back)
//   cols      its per-line columns, carved behind key' in the loader's pooled block
//   parse     launches its parse kernel, which fills grp / qs / qe (and its columns) for every line
struct RgPlain {
    NameTab chr;
    static constexpr uint32_t mid_bits = 0;
    static constexpr const char *efield = nullptr;
    void cols(Carver &, uint32_t) {}
    void parse(const TextLines &tl, uint32_t *grp, uint32_t *qs, uint32_t *qe, unsigned long long *, uint32_t nbr, hipStream_t st) const {
        hipLaunchKernelGGL(rg_parse_kernel, dim3(nbr), dim3(256), 0, st, tl, chr, grp, qs, qe);
    }
};

// The input of a load: the bytes of one file, or `files` (then bytes / n_bytes are not looked at).  One file given as
// `files` is loaded exactly as the bytes of one file are, and no file as zero bytes.  Several files are loaded as the
// reference loads them one after another (RgFileTab, above): by_file says what the buckets are.  Refused beyond
// kRgMaxFileCtg (file, ctg) pairs, the size of the tables by them.
struct RgInput {
    const char *bytes;
    uint64_t n_bytes;
    const TextFiles *files;
    bool by_file;
};
constexpr uint64_t kRgMaxFileCtg = 1ull << 24;

// Runs the stages up to the sort (`order` false: up to the offsets, for a size query) as `spec` shapes them and calls
// consume(cols, stage) -- stage(k, open) records the stopwatch event that opens or closes stage k -- which queues the
// gather and whatever follows.  One host wait of its own besides text_front's, behind the offsets.  `who` names the entry
// in error messages.
template <typename Spec, typename Consume>
int rg_load(gams_gpu_t *h, const std::string &who, const gams_index_t *ctg_ix, Spec &&spec, RgInput in, bool order,
            Consume consume) {
    if (in.files && in.files->n <= 1u) {
        in.bytes = in.files->n ? in.files->bytes[0] : nullptr;
        in.n_bytes = in.files->n ? in.files->n_bytes[0] : 0;
        in.files = nullptr;
    }
    const bool multi = in.files != nullptr;
    const uint64_t n_files = multi ? in.files->n : 1;
    if (multi && spec.mid_bits) return gams_fail(h, GAMS_EINVAL, who + ": several files with a middle key field");
    if (multi && n_files * ctg_ix->m > kRgMaxFileCtg)
        return gams_fail(h, GAMS_EUNSUPPORTED, who + ": more than 2^24 (file, ctg) pairs (use the host path)");
    GAMS_HIP(h, hipSetDevice(h->device));
    GAMS_HIP(h, gams_stopwatch_reserve(h, RG_STAGES));
    hipStream_t st = h->compute;
    const StageClock stage{h, st};
    PoolBlock s1(h, false);
    TextFront F(h);
    F.files = in.files;
    GAMS_TRY(h, who, stage(RG_LINES, true));
    const int rc_front = text_front(h, who, in.bytes, in.n_bytes, F);
    if (rc_front != GAMS_OK) return rc_front;
    const uint64_t n_ctg = ctg_ix->m, n_first = n_files * n_ctg, n_bkt = multi && in.by_file ? n_first : n_ctg;
    const uint32_t L = F.L;
    // the host's copy of bucket_off and first: page-locked, from the pool (a copy into the block may still be queued
    // when a step fails: the block waits for the stream like the others)
    PoolBlock pin(h, true);
    unsigned long long *h_off = nullptr, *h_foff = nullptr;
    uint32_t *h_first = nullptr;
    auto host_cols = [&](Carver &c) {
        h_off = c.take<unsigned long long>(n_bkt + 1);
        h_foff = c.take<unsigned long long>(multi ? n_files + 1 : 0);
        h_first = c.take_tight<uint32_t>(std::max<uint64_t>(n_first, 1));
    };
    GAMS_TRY(h, who, pin.alloc(layout_bytes(host_cols)));
    carve(pin.p, host_cols);
    RgCols C{};
    C.n_ctg = n_ctg;
    C.n_files = n_files;
    C.n_bkt = n_bkt;
    C.n_first = n_first;
    C.bucket_off = h_off;
    C.first = h_first;
    if (L == 0) {
        memset(h_off, 0, (n_bkt + 1) * 8);
        memset(h_first, 0xff, n_first * 4);
        GAMS_TRY(h, who, stage(RG_LINES, false));
        return consume(C, stage);
    }
    uint32_t line_bits = 1, ctg_bits = 1;
    while (line_bits < 32u && (L - 1u) >> line_bits) ++line_bits;
    while (ctg_bits < 32u && n_bkt >> ctg_bits) ++ctg_bits;
    const uint32_t key_bits = ctg_bits + spec.mid_bits + line_bits;      // (at most 64 without a middle field)
    if (key_bits > 64u)
        return gams_fail(h, GAMS_EUNSUPPORTED, who + ": (ctg, start, line) does not fit a 64-bit sort key (use the host path)");
    const uint32_t nbr = (L + 255u) / 256u;
    size_t sort_bytes = 0;
    GAMS_TRY(h, who, rocprim::radix_sort_keys(nullptr, sort_bytes, (unsigned long long *)nullptr, (unsigned long long *)nullptr,
                                              (size_t)L, 0u, key_bits, st));
    const size_t n_tab = std::max<uint64_t>(n_bkt, 1), n_ftab = std::max<uint64_t>(n_first, 1);
    unsigned long long *d_starts = nullptr, *d_key = nullptr, *d_key2 = nullptr, *d_off = nullptr, *d_foff = nullptr;
    uint32_t *d_grp = nullptr, *d_qs = nullptr, *d_qe = nullptr, *d_first = nullptr, *d_count = nullptr, *d_line0 = nullptr;
    int64_t *d_hit = nullptr;
    uint8_t *d_sort = nullptr;
    auto cols = [&](Carver &c) {   // starts | grp qs qe | hit key key' | the spec's | first count | bucket_off | sort storage
        d_starts = c.take<unsigned long long>((size_t)F.nl + 2);
        d_grp = c.take<uint32_t>(L);
        d_qs = c.take<uint32_t>(L);
        d_qe = c.take<uint32_t>(L);
        d_hit = c.take<int64_t>(L);
        d_key = c.take<unsigned long long>(L);
        d_key2 = c.take<unsigned long long>(L);
        spec.cols(c, L);
        d_first = c.take<uint32_t>(n_ftab);
        d_count = c.take<uint32_t>(n_tab);
        d_off = c.take<unsigned long long>(n_bkt + 1);
        d_sort = c.take<uint8_t>(std::max<size_t>(sort_bytes, 1));
        d_foff = c.take<unsigned long long>(multi ? n_files + 1 : 0);       // (several files: where they begin, their first lines)
        d_line0 = c.take<uint32_t>(multi ? n_files + 1 : 0);
    };
    GAMS_TRY(h, who, s1.alloc(layout_bytes(cols)));
    carve(s1.p, cols);
    hipLaunchKernelGGL(text_line_start_kernel, dim3(F.nbi), dim3(256), 0, st, h->text->d_in, F.n_in, F.n16, F.d_bnloff, F.nl,
                       d_starts);
    GAMS_TRY(h, who, hipMemsetAsync(d_first, 0xff, gams_align256(n_ftab * 4), st));
    GAMS_TRY(h, who, hipMemsetAsync(d_count, 0, gams_align256(n_tab * 4), st));
    const RgFileTab ftab{d_line0, (uint32_t)n_files, (uint32_t)n_ctg};
    if (multi) {
        memcpy(h_foff, F.file_off.data(), (n_files + 1) * 8);
        GAMS_TRY(h, who, hipMemcpyAsync(d_foff, h_foff, (n_files + 1) * 8, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(rg_file_lines_kernel, dim3((unsigned)(n_files / 256 + 1)), dim3(256), 0, st, d_starts, F.nl, d_foff,
                           (uint32_t)n_files, d_line0);
    }
    GAMS_TRY(h, who, stage(RG_LINES, false));
    C.t = TextLines{reinterpret_cast<const char *>(h->text->d_in), d_starts, F.nl, L};
    C.words = F.d_words;
    GAMS_TRY(h, who, stage(RG_PARSE, true));
    spec.parse(C.t, d_grp, d_qs, d_qe, F.d_words, nbr, st);
    GAMS_TRY(h, who, stage(RG_PARSE, false));
    GAMS_TRY(h, who, stage(RG_LOCATE, true));
    launch_interval_locate(ctg_ix, d_grp, d_qs, d_qe, L, d_hit, st);
    GAMS_TRY(h, who, stage(RG_LOCATE, false));
    GAMS_TRY(h, who, stage(RG_FIRST, true));
    hipLaunchKernelGGL(multi ? rg_first_kernel<true> : rg_first_kernel<false>, dim3(nbr), dim3(256), 0, st, L, d_hit, ftab, d_first);
    GAMS_TRY(h, who, stage(RG_FIRST, false));
    GAMS_TRY(h, who, stage(RG_KEEP, true));
    hipLaunchKernelGGL(multi ? rg_keep_kernel<true> : rg_keep_kernel<false>, dim3(nbr), dim3(256), 0, st, L, (uint32_t)n_bkt,
                       line_bits, d_hit, ftab, in.by_file ? 1u : 0u, d_first, d_count, d_key,
                       spec.mid_bits ? (const uint32_t *)d_qs : (const uint32_t *)nullptr, (uint32_t)spec.mid_bits);
    GAMS_TRY(h, who, stage(RG_KEEP, false));
    GAMS_TRY(h, who, stage(RG_OFFSETS, true));
    hipLaunchKernelGGL(blk_offsets_scan_kernel<uint32_t>, dim3(1), dim3(1024), 0, st, d_count, (uint32_t)n_bkt, d_off, F.d_words,
                       (uint32_t)W_ROWS);
    GAMS_TRY(h, who, stage(RG_OFFSETS, false));
    GAMS_TRY(h, who, hipGetLastError());
    GAMS_TRY(h, who, hipMemcpyAsync(h_off, d_off, (n_bkt + 1) * 8, hipMemcpyDeviceToHost, st));
    if (n_first) GAMS_TRY(h, who, hipMemcpyAsync(h_first, d_first, n_first * 4, hipMemcpyDeviceToHost, st));
    if (spec.efield) GAMS_TRY(h, who, hipMemcpyAsync(h->pin_scratch, F.d_words, W_COUNT * 8, hipMemcpyDeviceToHost, st));
    GAMS_TRY(h, who, hipStreamSynchronize(st));
    if (spec.efield && h->pin_scratch[W_EFIELD]) return gams_fail(h, GAMS_EINVAL, who + spec.efield);
    C.n_kept = h_off[n_bkt];
    if (C.n_kept > 0xfffffff0ull) return gams_fail(h, GAMS_EUNSUPPORTED, who + ": more than 2^32 - 16 kept ranges");
    C.ran = true;
    if (!order) return consume(C, stage);            // a size query: nothing is gathered, so nothing is sorted
    GAMS_TRY(h, who, stage(RG_ORDER, true));
    if (C.n_kept) GAMS_TRY(h, who, rocprim::radix_sort_keys(d_sort, sort_bytes, d_key, d_key2, (size_t)L, 0u, key_bits, st));
    GAMS_TRY(h, who, stage(RG_ORDER, false));
    if (C.n_kept) C.v = RgKept{d_key2, (uint16_t)line_bits, (uint16_t)spec.mid_bits, (uint32_t)C.n_kept, d_qs, d_qe, d_off};
    return consume(C, stage);
}

// slot `slot` of the seqset holds a sequence of the length of a ctg at [chr_start, chr_end] (UINT32_MAX names no slot)
bool seq_slot_holds(const gams_seqset_t *s, uint32_t slot, int32_t chr_start, int32_t chr_end) {
    return slot < s->n_ctg && (int64_t)s->len[slot] == (int64_t)chr_end - chr_start + 1;
}

// the stopwatch of a loader call whose input had lines: stages [0, n) of the handle's timed pairs were recorded (an
// input without lines leaves the stopwatch invalid, as text_front set it)
void rg_timed(gams_gpu_t *h, int n) {
    h->kq_used = n;
    h->kq_staged = true;
    h->k_valid = true;
}


// ---- the keyed row writer: one row per kept line, in key order, and where the rows of every bucket begin --------------
// Behind a consumer's own gather, two stages and two host waits:
//   rows     one lane per kept line k: the row is measured (or refused: nothing is measured, W_UNSUP is set) and its length
//            stored; the sums of the blocks of 256 rows and their prefix; the words are read back, the consumer's refusals
//            end the call here;
//   write    the rows at their offsets -- a block's rows composed in LDS and copied out in 16-B units, or written straight to
//            global memory when they exceed the stage (BlockWriter) -- and, by the lane that opens it, the offset of every
//            bucket's first row.  Never launched after a refusal: every row it writes was measured.
// A consumer describes its rows in a struct D:
//   Args     its kernel arguments, with the kept lines as `v` (RgKept) and this writer's part as `o` (KeyedText<Len>);
//   Len      the type of a row's length;
//   kStage   bytes of the LDS stage;
//   row<kWrite>(a, k, out, bad)   composes row k into a RowOut; bad: a value it has no text for;
//   bucket(a, k)                  the bucket of row k;
//   refused(a, k)                 device: row k cannot be written at all;
//   check(h, who, w)              host: GAMS_OK, or the failure the words w of the rows stage ask for.
template <typename Len>
struct KeyedText {
    Len *row_len;                         // per kept line
    unsigned long long *blk_bytes;        // per workgroup of 256 rows
    unsigned long long *blk_off;
    unsigned long long *text_off;         // per bucket with rows: the offset of its first row
    unsigned long long *words;
    char *text;
    void carve(Carver &c, uint32_t n_kept) {   // row lengths | the blocks' bytes and prefix
        const size_t nbk = (n_kept + 255u) / 256u;
        row_len = c.take<Len>(n_kept);
        blk_bytes = c.take<unsigned long long>(nbk + 1);
        blk_off = c.take<unsigned long long>(nbk + 1);
    }
};

template <typename D>
__global__ __launch_bounds__(256) void keyed_row_len_kernel(const typename D::Args a) {
    __shared__ uint64_t ws[4];
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    bool bad = false;
    RowOut<false, typename D::Len> n;
    if (k < a.v.n_kept) {
        if (D::refused(a, k))
            a.o.words[W_UNSUP] = 1ull;
        else
            D::template row<false>(a, k, n, bad);
        a.o.row_len[k] = n.n;
    }
    if (bad) a.o.words[W_UNSUP] = 1ull;
    uint64_t tot;
    (void)block_excl_scan_256<uint64_t>((uint64_t)n.n, ws, tot);
    if (threadIdx.x == 0) a.o.blk_bytes[blockIdx.x] = tot;
}

template <typename D>
__global__ __launch_bounds__(256) void keyed_row_write_kernel(const typename D::Args a) {
    __shared__ uint64_t ws[4];
    __shared__ __align__(16) char stage[D::kStage + 16];
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    const uint64_t l = k < a.v.n_kept ? a.o.row_len[k] : 0ull;
    BlockWriter<uint64_t> w(l, ws, a.o.blk_off, a.o.text, ~0ull);   // (the text holds all rows: no bound)
    w.stage_if(w.tot <= D::kStage, stage);
    if (k < a.v.n_kept) {
        const uint32_t b = D::bucket(a, k);
        if (k == (uint32_t)a.v.bucket_off[b]) a.o.text_off[b] = w.blk0 + w.rel;
        bool bad = false;                      // (the length pass flagged what has no text: nothing is written then)
        w.put(w.rel, [&](char *p) {
            RowOut<true, typename D::Len> o{p};
            D::template row<true>(a, k, o, bad);
        });
    }
    w.flush();
}

// The same writer behind a stage the launch sizes: a description with stage_bytes(a) instead of kStage gets its stage as
// dynamic LDS, stage_bytes(a) + 16 bytes of it (a static array ends at 64 KB; gfx950 gives a workgroup up to 160 KB).  The
// body is keyed_row_write_kernel's, kept apart so that the kernels of the static descriptions compile as they did.
template <typename D>
__global__ __launch_bounds__(256) void keyed_row_write_dyn_kernel(const typename D::Args a) {
    __shared__ uint64_t ws[4];
    extern __shared__ __align__(16) char dyn_stage[];
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    const uint64_t l = k < a.v.n_kept ? a.o.row_len[k] : 0ull;
    BlockWriter<uint64_t> w(l, ws, a.o.blk_off, a.o.text, ~0ull);
    w.stage_if(w.tot <= D::stage_bytes(a), dyn_stage);
    if (k < a.v.n_kept) {
        const uint32_t b = D::bucket(a, k);
        if (k == (uint32_t)a.v.bucket_off[b]) a.o.text_off[b] = w.blk0 + w.rel;
        bool bad = false;
        w.put(w.rel, [&](char *p) {
            RowOut<true, typename D::Len> o{p};
            D::template row<true>(a, k, o, bad);
        });
    }
    w.flush();
}

template <typename D, typename = void>
struct KeyedDynStage : std::false_type {};
template <typename D>
struct KeyedDynStage<D, std::void_t<decltype(&D::stage_bytes)>> : std::true_type {};

// The two stages, rows_stage and the one behind it, over the arguments `a` the consumer has filled but for o.text; the
// text into the entry's slot, text_off (one per bucket of the load and the end) through the page-locked h_toff.
template <typename D>
int keyed_text_run(gams_gpu_t *h, const std::string &who, const RgCols &C, const StageClock &stage, int rows_stage,
                   typename D::Args &a, TextSlot slot, unsigned long long *h_toff, const char **text, uint64_t *text_bytes,
                   uint64_t *text_off, uint64_t *n_rows) {
    hipStream_t st = h->compute;
    const uint32_t nbk = (a.v.n_kept + 255u) / 256u;
    GAMS_TRY(h, who, stage(rows_stage, true));
    hipLaunchKernelGGL(keyed_row_len_kernel<D>, dim3(nbk), dim3(256), 0, st, a);
    hipLaunchKernelGGL(blk_offsets_scan_kernel<unsigned long long>, dim3(1), dim3(1024), 0, st, a.o.blk_bytes, nbk, a.o.blk_off,
                       a.o.words, (uint32_t)W_BYTES);
    GAMS_TRY(h, who, stage(rows_stage, false));
    GAMS_TRY(h, who, read_words(h, a.o.words));
    const int rc = D::check(h, who, h->pin_scratch);
    if (rc != GAMS_OK) return rc;
    const uint64_t tb = h->pin_scratch[W_BYTES];
    gams_text_state *T = h->text;
    PoolBlock d_text(h, false);
    GAMS_TRY(h, who, gams_pool_grow(h, true, &T->out[slot], &T->out_cap[slot], tb, tb));
    GAMS_TRY(h, who, d_text.alloc(tb));
    a.o.text = reinterpret_cast<char *>(d_text.p);
    if constexpr (KeyedDynStage<D>::value)
        GAMS_TRY(h, who, gams_lds_attr(h, reinterpret_cast<const void *>(keyed_row_write_dyn_kernel<D>), D::stage_bytes(a) + 16u));
    GAMS_TRY(h, who, stage(rows_stage + 1, true));
    if constexpr (KeyedDynStage<D>::value)
        hipLaunchKernelGGL(keyed_row_write_dyn_kernel<D>, dim3(nbk), dim3(256), D::stage_bytes(a) + 16u, st, a);
    else
        hipLaunchKernelGGL(keyed_row_write_kernel<D>, dim3(nbk), dim3(256), 0, st, a);
    GAMS_TRY(h, who, stage(rows_stage + 1, false));
    GAMS_TRY(h, who, hipGetLastError());
    GAMS_TRY(h, who, hipMemcpyAsync(T->out[slot], d_text.p, tb, hipMemcpyDeviceToHost, st));
    GAMS_TRY(h, who, hipMemcpyAsync(h_toff, a.o.text_off, (C.n_bkt + 1) * 8, hipMemcpyDeviceToHost, st));
    GAMS_TRY(h, who, hipStreamSynchronize(st));
    // a bucket without rows begins where the next one does
    text_off[C.n_bkt] = tb;
    for (uint64_t b = C.n_bkt; b-- > 0;) text_off[b] = C.bucket_off[b + 1] > C.bucket_off[b] ? h_toff[b] : text_off[b + 1];
    rg_timed(h, rows_stage + 2);
    *text = T->out[slot];
    *text_bytes = tb;
    *n_rows = C.n_kept;
    return GAMS_OK;
}


// ---- `gams peak` on the device (utils.rs:83-116 read_peak, then peak.rs:41-160): the bytes of a wave TSV -> Peak rows --
// The range loader itself (rg_load with the PeakLoad spec), then a stage of its own and the two of the keyed row writer
// (PeakRows); ten stages in all:
//   lines .. order   the loader's, with these differences:
//     parse    peak_parse_kernel: parts[0] (the line up to its first tab) through Range::from_str; a valid range needs
//              parts[2], the signal (else W_EFIELD: refused at the loader's read-back of the offsets); five more columns
//              per line say where the chromosome, the "name." prefix and the signal lie in the input;
//     keep     the key is (ctg, start, line): utils.rs:109-112 drops the first located line of a ctg, peak.rs:49 sorts
//              the rest by start, stably;
//     order    the line number makes the keys unique and breaks ties on start in file order, which is what the
//              reference's stable sort leaves; a key wider than 64 bits is refused;
//   gc       gather (line, ctg, start, end) through the sorted keys, check every kept peak against its ctg and the ctg
//            for a sequence (flags), then round4(range_gc) of every kept peak (sw.hip);
//   rows     the length of every row (it reads the neighbours' end / start / gc / signal inside the bucket);
//   write    the rows at their offsets and the offset of every ctg's first row.
// Rows come out in key order: grouped by ctg in the caller's order, by start inside a ctg.
struct PeakLines {
    unsigned long long *cb, *sb;      // per line: where the chromosome and the signal field begin
    uint32_t *clen, *slen, *nlen;     // their lengths; nlen: bytes of the "name." prefix at the line's start (0: none)
};

__global__ __launch_bounds__(256) void peak_parse_kernel(const TextLines t, const NameTab chr, uint32_t *grp, uint32_t *qs,
                                                         uint32_t *qe, const PeakLines p, unsigned long long *words) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= t.n_lines) return;
    uint64_t b, e;
    line_of(t, i, b, e);
    const char *s = t.in;
    uint64_t f = b;
    while (f < e && s[f] != '\t') ++f;
    const RangeField r = parse_range(s, b, f);                 // utils.rs:96-99: parts[0]
    uint32_t g = UINT32_MAX;
    uint64_t sb = 0, se = 0;
    if (r.ok) {
        bool third = false;
        if (f < e) {
            uint64_t f2 = f + 1u;
            while (f2 < e && s[f2] != '\t') ++f2;
            if (f2 < e) {
                sb = se = f2 + 1u;
                while (se < e && s[se] != '\t') ++se;
                third = true;
            }
        }
        if (third)
            g = name_find(chr, s + r.cb, r.ce - r.cb);
        else
            words[W_EFIELD] = 1ull;                            // the reference panics (utils.rs:102)
    }
    grp[i] = g;
    qs[i] = r.start;
    qe[i] = r.end;
    p.cb[i] = r.cb;
    p.clen[i] = (uint32_t)(r.ce - r.cb);
    p.nlen[i] = r.ok && r.cb - b >= 2u ? (uint32_t)(r.cb - b) : 0u;   // an empty name prints no prefix (Range::to_string)
    p.sb[i] = sb;
    p.slen[i] = (uint32_t)(se - sb);
}

// what peak asks of the loader (see RgPlain)
struct PeakLoad {
    NameTab chr;
    PeakLines pl;
    static constexpr uint32_t mid_bits = 31;
    static constexpr const char *efield = ": a row has no signal column (the reference panics, utils.rs:102)";
    void cols(Carver &c, uint32_t L) {
        pl.cb = c.take<unsigned long long>(L);
        pl.sb = c.take<unsigned long long>(L);
        pl.clen = c.take<uint32_t>(L);
        pl.slen = c.take<uint32_t>(L);
        pl.nlen = c.take<uint32_t>(L);
    }
    void parse(const TextLines &tl, uint32_t *grp, uint32_t *qs, uint32_t *qe, unsigned long long *words, uint32_t nbr,
               hipStream_t st) const {
        hipLaunchKernelGGL(peak_parse_kernel, dim3(nbr), dim3(256), 0, st, tl, chr, grp, qs, qe, pl, words);
    }
};

struct PeakArgs {
    TextLines t;
    PeakLines p;
    RgKept v;                                 // the kept lines in (ctg, start, line) order
    const int32_t *cs, *ce;                   // per ctg
    const uint32_t *seq_len;                  // per ctg: 0 = no sequence in the seqset
    NameTab ids;
    uint32_t *kline, *kctg, *ks, *ke;         // per kept peak
    float *gc;
    KeyedText<uint32_t> o;
};

__global__ __launch_bounds__(256) void peak_gather_kernel(const PeakArgs a) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= a.v.n_kept) return;
    const uint32_t i = a.v.line(k), c = a.v.bucket(k);
    const uint32_t s = a.v.qs[i], e = a.v.qe[i];
    a.kline[k] = i;
    a.kctg[k] = c;
    a.ks[k] = s;
    a.ke[k] = e;
    // peak_check_inside: the reference slices the ctg's sequence with the range (utils.rs:155)
    if ((int32_t)s < a.cs[c] || (int32_t)e > a.ce[c] || e < s) a.o.words[W_EID] = 1ull;
    if (a.seq_len[c] == 0u) a.o.words[W_ENOSEQ] = 1ull;
}

// peak.rs:65-158 for kept peak k, as gams_host_peak prints it
template <bool kWrite>
__device__ void peak_row(const PeakArgs &a, uint32_t k, RowOut<kWrite> &o, bool &bad) {
    const uint32_t c = a.kctg[k];
    const uint32_t o0 = (uint32_t)a.v.bucket_off[c], o1 = (uint32_t)a.v.bucket_off[c + 1u];
    const bool has_prev = k > o0, has_next = k + 1u < o1;
    const uint32_t i = a.kline[k], ip = has_prev ? a.kline[k - 1u] : i, in = has_next ? a.kline[k + 1u] : i;
    const uint32_t s = a.ks[k], e = a.ke[k];
    const float g = a.gc[k], gp = has_prev ? a.gc[k - 1u] : g, gn = has_next ? a.gc[k + 1u] : g;
    const uint32_t prev_end = has_prev ? a.ke[k - 1u] : (uint32_t)a.cs[c];           // peak.rs:112-133
    const uint32_t next_start = has_next ? a.ks[k + 1u] : (uint32_t)a.ce[c];         // peak.rs:135-157
    const char *in_ = a.t.in;
    o.bytes("peak:", 5u);
    const unsigned long long io = a.ids.off[c];
    o.bytes(a.ids.bytes + io, (uint32_t)(a.ids.off[c + 1u] - io));
    o.ch(':');
    o.dec(k - o0 + 1u);
    o.ch('\t');
    o.bytes(in_ + a.t.starts[i], a.p.nlen[i]);                 // Range::to_string() with the strand cleared
    o.bytes(in_ + a.p.cb[i], a.p.clen[i]);
    o.ch(':');
    o.dec(s);
    if (e != s) {
        o.ch('-');
        o.dec(e);
    }
    o.ch('\t');
    o.i32((int32_t)(e - s + 1u));
    o.ch('\t');
    o.f4(g, bad);
    o.ch('\t');
    o.bytes(in_ + a.p.sb[i], a.p.slen[i]);
    o.ch('\t');
    o.i32((int32_t)(s - prev_end + 1u));
    o.ch('\t');
    o.f32s(fabsf(g - gp), bad);
    o.ch('\t');
    o.bytes(in_ + a.p.sb[ip], a.p.slen[ip]);
    o.ch('\t');
    o.i32((int32_t)(next_start - e + 1u));
    o.ch('\t');
    o.f32s(fabsf(g - gn), bad);
    o.ch('\t');
    o.bytes(in_ + a.p.sb[in], a.p.slen[in]);
    o.ch('\n');
}

// bytes of a block's rows staged in LDS: 256 rows of ~90 B are 23 KB; a block beyond the stage (long names, ids or
// signals) writes its rows to global memory directly
constexpr uint32_t kPeakStage = 32768;

// the Peak rows for the keyed row writer: every kept peak has a row
struct PeakRows {
    using Args = PeakArgs;
    using Len = uint32_t;
    static constexpr uint32_t kStage = kPeakStage;
    template <bool kWrite>
    static __device__ __forceinline__ void row(const Args &a, uint32_t k, RowOut<kWrite> &o, bool &bad) { peak_row(a, k, o, bad); }
    static __device__ __forceinline__ uint32_t bucket(const Args &a, uint32_t k) { return a.kctg[k]; }
    static __device__ __forceinline__ bool refused(const Args &, uint32_t) { return false; }
    static int check(gams_gpu_t *h, const std::string &who, const unsigned long long *w) {
        if (w[W_EID])
            return gams_fail(h, GAMS_EINVAL, who + ": a peak is not inside its ctg (the reference panics on the slice, utils.rs:155)");
        if (w[W_ENOSEQ]) return gams_fail(h, GAMS_EINVAL, who + ": a ctg with peaks has no sequence in the seqset");
        if (w[W_UNSUP])
            return gams_fail(h, GAMS_EUNSUPPORTED, who + ": a gc or an amplitude the device formatters do not cover (use the host path)");
        return GAMS_OK;
    }
};

// ---- the records `gams peak` stores (peak.rs:68-78,163-171: SET peak:{ctg_id}:{serial} serde_json(Peak)) as text --------
// The stages of gams_gpu_peak_text up to the gc, then the keyed row writer over a second description of the same eleven
// fields: the serial continues cnt:peak:{ctg} (sbase, the host's: one file, so a bucket is a ctg), the row is the TSV row,
// "{id}\t{json}\n" or the RESP SET command (the formats of the rg / feature records, rec_row), and a block's rows are
// staged in LDS the launch sizes.  The JSON is data.rs:30-43 in serde's field order, without spaces.
struct PeakRecArgs {
    PeakArgs pk;                              // what peak_gather_kernel and the gc fill (of its `o` only the words are used)
    RgKept v;                                 // pk.v, where the keyed row writer looks for it
    const uint32_t *sbase;                    // per ctg: cnt:peak:{ctg} before the load
    int format;
    uint32_t stage;                           // bytes of the LDS stage of this launch
    KeyedText<unsigned long long> o;
};

// a name prefix or a signal of this many bytes is refused (RECORDS, RESP): a row's lengths stay below 2^32
constexpr uint32_t kPeakRecMaxField = 1u << 30;

// the fields of kept peak k (peak.rs:65-158, as peak_row takes them) and its serial
struct PeakRec {
    uint32_t c, serial, i, ip, in, s, e;      // ctg; the lines of the peak and of its neighbours (its own at a ctg's ends)
    float g, la, ra;
    int32_t lw, rw;
};

__device__ __forceinline__ PeakRec peak_rec(const PeakRecArgs &A, uint32_t k) {
    const PeakArgs &a = A.pk;
    PeakRec r;
    r.c = a.kctg[k];
    const uint32_t o0 = (uint32_t)a.v.bucket_off[r.c], o1 = (uint32_t)a.v.bucket_off[r.c + 1u];
    const bool has_prev = k > o0, has_next = k + 1u < o1;
    r.serial = A.sbase[r.c] + (k - o0) + 1u;                                          // peak.rs:71-77
    r.i = a.kline[k];
    r.ip = has_prev ? a.kline[k - 1u] : r.i;
    r.in = has_next ? a.kline[k + 1u] : r.i;
    r.s = a.ks[k];
    r.e = a.ke[k];
    r.g = a.gc[k];
    r.la = fabsf(r.g - (has_prev ? a.gc[k - 1u] : r.g));
    r.ra = fabsf(r.g - (has_next ? a.gc[k + 1u] : r.g));
    r.lw = (int32_t)(r.s - (has_prev ? a.ke[k - 1u] : (uint32_t)a.cs[r.c]) + 1u);     // peak.rs:112-133
    r.rw = (int32_t)((has_next ? a.ks[k + 1u] : (uint32_t)a.ce[r.c]) - r.e + 1u);     // peak.rs:135-157
    return r;
}

template <typename Out, size_t N>
__device__ __forceinline__ void put_lit(Out &o, const char (&s)[N]) { o.bytes(s, (uint64_t)(N - 1)); }

// a length below 10^18 in decimal (four fields of up to 2^30 bytes, every byte escaped, pass 2^32)
__device__ __forceinline__ uint32_t u64_digits(uint64_t v) {
    return v < 1000000000ull ? dec_digits((uint32_t)v) : 9u + dec_digits((uint32_t)(v / 1000000000ull));
}
template <typename Out>
__device__ __forceinline__ void put_u64(Out &o, uint64_t v) {
    if (v < 1000000000ull) {
        o.dec((uint32_t)v);
        return;
    }
    o.dec((uint32_t)(v / 1000000000ull));
    const uint32_t lo = (uint32_t)(v % 1000000000ull);
    for (uint32_t p = 100000000u; p; p /= 10u) o.ch((char)('0' + lo / p % 10u));
}

// "peak:{ctg_id}:{serial}"; json: inside a JSON string
template <bool kWrite>
__device__ __forceinline__ void peak_rec_id(const PeakRecArgs &A, const PeakRec &r, RowOut<kWrite, uint64_t> &o, bool json) {
    put_lit(o, "peak:");
    const unsigned long long io = A.pk.ids.off[r.c], il = A.pk.ids.off[r.c + 1u] - io;
    if (json)
        o.esc(A.pk.ids.bytes + io, il);
    else
        o.bytes(A.pk.ids.bytes + io, il);
    o.ch(':');
    o.dec(r.serial);
}

// Range::to_string() with the strand cleared, as peak_row reprints it
template <bool kWrite>
__device__ __forceinline__ void peak_rec_range(const PeakRecArgs &A, const PeakRec &r, RowOut<kWrite, uint64_t> &o, bool json) {
    const PeakArgs &a = A.pk;
    if (json)
        o.esc(a.t.in + a.t.starts[r.i], (uint64_t)a.p.nlen[r.i]);
    else
        o.bytes(a.t.in + a.t.starts[r.i], (uint64_t)a.p.nlen[r.i]);
    o.bytes(a.t.in + a.p.cb[r.i], (uint64_t)a.p.clen[r.i]);
    o.ch(':');
    o.dec(r.s);
    if (r.e != r.s) {
        o.ch('-');
        o.dec(r.e);
    }
}

// the signal of line i
template <bool kWrite>
__device__ __forceinline__ void peak_rec_signal(const PeakRecArgs &A, uint32_t i, RowOut<kWrite, uint64_t> &o, bool json) {
    if (json)
        o.esc(A.pk.t.in + A.pk.p.sb[i], (uint64_t)A.pk.p.slen[i]);
    else
        o.bytes(A.pk.t.in + A.pk.p.sb[i], (uint64_t)A.pk.p.slen[i]);
}

template <bool kWrite>
__device__ __forceinline__ void peak_rec_json(const PeakRecArgs &A, const PeakRec &r, RowOut<kWrite, uint64_t> &o, bool &bad) {
    put_lit(o, "{\"id\":\"");
    peak_rec_id(A, r, o, true);
    put_lit(o, "\",\"range\":\"");
    peak_rec_range(A, r, o, true);
    put_lit(o, "\",\"length\":");
    o.i32((int32_t)(r.e - r.s + 1u));
    put_lit(o, ",\"gc\":");
    o.f4j(r.g, bad);
    put_lit(o, ",\"signal\":\"");
    peak_rec_signal(A, r.i, o, true);
    put_lit(o, "\",\"left_wave_length\":");
    o.i32(r.lw);
    put_lit(o, ",\"left_amplitude\":");
    o.f32j(r.la, bad);
    put_lit(o, ",\"left_signal\":\"");
    peak_rec_signal(A, r.ip, o, true);
    put_lit(o, "\",\"right_wave_length\":");
    o.i32(r.rw);
    put_lit(o, ",\"right_amplitude\":");
    o.f32j(r.ra, bad);
    put_lit(o, ",\"right_signal\":\"");
    peak_rec_signal(A, r.in, o, true);
    put_lit(o, "\"}");
}

template <bool kWrite>
__device__ void peak_rec_row(const PeakRecArgs &A, uint32_t k, RowOut<kWrite, uint64_t> &o, bool &bad) {
    const PeakRec r = peak_rec(A, k);
    if (A.format == GAMS_LOADER_TSV) {                         // the row of peak_row but for the serial
        peak_rec_id(A, r, o, false);
        o.ch('\t');
        peak_rec_range(A, r, o, false);
        o.ch('\t');
        o.i32((int32_t)(r.e - r.s + 1u));
        o.ch('\t');
        o.f4(r.g, bad);
        o.ch('\t');
        peak_rec_signal(A, r.i, o, false);
        o.ch('\t');
        o.i32(r.lw);
        o.ch('\t');
        o.f32s(r.la, bad);
        o.ch('\t');
        peak_rec_signal(A, r.ip, o, false);
        o.ch('\t');
        o.i32(r.rw);
        o.ch('\t');
        o.f32s(r.ra, bad);
        o.ch('\t');
        peak_rec_signal(A, r.in, o, false);
        o.ch('\n');
    } else if (A.format == GAMS_LOADER_RESP) {                 // wire::resp_command({"SET", id, json})
        // The two lengths go in front of what they count.  The length pass measures the JSON with a counting RowOut (three
        // floats formatted, every string scanned for escapes); the write pass takes it from the row's stored length instead,
        // which is 23 + li + digits(li) + lj + digits(lj): x + digits(x) grows with x, so one lj fits.
        RowOut<false, uint64_t> li, lj;
        peak_rec_id(A, r, li, false);
        if constexpr (kWrite) {
            const uint64_t t = A.o.row_len[k] - 23u - li.n - u64_digits(li.n);
            uint32_t d = 1u;
            while (d < 19u && u64_digits(t - d) != d) ++d;     // (d <= 10 for a measured row; bounded whatever is stored)
            lj.n = t - d;
        } else {
            bool b2 = false;                                   // (flagged where the JSON itself is counted, below)
            peak_rec_json(A, r, lj, b2);
        }
        put_lit(o, "*3\r\n$3\r\nSET\r\n$");
        put_u64(o, li.n);
        put_lit(o, "\r\n");
        peak_rec_id(A, r, o, false);
        put_lit(o, "\r\n$");
        put_u64(o, lj.n);
        put_lit(o, "\r\n");
        peak_rec_json(A, r, o, bad);
        put_lit(o, "\r\n");
    } else {                                                   // "{id}\t{json}\n"
        peak_rec_id(A, r, o, false);
        o.ch('\t');
        peak_rec_json(A, r, o, bad);
        o.ch('\n');
    }
}

// Bytes of a block's rows staged in LDS.  256 RESP rows of ~305 B are 78 KB (RECORDS: ~270 B, 69 KB), beyond kPeakStage,
// where every block would go byte by byte to global memory; 96 KB holds them, and a block beyond it (long names, ids or
// signals) still takes that path.  A stage of this size leaves room for ONE workgroup per CU (160 KB of LDS a CU), four
// waves: the write stage trades occupancy for 16-B stores, which pays for these rows and not for the TSV ones.  Those are
// the rows of peak_text (~90 B) and keep its stage: behind the big one they are written no faster when every CU has one
// block and 2.6 times slower when it has fifteen (profiles/peak_records.txt has both formats measured either way; the two
// constants can be set when compiling, which is how that file was made).
#ifndef GAMS_PEAK_REC_STAGE
#define GAMS_PEAK_REC_STAGE 98304
#endif
#ifndef GAMS_PEAK_REC_TSV_STAGE
#define GAMS_PEAK_REC_TSV_STAGE kPeakStage
#endif
constexpr uint32_t kPeakRecStage = GAMS_PEAK_REC_STAGE, kPeakRecTsvStage = GAMS_PEAK_REC_TSV_STAGE;
static_assert(kPeakRecStage + 16u <= 160u * 1024u && kPeakRecTsvStage + 16u <= 160u * 1024u, "a workgroup's LDS on gfx950");

// the Peak records for the keyed row writer: every kept peak has a row
struct PeakRecRows {
    using Args = PeakRecArgs;
    using Len = uint64_t;
    static __host__ __device__ __forceinline__ uint32_t stage_bytes(const Args &a) { return a.stage; }
    template <bool kWrite>
    static __device__ __forceinline__ void row(const Args &a, uint32_t k, RowOut<kWrite, uint64_t> &o, bool &bad) { peak_rec_row(a, k, o, bad); }
    static __device__ __forceinline__ uint32_t bucket(const Args &a, uint32_t k) { return a.pk.kctg[k]; }
    // RECORDS / RESP: a name prefix or signal of kPeakRecMaxField bytes, or with a control byte (serde_json writes \uXXXX and
    // the short escapes, this writer does not).  Every neighbour is a kept line itself, so a row checks its own line only.
    static __device__ __forceinline__ bool refused(const Args &a, uint32_t k) {
        if (a.format == GAMS_LOADER_TSV) return false;
        const uint32_t i = a.pk.kline[k];
        const uint32_t nlen = a.pk.p.nlen[i], slen = a.pk.p.slen[i];
        bool bad = nlen >= kPeakRecMaxField || slen >= kPeakRecMaxField;
        if (!bad) {
            const char *nm = a.pk.t.in + a.pk.t.starts[i], *sg = a.pk.t.in + a.pk.p.sb[i];
            for (uint32_t j = 0; j < nlen; ++j) bad |= (uint8_t)nm[j] < 0x20u;
            for (uint32_t j = 0; j < slen; ++j) bad |= (uint8_t)sg[j] < 0x20u;
        }
        return bad;
    }
    static int check(gams_gpu_t *h, const std::string &who, const unsigned long long *w) {
        if (w[W_UNSUP] && !w[W_EID] && !w[W_ENOSEQ])
            return gams_fail(h, GAMS_EUNSUPPORTED, who + ": a kept line's name or signal holds a control byte or 2^30 bytes, or a gc or "
                                                         "an amplitude the device formatters do not cover (use the host path)");
        return PeakRows::check(h, who, w);
    }
};

enum : int { PK_GC = RG_GATHER, PK_ROWS, PK_WRITE, PK_STAGES };   // behind the loader's lines .. order

struct PeakJob {
    gams_seqset_t *s;
    const gams_index_t *ctg_ix;
    const gams_names_t *chr, *ids;
    const uint32_t *ctg_index;
    const int32_t *chr_start, *chr_end;
};

// what gams_gpu_peak_records_text asks on top of the job (nullptr: the rows of gams_gpu_peak_text)
struct PeakRecJob {
    int format;
    const int32_t *serial_base;
    int32_t *serial_next;
};

int peak_run(gams_gpu_t *h, const PeakJob &J, const PeakRecJob *R, const char *bytes, uint64_t n_bytes, const char **text,
             uint64_t *text_bytes, uint64_t *text_off, uint64_t *n_rows) {
    const std::string who = R ? "gpu_peak_records_text" : "gpu_peak_text";
    const uint64_t n_ctg = J.ctg_ix->m;
    *text = "";
    *text_bytes = 0;
    *n_rows = 0;
    memset(text_off, 0, (n_ctg + 1) * 8);
    for (uint64_t c = 0; R && c < n_ctg; ++c) {
        const int32_t base = R->serial_base ? R->serial_base[c] : 0;
        if (base < 0) return gams_fail(h, GAMS_EINVAL, who + ": a negative serial_base");
        if (R->serial_next) R->serial_next[c] = base;
    }
    for (uint64_t c = 0; c < n_ctg; ++c) {
        if (J.chr_end[c] < J.chr_start[c]) return gams_fail(h, GAMS_EINVAL, who + ": a ctg ends before it starts");
        if (J.ctg_index[c] != UINT32_MAX && !seq_slot_holds(J.s, J.ctg_index[c], J.chr_start[c], J.chr_end[c]))
            return gams_fail(h, GAMS_EINVAL, who + ": ctg_index does not name a sequence of the ctg's length");
    }
    GAMS_HIP(h, hipSetDevice(h->device));
    const int rc_gc = gams_seqset_gcindex(h, J.s);             // GAMS_ESTATE for a plane-only seqset
    if (rc_gc != GAMS_OK) return rc_gc;
    GAMS_HIP(h, gams_stopwatch_reserve(h, PK_STAGES));
    hipStream_t st = h->compute;
    // the per-ctg tables: one page-locked image, one copy, queued in front of the loader (the text offsets come back
    // into the image)
    PoolBlock d_tab(h, false), pin(h, true);
    const size_t n_tab = std::max<uint64_t>(n_ctg, 1);
    struct Tabs {
        unsigned long long *seq_off, *toff;
        int32_t *cs, *ce;
        uint32_t *seq_len, *sbase;                               // sbase: the records only
    };
    auto tabs = [&](Carver &c) {
        Tabs t{};
        t.seq_off = c.take<unsigned long long>(n_tab);
        t.cs = c.take<int32_t>(n_tab);
        t.ce = c.take<int32_t>(n_tab);
        t.seq_len = c.take<uint32_t>(n_tab);
        t.sbase = c.take<uint32_t>(R ? n_tab : 0);
        t.toff = c.take<unsigned long long>(n_ctg + 1);
        return t;
    };
    const size_t b_tabs = layout_bytes(tabs);
    GAMS_TRY(h, who, pin.alloc(b_tabs));
    GAMS_TRY(h, who, d_tab.alloc(b_tabs));
    const Tabs ht = carve(pin.p, tabs), dt = carve(d_tab.p, tabs);
    for (uint64_t c = 0; c < n_ctg; ++c) {
        const uint32_t slot = J.ctg_index[c];
        ht.seq_off[c] = slot == UINT32_MAX ? 0ull : J.s->off[slot];
        ht.seq_len[c] = slot == UINT32_MAX ? 0u : J.s->len[slot];
        ht.cs[c] = J.chr_start[c];
        ht.ce[c] = J.chr_end[c];
        if (R) ht.sbase[c] = (uint32_t)(R->serial_base ? R->serial_base[c] : 0);
    }
    const size_t b_in = reinterpret_cast<uint8_t *>(ht.toff) - pin.p;    // the input columns
    GAMS_TRY(h, who, hipMemcpyAsync(d_tab.p, pin.p, b_in, hipMemcpyHostToDevice, st));
    PeakLoad load{J.chr->t, PeakLines{}};
    return rg_load(h, who, J.ctg_ix, load, RgInput{bytes, n_bytes, nullptr, false}, true,
                   [&](const RgCols &C, const StageClock &stage) -> int {
        // (no rg_timed on the two early ends: an input without lines, or without a kept line, leaves the stopwatch invalid)
        if (C.n_kept == 0) return GAMS_OK;
        // the records: a serial beyond INT32_MAX is decided here, from the buckets' sizes, before anything is written
        for (uint64_t c = 0; R && c < n_ctg; ++c) {
            const uint64_t n = C.bucket_off[c + 1] - C.bucket_off[c];
            if (n && (uint64_t)ht.sbase[c] + n > (uint64_t)INT32_MAX) return gams_fail(h, GAMS_EINVAL, who + ": a serial beyond INT32_MAX");
        }
        const uint32_t K = C.v.n_kept;
        PoolBlock s2(h, false);
        PeakRecArgs ra{};
        PeakArgs &a = ra.pk;
        a.t = C.t;
        a.p = load.pl;
        a.v = C.v;
        a.cs = dt.cs;
        a.ce = dt.ce;
        a.seq_len = dt.seq_len;
        a.ids = J.ids->t;
        a.o.text_off = dt.toff;
        a.o.words = C.words;
        auto kept = [&](Carver &c) {   // line ctg start end | gc | the writer's
            a.kline = c.take<uint32_t>(K);
            a.kctg = c.take<uint32_t>(K);
            a.ks = c.take<uint32_t>(K);
            a.ke = c.take<uint32_t>(K);
            a.gc = c.take<float>(K);
            if (R)
                ra.o.carve(c, K);
            else
                a.o.carve(c, K);
        };
        GAMS_TRY(h, who, s2.alloc(layout_bytes(kept)));
        carve(s2.p, kept);
        GAMS_TRY(h, who, stage(PK_GC, true));
        hipLaunchKernelGGL(peak_gather_kernel, dim3((K + 255u) / 256u), dim3(256), 0, st, a);
        gams_launch_range_gc_cols(J.s, dt.seq_off, dt.seq_len, dt.cs, a.kctg, a.ks, a.ke, K, a.gc, st);
        GAMS_TRY(h, who, stage(PK_GC, false));
        if (!R) return keyed_text_run<PeakRows>(h, who, C, stage, PK_ROWS, a, TEXT_PEAK, ht.toff, text, text_bytes, text_off, n_rows);
        ra.v = a.v;
        ra.sbase = dt.sbase;
        ra.format = R->format;
        ra.stage = R->format == GAMS_LOADER_TSV ? kPeakRecTsvStage : kPeakRecStage;
        ra.o.text_off = a.o.text_off;
        ra.o.words = a.o.words;
        const int rc = keyed_text_run<PeakRecRows>(h, who, C, stage, PK_ROWS, ra, TEXT_PEAK_RECORDS, ht.toff, text, text_bytes, text_off,
                                                   n_rows);
        if (rc != GAMS_OK) return rc;
        if (R->serial_next)
            for (uint64_t c = 0; c < n_ctg; ++c) R->serial_next[c] = (int32_t)(ht.sbase[c] + (C.bucket_off[c + 1] - C.bucket_off[c]));
        return GAMS_OK;
    });
}


// ---- `gams sw` from the bytes of a feature file (feature.rs:50-54 read_range, then sw.rs:132-191) ---------------------
// The range loader as it is (key (ctg, line): the kept lines of a ctg in file order, which is the order feature.rs:74-86
// numbers them in), then, one lane per kept feature, the gather below; the stages behind it are sw.hip's
// (gams_launch_sw_cols): the rows per feature and their prefix, sw_kernel over these columns, and the text with
// "feature:{ctg id}:{k}" composed on the device.
static_assert(SWF_GATHER == RG_GATHER, "the sw stages continue the loader's stopwatch behind `order`");

struct SwGather {
    RgKept v;                                 // the kept lines in (ctg, line) order
    uint32_t n_ctg;
    const int32_t *cs, *ce;                   // per interval
    const CountGroup *groups;                 // the ctg index's groups: group g owns intervals [off, off + n)
    uint32_t n_groups;
    int32_t *fs, *fe;                         // per kept feature
    uint32_t *fctg;
    uint32_t *igrp;                           // per interval: its group (UINT32_MAX: none owns it)
    unsigned long long *words;                // [1] a kept feature leaves its ctg with its middle, [2] the smallest such line
};

__global__ __launch_bounds__(256) void sw_gather_kernel(const SwGather a) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k < a.v.n_kept) {
        const uint32_t i = a.v.line(k), c = a.v.bucket(k);
        const int64_t s = a.v.qs[i], e = a.v.qe[i];
        a.fs[k] = (int32_t)s;
        a.fe[k] = (int32_t)e;
        a.fctg[k] = c;
        // window.rs:98-110: the middle pair of the feature must be members of the ctg span (sw_host_rows on the host);
        // located by overlap does not imply it.  Integer min: the line reported does not depend on arrival order
        const int64_t flen = e - s + 1, half = flen / 2;
        const int64_t mid_l = half == 0 ? s : s + half - 1, mid_r = half == 0 ? s : s + half;
        if (flen < 1 || mid_l < a.cs[c] || mid_r > a.ce[c]) {
            a.words[1] = 1ull;
            atomicMin(a.words + 2, (unsigned long long)i);
        }
    }
    if (k < a.n_ctg) {                        // the last group that begins at or before interval k holds it
        uint32_t lo = 0, hi = a.n_groups;
        while (hi - lo > 1u) {
            const uint32_t mid = (lo + hi) >> 1;
            if (a.groups[mid].off <= k)
                lo = mid;
            else
                hi = mid;
        }
        a.igrp[k] = a.n_groups && k - a.groups[lo].off < a.groups[lo].n ? lo : UINT32_MAX;
    }
}

struct SwFeatJob {
    SwCall call;                              // (with call.summary the three text outputs below are NULL)
    gams_seqset_t *s;
    const gams_index_t *ctg_ix;
    const gams_names_t *chr, *ids;
    const uint32_t *ctg_index;
    const int32_t *chr_start, *chr_end;
};

int sw_feature_run(gams_gpu_t *h, const SwFeatJob &J, const char *bytes, uint64_t n_bytes, const char **text,
                   uint64_t *text_bytes, uint64_t *text_off, uint64_t *n_features, uint64_t *n_rows) {
    const SwCall &call = J.call;
    const std::string who = call.summary ? "gpu_sw_feature_summary" : "gpu_sw_feature_text";
    const uint64_t n_ctg = J.ctg_ix->m;
    const bool do_gc = call.gc();
    *n_features = 0;
    *n_rows = 0;
    if (!call.summary) {
        *text = "";
        *text_bytes = 0;
        memset(text_off, 0, (n_ctg + 1) * 8);
    }
    for (uint64_t c = 0; c < n_ctg; ++c)
        if (J.chr_end[c] < J.chr_start[c]) return gams_fail(h, GAMS_EINVAL, who + ": a ctg ends before it starts");
    GAMS_HIP(h, hipSetDevice(h->device));
    if (do_gc) {
        const int rc_gc = gams_seqset_gcindex(h, J.s);             // GAMS_ESTATE for a plane-only seqset
        if (rc_gc != GAMS_OK) return rc_gc;
    }
    GAMS_HIP(h, gams_stopwatch_reserve(h, SWF_STAGES));
    return rg_load(h, who, J.ctg_ix, RgPlain{J.chr->t}, RgInput{bytes, n_bytes, nullptr, false}, true,
                   [&](const RgCols &C, const StageClock &stage) -> int {
        *n_features = C.n_kept;
        if (C.n_kept == 0) {
            if (C.ran) rg_timed(h, RG_ORDER + 1);
            return GAMS_OK;
        }
        // one thread per (feature, slot), as sw_check bounds it
        const int rs = gams_sw_call_check(h, who, call, SWC_SLOTS, n_ctg, true, C.n_kept);
        if (rs != GAMS_OK) return rs;
        if (do_gc)
            for (uint64_t c = 0; c < n_ctg; ++c) {
                if (C.bucket_off[c + 1] == C.bucket_off[c]) continue;
                const uint32_t slot = J.ctg_index[c];
                if (slot == UINT32_MAX) return gams_fail(h, GAMS_EINVAL, who + ": a ctg with features has no sequence in the seqset");
                if (!seq_slot_holds(J.s, slot, J.chr_start[c], J.chr_end[c]))
                    return gams_fail(h, GAMS_EINVAL, who + ": ctg_index does not name a sequence of the ctg's length");
            }
        const uint32_t K = (uint32_t)C.n_kept, nc = (uint32_t)n_ctg;
        hipStream_t st = h->compute;
        PoolBlock d_cols(h, false), pin(h, true);
        SwGather g{};
        int32_t *d_cs = nullptr, *d_ce = nullptr;
        auto cols = [&](Carver &c) {   // cs ce | fs fe fctg | igrp | words
            d_cs = c.take<int32_t>(nc);
            d_ce = c.take<int32_t>(nc);
            g.fs = c.take<int32_t>(K);
            g.fe = c.take<int32_t>(K);
            g.fctg = c.take<uint32_t>(K);
            g.igrp = c.take<uint32_t>(nc);
            g.words = c.take<unsigned long long>(3);
        };
        GAMS_TRY(h, who, d_cols.alloc(layout_bytes(cols)));
        carve(d_cols.p, cols);
        const size_t b_place = 2 * gams_align256((size_t)nc * 4);       // cs | ce, as the layout places them
        GAMS_TRY(h, who, pin.alloc(b_place));
        int32_t *const h_cs = reinterpret_cast<int32_t *>(pin.p), *const h_ce = reinterpret_cast<int32_t *>(pin.p + b_place / 2);
        memcpy(h_cs, J.chr_start, (size_t)nc * 4);
        memcpy(h_ce, J.chr_end, (size_t)nc * 4);
        GAMS_TRY(h, who, hipMemcpyAsync(d_cs, pin.p, b_place, hipMemcpyHostToDevice, st));
        unsigned long long *const hw = h->pin_scratch;                  // words: rows, flag, smallest offending line
        hw[0] = hw[1] = 0ull;
        hw[2] = ~0ull;
        GAMS_TRY(h, who, hipMemcpyAsync(g.words, hw, 3 * 8, hipMemcpyHostToDevice, st));
        g.v = C.v;
        g.n_ctg = nc;
        g.cs = d_cs;
        g.ce = d_ce;
        g.groups = J.ctg_ix->d_cgroups;
        g.n_groups = J.ctg_ix->n_groups;
        GAMS_TRY(h, who, stage(SWF_GATHER, true));
        hipLaunchKernelGGL(sw_gather_kernel, dim3((std::max(K, nc) + 255u) / 256u), dim3(256), 0, st, g);
        GAMS_TRY(h, who, hipGetLastError());
        GAMS_TRY(h, who, stage(SWF_GATHER, false));
        // (the copy of the words must have left pin_scratch before the launcher reads back into it: same stream, in order)
        SwColsJob S{};
        S.call = call;
        S.s = do_gc ? J.s : nullptr;
        S.n_ctg = nc;
        S.nf = K;
        S.fs = g.fs;
        S.fe = g.fe;
        S.fctg = g.fctg;
        S.d_bucket_off = C.v.bucket_off;
        S.bucket_off = C.bucket_off;
        S.ctg_index = J.ctg_index;
        S.chr_start = J.chr_start;
        S.chr_end = J.chr_end;
        S.igrp = g.igrp;
        S.chr_off = J.chr->t.off;
        S.chr_bytes = J.chr->t.bytes;
        S.id_off = J.ids->t.off;
        S.id_bytes = J.ids->t.bytes;
        S.max_chr = J.chr->max_len;
        S.max_id = J.ids->max_len;
        S.words = g.words;
        const int rc = gams_launch_sw_cols(h, S, text, text_bytes, text_off, n_rows);
        if (rc != GAMS_OK) return rc;
        rg_timed(h, call.summary ? SWF_ROWS + 1 : SWF_STAGES);
        return GAMS_OK;
    });
}

// What the feature entries test behind their own null arguments, in this order: the actions, gc without a seqset, count
// without an index, the bounds (GAMS_EINVAL), the name tables, max beyond 2^24 (GAMS_EUNSUPPORTED) and, for a summary, the
// accumulator and its span sets; then the run.
int sw_feature_checked(gams_gpu_t *h, const std::string &who, const SwFeatJob &J, const char *bytes, uint64_t n_bytes,
                       const char **text, uint64_t *text_bytes, uint64_t *text_off, uint64_t *n_features, uint64_t *n_rows) {
    const uint64_t m = J.ctg_ix->m;
    int rc = gams_sw_call_check(h, who, J.call, SWC_ACTIONS | SWC_WINDOW, m, J.s && (!m || J.ctg_index));
    if (rc != GAMS_OK) return rc;
    if (J.ids->t.n != m) return gams_fail(h, GAMS_EINVAL, who + ": ctg_ids must name every interval of ctg_ix");
    if (J.chr->t.n < J.ctg_ix->n_groups) return gams_fail(h, GAMS_EINVAL, who + ": chr_names must name every group of ctg_ix");
    if ((rc = gams_sw_call_check(h, who, J.call, SWC_MAX | (J.call.summary ? SWC_SUMMARY : 0u), m)) != GAMS_OK) return rc;
    return sw_feature_run(h, J, bytes, n_bytes, text, text_bytes, text_off, n_features, n_rows);
}

// ---- the records of `gams rg` / `gams feature` (rg.rs:40-82, feature.rs:47-96) as text -----------------------------------
// The range loader over several files with (file, ctg) buckets (RgInput::files, by_file) and a parse kernel that also says
// where the name, the chromosome and the strand of every line lie, then a stage of its own and the two of the keyed row
// writer (RecRows); ten in all:
//   serials  per kept line in key order -- grouped by (file, ctg), in line order inside a group --: its line, its bucket
//            and its serial = sbase[bucket] + its rank in the bucket + 1.  sbase is the host's, from the buckets' sizes:
//            cnt:{kind}:{ctg} before the load plus the kept lines of the ctg in the files in front (rg.rs:63-75);
//   rows     the check of a row's name and strand for control bytes, and its length;
//   write    the rows at their offsets and the offset of every bucket's first row.
// A row is described once (rec_row) for the three formats; RESP needs the lengths of the id and of the JSON in front of
// them, which the same descriptions give through a counting RowOut.
struct RecLines {
    unsigned long long *cb;           // per line: where the chromosome begins
    uint32_t *clen, *nlen, *slen;     // its length; the name's (without the '.'; 0: none); the strand's (0: none), which
};                                    // begins behind the '(' that follows the chromosome

__global__ __launch_bounds__(256) void rec_parse_kernel(const TextLines t, const NameTab chr, uint32_t *grp, uint32_t *qs,
                                                        uint32_t *qe, const RecLines p) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= t.n_lines) return;
    uint64_t b, e;
    line_of(t, i, b, e);
    const char *s = t.in;
    const RangeField r = parse_range(s, b, e);                 // utils.rs:50: the line, not its first field
    uint64_t nlen = 0, slen = 0;
    if (r.ok) {
        nlen = r.cb > b ? r.cb - b - 1u : 0u;                  // the name ends at the first '.', which the chromosome follows
        if (s[r.ce] == '(') {                                  // "(strand)" up to the last ':' of the trimmed line
            uint64_t c = e;
            while (c > r.ce && s[c - 1u] != ':') --c;
            slen = c - r.ce - 3u;                              // c - 1: the colon, c - 2: the ')'
        }
    }
    grp[i] = r.ok ? name_find(chr, s + r.cb, r.ce - r.cb) : UINT32_MAX;
    qs[i] = r.start;
    qe[i] = r.end;
    p.cb[i] = r.cb;
    p.clen[i] = (uint32_t)(r.ce - r.cb);
    p.nlen[i] = (uint32_t)(nlen < 0xffffffffull ? nlen : 0xffffffffull);
    p.slen[i] = (uint32_t)(slen < 0xffffffffull ? slen : 0xffffffffull);
}

// what the records ask of the loader (see RgPlain)
struct RecLoad {
    NameTab chr;
    RecLines rl;
    static constexpr uint32_t mid_bits = 0;
    static constexpr const char *efield = nullptr;
    void cols(Carver &c, uint32_t L) {
        rl.cb = c.take<unsigned long long>(L);
        rl.clen = c.take<uint32_t>(L);
        rl.nlen = c.take<uint32_t>(L);
        rl.slen = c.take<uint32_t>(L);
    }
    void parse(const TextLines &tl, uint32_t *grp, uint32_t *qs, uint32_t *qe, unsigned long long *, uint32_t nbr, hipStream_t st) const {
        hipLaunchKernelGGL(rec_parse_kernel, dim3(nbr), dim3(256), 0, st, tl, chr, grp, qs, qe, rl);
    }
};

constexpr uint32_t kRecMaxField = 1u << 30;   // a name or strand of this many bytes is refused: a row's lengths stay below 2^32

struct RecArgs {
    TextLines t;
    RecLines p;
    RgKept v;                                 // the kept lines in (file, ctg, line) order
    uint32_t n_ctg;
    const uint32_t *sbase;                    // per bucket: the serial in front of its first row's
    NameTab ids;
    const char *tag;
    uint32_t tag_len;
    int kind, format;
    uint32_t *kline, *kbkt, *kserial;         // per kept line
    KeyedText<unsigned long long> o;
};

__global__ __launch_bounds__(256) void rec_serial_kernel(const RecArgs a) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= a.v.n_kept) return;
    const uint32_t b = a.v.bucket(k);
    a.kline[k] = a.v.line(k);
    a.kbkt[k] = b;
    a.kserial[k] = a.sbase[b] + (k - (uint32_t)a.v.bucket_off[b]) + 1u;
}

// "{kind}:{ctg_id}:{serial}" (rg.rs:64-66, feature.rs:81-83); json: inside a JSON string
template <bool kWrite>
__device__ __forceinline__ void rec_id(const RecArgs &a, uint32_t k, RowOut<kWrite, uint64_t> &o, bool json) {
    if (a.kind == GAMS_LOADER_FEATURE)
        o.bytes("feature:", 8u);
    else
        o.bytes("rg:", 3u);
    const uint32_t c = a.kbkt[k] % a.n_ctg;
    const unsigned long long io = a.ids.off[c], il = a.ids.off[c + 1u] - io;
    if (json)
        o.esc(a.ids.bytes + io, il);
    else
        o.bytes(a.ids.bytes + io, il);
    o.ch(':');
    o.dec(a.kserial[k]);
}

// Range::to_string() of the parsed line: canonical, not echoed
template <bool kWrite>
__device__ __forceinline__ void rec_range(const RecArgs &a, uint32_t i, RowOut<kWrite, uint64_t> &o, bool json) {
    const char *in_ = a.t.in;
    const uint64_t cb = a.p.cb[i], clen = a.p.clen[i], nlen = a.p.nlen[i], slen = a.p.slen[i];
    if (nlen) {
        if (json)
            o.esc(in_ + a.t.starts[i], nlen);
        else
            o.bytes(in_ + a.t.starts[i], nlen);
        o.ch('.');
    }
    o.bytes(in_ + cb, clen);
    if (slen) {
        o.ch('(');
        if (json)
            o.esc(in_ + cb + clen + 1u, slen);
        else
            o.bytes(in_ + cb + clen + 1u, slen);
        o.ch(')');
    }
    o.ch(':');
    const uint32_t s = a.v.qs[i], e = a.v.qe[i];
    o.dec(s);
    if (e != s) {
        o.ch('-');
        o.dec(e);
    }
}

// serde_json of Rg / Feature (data.rs:16-28): field order, no spaces
template <bool kWrite>
__device__ __forceinline__ void rec_json(const RecArgs &a, uint32_t k, RowOut<kWrite, uint64_t> &o) {
    const uint32_t i = a.kline[k];
    o.bytes("{\"id\":\"", 7u);
    rec_id(a, k, o, true);
    o.bytes("\",\"range\":\"", 11u);
    rec_range(a, i, o, true);
    if (a.kind == GAMS_LOADER_FEATURE) {
        o.bytes("\",\"length\":", 11u);
        o.i32((int32_t)(a.v.qe[i] - a.v.qs[i] + 1u));              // feature.rs:88: end - start + 1, an i32
        o.bytes(",\"tag\":\"", 8u);
        o.esc(a.tag, (uint64_t)a.tag_len);
    }
    o.bytes("\"}", 2u);
}

template <bool kWrite>
__device__ void rec_row(const RecArgs &a, uint32_t k, RowOut<kWrite, uint64_t> &o) {
    if (a.format == GAMS_LOADER_TSV) {                         // tsv.rs: the values in field order
        const uint32_t i = a.kline[k];
        rec_id(a, k, o, false);
        o.ch('\t');
        rec_range(a, i, o, false);
        if (a.kind == GAMS_LOADER_FEATURE) {
            o.ch('\t');
            o.i32((int32_t)(a.v.qe[i] - a.v.qs[i] + 1u));
            o.ch('\t');
            o.bytes(a.tag, (uint64_t)a.tag_len);
        }
        o.ch('\n');
    } else if (a.format == GAMS_LOADER_RESP) {                 // wire::resp_command({"SET", id, json})
        RowOut<false, uint64_t> li, lj;
        rec_id(a, k, li, false);
        rec_json(a, k, lj);
        o.bytes("*3\r\n$3\r\nSET\r\n$", 14u);
        o.dec((uint32_t)li.n);
        o.bytes("\r\n", 2u);
        rec_id(a, k, o, false);
        o.bytes("\r\n$", 3u);
        o.dec((uint32_t)lj.n);
        o.bytes("\r\n", 2u);
        rec_json(a, k, o);
        o.bytes("\r\n", 2u);
    } else {                                                   // "{id}\t{json}\n"
        rec_id(a, k, o, false);
        o.ch('\t');
        rec_json(a, k, o);
        o.ch('\n');
    }
}

// bytes of a block's rows staged in LDS: 256 RESP rows of a feature are ~36 KB; a block beyond the stage (long names or
// tags) writes its rows to global memory directly
constexpr uint32_t kRecStage = 49152;

// the records for the keyed row writer
struct RecRows {
    using Args = RecArgs;
    using Len = uint64_t;
    static constexpr uint32_t kStage = kRecStage;
    template <bool kWrite>
    static __device__ __forceinline__ void row(const Args &a, uint32_t k, RowOut<kWrite, uint64_t> &o, bool &) { rec_row(a, k, o); }
    static __device__ __forceinline__ uint32_t bucket(const Args &a, uint32_t k) { return a.kbkt[k]; }
    // a name or strand of kRecMaxField bytes, or with a control byte: serde_json writes \uXXXX and the like, this writer does not
    static __device__ __forceinline__ bool refused(const Args &a, uint32_t k) {
        const uint32_t i = a.kline[k];
        const uint32_t nlen = a.p.nlen[i], slen = a.p.slen[i];
        bool bad = nlen >= kRecMaxField || slen >= kRecMaxField;
        if (!bad) {
            const char *nm = a.t.in + a.t.starts[i], *sd = a.t.in + a.p.cb[i] + a.p.clen[i] + 1u;
            for (uint32_t j = 0; j < nlen; ++j) bad |= (uint8_t)nm[j] < 0x20u;
            for (uint32_t j = 0; j < slen; ++j) bad |= (uint8_t)sd[j] < 0x20u;
        }
        return bad;
    }
    static int check(gams_gpu_t *h, const std::string &who, const unsigned long long *w) {
        if (w[W_UNSUP])
            return gams_fail(h, GAMS_EUNSUPPORTED, who + ": a kept line's name or strand holds a control byte, or 2^30 bytes (use the host path)");
        return GAMS_OK;
    }
};

enum : int { LT_SERIALS = RG_GATHER, LT_ROWS, LT_WRITE, LT_STAGES };   // behind the loader's lines .. order

struct RecJob {
    const gams_index_t *ctg_ix;
    const gams_names_t *chr, *ids;
    TextFiles files;
    int kind, format;
    const char *tag;
    uint64_t tag_bytes;
    const int32_t *serial_base;
};

int loader_text_run(gams_gpu_t *h, const RecJob &J, const char **text, uint64_t *text_bytes, uint64_t *text_off,
                    int32_t *serial_next, uint64_t *n_in_file, uint64_t *n_rows) {
    const std::string who = "gpu_loader_text";
    const uint64_t n_ctg = J.ctg_ix->m, n_files = J.files.n, n_pairs = n_files * n_ctg;
    *text = "";
    *text_bytes = 0;
    *n_rows = 0;
    memset(text_off, 0, (n_pairs + 1) * 8);
    for (uint64_t f = 0; f < n_files; ++f)
        if (n_in_file) n_in_file[f] = 0;
    for (uint64_t c = 0; c < n_ctg; ++c) {
        const int32_t base = J.serial_base ? J.serial_base[c] : 0;
        if (base < 0) return gams_fail(h, GAMS_EINVAL, who + ": a negative serial_base");
        if (serial_next) serial_next[c] = base;
    }
    GAMS_HIP(h, hipSetDevice(h->device));
    GAMS_HIP(h, gams_stopwatch_reserve(h, LT_STAGES));
    RecLoad load{J.chr->t, RecLines{}};
    return rg_load(h, who, J.ctg_ix, load, RgInput{nullptr, 0, &J.files, true}, true, [&](const RgCols &C, const StageClock &stage) -> int {
        if (C.n_kept == 0) {
            if (C.ran) rg_timed(h, RG_ORDER + 1);
            return GAMS_OK;
        }
        // (kept lines: there is a file, and with one file the buckets are the ctgs: n_bkt = n_files * n_ctg either way)
        const uint64_t n_bkt = C.n_bkt;
        const uint32_t K = C.v.n_kept;
        hipStream_t st = h->compute;
        PoolBlock s2(h, false), pin(h, true);
        // the serials: the buckets of a ctg, file by file, continue its counter
        struct Tabs {
            uint32_t *sbase;
            unsigned long long *toff;
        };
        auto tabs = [&](Carver &c) {
            Tabs t{};
            t.sbase = c.take<uint32_t>(n_bkt);
            t.toff = c.take<unsigned long long>(n_bkt + 1);
            return t;
        };
        GAMS_TRY(h, who, pin.alloc(layout_bytes(tabs)));
        const Tabs ht = carve(pin.p, tabs);
        std::vector<int64_t> next(n_ctg);
        for (uint64_t c = 0; c < n_ctg; ++c) next[c] = J.serial_base ? J.serial_base[c] : 0;
        for (uint64_t b = 0; b < n_bkt; ++b) {
            const uint64_t c = b % n_ctg, n = C.bucket_off[b + 1] - C.bucket_off[b];
            ht.sbase[b] = (uint32_t)next[c];
            next[c] += (int64_t)n;
            if (n && next[c] > INT32_MAX) return gams_fail(h, GAMS_EINVAL, who + ": a serial beyond INT32_MAX");
        }
        RecArgs a{};
        char *d_tag = nullptr;
        Tabs dt{};
        auto kept = [&](Carver &c) {   // sbase text_off | line bucket serial | the writer's | tag
            dt = tabs(c);
            a.kline = c.take<uint32_t>(K);
            a.kbkt = c.take<uint32_t>(K);
            a.kserial = c.take<uint32_t>(K);
            a.o.carve(c, K);
            d_tag = c.take<char>(std::max<uint64_t>(J.tag_bytes, 1));
        };
        GAMS_TRY(h, who, s2.alloc(layout_bytes(kept)));
        carve(s2.p, kept);
        a.t = C.t;
        a.p = load.rl;
        a.v = C.v;
        a.n_ctg = (uint32_t)n_ctg;
        a.sbase = dt.sbase;
        a.ids = J.ids->t;
        a.tag = d_tag;
        a.tag_len = (uint32_t)J.tag_bytes;
        a.kind = J.kind;
        a.format = J.format;
        a.o.text_off = dt.toff;
        a.o.words = C.words;
        GAMS_TRY(h, who, stage(LT_SERIALS, true));
        GAMS_TRY(h, who, hipMemcpyAsync(dt.sbase, ht.sbase, n_bkt * 4, hipMemcpyHostToDevice, st));
        if (J.tag_bytes) GAMS_TRY(h, who, hipMemcpyAsync(d_tag, J.tag, J.tag_bytes, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(rec_serial_kernel, dim3((K + 255u) / 256u), dim3(256), 0, st, a);
        GAMS_TRY(h, who, stage(LT_SERIALS, false));
        const int rc = keyed_text_run<RecRows>(h, who, C, stage, LT_ROWS, a, TEXT_RECORDS, ht.toff, text, text_bytes, text_off, n_rows);
        if (rc != GAMS_OK) return rc;
        for (uint64_t f = 0; f < n_files; ++f)
            if (n_in_file) n_in_file[f] = C.bucket_off[(f + 1) * n_ctg] - C.bucket_off[f * n_ctg];
        if (serial_next)
            for (uint64_t c = 0; c < n_ctg; ++c) serial_next[c] = (int32_t)next[c];
        return GAMS_OK;
    });
}


// ---- `locate --seq` (locate.rs:124-134): the bytes of a range file -> ">{rg}\n{bases}\n" of every located line --------
// Behind the front of locate_text (line index, text_parse_rg_kernel, interval_locate_kernel), six stages in all:
//   lines, parse, locate   as for locate_text;
//   lengths  one lane per line: a located line must lie inside its ctg and the ctg needs a slot of its length (flags,
//            and the smallest line that leaves its ctg); its row is 1 + rg + 1 + bases + 1 bytes, and its first base is
//            byte src of the seqset's buffer; the block sums of the lengths;
//   offsets  their prefix over the blocks, then row_off[line] = the block's offset + the prefix inside the block.
//            Unlike the other entries the per-line offsets are kept: the copy searches them;
//   copy     seq_copy_kernel, below.
// A row is 3 bytes or a whole ctg, so the writer gives lanes to bytes of the text, not to rows (seq_text_plan.hpp): one
// workgroup per chunk of kSeqTextChunk bytes, one thread per 16-B unit of the text at a time.  A unit that lies inside
// the bases of one row -- nearly all of them once rows are long -- is four aligned dwords and a fifth of the seqset,
// realigned in registers (v_alignbyte) and stored as one dwordx4; a unit that holds a seam between pieces or rows -- all of
// them when the rows are point ranges -- is put together run by run, each run the aligned dwords that hold it, shifted to
// its place in two 64-bit registers, and leaves as one dwordx4 all the same.  Only the last unit of the whole text, when
// the text is no multiple of 16, is stored byte by byte.  Thread 0 searches row_off for the chunk's first and last row;
// their offsets go to LDS and every unit finds its row there by binary search; a line without a row has zero bytes and
// is never found.
enum : uint32_t { W_SEQ_LINE = W_EFIELD };   // this entry's use of the word: the smallest line that leaves its ctg
enum : int { SQ_LINES = 0, SQ_PARSE, SQ_LOCATE, SQ_LENGTHS, SQ_OFFSETS, SQ_COPY, SQ_STAGES };

struct SeqTextArgs {
    TextLines t;
    const unsigned long long *fend;           // per line: where rg ends
    const int64_t *hit;                       // per line: the located interval, or -1
    const uint32_t *qs, *qe;                  // per line
    const unsigned long long *seq_off;        // per interval: the first byte of its slot in seq (~0: no slot of the ctg's length)
    const int32_t *cs, *ce;                   // per interval
    unsigned long long *row_off;              // n_lines + 1 (the lengths pass leaves the lengths here)
    unsigned long long *src;                  // per line with a row: its first base in seq
    unsigned long long *blk_bytes;            // per workgroup of 256 lines
    const unsigned long long *blk_off;
    unsigned long long *words;
    const uint8_t *seq;
    char *text;
    uint64_t total;                           // bytes of the text
};

__global__ __launch_bounds__(256) void seq_row_len_kernel(const SeqTextArgs a) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    uint64_t l = 0;
    if (i < a.t.n_lines) {
        const int64_t c = a.hit[i];
        if (c >= 0) {
            const int64_t s = a.qs[i], e = a.qe[i];
            const unsigned long long so = a.seq_off[c];
            if (s < a.cs[c] || e > a.ce[c] || e < s) {       // the reference panics on the slice (locate.rs:133)
                a.words[W_EID] = 1ull;
                atomicMin(a.words + W_SEQ_LINE, (unsigned long long)i);   // integer min: whatever order lanes ran in
            } else if (so == ~0ull) {
                a.words[W_ENOSEQ] = 1ull;
            } else {
                l = seq_plan_row_len(a.fend[i] - a.t.starts[i], (uint64_t)(e - s + 1));
                a.src[i] = so + (uint64_t)(s - a.cs[c]);
            }
        }
        a.row_off[i] = l;
    }
    row_block_totals(l, a.blk_bytes, a.words);
}

__global__ __launch_bounds__(256) void seq_row_off_kernel(const SeqTextArgs a) {
    __shared__ uint64_t ws[4];
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const uint64_t l = i < a.t.n_lines ? a.row_off[i] : 0ull;
    uint64_t tot;
    const uint64_t at = a.blk_off[blockIdx.x] + block_excl_scan_256<uint64_t>(l, ws, tot);
    if (i < a.t.n_lines) a.row_off[i] = at;
    if (i + 1u == a.t.n_lines) a.row_off[i + 1u] = at + l;
}

// 16 bytes from p, which is 4-B aligned: one dwordx4 load (global memory takes it at dword alignment)
struct __attribute__((packed, aligned(4))) Dwords4 {
    uint32_t x, y, z, w;
};

// Bytes [0, len) of `from`, 1 <= len <= 16, as a little-endian value of 128 bits (lo, hi), zero above them: aligned
// dword loads, issued together, of the dwords that hold a byte of the run and of no other -- each lies inside the
// buffer the run lies in --, realigned in registers.
__device__ __forceinline__ void load_run16(const uint8_t *from, uint32_t len, uint64_t &lo, uint64_t &hi) {
    const uint32_t sh = (uint32_t)reinterpret_cast<uintptr_t>(from) & 3u, need = sh + len;
    const uint32_t *const w = reinterpret_cast<const uint32_t *>(from - sh);
    const uint32_t w0 = w[0], w1 = need > 4u ? w[1] : 0u, w2 = need > 8u ? w[2] : 0u, w3 = need > 12u ? w[3] : 0u,
                   w4 = need > 16u ? w[4] : 0u;
    lo = __builtin_amdgcn_alignbyte(w1, w0, sh) | (uint64_t)__builtin_amdgcn_alignbyte(w2, w1, sh) << 32;
    hi = __builtin_amdgcn_alignbyte(w3, w2, sh) | (uint64_t)__builtin_amdgcn_alignbyte(w4, w3, sh) << 32;
    if (len < 8u) {
        lo &= (1ull << (8u * len)) - 1ull;
        hi = 0ull;
    } else if (len < 16u) {
        hi &= (1ull << (8u * (len - 8u))) - 1ull;
    }
}

// rows of a chunk whose offsets are searched in LDS (16 KiB of it); a chunk with more -- long runs of lines without
// rows -- searches them in global memory
constexpr uint32_t kSeqStageRows = 2048;

// The units of chunk [c0, c1) that belong to this thread.  `ro` holds the offsets of the chunk's rows and the one behind
// them, n_rows + 1 entries, entry 0 being row `base` of the text: a.row_off + base itself, or its copy in LDS.
__device__ __forceinline__ void seq_copy_units(const SeqTextArgs &a, const unsigned long long *ro, uint64_t base, uint64_t n_rows,
                                               uint64_t c0, uint64_t c1) {
    for (uint64_t p = c0 + 16u * threadIdx.x; p < c1; p += 16u * 256u) {
        const uint64_t pe = p + 16u < c1 ? p + 16u : c1;
        uint64_t r = seq_plan_row_at(ro, 0, n_rows, p);
        // the row: where it begins and ends in the text, its rg in the input, its first base in the seqset
        uint64_t r_at = ro[r], r_end = ro[r + 1u], rg_at = a.t.starts[base + r], rg_len = a.fend[base + r] - rg_at, src = a.src[base + r];
        SeqRun u = seq_plan_run(r_at, rg_len, r_end - r_at - rg_len - 3u, p, pe);
        uint64_t lo = 0, hi = 0;
        if (u.piece == SEQ_BASES && u.len == 16u) {
            // the unit lies inside the bases of one row: four aligned dwords and, off the dword grid, a fifth (it holds
            // byte 15 of the unit, so it begins inside the ctg)
            const uint64_t s = src + u.src_off;
            const uint8_t *const s4 = a.seq + (s & ~3ull);
            const uint32_t sh = (uint32_t)s & 3u;
            const Dwords4 v = *reinterpret_cast<const Dwords4 *>(s4);
            const uint32_t v4 = sh ? *reinterpret_cast<const uint32_t *>(s4 + 16) : 0u;
            lo = __builtin_amdgcn_alignbyte(v.y, v.x, sh) | (uint64_t)__builtin_amdgcn_alignbyte(v.z, v.y, sh) << 32;
            hi = __builtin_amdgcn_alignbyte(v.w, v.z, sh) | (uint64_t)__builtin_amdgcn_alignbyte(v4, v.w, sh) << 32;
        } else {
            // a seam inside the unit: run by run, each shifted to its place
            for (;;) {
                uint64_t b_lo = u.piece == SEQ_GT ? (uint64_t)'>' : (uint64_t)'\n', b_hi = 0;
                if (u.piece == SEQ_RG) load_run16(reinterpret_cast<const uint8_t *>(a.t.in) + rg_at + u.src_off, (uint32_t)u.len, b_lo, b_hi);
                if (u.piece == SEQ_BASES) load_run16(a.seq + src + u.src_off, (uint32_t)u.len, b_lo, b_hi);
                const uint32_t j = (uint32_t)(u.dst_off - p);  // the run's first byte in the unit; it ends inside it
                if (j == 0u) {
                    lo |= b_lo;
                    hi |= b_hi;
                } else if (j < 8u) {
                    lo |= b_lo << (8u * j);
                    hi |= (b_hi << (8u * j)) | (b_lo >> (64u - 8u * j));
                } else {
                    hi |= b_lo << (8u * (j - 8u));
                }
                const uint64_t pos = u.dst_off + u.len;
                if (pos >= pe) break;
                if (pos == r_end) {
                    r = seq_plan_next_row(ro, r, n_rows, pos);
                    r_at = ro[r], r_end = ro[r + 1u], rg_at = a.t.starts[base + r], rg_len = a.fend[base + r] - rg_at, src = a.src[base + r];
                }
                u = seq_plan_run(r_at, rg_len, r_end - r_at - rg_len - 3u, pos, pe);
            }
        }
        if (pe - p == 16u) {
            *reinterpret_cast<uint4 *>(a.text + p) = make_uint4((uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32));
        } else {                                               // the ragged tail of the whole text
            for (uint32_t j = 0; j < (uint32_t)(pe - p); ++j) a.text[p + j] = (char)((j < 8u ? lo >> (8u * j) : hi >> (8u * (j - 8u))) & 0xffu);
        }
    }
}

// Never launched when the lengths pass set an error word, nor for an empty text: every row it reads was checked there.
__global__ __launch_bounds__(256) void seq_copy_kernel(const SeqTextArgs a) {
    __shared__ uint64_t rows[2];
    __shared__ unsigned long long srow[kSeqStageRows + 1];
    const uint64_t c0 = seq_plan_chunk_begin(blockIdx.x), c1 = seq_plan_chunk_end(blockIdx.x, a.total);
    if (threadIdx.x == 0) {
        rows[0] = seq_plan_row_at(a.row_off, 0, a.t.n_lines, c0);
        rows[1] = seq_plan_row_at(a.row_off, rows[0], a.t.n_lines, c1 - 1u) + 1u;
    }
    __syncthreads();
    const uint64_t r_lo = rows[0], n_rows = rows[1] - rows[0];   // the chunk's rows: [r_lo, r_lo + n_rows)
    if (n_rows <= kSeqStageRows) {
        for (uint32_t k = threadIdx.x; k <= (uint32_t)n_rows; k += 256u) srow[k] = a.row_off[r_lo + k];
        __syncthreads();
        seq_copy_units(a, srow, r_lo, n_rows, c0, c1);
    } else {
        seq_copy_units(a, a.row_off + r_lo, r_lo, n_rows, c0, c1);
    }
}

struct SeqJob {
    gams_seqset_t *s;
    const gams_index_t *ctg_ix;
    const gams_names_t *chr;
    const uint32_t *ctg_index;
    const int32_t *chr_start, *chr_end;
};

int locate_seq_run(gams_gpu_t *h, const SeqJob &J, const char *bytes, uint64_t n_bytes, const char **text, uint64_t *text_bytes,
                   uint64_t *n_rows) {
    const std::string who = "gpu_locate_seq_text";
    const uint64_t n_ctg = J.ctg_ix->m;
    *text = "";
    *text_bytes = 0;
    *n_rows = 0;
    if (!J.s->have_bytes)
        return gams_fail(h, GAMS_ESTATE, who + ": the seqset holds the G/C plane only: this call needs the sequence bytes");
    GAMS_HIP(h, hipSetDevice(h->device));
    GAMS_HIP(h, gams_stopwatch_reserve(h, SQ_STAGES));
    hipStream_t st = h->compute;
    const StageClock stage{h, st};
    // the per-ctg tables: one page-locked image, one copy, queued in front of the line index
    PoolBlock d_tab(h, false), pin(h, true), s1(h, false);
    const size_t n_tab = std::max<uint64_t>(n_ctg, 1);
    struct Tabs {
        unsigned long long *seq_off;
        int32_t *cs, *ce;
    };
    auto tabs = [&](Carver &c) {
        Tabs t{};
        t.seq_off = c.take<unsigned long long>(n_tab);
        t.cs = c.take<int32_t>(n_tab);
        t.ce = c.take<int32_t>(n_tab);
        return t;
    };
    const size_t b_tabs = layout_bytes(tabs);
    GAMS_TRY(h, who, pin.alloc(b_tabs));
    GAMS_TRY(h, who, d_tab.alloc(b_tabs));
    const Tabs ht = carve(pin.p, tabs), dt = carve(d_tab.p, tabs);
    for (uint64_t c = 0; c < n_ctg; ++c) {
        // a slot that does not hold the ctg is an error only where a line is located to the ctg: the lengths pass says so
        const uint32_t slot = J.ctg_index[c];
        ht.seq_off[c] = seq_slot_holds(J.s, slot, J.chr_start[c], J.chr_end[c]) ? J.s->off[slot] : ~0ull;
        ht.cs[c] = J.chr_start[c];
        ht.ce[c] = J.chr_end[c];
    }
    GAMS_TRY(h, who, hipMemcpyAsync(d_tab.p, pin.p, b_tabs, hipMemcpyHostToDevice, st));
    TextFront F(h);
    GAMS_TRY(h, who, stage(SQ_LINES, true));
    const int rc_front = text_front(h, who, bytes, n_bytes, F);
    if (rc_front != GAMS_OK) return rc_front;
    const uint32_t L = F.L;
    if (L == 0) return GAMS_OK;                                // (the stopwatch stays invalid, as text_front left it)
    gams_text_state *T = h->text;
    const uint32_t nbr = (L + 255u) / 256u;
    SeqTextArgs a{};
    unsigned long long *d_starts = nullptr, *d_fend = nullptr, *d_blk_off = nullptr;
    uint32_t *d_grp = nullptr, *d_qs = nullptr, *d_qe = nullptr;
    int64_t *d_hit = nullptr;
    auto cols = [&](Carver &c) {   // starts | grp qs qe | fend hit | src row_off | the blocks' bytes and prefix
        d_starts = c.take<unsigned long long>((size_t)F.nl + 2);
        d_grp = c.take<uint32_t>(L);
        d_qs = c.take<uint32_t>(L);
        d_qe = c.take<uint32_t>(L);
        d_fend = c.take<unsigned long long>(L);
        d_hit = c.take<int64_t>(L);
        a.src = c.take<unsigned long long>(L);
        a.row_off = c.take<unsigned long long>((size_t)L + 1);
        a.blk_bytes = c.take<unsigned long long>((size_t)nbr + 1);
        d_blk_off = c.take<unsigned long long>((size_t)nbr + 1);
    };
    GAMS_TRY(h, who, s1.alloc(layout_bytes(cols)));
    carve(s1.p, cols);
    hipLaunchKernelGGL(text_line_start_kernel, dim3(F.nbi), dim3(256), 0, st, T->d_in, n_bytes, F.n16, F.d_bnloff, F.nl, d_starts);
    GAMS_TRY(h, who, hipMemsetAsync(F.d_words + W_SEQ_LINE, 0xff, 8, st));
    GAMS_TRY(h, who, stage(SQ_LINES, false));
    a.t = TextLines{reinterpret_cast<const char *>(T->d_in), d_starts, F.nl, L};
    a.fend = d_fend;
    a.hit = d_hit;
    a.qs = d_qs;
    a.qe = d_qe;
    a.seq_off = dt.seq_off;
    a.cs = dt.cs;
    a.ce = dt.ce;
    a.blk_off = d_blk_off;
    a.words = F.d_words;
    a.seq = J.s->d_seq;
    GAMS_TRY(h, who, stage(SQ_PARSE, true));
    hipLaunchKernelGGL(text_parse_rg_kernel, dim3(nbr), dim3(256), 0, st, a.t, J.chr->t, d_grp, d_qs, d_qe, d_fend);
    GAMS_TRY(h, who, stage(SQ_PARSE, false));
    GAMS_TRY(h, who, stage(SQ_LOCATE, true));
    launch_interval_locate(J.ctg_ix, d_grp, d_qs, d_qe, L, d_hit, st);
    GAMS_TRY(h, who, stage(SQ_LOCATE, false));
    GAMS_TRY(h, who, stage(SQ_LENGTHS, true));
    hipLaunchKernelGGL(seq_row_len_kernel, dim3(nbr), dim3(256), 0, st, a);
    GAMS_TRY(h, who, stage(SQ_LENGTHS, false));
    GAMS_TRY(h, who, stage(SQ_OFFSETS, true));
    hipLaunchKernelGGL(blk_offsets_scan_kernel<unsigned long long>, dim3(1), dim3(1024), 0, st, a.blk_bytes, nbr, d_blk_off,
                       F.d_words, (uint32_t)W_BYTES);
    hipLaunchKernelGGL(seq_row_off_kernel, dim3(nbr), dim3(256), 0, st, a);
    GAMS_TRY(h, who, stage(SQ_OFFSETS, false));
    GAMS_TRY(h, who, read_words(h, F.d_words));
    const unsigned long long *w = h->pin_scratch;
    // an error word ends the call here: the copy kernel is never launched over rows the lengths pass refused
    if (w[W_EID])
        return gams_fail(h, GAMS_EINVAL, who + ": the range on 0-based line " + std::to_string(w[W_SEQ_LINE]) +
                                             " is not inside the ctg it is located to (the reference panics, locate.rs:133)");
    if (w[W_ENOSEQ])
        return gams_fail(h, GAMS_EINVAL, who + ": a located ctg has no slot of the seqset, or one of another length");
    const uint64_t tb = w[W_BYTES], rows = w[W_ROWS];
    if (tb == 0) return GAMS_OK;                               // no located line: nothing to copy, no stages to report
    if (seq_plan_chunks(tb) > 0x7fffffffull) return gams_fail(h, GAMS_EUNSUPPORTED, who + ": more text than one launch copies");
    GAMS_TRY(h, who, gams_pool_grow(h, true, &T->out[TEXT_SEQ], &T->out_cap[TEXT_SEQ], tb, tb));
    PoolBlock d_text(h, false);
    GAMS_TRY(h, who, d_text.alloc(tb));
    a.text = reinterpret_cast<char *>(d_text.p);
    a.total = tb;
    const int wrc = gams_seqset_read_begin(h, J.s);   // the copy reads the sequence bytes
    if (wrc != GAMS_OK) return wrc;
    GAMS_TRY(h, who, stage(SQ_COPY, true));
    hipLaunchKernelGGL(seq_copy_kernel, dim3((uint32_t)seq_plan_chunks(tb)), dim3(256), 0, st, a);
    GAMS_TRY(h, who, stage(SQ_COPY, false));
    GAMS_TRY(h, who, hipGetLastError());
    GAMS_TRY(h, who, hipMemcpyAsync(T->out[TEXT_SEQ], d_text.p, tb, hipMemcpyDeviceToHost, st));
    GAMS_TRY(h, who, hipStreamSynchronize(st));
    rg_timed(h, SQ_STAGES);
    *text = T->out[TEXT_SEQ];
    *text_bytes = tb;
    *n_rows = rows;
    return GAMS_OK;
}
// The rg index of a load (one file or several, the buckets by ctg): the gather into the builder's columns, then the build.
int rg_index_run(gams_gpu_t *h, const std::string &who, const gams_index_t *ctg_ix, const gams_names_t *chr_names, const RgInput &in,
                 gams_index_t **rg_ix, uint32_t *rg_group, uint64_t *n_kept) {
    *rg_ix = nullptr;
    *n_kept = 0;
    return rg_load(h, who, ctg_ix, RgPlain{chr_names->t}, in, true, [&](const RgCols &C, const StageClock &stage) -> int {
        uint32_t max_n = 0;
        for (uint64_t i = 0; i < C.n_ctg; ++i)
            max_n = std::max<uint32_t>(max_n, (uint32_t)(C.bucket_off[i + 1] - C.bucket_off[i]));
        IndexBuild B(h);
        const int rc = gams_index_build_begin(h, (uint32_t)C.n_ctg, C.n_kept, &B);
        if (rc != GAMS_OK) return rc;
        hipStream_t st = h->compute;
        hipError_t e = stage(RG_GATHER, true);
        if (C.n_kept) {
            RgGather g{};
            g.v = C.v;
            g.start = B.cols.starts_in;
            g.end = B.cols.stops_in;            // [start, end + 1) (redis.rs:291-294)
            g.line = nullptr;
            g.end_plus = 1;
            g.off32 = B.cols.off32;
            g.n_off = C.n_ctg + 1;
            const uint64_t lanes = std::max<uint64_t>(C.n_kept, g.n_off);
            hipLaunchKernelGGL(rg_gather_kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, st, g);
            if (e == hipSuccess) e = hipGetLastError();
        } else if (e == hipSuccess) {
            e = hipMemsetAsync(B.cols.off32, 0, (C.n_ctg + 1) * 4, st);   // every group empty
        }
        if (e == hipSuccess) e = stage(RG_GATHER, false);
        if (e == hipSuccess) e = stage(RG_BUILD, true);
        if (e != hipSuccess) return gams_index_build_fail(h, &B, e, "range text columns");
        // the stage's closing event goes in behind the builder's last kernel, before its host wait
        const int rb = gams_index_build_run(h, &B, max_n, rg_ix, h->kq[(size_t)RG_BUILD].second);
        if (rb != GAMS_OK) return rb;
        for (uint64_t i = 0; i < C.n_ctg; ++i) rg_group[i] = C.seen(i) ? (uint32_t)i : UINT32_MAX;
        *n_kept = C.n_kept;
        if (C.ran) rg_timed(h, RG_STAGES);
        return GAMS_OK;
    });
}
}  // namespace

extern "C" {

int gams_names_create(gams_gpu_t *h, uint32_t n, const char *const *names, gams_names_t **out) {
    if (!h || !out || (n && !names)) return gams_fail(h, GAMS_EINVAL, "names_create: null argument");
    if (n > 0x7fffffffu) return gams_fail(h, GAMS_EUNSUPPORTED, "names_create: more than 2^31 - 1 names");
    std::vector<unsigned long long> off((size_t)n + 1, 0);
    std::string bytes;
    std::unordered_set<std::string> seen;
    size_t max_len = 0;
    for (uint32_t i = 0; i < n; ++i) {
        if (!names[i]) return gams_fail(h, GAMS_EINVAL, "names_create: null name");
        const std::string s(names[i]);
        if (!seen.insert(s).second) return gams_fail(h, GAMS_EINVAL, "names_create: duplicate name '" + s + "'");
        bytes += s;
        off[i + 1] = bytes.size();
        max_len = std::max<size_t>(max_len, s.size());
    }
    uint32_t slots = 2;
    while (slots < 2ull * n) slots <<= 1;
    std::vector<NameSlot> tab(slots, NameSlot{0ull, UINT32_MAX, 0u});
    for (uint32_t i = 0; i < n; ++i) {
        const unsigned long long x = name_hash(bytes.data() + off[i], off[i + 1] - off[i]);
        uint32_t k = (uint32_t)x & (slots - 1u);
        while (tab[k].idx != UINT32_MAX) k = (k + 1u) & (slots - 1u);
        tab[k] = NameSlot{x, i, 0u};
    }
    GAMS_HIP(h, hipSetDevice(h->device));
    const size_t b_tab = gams_align256((size_t)slots * sizeof(NameSlot)), b_off = gams_align256(off.size() * 8),
                 b_bytes = gams_align256(bytes.size() + 1);
    gams_names_t *nm = new gams_names_t();
    hipError_t e = gams_pool_alloc(h, false, b_tab + b_off + b_bytes, reinterpret_cast<void **>(&nm->arena), &nm->arena_bytes);
    if (e == hipSuccess) e = hipMemcpy(nm->arena, tab.data(), tab.size() * sizeof(NameSlot), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(nm->arena + b_tab, off.data(), off.size() * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess && !bytes.empty()) e = hipMemcpy(nm->arena + b_tab + b_off, bytes.data(), bytes.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        gams_names_destroy(h, nm);
        return gams_fail(h, e == hipErrorOutOfMemory ? GAMS_ENOMEM : GAMS_EHIP, std::string("names_create: ") + hipGetErrorString(e));
    }
    nm->t.slot = reinterpret_cast<const NameSlot *>(nm->arena);
    nm->t.off = reinterpret_cast<const unsigned long long *>(nm->arena + b_tab);
    nm->t.bytes = reinterpret_cast<const char *>(nm->arena + b_tab + b_off);
    nm->t.mask = slots - 1u;
    nm->t.n = n;
    nm->max_len = (uint32_t)std::min<size_t>(max_len, UINT32_MAX);
    *out = nm;
    return GAMS_OK;
}

int gams_names_read(gams_gpu_t *h, const gams_names_t *nm, uint32_t *n, uint64_t *n_bytes, char *bytes, uint64_t *off) {
    if (!h || !nm || !n || !n_bytes) return gams_fail(h, GAMS_EINVAL, "names_read: null argument");
    GAMS_HIP(h, hipSetDevice(h->device));
    std::vector<unsigned long long> o((size_t)nm->t.n + 1);
    GAMS_HIP(h, hipMemcpy(o.data(), nm->t.off, o.size() * 8, hipMemcpyDeviceToHost));
    *n = nm->t.n;
    *n_bytes = o[nm->t.n];
    if (off) std::copy(o.begin(), o.end(), off);
    if (bytes && o[nm->t.n]) GAMS_HIP(h, hipMemcpy(bytes, nm->t.bytes, o[nm->t.n], hipMemcpyDeviceToHost));
    return GAMS_OK;
}

void gams_names_destroy(gams_gpu_t *h, gams_names_t *nm) {
    if (!nm) return;
    if (h) {
        (void)hipSetDevice(h->device);
        (void)hipStreamSynchronize(h->compute);
    }
    gams_pool_free(h, false, nm->arena, nm->arena_bytes);
    delete nm;
}

int gams_gpu_locate_text(gams_gpu_t *h, gams_index_t *ctg_ix, const gams_names_t *chr_names, const gams_names_t *ctg_ids,
                         const char *bytes, uint64_t n_bytes, const char **text, uint64_t *text_bytes, uint64_t *n_rows) {
    if (!h || !ctg_ix || !chr_names || !ctg_ids || (n_bytes && !bytes) || !text || !text_bytes || !n_rows)
        return gams_fail(h, GAMS_EINVAL, "gpu_locate_text: null argument");
    if (ctg_ids->t.n != ctg_ix->m) return gams_fail(h, GAMS_EINVAL, "gpu_locate_text: ctg_ids must name every interval of ctg_ix");
    TextJob j{};
    j.kind = K_LOCATE;
    j.ctg_ix = ctg_ix;
    j.chr = chr_names;
    j.ids = ctg_ids;
    return text_run(h, j, bytes, n_bytes, text, text_bytes, n_rows);
}

int gams_gpu_count_text(gams_gpu_t *h, gams_index_t *ctg_ix, const gams_names_t *chr_names, gams_index_t *rg_ix,
                        const uint32_t *rg_group, const char *bytes, uint64_t n_bytes, const char **text,
                        uint64_t *text_bytes, uint64_t *n_rows) {
    if (!h || !ctg_ix || !chr_names || !rg_ix || (ctg_ix->m && !rg_group) || (n_bytes && !bytes) || !text || !text_bytes ||
        !n_rows)
        return gams_fail(h, GAMS_EINVAL, "gpu_count_text: null argument");
    TextJob j{};
    j.kind = K_COUNT;
    j.ctg_ix = ctg_ix;
    j.rg_ix = rg_ix;
    j.chr = chr_names;
    j.rg_group = rg_group;
    return text_run(h, j, bytes, n_bytes, text, text_bytes, n_rows);
}

int gams_gpu_anno_text(gams_gpu_t *h, gams_spans_t *sp, const gams_names_t *chr_names, const gams_names_t *ctg_ids,
                       const int32_t *ctg_start, const int32_t *ctg_end, const char *bytes, uint64_t n_bytes, int header,
                       const char *prefix, uint32_t idx_id, uint32_t idx_range, const char **text, uint64_t *text_bytes,
                       uint64_t *n_rows) {
    if (!h || !sp || !chr_names || !ctg_ids || (ctg_ids->t.n && (!ctg_start || !ctg_end)) || (n_bytes && !bytes) || !text ||
        !text_bytes || !n_rows)
        return gams_fail(h, GAMS_EINVAL, "gpu_anno_text: null argument");
    TextJob j{};
    j.kind = K_ANNO;
    j.sp = sp;
    j.chr = chr_names;
    j.ids = ctg_ids;
    j.ctg_start = ctg_start;
    j.ctg_end = ctg_end;
    j.header = header;
    j.prefix = prefix;
    j.idx_id = idx_id;
    j.idx_range = idx_range;
    return text_run(h, j, bytes, n_bytes, text, text_bytes, n_rows);
}

int gams_gpu_read_range_text(gams_gpu_t *h, gams_index_t *ctg_ix, const gams_names_t *chr_names, const char *bytes,
                             uint64_t n_bytes, uint64_t *bucket_off, uint8_t *seen, int32_t *start, int32_t *end,
                             uint32_t *line, uint64_t cap, uint64_t *n_kept) {
    if (!h || !ctg_ix || !chr_names || (n_bytes && !bytes) || !bucket_off || !n_kept || (cap && (!start || !end || !line)))
        return gams_fail(h, GAMS_EINVAL, "gpu_read_range_text: null argument");
    const std::string who = "gpu_read_range_text";
    *n_kept = 0;
    return rg_load(h, who, ctg_ix, RgPlain{chr_names->t}, RgInput{bytes, n_bytes, nullptr, false}, cap != 0,
                   [&](const RgCols &C, const StageClock &stage) -> int {
        for (uint64_t i = 0; i <= C.n_ctg; ++i) bucket_off[i] = C.bucket_off[i];
        if (seen)
            for (uint64_t i = 0; i < C.n_ctg; ++i) seen[i] = C.first[i] != UINT32_MAX;
        *n_kept = C.n_kept;
        if (cap == 0 || C.n_kept == 0) {
            if (C.ran) rg_timed(h, cap ? RG_GATHER : RG_ORDER);
            return GAMS_OK;
        }
        if (cap < C.n_kept) return gams_fail(h, GAMS_EINVAL, who + ": cap is smaller than the kept ranges (*n_kept has them)");
        // the three columns on the device, one read-back into pooled page-locked memory, then the caller's arrays
        PoolBlock d_out(h, false), p_out(h, true);
        RgGather g{};
        g.v = C.v;
        auto three = [&](Carver &c) {
            g.start = c.take<uint32_t>(C.n_kept);
            g.end = c.take<uint32_t>(C.n_kept);
            g.line = c.take<uint32_t>(C.n_kept);
        };
        const size_t b_cols = layout_bytes(three);
        GAMS_TRY(h, who, d_out.alloc(b_cols));
        GAMS_TRY(h, who, p_out.alloc(b_cols));
        carve(p_out.p, three);
        const uint32_t *p_start = g.start, *p_end = g.end, *p_line = g.line;
        carve(d_out.p, three);
        g.end_plus = 0;
        hipStream_t st = h->compute;
        GAMS_TRY(h, who, stage(RG_GATHER, true));
        hipLaunchKernelGGL(rg_gather_kernel, dim3((unsigned)((C.n_kept + 255) / 256)), dim3(256), 0, st, g);
        GAMS_TRY(h, who, hipGetLastError());
        GAMS_TRY(h, who, stage(RG_GATHER, false));
        GAMS_TRY(h, who, hipMemcpyAsync(p_out.p, d_out.p, b_cols, hipMemcpyDeviceToHost, st));
        GAMS_TRY(h, who, hipStreamSynchronize(st));
        memcpy(start, p_start, C.n_kept * 4);
        memcpy(end, p_end, C.n_kept * 4);
        memcpy(line, p_line, C.n_kept * 4);
        rg_timed(h, RG_GATHER + 1);
        return GAMS_OK;
    });
}

int gams_index_create_range_text(gams_gpu_t *h, gams_index_t *ctg_ix, const gams_names_t *chr_names, const char *bytes,
                                 uint64_t n_bytes, gams_index_t **rg_ix, uint32_t *rg_group, uint64_t *n_kept) {
    if (!h || !ctg_ix || !chr_names || (n_bytes && !bytes) || !rg_ix || (ctg_ix->m && !rg_group) || !n_kept)
        return gams_fail(h, GAMS_EINVAL, "index_create_range_text: null argument");
    return rg_index_run(h, "index_create_range_text", ctg_ix, chr_names, RgInput{bytes, n_bytes, nullptr, false}, rg_ix, rg_group, n_kept);
}

int gams_index_create_range_files(gams_gpu_t *h, gams_index_t *ctg_ix, const gams_names_t *chr_names, uint32_t n_files,
                                  const char *const *bytes, const uint64_t *n_bytes, gams_index_t **rg_ix, uint32_t *rg_group,
                                  uint64_t *n_kept) {
    if (!h || !ctg_ix || !chr_names || (n_files && (!bytes || !n_bytes)) || !rg_ix || (ctg_ix->m && !rg_group) || !n_kept)
        return gams_fail(h, GAMS_EINVAL, "index_create_range_files: null argument");
    for (uint32_t f = 0; f < n_files; ++f)
        if (n_bytes[f] && !bytes[f]) return gams_fail(h, GAMS_EINVAL, "index_create_range_files: null argument");
    const TextFiles files{n_files, bytes, n_bytes};
    return rg_index_run(h, "index_create_range_files", ctg_ix, chr_names, RgInput{nullptr, 0, &files, false}, rg_ix, rg_group, n_kept);
}

int gams_gpu_loader_text(gams_gpu_t *h, gams_index_t *ctg_ix, const gams_names_t *chr_names, const gams_names_t *ctg_ids,
                         uint32_t n_files, const char *const *bytes, const uint64_t *n_bytes, int kind, const char *tag,
                         uint64_t tag_bytes, int format, const int32_t *serial_base, const char **text, uint64_t *text_bytes,
                         uint64_t *text_off, int32_t *serial_next, uint64_t *n_in_file, uint64_t *n_rows) {
    if (!h || !ctg_ix || !chr_names || !ctg_ids || (n_files && (!bytes || !n_bytes)) || !text || !text_bytes || !text_off || !n_rows)
        return gams_fail(h, GAMS_EINVAL, "gpu_loader_text: null argument");
    for (uint32_t f = 0; f < n_files; ++f)
        if (n_bytes[f] && !bytes[f]) return gams_fail(h, GAMS_EINVAL, "gpu_loader_text: null argument");
    if (kind != GAMS_LOADER_RG && kind != GAMS_LOADER_FEATURE) return gams_fail(h, GAMS_EINVAL, "gpu_loader_text: unknown kind");
    if (format != GAMS_LOADER_RECORDS && format != GAMS_LOADER_TSV && format != GAMS_LOADER_RESP)
        return gams_fail(h, GAMS_EINVAL, "gpu_loader_text: unknown format");
    if (ctg_ids->t.n != ctg_ix->m) return gams_fail(h, GAMS_EINVAL, "gpu_loader_text: ctg_ids must name every interval of ctg_ix");
    if (kind != GAMS_LOADER_FEATURE) tag_bytes = 0;
    if (tag_bytes && !tag) return gams_fail(h, GAMS_EINVAL, "gpu_loader_text: null argument");
    if ((uint64_t)n_files * ctg_ix->m > kRgMaxFileCtg)     // (before text_off, which has an entry per pair, is touched)
        return gams_fail(h, GAMS_EUNSUPPORTED, "gpu_loader_text: more than 2^24 (file, ctg) pairs (use the host path)");
    if (tag_bytes >= kRecMaxField) return gams_fail(h, GAMS_EUNSUPPORTED, "gpu_loader_text: a tag of 2^30 bytes or more (use the host path)");
    for (uint64_t k = 0; k < tag_bytes; ++k)
        if ((uint8_t)tag[k] < 0x20u || (uint8_t)tag[k] >= 0x80u)
            return gams_fail(h, GAMS_EUNSUPPORTED, "gpu_loader_text: the tag holds a control byte or a byte >= 0x80 (use the host path)");
    return loader_text_run(h, RecJob{ctg_ix, chr_names, ctg_ids, TextFiles{n_files, bytes, n_bytes}, kind, format, tag, tag_bytes, serial_base},
                           text, text_bytes, text_off, serial_next, n_in_file, n_rows);
}

int gams_gpu_peak_text(gams_gpu_t *h, gams_seqset_t *s, gams_index_t *ctg_ix, const gams_names_t *chr_names,
                       const gams_names_t *ctg_ids, const uint32_t *ctg_index, const int32_t *chr_start, const int32_t *chr_end,
                       const char *bytes, uint64_t n_bytes, const char **text, uint64_t *text_bytes, uint64_t *text_off,
                       uint64_t *n_rows) {
    if (!h || !s || !ctg_ix || !chr_names || !ctg_ids || (ctg_ix->m && (!ctg_index || !chr_start || !chr_end)) ||
        (n_bytes && !bytes) || !text || !text_bytes || !text_off || !n_rows)
        return gams_fail(h, GAMS_EINVAL, "gpu_peak_text: null argument");
    if (ctg_ids->t.n != ctg_ix->m) return gams_fail(h, GAMS_EINVAL, "gpu_peak_text: ctg_ids must name every interval of ctg_ix");
    return peak_run(h, PeakJob{s, ctg_ix, chr_names, ctg_ids, ctg_index, chr_start, chr_end}, nullptr, bytes, n_bytes, text, text_bytes,
                    text_off, n_rows);
}

int gams_gpu_peak_records_text(gams_gpu_t *h, gams_seqset_t *s, gams_index_t *ctg_ix, const gams_names_t *chr_names,
                               const gams_names_t *ctg_ids, const uint32_t *ctg_index, const int32_t *chr_start,
                               const int32_t *chr_end, const char *bytes, uint64_t n_bytes, int format, const int32_t *serial_base,
                               const char **text, uint64_t *text_bytes, uint64_t *text_off, int32_t *serial_next, uint64_t *n_rows) {
    if (!h || !s || !ctg_ix || !chr_names || !ctg_ids || (ctg_ix->m && (!ctg_index || !chr_start || !chr_end)) ||
        (n_bytes && !bytes) || !text || !text_bytes || !text_off || !n_rows)
        return gams_fail(h, GAMS_EINVAL, "gpu_peak_records_text: null argument");
    if (format != GAMS_LOADER_RECORDS && format != GAMS_LOADER_TSV && format != GAMS_LOADER_RESP)
        return gams_fail(h, GAMS_EINVAL, "gpu_peak_records_text: unknown format");
    if (ctg_ids->t.n != ctg_ix->m)
        return gams_fail(h, GAMS_EINVAL, "gpu_peak_records_text: ctg_ids must name every interval of ctg_ix");
    const PeakRecJob R{format, serial_base, serial_next};
    return peak_run(h, PeakJob{s, ctg_ix, chr_names, ctg_ids, ctg_index, chr_start, chr_end}, &R, bytes, n_bytes, text, text_bytes,
                    text_off, n_rows);
}

int gams_gpu_sw_feature_text(gams_gpu_t *h, gams_seqset_t *s, gams_index_t *ctg_ix, const gams_names_t *chr_names,
                             const gams_names_t *ctg_ids, const uint32_t *ctg_index, const int32_t *chr_start,
                             const int32_t *chr_end, const char *bytes, uint64_t n_bytes, int32_t size, int32_t max,
                             int32_t resize, uint32_t actions, gams_index_t *rg_ix, const uint32_t *rg_group,
                             const char **text, uint64_t *text_bytes, uint64_t *text_off, uint64_t *n_features,
                             uint64_t *n_rows) {
    if (!h || !ctg_ix || !chr_names || !ctg_ids || (ctg_ix->m && (!chr_start || !chr_end)) || (n_bytes && !bytes) || !text ||
        !text_bytes || !text_off || !n_features || !n_rows)
        return gams_fail(h, GAMS_EINVAL, "gpu_sw_feature_text: null argument");
    SwCall c(size, max, resize, actions, rg_ix, rg_group);
    return sw_feature_checked(h, "gpu_sw_feature_text", SwFeatJob{c, s, ctg_ix, chr_names, ctg_ids, ctg_index, chr_start, chr_end}, bytes,
                              n_bytes, text, text_bytes, text_off, n_features, n_rows);
}

int gams_gpu_sw_feature_summary_anno(gams_gpu_t *h, gams_seqset_t *s, gams_index_t *ctg_ix, const gams_names_t *chr_names,
                                const gams_names_t *ctg_ids, const uint32_t *ctg_index, const int32_t *chr_start,
                                const int32_t *chr_end, const char *bytes, uint64_t n_bytes, int32_t size, int32_t max,
                                int32_t resize, uint32_t actions, gams_index_t *rg_ix, const uint32_t *rg_group,
                                gams_sw_summary_t *sum, uint32_t tag, uint32_t n_anno, gams_spans_t *const *sets,
                                const uint32_t *const *set_group, uint64_t *n_features, uint64_t *n_rows) {
    if (!h || !ctg_ix || !chr_names || !ctg_ids || (ctg_ix->m && (!chr_start || !chr_end)) || (n_bytes && !bytes) || !sum ||
        !n_features || !n_rows)
        return gams_fail(h, GAMS_EINVAL, "gpu_sw_feature_summary: null argument");
    SwCall c(size, max, resize, actions, rg_ix, rg_group);
    c.summary = sum;
    c.tag = tag;
    c.n_anno = n_anno;
    c.sets = sets;
    c.set_group = set_group;
    return sw_feature_checked(h, "gpu_sw_feature_summary", SwFeatJob{c, s, ctg_ix, chr_names, ctg_ids, ctg_index, chr_start, chr_end},
                              bytes, n_bytes, nullptr, nullptr, nullptr, n_features, n_rows);
}

int gams_gpu_sw_feature_summary(gams_gpu_t *h, gams_seqset_t *s, gams_index_t *ctg_ix, const gams_names_t *chr_names,
                                const gams_names_t *ctg_ids, const uint32_t *ctg_index, const int32_t *chr_start,
                                const int32_t *chr_end, const char *bytes, uint64_t n_bytes, int32_t size, int32_t max,
                                int32_t resize, uint32_t actions, gams_index_t *rg_ix, const uint32_t *rg_group,
                                gams_sw_summary_t *sum, uint32_t tag, uint64_t *n_features, uint64_t *n_rows) {
    return gams_gpu_sw_feature_summary_anno(h, s, ctg_ix, chr_names, ctg_ids, ctg_index, chr_start, chr_end, bytes, n_bytes, size,
                                            max, resize, actions, rg_ix, rg_group, sum, tag, 0u, nullptr, nullptr, n_features,
                                            n_rows);
}

int gams_gpu_locate_seq_text(gams_gpu_t *h, gams_seqset_t *s, gams_index_t *ctg_ix, const gams_names_t *chr_names,
                             const uint32_t *ctg_index, const int32_t *chr_start, const int32_t *chr_end, const char *bytes,
                             uint64_t n_bytes, const char **text, uint64_t *text_bytes, uint64_t *n_rows) {
    if (!h || !s || !ctg_ix || !chr_names || (ctg_ix->m && (!ctg_index || !chr_start || !chr_end)) || (n_bytes && !bytes) ||
        !text || !text_bytes || !n_rows)
        return gams_fail(h, GAMS_EINVAL, "gpu_locate_seq_text: null argument");
    return locate_seq_run(h, SeqJob{s, ctg_ix, chr_names, ctg_index, chr_start, chr_end}, bytes, n_bytes, text, text_bytes, n_rows);
}

uint32_t gams_gpu_locate_seq_chunk(void) { return kSeqTextChunk; }

}  // extern "C"
