"""Builders and the case battery for the edges of `gams peak` on the device (gams_gpu_peak_text, gams_amd/csrc/text.hip):
the row writer at its LDS stage limit and at every kind of 16-byte misalignment, buckets that begin and end on the seams
of the 256-row blocks, the (ctg, start, line) sort key at its ties, its high start bits and its 64-bit limit, the device
formatters over the gc and amplitude domain, more row blocks than the offsets scan has threads, and the line edges of the
parser.  test_peak_edges_cpu.py proves on the CPU that every case carries what it is built for;
test_gpu_peak_edges.py holds the device to the model on them, byte for byte.

The expected text is always made of peak_text.buckets and peak_text.ctg_rows, the two halves of peak_text.model (the CPU
test holds the two to each other on every case).  A "row block" is 256 consecutive kept rows in output order: the ctgs in
the Locator's order, by start inside a ctg, by line inside a start.  Nothing here imports the GPU package."""
import functools

import numpy as np

import helpers
import peak_text as pt
from test_rg_text_cpu import locator_order, rust_lines

ROW_BLOCK = 256          # rows per workgroup of peak_row_len_kernel / peak_row_write_kernel
STAGE = 32_768           # kPeakStage: a block of at most this many bytes is composed in LDS
SCAN_THREADS = 1024      # threads of blk_offsets_scan_kernel: beyond that many entries a thread takes several
NONE = 0xffffffff


def ctg(cid, chr_id, start, seq):
    """a ctg dict; `seq`: bytes / array of bases, or an int: that many bases and none of them at hand (a ctg that gets
    no slot in the seqset and must not have kept peaks)"""
    if isinstance(seq, int):
        return dict(id=cid, chr_id=chr_id, chr_start=start, chr_end=start + seq - 1, seq=b"")
    seq = seq.tobytes() if isinstance(seq, np.ndarray) else bytes(seq)
    return dict(id=cid, chr_id=chr_id, chr_start=start, chr_end=start + len(seq) - 1, seq=seq)


def key_bits(n_lines, n_ctg):
    """(line_bits, ctg_bits) as peak_run computes them: the bits of the last line number and of n_ctg itself (the key
    of a line that is not kept carries n_ctg), each at least 1; the key has ctg_bits + 31 + line_bits bits"""
    return max(1, (n_lines - 1).bit_length()), max(1, n_ctg.bit_length())


class Expected:
    """what the model says of one case: the ctgs in the Locator's order, their kept peaks, their rows"""

    def __init__(self, ctgs, data):
        self.located, kept = pt.buckets(ctgs, data)
        at = {c["id"]: i for i, c in enumerate(ctgs)}
        self.order = locator_order(ctgs)
        self.kept = [kept[at[c["id"]]] for c in self.order]
        self.n_located = [self.located[at[c["id"]]] for c in self.order]
        self.rows = []                                            # per ctg: its rows, each with its newline
        for c, pk in zip(self.order, self.kept):
            text = pt.ctg_rows(c, pk).encode("latin-1") if pk else b""
            self.rows.append([r + b"\n" for r in text.split(b"\n")[:-1]])
            assert len(self.rows[-1]) == len(pk)
        self.parts = [b"".join(r) for r in self.rows]             # what text_off slices
        self.text = b"".join(self.parts)                          # the entry's text: the Locator's order
        ids = sorted(range(len(self.order)), key=lambda i: self.order[i]["id"].encode())
        self.by_id = b"".join(self.parts[i] for i in ids)         # host.peak_text's and peak_text.model's order
        self.n_kept = sum(len(r) for r in self.rows)
        self.bucket_off = np.concatenate(([0], np.cumsum([len(r) for r in self.rows]))).astype(np.int64)
        self.text_off = np.concatenate(([0], np.cumsum([len(p) for p in self.parts]))).astype(np.int64)
        self.row_len = np.array([len(r) for rows in self.rows for r in rows], np.int64)

    def fields(self):
        """every row split at its tabs, in output order"""
        return [r[:-1].decode("latin-1").split("\t") for rows in self.rows for r in rows]

    def block_totals(self):
        if self.row_len.size == 0:
            return np.zeros(0, np.int64)
        return np.add.reduceat(self.row_len, np.arange(0, self.row_len.size, ROW_BLOCK))

    def block_starts(self):
        t = self.block_totals()
        return np.concatenate(([0], np.cumsum(t)[:-1])).astype(np.int64) if t.size else t


def join_lines(lines):
    return ("\n".join(lines) + "\n").encode("latin-1")


# ---- 1. the stage limit and its alignment --------------------------------------------------------------------------
def _stage_lines(ctgs, n_first, n, plen):
    """a sacrificial line per ctg, then n position-sorted peaks (the first n_first in ctgs[0]) with signals 1 / -1; line
    j carries a "name." prefix of plen[j] bytes (0: none)"""
    lines = ["#range\tgc_content\tsignal"]
    lines += ["%s:%d-%d\t0.5\t1" % (c["chr_id"], c["chr_start"] + 2, c["chr_start"] + 5) for c in ctgs]
    for j in range(n):
        c, k = (ctgs[0], j) if j < n_first else (ctgs[1], j - n_first)
        s = c["chr_start"] + 10 + 12 * k
        head = ("n" * (int(plen[j]) - 1) + ".") if plen[j] else ""
        lines.append("%s%s:%d-%d\t0.5\t%s" % (head, c["chr_id"], s, s + 7 + j % 3, "1" if j % 2 == 0 else "-1"))
    return lines


def stage_case(targets, tail, n_first):
    """Two ctgs and the bytes of a TSV whose row blocks total what `targets` names: targets[b] is the byte total of row
    block b (without prefixes it is about 17 KB), `tail` rows follow in a last partial block, and the first n_first rows
    lie in the first ctg.  A row's length hangs on its own fields and its neighbours' signals; the "name." prefix of a line
    is printed in that line's row only, so a block is brought to its total with the prefixes of its lines: the lengths
    are taken from the model's rows without prefixes, and the difference is spread over the block's lines (every
    prefix at least 2 bytes: a name and its dot)."""
    n = ROW_BLOCK * len(targets) + tail
    n_first = min(n_first, n)
    seq_len = 12 * max(n_first, n - n_first) + 100
    ctgs = [ctg("ctg:I:1", "I", 1, helpers.synth(seq_len, 101)), ctg("ctg:II:1", "II", 1001, helpers.synth(seq_len, 102))]
    plen = np.zeros(n, np.int64)
    base = Expected(ctgs, join_lines(_stage_lines(ctgs, n_first, n, plen))).block_totals()
    for b, want in enumerate(targets):
        d = int(want - base[b])
        assert d >= 2 * ROW_BLOCK, (b, want, int(base[b]))
        plen[b * ROW_BLOCK:(b + 1) * ROW_BLOCK] = d // ROW_BLOCK
        plen[b * ROW_BLOCK] += d % ROW_BLOCK
    return dict(ctgs=ctgs, data=join_lines(_stage_lines(ctgs, n_first, n, plen)))


# name -> (targets, tail, n_first).  The block in front sets blk0 % 16 of the block under test (20,000 = 0 mod 16); a
# block of 40,000 bytes gives every case but the single-block ones a block that is not staged.
STAGE_CASES = {
    "exact_r0": ([20_000, STAGE, 40_000], 100, 300),
    "exact_r15": ([20_015, STAGE, 40_000], 100, 300),
    "exact_r7": ([20_007, STAGE, 40_000], 33, 700),
    "over_r0": ([20_000, STAGE + 1], 100, 300),
    "over_r15": ([20_015, STAGE + 1], 1, 256),
    "under_r0": ([20_000, STAGE - 18, 40_000], 100, 300),
    "under_r15": ([20_015, STAGE - 18, 40_000], 100, 520),
    "under_r9": ([20_009, STAGE - 63, 40_000], 255, 300),
    "alternate": ([24_003, 40_000, STAGE, STAGE + 1], 77, 600),      # staged, not, staged, not, a partial block
    "single_exact": ([STAGE], 0, 100),
    "single_over": ([STAGE + 1], 0, 100),
}
STAGE_SINGLE = ("single_exact", "single_over")


# ---- 2. bucket and block seams --------------------------------------------------------------------------------------
SEAM_LAYOUT = [("ctg:I:1", "I", 1, 4000), ("ctg:I:2", "I", 4101, 4000), ("ctg:II:1", "II", 1001, 4000),
               ("ctg:II:2", "II", 5001, 4000), ("ctg:III:1", "III", 1, 4000)]       # the Locator's order


def seam_case(located, shuffle, seed=3):
    """Five ctgs of 4 kb; ctg i has located[i] located lines, so located[i] - 1 kept rows (1: an empty bucket, 0: no
    bucket).  The first located line of every ctg, the one the reference drops, stands in front; the others follow
    sorted by position or shuffled.  A bucket of two kept rows or more holds a peak that starts on chr_start (not a
    point range: that one is not located), one of three or more a peak that ends on chr_end; the rest are up to 300
    bases long at random places, so neighbours overlap and wave lengths turn negative.  In front of every ctg's lines
    stands the point range on its chr_start, which the half-open lookup does not locate."""
    rng = np.random.default_rng(seed)
    ctgs = [ctg(cid, ch, s, helpers.synth(n, 110 + k)) for k, (cid, ch, s, n) in enumerate(SEAM_LAYOUT)]
    head, body = [], []
    for c, m in zip(ctgs, located):
        cs, ce = c["chr_start"], c["chr_end"]
        head.append("%s:%d\t0.5\t1" % (c["chr_id"], cs))                # the point range on chr_start: not located
        if m == 0:
            continue
        head.append("%s:%d-%d\t0.5\t1" % (c["chr_id"], cs + 50, cs + 60))
        kept = []
        if m - 1 >= 2:
            kept.append((cs, cs + int(rng.integers(1, 200))))
        if m - 1 >= 3:
            kept.append((ce - int(rng.integers(0, 200)), ce))
        while len(kept) < m - 1:
            s = int(rng.integers(cs + 1, ce - 300))
            kept.append((s, s + int(rng.integers(0, 300))))
        for j, (s, e) in enumerate(sorted(kept)):
            rg = "%s:%d" % (c["chr_id"], s) if e == s else "%s:%d-%d" % (c["chr_id"], s, e)
            body.append("%s\t0.5\t%s" % (rg, ("1", "-1", "", "s%d" % j)[j % 4]))
    if shuffle:
        rng.shuffle(body)
    return dict(ctgs=ctgs, data=join_lines(["#range\tgc_content\tsignal"] + head + body))


# name -> located lines per ctg; the kept rows are one fewer.  n513: bucket 0 is rows 0..254, bucket 1 is ONE row on slot
# 255, then an empty bucket and a ctg without lines, and bucket 4 begins on slot 0 of block 1 and ends on slot 0 of
# block 2.  n512: bucket 0 ends on slot 255, bucket 1 is one row on slot 0.
SEAM_LOCATED = {
    "n513": [256, 2, 1, 0, 258],
    "n512": [257, 2, 1, 0, 256],
    "n1": [0, 2, 1, 0, 0],
    "n255": [101, 1, 156, 0, 0],
    "n256": [2, 256, 0, 1, 0],
    "n257": [257, 1, 2, 0, 0],
}
SEAM_TOTALS = {"n513": 513, "n512": 512, "n1": 1, "n255": 255, "n256": 256, "n257": 257}
SEAM_CASES = {"%s_%s" % (k, v): (k, v == "shuffled") for k in SEAM_LOCATED for v in ("sorted", "shuffled")}


# ---- 3. the sort key --------------------------------------------------------------------------------------------------
TIE_RUN = 300
TIE_A, TIE_B = 15_000, 20_000          # the starts of the scattered and of the adjacent run


def ties_case():
    """One ctg of 30 kb (and a small second one): 500 peaks at random places, a run of 300 lines that all start at 15,000
    with 300 ends and 300 signals, scattered through the shuffled file, and a run of 300 that start at 20,000 and stand
    next to each other in the file.  A row prints its neighbours' signals, so the order inside a run shows in the text."""
    rng = np.random.default_rng(5)
    ctgs = [ctg("ctg:I:1", "I", 1, helpers.synth(30_000, 120)), ctg("ctg:II:1", "II", 1, helpers.synth(2000, 121))]
    body = []
    for k in range(500):
        s = int(rng.integers(2, 29_000))
        if s in (TIE_A, TIE_B):
            s += 1
        body.append("I:%d-%d\t0.5\t%s" % (s, s + int(rng.integers(1, 300)), "1" if k % 2 else "-1"))
    body += ["I:%d-%d\t0.5\ta%d" % (TIE_A, TIE_A + 299 - j, j) if j != 299 else "I:%d\t0.5\ta%d" % (TIE_A, j)
             for j in range(TIE_RUN)]                                      # the longer ranges first; the last one a point
    body += ["II:%d-%d\t0.5\t1" % (10 * k + 1, 10 * k + 30) for k in range(1, 20)]
    rng.shuffle(body)
    at = int(rng.integers(100, len(body) - 100))
    body[at:at] = ["I:%d-%d\t0.5\tb%d" % (TIE_B, TIE_B + 1 + (7 * j) % TIE_RUN, j) for j in range(TIE_RUN)]
    head = ["#range\tgc_content\tsignal", "I:100-200\t0.5\t1", "II:5-9\t0.5\t1"]
    return dict(ctgs=ctgs, data=join_lines(head + body))


INT32_MAX = 2_147_483_647


def high_case():
    """A ctg that ends on 2,147,483,647 (40 kb of sequence) beside one at coordinate 1: every start there has bits 30 and
    29 set, the ranges print with ten digits, and both wave lengths are computed at the top of the range -- a peak on
    chr_start, one that ends on chr_end, the point range on chr_end itself."""
    rng = np.random.default_rng(6)
    n = 40_000
    ctgs = [ctg("ctg:I:1", "I", 1, helpers.synth(20_000, 122)),
            ctg("ctg:H:1", "H", INT32_MAX - n + 1, helpers.synth(n, 123))]
    cs, ce = ctgs[1]["chr_start"], ctgs[1]["chr_end"]
    body = ["H:%d-%d\t0.5\t1" % (cs, cs + 100), "H:%d-%d\t0.5\t-1" % (ce - 50, ce), "H:%d\t0.5\t1" % ce]
    for k in range(300):
        s = int(rng.integers(cs + 1, ce - 400))
        body.append("H:%d-%d\t0.5\t%s" % (s, s + int(rng.integers(0, 300)), "1" if k % 2 else "-1"))
        s = int(rng.integers(2, 19_000))
        body.append("I:%d-%d\t0.5\t%s" % (s, s + int(rng.integers(0, 300)), "1" if k % 2 else "-1"))
    rng.shuffle(body)
    head = ["#range\tgc_content\tsignal", "H:%d-%d\t0.5\t1" % (cs + 7, cs + 9), "I:100-200\t0.5\t1"]
    return dict(ctgs=ctgs, data=join_lines(head + body))


WIDTH_LINES = 65_537


def width_ctg_counts():
    """the ctg counts that make the key 64 and 65 bits wide with WIDTH_LINES lines"""
    line_bits, _ = key_bits(WIDTH_LINES, 1)
    n64 = (1 << (64 - 31 - line_bits)) - 1              # the most ctgs whose count has 64 - 31 - line_bits bits
    return n64, n64 + 1


def width_case(n_ctg):
    """65,537 lines, all but 245 of them comments, over n_ctg ctgs: one on chromosome A (the first in the Locator's
    order), n_ctg - 2 of ten bases each on chromosome M, one on chromosome Z (the last).  Only A, the middle one of M and
    Z have a sequence (slots 0, 1, 2) and kept peaks; every other ctg passes no slot.  The ids sort otherwise than the
    Locator orders the ctgs: "ctg:a:1" of chromosome A behind all others, "ctg:M:10" before "ctg:M:2"."""
    rng = np.random.default_rng(7)
    mid = n_ctg // 2
    ctgs = [ctg("ctg:a:1", "A", 1, helpers.synth(5000, 124))]
    for k in range(1, n_ctg - 1):
        ctgs.append(ctg("ctg:M:%d" % k, "M", 10 * k + 1, b"GGCCAATTGC" if k == mid else 10))
    ctgs.append(ctg("ctg:Z:1", "Z", 1, helpers.synth(5000, 125)))
    slot = 0
    for c in ctgs:
        c["slot"] = None
        if c["seq"]:
            c["slot"], slot = slot, slot + 1
    peaks = ["A:100-200\t0.5\t1", "M:%d-%d\t0.5\t1" % (10 * mid + 2, 10 * mid + 3), "Z:100-200\t0.5\t1"]     # dropped
    for k in range(118):
        for ch in "AZ":
            s = int(rng.integers(2, 4600))
            peaks.append("%s:%d-%d\t0.5\t%s" % (ch, s, s + int(rng.integers(0, 300)), "1" if k % 2 else "-1"))
    peaks += ["M:%d-%d\t0.5\t-1" % (10 * mid + a, 10 * mid + b) for a, b in ((2, 9), (1, 10), (5, 5), (3, 4), (7, 10))]
    peaks.append("M:%d-%d\t0.5\t1" % (10 * (mid + 1) + 2, 10 * (mid + 1) + 4))       # one located line: no row
    lines = ["#c"] * WIDTH_LINES
    where = np.sort(rng.choice(np.arange(1, WIDTH_LINES), len(peaks), replace=False))
    where[-1] = WIDTH_LINES - 1                          # the last line is a kept peak: the highest line number
    order = [0, 1, 2] + (3 + rng.permutation(len(peaks) - 3)).tolist()
    for w, k in zip(where, order):
        lines[int(w)] = peaks[k]
    return dict(ctgs=ctgs, data=join_lines(lines), n_peaks=len(peaks))


# ---- 4. the device formatters over their domain -------------------------------------------------------------------------
FMT_HALF = 10_000


def fmt_case():
    """One ctg of G x 10,000 then A x 10,000 at 1.  The range [s, s + 9999] has gc (10001 - s) / 10^4: s = 1 .. 10001
    prints every m / 10^4 through sw_put_f4, in the order of the file (line s + 1).  A range [s, e] with s <= 10000 < e
    has gc (10001 - s) / (e - s + 1); such lines stand behind the series in the file, so that after the sort they lie
    between the series' rows of start s and s + 1 (ties keep the file's order), and the amplitudes are the f32
    differences of pairs (i / 10^4, j / 10^4) far apart: at random over the band a start can reach, and aimed at
    2^-k above and below a series value for k = 1 .. 10."""
    rng = np.random.default_rng(8)
    h = FMT_HALF
    c = ctg("ctg:I:1", "I", 1, b"G" * h + b"A" * h)
    lines = ["#range\tgc_content\tsignal", "I:3-4\t0\t1"]                 # the sacrificial first located line
    lines += ["I:%d-%d\t0\t%s" % (s, s + h - 1, "1" if s % 2 else "-1") for s in range(1, h + 2)]
    extra = []

    def aimed(s, want):
        """a range from s whose gc is as near `want` as a length allows, if one inside the ctg does"""
        g = h + 1 - s
        if want <= 0:
            return
        ln = int(round(g / want))
        if g < ln <= 2 * h + 1 - s:
            extra.append("I:%d-%d\t0\t-1" % (s, s + ln - 1))

    for s in rng.integers(1, h + 1, 4000).tolist():
        g = h + 1 - s
        aimed(s, rng.uniform(g / (g + h), 1.0))
    for k in range(1, 11):
        for s in rng.integers(1, h + 1, 120).tolist():
            g = h + 1 - s                                                   # the series: g / 10^4 at s, (g - 1) / 10^4 next
            for base in (g, g - 1):
                for sign in (1, -1):
                    aimed(s, base / 1e4 + sign * 2.0 ** -k)
    rng.shuffle(extra)
    # Behind everything else, so the last of their starts: pairs from one start at the two ends of the band it reaches
    # (amplitudes above 0.5), and the last G alone, in front of the all-A range of the series (|1 - 0|).
    for s in range(5001, 9001, 40):
        g = h + 1 - s
        aimed(s, g / (g + h) + 0.004)
        aimed(s, 0.998)
    # Few f32 differences need 9 significant digits: those whose 8-digit decimals lie further apart than the floats, as
    # in [0.1, 0.125) and [0.01, 0.015625).  Pairs from one start with such a difference are drawn at random, and those
    # kept whose difference, as the input predicts it, prints with 9 and has not been seen.
    n_try = 400_000
    gs = rng.integers(1, h + 1, n_try)
    l1 = gs + rng.integers(1, h + 1, n_try)
    d = np.where(rng.random(n_try) < 0.5, rng.uniform(0.1, 0.125, n_try), rng.uniform(0.01, 0.015625, n_try))
    lo = gs / l1 - d
    l2 = np.rint(gs / np.where(lo > 0, lo, 1.0)).astype(np.int64)
    ok = (lo > 0) & (l2 > gs) & (l2 <= gs + h)
    q = np.float32(1e4)
    v = np.abs(np.rint(gs / l1 * 1e4).astype(np.float32) / q - np.rint(gs / l2 * 1e4).astype(np.float32) / q)
    with np.errstate(divide="ignore"):
        unit = 10.0 ** (np.floor(np.log10(v.astype(np.float64))) - 7)          # the last of 8 significant digits
    ok &= (v > 0) & ((np.rint(v / unit) * unit).astype(np.float32) != v)        # 8 digits do not give the float back
    nine = set()
    for g, a, b, x in zip(gs[ok].tolist(), l1[ok].tolist(), l2[ok].tolist(), v[ok].tolist()):
        if len(nine) >= 1000 or x in nine:
            continue
        if pt.sig_digits(np.format_float_positional(np.float32(x), unique=True, trim="-")) == 9:
            nine.add(x)
            s = h + 1 - g
            extra += ["I:%d-%d\t0\t1" % (s, s + a - 1), "I:%d-%d\t0\t-1" % (s, s + b - 1)]
    extra.append("I:%d\t0\t1" % h)
    return dict(ctgs=[c], data=join_lines(lines + extra))


def amplitude_pairs(fields):
    """per row of ONE ctg (fields: the rows split at tabs, in order): (gc, gc of the row in front, gc of the row behind) as
    f32, the ends taking their own"""
    g = np.array([np.float32(f[3]) for f in fields], np.float32)
    return g, np.concatenate((g[:1], g[:-1])), np.concatenate((g[1:], g[-1:]))


# ---- 5. more row blocks than the scan has threads ------------------------------------------------------------------------
BIG_KEPT = SCAN_THREADS * ROW_BLOCK + 1


def big_case():
    """262,147 kept rows (1,025 row blocks: a thread of blk_offsets_scan_kernel<unsigned long long> takes two) in three
    ctgs, shuffled, signals 1 / -1, no prefixes"""
    rng = np.random.default_rng(9)
    ctgs = [ctg("ctg:I:1", "I", 1, helpers.synth(400_000, 126)), ctg("ctg:I:2", "I", 400_101, helpers.synth(300_000, 127)),
            ctg("ctg:II:1", "II", 1, helpers.synth(350_000, 128))]
    per = [100_001, 90_001, BIG_KEPT + 2 - 190_002]
    body = []
    for c, m in zip(ctgs, per):
        s = rng.integers(c["chr_start"] + 1, c["chr_end"] - 120, m)
        e = s + rng.integers(0, 100, m)
        sg = rng.integers(0, 2, m)
        body += ["%s:%d-%d\t0\t%s" % (c["chr_id"], a, b, "1" if g else "-1")
                 for a, b, g in zip(s.tolist(), e.tolist(), sg.tolist())]
    rng.shuffle(body)
    head = ["%s:%d-%d\t0\t1" % (c["chr_id"], c["chr_start"] + 5, c["chr_start"] + 9) for c in ctgs]
    return dict(ctgs=ctgs, data=join_lines(head + body))


# ---- 6. line edges of peak_parse_kernel -------------------------------------------------------------------------------
def line_ctgs():
    return [ctg("ctg:I:1", "I", 1, b"ACGT" * 250)]


FIRST = b"I:20-30\t0\t-1\n"            # the sacrificial first located line
LINE_CASES = {
    # the signal keeps the \r of a last line without a newline, and three rows print it
    "cr_at_the_end": FIRST + b"I:1-3\t0\t-1\nI:50-60\t0\tx\nI:5-9\t0.1\t1\r",
    "empty_signal_in_a_line": FIRST + b"I:1-3\t0\t-1\nI:5-9\t0.1\t\nI:50-60\t0\tx\n",
    "empty_signal_at_the_end": FIRST + b"I:1-3\t0\t-1\nI:50-60\t0\tx\nI:5-9\t0.1\t",
    "padded_first_field": FIRST + b"I:1-3\t0\t-1\nI:5-9 \t0.1\t1\nI:50-60\t0\tx\n",
    "empty_name": FIRST + b"m.I:1-3\t0\t-1\n.I:5-9\t0\t1\nI:50-60\t0\tx\n",
    "strand_and_reprinted_numbers": FIRST + b"I:5-9\t0\t1\na.I(-):0021_24\t0\t-1\tx\nI:11\t0\t\n",
    "two_tabs": FIRST + b"I:1-3\t0\t-1\n\t\t\nI:5-9\t0\t1\n\t\t",
}


def efield_data():
    """256 valid lines, then a valid range with two fields: the lane that raises W_EFIELD is in the second workgroup"""
    return FIRST + b"".join(b"I:%d-%d\t0\t1\n" % (3 * k + 1, 3 * k + 2) for k in range(255)) + b"I:5-9\t0.1\n"


# ---- the battery ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(ctgs, data, ...) of the named case"""
    if name in STAGE_CASES:
        return stage_case(*STAGE_CASES[name])
    if name in SEAM_CASES:
        k, shuffle = SEAM_CASES[name]
        return seam_case(SEAM_LOCATED[k], shuffle)
    if name in LINE_CASES:
        return dict(ctgs=line_ctgs(), data=LINE_CASES[name])
    if name.startswith("width_"):
        return width_case(int(name[6:]))
    return {"ties": ties_case, "high": high_case, "fmt": fmt_case, "big": big_case}[name]()


@functools.lru_cache(maxsize=None)
def expected(name):
    c = case(name)
    return Expected(c["ctgs"], c["data"])


@functools.lru_cache(maxsize=None)
def big_text():
    """peak_text.model of the big case (the pure-Python model takes about 5 s for it), made once"""
    c = case("big")
    return pt.model(c["ctgs"], c["data"])


SMALL_CASES = list(STAGE_CASES) + list(SEAM_CASES) + ["ties", "high", "fmt"] + list(LINE_CASES)


def n_lines(data):
    return len(rust_lines(data))
