"""Builders and the case battery for the edges of `gams sw` from the bytes of a feature file on the device
(gams_gpu_sw_feature_text: sw_gather_kernel in gams_amd/csrc/text.hip, the row-offset and text kernels of sw.hip):
text blocks at, one under and one over the writer's LDS stage at every offset inside a 16-byte unit, ctgs that begin on
the seams of the 512-row text blocks with empty intervals around them, ctg boundaries on the seams of the 256-feature
workgroups of the row prefix, more feature workgroups and text blocks than the offsets scan has threads, more
intervals than features (and than one workgroup of the gather), the middle check on its knife edge with several
offenders, line and interval counts on powers of two, the smallest window geometries and the widest id fields.
test_sw_edges_cpu.py proves on the CPU that every case carries what it is built for; test_gpu_sw_edges.py holds the
device to the model on them, byte for byte.

The expected text is always sw_text.slices (the oracle's sw_proc_ctg over sw_text.features), laid out by interval as
sw_text.interval_text does and by id as sw_text.model does; the CPU test holds Expected to both.  A "text block" is
512 consecutive rows in output order (the ctgs in the Locator's order), a "feature workgroup" 256 consecutive kept
features in that order.  Nothing here imports the GPU package."""
import functools

import numpy as np

import helpers
import sw_text as swt
from test_rg_text_cpu import locator_order, rust_lines
from test_rg_text_cpu import model as rg_model

BLOCK = 512              # kSwTextBlock: rows per workgroup of the text kernels
STAGE = 49_152           # kSwTextStage: a block of at most this many bytes is composed in LDS
FEAT_BLOCK = 256         # features per workgroup of sw_gather_kernel, sw_geom_kernel and sw_row_off_kernel
SCAN_THREADS = 1024      # threads of blk_offsets_scan_kernel: beyond that many entries a thread takes several
PARAMS = dict(size=10, mx=3, resize=40)          # what a case runs with unless it names its own


def ctg(cid, chr_id, start, seq):
    seq = seq.tobytes() if isinstance(seq, np.ndarray) else bytes(seq)
    return dict(id=cid, chr_id=chr_id, chr_start=start, chr_end=start + len(seq) - 1, seq=seq)


def join_lines(lines):
    return ("\n".join(lines) + "\n").encode("latin-1")


def rng_line(c, s, e):
    return "%s:%d" % (c["chr_id"], s) if e == s else "%s:%d-%d" % (c["chr_id"], s, e)


def sacrificial(c):
    """the first located line of a ctg, the one the reference drops: inside the ctg whatever its length"""
    n = c["chr_end"] - c["chr_start"] + 1
    return rng_line(c, c["chr_start"] + min(30, n // 2), c["chr_start"] + min(35, n - 1))


def offenders(ctgs, data):
    """the 1-based numbers of all kept lines whose middle leaves their ctg (or that are empty), ascending: the entry
    reports the smallest, sw_text.features raises at the first in ctg order"""
    _, kept = swt.buckets(ctgs, data)
    return sorted(line + 1 for c, b in zip(ctgs, kept) for s, e, line in b if not swt.middle_inside(c, s, e))


class Expected:
    """what the model says of one case: the ctgs in the Locator's order, their kept features, their rows"""

    def __init__(self, ctgs, data, size=10, mx=3, resize=40):
        at = {c["id"]: i for i, c in enumerate(ctgs)}
        self.order = locator_order(ctgs)
        self.located, kept = swt.buckets(ctgs, data)
        parts = swt.slices(ctgs, data, size, mx, resize)
        self.kept = [kept[at[c["id"]]] for c in self.order]
        self.n_located = [self.located[at[c["id"]]] for c in self.order]
        self.parts = [parts[at[c["id"]]] for c in self.order]         # what text_off slices
        self.rows = [[r + b"\n" for r in p.split(b"\n")[:-1]] for p in self.parts]
        self.text = b"".join(self.parts)                              # the entry's text: the Locator's order
        ids = sorted(range(len(self.order)), key=lambda i: self.order[i]["id"].encode())
        self.by_id = b"".join(self.parts[i] for i in ids)             # host.sw_text's and sw_text.model's order
        self.n_features = sum(len(b) for b in self.kept)
        self.n_rows = sum(len(r) for r in self.rows)
        self.bucket_off = np.concatenate(([0], np.cumsum([len(b) for b in self.kept]))).astype(np.int64)
        self.row_off = np.concatenate(([0], np.cumsum([len(r) for r in self.rows]))).astype(np.int64)
        self.text_off = np.concatenate(([0], np.cumsum([len(p) for p in self.parts]))).astype(np.int64)
        self.row_len = np.array([len(r) for rows in self.rows for r in rows], np.int64)

    def heads(self):
        """(interval, feature number, serial) of every row, in output order"""
        out = []
        for i, rows in enumerate(self.rows):
            for r in rows:
                _, num, serial = r.split(b"\t", 1)[0].rsplit(b":", 2)
                out.append((i, int(num), int(serial)))
        return out

    def rows_per_feature(self):
        """the rows of every kept feature, in output order"""
        n = {}
        for i, num, _ in self.heads():
            n[(i, num)] = n.get((i, num), 0) + 1
        return [n[k] for k in sorted(n)]

    def fields(self):
        return [r[:-1].decode("latin-1").split("\t") for rows in self.rows for r in rows]

    def block_totals(self):
        if self.row_len.size == 0:
            return np.zeros(0, np.int64)
        return np.add.reduceat(self.row_len, np.arange(0, self.row_len.size, BLOCK))

    def block_starts(self):
        t = self.block_totals()
        return np.concatenate(([0], np.cumsum(t)[:-1])).astype(np.int64) if t.size else t


# ---- ctgs of a given number of rows (groups 1, 2, 8) ------------------------------------------------------------------
def _row_lines(c, w, mx):
    """the kept lines that give ctg `c` exactly w rows at size 10 and max `mx` (0 or 1): features of 8-10 bases every 12
    bases give 1 + 2 * mx rows each; at max 1 a feature on the first bases has no L window and one on the last bases no
    R window, 2 rows each, which settle what 3 does not divide"""
    cs, ce = c["chr_start"], c["chr_end"]
    if mx == 0:
        n_mid, ends = w, 0
    else:
        assert mx == 1 and w != 1
        ends = (0, 2, 1)[w % 3]
        n_mid = (w - 2 * ends) // 3
    lines = [rng_line(c, cs + 60 + 12 * k, cs + 67 + 12 * k + k % 3) for k in range(n_mid)]
    assert not n_mid or cs + 80 + 12 * n_mid < ce - 40
    if ends >= 1:
        lines.append(rng_line(c, cs + 2, cs + 6))
    if ends == 2:
        lines.append(rng_line(c, ce - 6, ce - 2))
    return lines


def rows_case(spec, mx, seed=1, id_len=None):
    """Ctgs with the given number of rows each, in the Locator's order.  spec: [(chr_id, rows)] with the chromosomes in
    byte order; rows 0 is an interval without a located line, -1 one with a single located line (dropped: an empty
    bucket).  The sacrificial first lines stand in front, the kept lines follow shuffled.  id_len[i] pads ctg i's id to
    that many bytes."""
    rng = np.random.default_rng(seed)
    ctgs, head, body, at = [], [], [], {}
    for k, (chr_id, w) in enumerate(spec):
        n = max(2000, 12 * max(w, 0) + 400)
        start = at.get(chr_id, 1001)
        at[chr_id] = start + n + 100
        cid = "c%03d" % k
        if id_len is not None:
            assert id_len[k] >= len(cid)
            cid += "_" * (id_len[k] - len(cid))
        c = ctg(cid, chr_id, start, helpers.synth(n, 200 + k))
        ctgs.append(c)
        if w != 0:
            head.append(sacrificial(c))
        if w > 0:
            body += _row_lines(c, w, mx)
    rng.shuffle(body)
    return dict(ctgs=ctgs, data=join_lines(["# features"] + head + body), size=10, mx=mx, resize=40,
                want_rows=[max(w, 0) for _, w in spec])


# ---- 1. the stage limit and its alignment ----------------------------------------------------------------------------
WEIGHTS = [2, 3, 4, 8, 16, 32, 64, 128, 255]        # the rows of the ctgs of one text block: 512 together


def _spread(d):
    """d = sum(x[j] * WEIGHTS[j]) with small x: what to add to the id length of every ctg of a block to add d bytes"""
    q, r = divmod(d, BLOCK)
    x = [q] * len(WEIGHTS)
    for j in range(len(WEIGHTS) - 1, 1, -1):        # 255 .. 4
        x[j] += r // WEIGHTS[j]
        r %= WEIGHTS[j]
    if r == 1:                                      # 3 - 2
        x[1] += 1
        x[0] -= 1
    elif r:
        x[r - 2] += 1
    return x


def stage_case(targets, tail, mx=1):
    """Nine ctgs of 2 .. 255 rows for every text block (512 rows: block b is chromosome b) and a last ctg of `tail`
    rows.  A row prints its ctg's id once, so a block's bytes are linear in the id lengths of its ctgs: the totals are
    measured on the model with ids of 10 bytes, and the difference to targets[b] is spread over the ids of block b"""
    spec = [("b%02d" % b, w) for b in range(len(targets)) for w in WEIGHTS] + ([("t", tail)] if tail else [])
    base_len = [10] * len(spec)
    c = rows_case(spec, mx, id_len=base_len)
    base = Expected(c["ctgs"], c["data"], 10, mx, 40).block_totals()
    id_len = list(base_len)
    for b, want in enumerate(targets):
        for j, x in enumerate(_spread(int(want - base[b]))):
            id_len[b * len(WEIGHTS) + j] += x
    assert all(4 <= n <= 80 for n in id_len), id_len
    return rows_case(spec, mx, id_len=id_len)


# name -> (targets, tail).  40,001 = 1 mod 16: sixteen such blocks begin at every offset inside a 16-byte unit.
STAGE_CASES = {
    "under": ([STAGE - 1], 100),
    "exact": ([STAGE], 100),
    "over": ([STAGE + 1], 100),
    "exact_alone": ([STAGE], 0),
    "second_exact_r15": ([40_015, STAGE, 40_000], 77),
    "over_then_staged": ([STAGE + 3, 45_000, STAGE - 5], 2),
    "ladder": ([40_001] * 16, 33),
}


# ---- 2. text block seams and empty intervals ------------------------------------------------------------------------------
# name -> (spec, max).  seam_2048: ctgs begin on rows 0, 512, 1025, 1535 and 1537 (0, 0, 1, 511 and 1 mod 512), the
# total is 4 blocks, and empty intervals of both kinds stand first, last and in runs between.  seam_1025: a ctg ends
# on row 511, an empty run begins on the seam, the total is two blocks and a row.
SEAM_CASES = {
    "seam_2048": ([("I", 0), ("I", -1), ("I", 512), ("II", -1), ("II", 0), ("II", 0), ("II", 513), ("III", 510),
                   ("III", 0), ("IV", 2), ("IV", 511), ("V", -1), ("V", 0)], 1),
    "seam_1025": ([("I", -1), ("I", 509), ("I", 3), ("II", 0), ("II", -1), ("III", 513), ("III", 0)], 1),
    "seam_max0": ([("I", 511), ("I", 1), ("II", 0), ("II", 1), ("II", 511), ("III", -1)], 0),
    "single_row": ([("I", 0), ("I", 1), ("II", -1), ("II", 0)], 0),
}


# ---- 3. feature prefix seams -----------------------------------------------------------------------------------------
TINY = 12                # a ctg of 12 bases holds one window of 10: its features have the M row alone


def prefix_case(spec, seed, size=10, mx=3, resize=40):
    """spec: [(chr_id, bases, kept features)] in the Locator's order.  A ctg's kept features are short ranges at random
    places, the first of them on and next to its first and last bases (a point on chr_start + 1 and on chr_end, ranges
    from chr_start and to chr_end, and within three windows of either), so that the rows of a feature vary between 1
    and 1 + 2 * max; the lines of all ctgs are shuffled behind the sacrificial ones"""
    rng = np.random.default_rng(seed)
    ctgs, head, body, at = [], [], [], {}
    for k, (chr_id, n, m) in enumerate(spec):
        start = at.get(chr_id, 1001)
        at[chr_id] = start + n + 100
        c = ctg("ctg:%s:%d" % (chr_id, k + 1), chr_id, start, helpers.synth(n, 300 + k))
        ctgs.append(c)
        cs, ce = c["chr_start"], c["chr_end"]
        if m < 0:
            continue
        head.append(sacrificial(c))
        fixed = [(cs + 1, cs + 1), (ce, ce), (cs, cs + 5), (ce - 4, ce), (cs + 12, cs + 20), (ce - 17, ce - 9),
                 (cs + 25, cs + 26), (ce - 33, ce - 30)] if n > 100 else [(cs + 1, ce - 1), (ce, ce), (cs, cs + 1)]
        feats = fixed[:m]
        while len(feats) < m:
            s = int(rng.integers(cs + 1, max(cs + 2, ce - 40)))
            feats.append((s, min(ce, s + int(rng.integers(0, 30)))))
        body += [rng_line(c, s, e) for s, e in feats]
    rng.shuffle(body)
    return dict(ctgs=ctgs, data=join_lines(["# features"] + head + body), size=size, mx=mx, resize=resize)


# name -> the spec; m = -1: a ctg without a line.  nf256: the ctg boundary lies between kept features 255 and 256,
# nf257 and nf513: between 256 and 257 (and nf513 between 255 and 256 as well)
PREFIX_CASES = {
    "nf255": [("I", 3000, 100), ("I", TINY, 3), ("II", 3000, 152)],
    "nf256": [("I", 3000, 255), ("II", 3000, 1)],
    "nf257": [("I", 3000, 256), ("I", TINY, 1)],
    "nf513": [("I", 3000, 255), ("I", TINY, 1), ("II", 3000, -1), ("II", 3000, 0), ("III", 4000, 257)],
}
PREFIX_NF = {"nf255": 255, "nf256": 256, "nf257": 257, "nf513": 513}

BIG_KEPT = SCAN_THREADS * FEAT_BLOCK + 1 + 3
BIG_PARAMS = dict(size=10, mx=1, resize=20)


def big_case():
    """262,148 kept features (1,025 feature workgroups) in three ctgs, shuffled, 2 or 3 rows each at max 1 (features on
    the first and last bases of every ctg among them): more than 524,288 rows, so more than 1,024 text blocks too, and a
    thread of either blk_offsets_scan_kernel takes two"""
    rng = np.random.default_rng(9)
    ctgs = [ctg("ctg:I:1", "I", 1, helpers.synth(400_000, 126)), ctg("ctg:I:2", "I", 400_101, helpers.synth(300_000, 127)),
            ctg("ctg:II:1", "II", 1, helpers.synth(350_000, 128))]
    per = [100_001, 90_001, BIG_KEPT - 190_002]
    body = []
    for c, m in zip(ctgs, per):
        cs, ce = c["chr_start"], c["chr_end"]
        s = rng.integers(cs + 1, ce - 40, m)
        e = s + rng.integers(0, 30, m)
        near = m // 50                                    # within a window or two of either end
        s[:near] = rng.integers(cs + 1, cs + 15, near)
        e[:near] = s[:near] + rng.integers(0, 5, near)
        e[near:2 * near] = rng.integers(ce - 14, ce + 1, near)
        s[near:2 * near] = e[near:2 * near] - rng.integers(0, 5, near)
        body += ["%s:%d-%d" % (c["chr_id"], a, b) for a, b in zip(s.tolist(), e.tolist())]
    rng.shuffle(body)
    head = [sacrificial(c) for c in ctgs]
    return dict(ctgs=ctgs, data=join_lines(head + body), **BIG_PARAMS)


# ---- 4. intervals beyond the features -----------------------------------------------------------------------------------
MANY_CHRS = ["A", "B-2", "chr-III", "d" * 17, "e" * 40, "f_6"]          # 1 .. 40 bytes, in byte order
MANY_SIZES = [100, 156, 44, 200, 99, 1]                                 # ctgs per chromosome: seams at 100, 256, ..., 599
MANY_COUNTS = (600, 255, 256, 257)


def many_kept(n):
    """the intervals (in the Locator's order) that have kept features"""
    return sorted({0, 255, 256, n - 1} & set(range(n)))


def many_case(n, seed=4):
    """n ctgs of 300-600 bases on the chromosomes above (as many as n fills), ids of 1 .. 80 bytes; kept features, three
    or four each, only in the intervals many_kept(n); a dozen other ctgs get one located line, which is dropped"""
    rng = np.random.default_rng(seed)
    ctgs, at = [], {}
    left = n
    letters = list("mnopqrstuvwxyz")          # the ids of one byte: "z" for interval 0, so the ids sort otherwise
    for chr_id, m in zip(MANY_CHRS, MANY_SIZES):
        for _ in range(min(m, left)):
            k = len(ctgs)
            ln = int(rng.integers(300, 601))
            start = at.get(chr_id, 1)
            at[chr_id] = start + ln + int(rng.integers(0, 50))
            want = 80 if k == n - 1 else 1 if k == 256 else 1 + (k * 7) % 80      # the id's length: 1 .. 80
            cid = letters.pop() if want == 1 else ("t%d" % k).ljust(want, "-")
            ctgs.append(ctg(cid, chr_id, start, helpers.synth(ln, 400 + k)))
        left -= min(m, left)
    assert left == 0 and len(ctgs) == n and len({c["id"] for c in ctgs}) == n
    order = locator_order(ctgs)
    assert [c["id"] for c in order] == [c["id"] for c in ctgs]
    head, body = [], []
    for i in many_kept(n):
        c = ctgs[i]
        cs, ce = c["chr_start"], c["chr_end"]
        head.append(sacrificial(c))
        feats = [(cs + 1, cs + 1), (ce - 3, ce), (cs + 100, cs + 130)] + ([(cs + 50, cs + 55)] if i % 2 else [])
        body += [rng_line(c, s, e) for s, e in feats]
    for i in rng.choice(n, 12, replace=False).tolist():
        if i not in many_kept(n):
            head.append(sacrificial(ctgs[i]))
    rng.shuffle(body)
    return dict(ctgs=ctgs, data=join_lines(["# features"] + head + body), **PARAMS)


# ---- 5. the middle check -------------------------------------------------------------------------------------------
def middle_ctgs():
    return [ctg("ctg:I:1", "I", 1001, helpers.synth(3000, 501)), ctg("ctg:I:2", "I", 4101, helpers.synth(3000, 502)),
            ctg("ctg:II:1", "II", 1001, helpers.synth(3000, 503))]


# the probes of the issue for ctg 1001 .. 4000: line -> accepted
MIDDLE_TABLE = {
    "I:901-1102": True, "I:901-1101": False, "I:901-1100": False, "I:3900-4100": True, "I:3899-4101": True,
    "I:3900-4101": False, "I:3901-4101": False, "I:1001-4000": True, "I:1-9000": False, "I:2000-1990": False,
}


def middle_probes(c):
    """[(line, accepted)] around the ends of ctg `c`, made of its coordinates: for h = 2, 7 and 101 a feature of 2h and
    of 2h + 1 bases whose left middle is chr_start (accepted) and chr_start - 1 (refused), one whose right middle is
    chr_end (accepted) and chr_end + 1 (refused); the point on the last base; the ctg itself; a feature over both
    ends with its middle inside, one with its middle behind the end; end < start"""
    cs, ce = c["chr_start"], c["chr_end"]
    out = []
    for h in (2, 7, 101):
        for flen in (2 * h, 2 * h + 1):
            s = cs - h + 1                                   # mid_l = s + h - 1 = chr_start
            out += [(rng_line(c, s, s + flen - 1), True), (rng_line(c, s - 1, s + flen - 2), False)]
            s = ce - h                                       # mid_r = s + h = chr_end
            out += [(rng_line(c, s, s + flen - 1), True), (rng_line(c, s + 1, s + flen), False)]
    out += [(rng_line(c, ce, ce), True), (rng_line(c, cs, ce), True), (rng_line(c, cs - 500, ce + 500), True),
            (rng_line(c, cs + 10, ce + 3200), False), ("%s:%d-%d" % (c["chr_id"], cs + 999, cs + 989), False)]
    return out


def probe_data(c, line, first=False):
    """the probe as a kept line (line 2) behind the ctg's sacrificial line, or as the dropped first line itself"""
    return join_lines([line, sacrificial(c)] if first else [sacrificial(c), line])


MIDDLE_OFFENDERS = ["I:7050-7200", "I:901-1100", "I:5000-4990", "II:3990-4100"]


def offenders_data(reverse=False, prefix=b""):
    """300 good features in ctg:I:1 (the first interval) and a few in the others, and four offenders: one of ctg:I:1,
    two of ctg:I:2 (middle behind the end; end < start), one of ctg:II:1.  In both line orders the smallest offending
    line belongs to ctg:I:2, behind the 300 kept features of ctg:I:1 in key order, while ctg:I:1's own offender stands
    further down the file.  `prefix`: bytes in front of everything (comment, blank and \\r\\n lines shift the number)"""
    ctgs = middle_ctgs()
    a, b, c2 = ctgs
    body = [rng_line(a, a["chr_start"] + 9 * k + 1, a["chr_start"] + 9 * k + 1 + k % 20) for k in range(300)]
    body += [rng_line(b, b["chr_start"] + 50 * k + 3, b["chr_start"] + 50 * k + 30) for k in range(10)]
    body += [rng_line(c2, c2["chr_start"] + 70 * k + 3, c2["chr_start"] + 70 * k + 9) for k in range(10)]
    for at, ln in zip((40, 200, 290, 150), MIDDLE_OFFENDERS):
        body.insert(at, ln)
    if reverse:
        body.reverse()
    return prefix + join_lines([sacrificial(c) for c in ctgs] + body)


# ---- 6. key decode ---------------------------------------------------------------------------------------------------
KEY_CASES = [(2, 1), (3, 2), (256, 3), (257, 4), (65_536, 7), (65_537, 8), (65_536, 8), (257, 1)]    # (lines, ctgs)
KEY_CHRS = ["I", "I", "II", "II", "II", "III", "IV", "IV"]


def key_case(n_lines, n_ctg, seed=6):
    """A file of exactly n_lines lines over n_ctg ctgs of 2 kb, most of the lines comments; the last line is a kept
    feature of the last interval.  Where the file has room, every ctg has a sacrificial line and kept features"""
    rng = np.random.default_rng(seed + n_lines + n_ctg)
    chrs = sorted(KEY_CHRS[:n_ctg - 1]) + ["V"]
    ctgs, at = [], {}
    for k, chr_id in enumerate(chrs):
        start = at.get(chr_id, 1001)
        at[chr_id] = start + 2100
        ctgs.append(ctg("ctg:%s:%d" % (chr_id, k + 1), chr_id, start, helpers.synth(2000, 600 + k)))
    last = ctgs[-1]

    def feature(c):
        s = int(rng.integers(c["chr_start"] + 1, c["chr_end"] - 40))
        return rng_line(c, s, s + int(rng.integers(0, 30)))

    planned = [sacrificial(last)] + [sacrificial(c) for c in ctgs[:-1]] + [feature(c) for c in ctgs[:-1]]
    planned += [feature(ctgs[int(rng.integers(0, n_ctg))]) for _ in range(300)]
    planned = planned[:n_lines - 1]
    lines = ["#c"] * n_lines
    where = np.sort(rng.choice(n_lines - 1, len(planned), replace=False))
    for w, ln in zip(where.tolist(), planned):
        lines[w] = ln
    lines[-1] = rng_line(last, last["chr_end"] - 20, last["chr_end"] - 3)
    return dict(ctgs=ctgs, data=join_lines(lines), **PARAMS)


# ---- 7. smallest geometries and widths -------------------------------------------------------------------------------
def points_case(mx, resize):
    """size 2 over point features: the ctg's second base (the point on the first is not located) and its last base, the
    bases next to them and a dozen elsewhere"""
    c = ctg("ctg:I:1", "I", 1001, helpers.synth(2000, 701))
    cs, ce = c["chr_start"], c["chr_end"]
    pos = [cs + 1, ce, cs + 2, ce - 1, cs + 3, ce - 2] + list(range(cs + 100, cs + 1300, 100))
    return dict(ctgs=[c], data=join_lines([sacrificial(c)] + [rng_line(c, p, p) for p in pos]), size=2, mx=mx, resize=resize)


POINT_CASES = {"points_m%d_r%d" % (mx, rs): (mx, rs) for mx in (0, 3) for rs in (2, 4)}
TINY_LENGTHS = (2, 15, 16, 17, 50)


def tiny_case(size):
    """ctgs of 2, 15, 16, 17 and 50 bases next to an ordinary one: the whole ctg, its last base, its second base and a
    short range as kept features of each (at size 2 the flank is one window, resize 2)"""
    ctgs = [ctg("ctg:I:1", "I", 1001, helpers.synth(3000, 710))]
    at = 101
    for k, n in enumerate(TINY_LENGTHS):
        ctgs.append(ctg("ctg:T:%d" % (k + 1), "T", at, helpers.synth(n, 711 + k, nrate=0)))
        at += n + 7
    lines = [rng_line(c, c["chr_start"], c["chr_end"]) for c in ctgs]            # dropped
    for c in ctgs:
        cs, ce = c["chr_start"], c["chr_end"]
        lines += [rng_line(c, cs, ce), rng_line(c, ce, ce), rng_line(c, cs + 1, cs + 1), rng_line(c, cs, cs + 1),
                  rng_line(c, (cs + ce) // 2, min(ce, (cs + ce) // 2 + 3))]
    return dict(ctgs=ctgs, data=join_lines(lines), size=size, mx=3, resize=2 if size == 2 else 40)


def serial_case():
    """max 50: one feature in the middle of a ctg of 1,200 bases has 101 rows, one near the start fewer"""
    c = ctg("ctg:I:1", "I", 1001, helpers.synth(1200, 720))
    lines = [sacrificial(c), rng_line(c, 1596, 1605), rng_line(c, 1101, 1104)]
    return dict(ctgs=[c], data=join_lines(lines), size=10, mx=50, resize=40)


def ids_case():
    """10,001 kept point features in one ctg at max 0: the feature numbers reach five digits"""
    c = ctg("ctg:I:1", "I", 1001, helpers.synth(12_000, 721))
    lines = [sacrificial(c)] + [rng_line(c, c["chr_start"] + 1 + k, c["chr_start"] + 1 + k) for k in range(10_001)]
    return dict(ctgs=[c], data=join_lines(lines), size=10, mx=0, resize=40)


# ---- 8. an rg source for -a count --------------------------------------------------------------------------------------
def rg_source(ctgs, chrs, seed=8):
    """The lines of an rg file over the ctgs of the chromosomes `chrs` only (no tab in a line: read_range cuts there,
    the loader does not): per ctg a first line, which the loader drops, and five ranges at random places.
    -> (bytes, [(ctg id, range string)] the rg: records read_range makes of them, per the rg loader's model)"""
    rng = np.random.default_rng(seed)
    lines = []
    for c in ctgs:
        if c["chr_id"] not in chrs:
            continue
        cs, ce = c["chr_start"], c["chr_end"]
        lines.append(sacrificial(c))
        for _ in range(5):
            s = int(rng.integers(cs + 1, ce - 40))
            lines.append(rng_line(c, s, s + int(rng.integers(0, 40))))
    data = join_lines(lines)
    buckets = rg_model(ctgs, data)["buckets"]
    records = [(c["id"], rng_line(c, s, e)) for c, b in zip(ctgs, buckets) for s, e, _ in b]
    return data, records


# the cases of groups 2 and 4 -> the chromosomes their rg source covers (single_row has one ctg with rows: its own)
COUNT_CASES = {"seam_2048": ("I", "III"), "seam_1025": ("III",), "seam_max0": ("II",), "single_row": ("I",),
               "many_600": (MANY_CHRS[0], MANY_CHRS[2]), "many_255": (MANY_CHRS[0],), "many_256": (MANY_CHRS[1],),
               "many_257": (MANY_CHRS[1],)}


# ---- the battery -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(ctgs, data, size, mx, resize) of the named case"""
    if name in STAGE_CASES:
        return stage_case(*STAGE_CASES[name])
    if name in SEAM_CASES:
        return rows_case(*SEAM_CASES[name])
    if name in PREFIX_CASES:
        return prefix_case(PREFIX_CASES[name], seed=PREFIX_NF[name])
    if name.startswith("many_"):
        return many_case(int(name[5:]))
    if name.startswith("key_"):
        return key_case(*(int(x) for x in name[4:].split("_")))
    if name in POINT_CASES:
        return points_case(*POINT_CASES[name])
    if name.startswith("tiny_"):
        return tiny_case(int(name[5:]))
    return {"serial": serial_case, "ids": ids_case, "big": big_case}[name]()


def params(c):
    return c["size"], c["mx"], c["resize"]


@functools.lru_cache(maxsize=None)
def expected(name):
    c = case(name)
    return Expected(c["ctgs"], c["data"], *params(c))


@functools.lru_cache(maxsize=None)
def big_text():
    """sw_text.model of the big case (the pure-Python model takes some seconds for it), made once"""
    c = case("big")
    return swt.model(c["ctgs"], c["data"], *params(c))


MANY_CASES = ["many_%d" % n for n in MANY_COUNTS]
KEY_NAMES = ["key_%d_%d" % k for k in KEY_CASES]
TINY_CASES = ["tiny_2", "tiny_100"]
WIDTH_CASES = list(POINT_CASES) + TINY_CASES + ["serial", "ids"]
SMALL_CASES = list(STAGE_CASES) + list(SEAM_CASES) + list(PREFIX_CASES) + MANY_CASES + KEY_NAMES + WIDTH_CASES


def n_lines(data):
    return len(rust_lines(data))
