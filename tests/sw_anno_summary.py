"""A pure-Python model of the sw summary with Prop columns (host.sw_summary(..., anno=)): the reference's
pipeline `gams sw ... | gams anno a.json stdin -H | gams anno b.json stdin -H | load | fsw-distance-tag.tera.sql` over TEXT.

The rows come as text -- tests/sw_text.py's model or host.sw_text --, every set appends its `{:.4}` column -- annotate()
here with the oracle's cover (ora.anno_prop) on the CPU, host.anno_text on the GPU --, and the table parses the decimal
fields into integers, sums with Python ints, rounds P / COUNT to the nearest integer with ties to even in integer
arithmetic and prints q / 10^4 with the trailing zeros dropped.  Nothing here comes from the code under test."""
import json
import re

import numpy as np

import sw_summary as sws
from oracle import oracle as ora

CTG_ID = re.compile(r"(?i)ctg:[\w_]+:\d+")                 # utils.rs:118-129
RANGE = re.compile(rb"^([^:]+):(\d+)(?:-(\d+))?$")


def prop_units(field):
    """a printed `{:.4}` prop as the integer q of q / 10^4"""
    assert re.fullmatch(rb"[01]\.\d{4}", field), field
    q = int(field[:1]) * 10000 + int(field[2:])
    assert q <= 10000, field
    return q


def annotate(rows_text, ctgs, spans):
    """`gams anno set.json stdin` over the rows of `gams sw` (anno.rs:97-140), the cover from the oracle: every row gains
    "\\t%.4f" of prop = |set[chr] n [ctg] n range| as f32 / |range| as f32, 0 when the set lacks the chromosome.
    spans: {chr: (lo, hi)} of sorted disjoint inclusive spans."""
    by_id = {c["id"]: c for c in ctgs}
    out = []
    for row in rows_text.split(b"\n")[:-1]:
        f = row.split(b"\t")
        m = CTG_ID.search(f[0].decode("latin-1"))
        assert m, row                                           # (upstream skips the row; the inputs here never do that)
        r = RANGE.match(f[1])
        chr_id, s, e = r.group(1).decode(), int(r.group(2)), int(r.group(3) or r.group(2))
        prop = 0.0
        if chr_id in spans:
            c = by_id[m.group(0)]                               # (unknown: upstream panics)
            lo, hi = spans[chr_id]
            prop = ora.anno_prop(lo, hi, c["chr_start"], c["chr_end"], s, e)
        out.append(row + b"\t" + (b"%.4f" % float(np.float32(prop))))
    return b"".join(r + b"\n" for r in out)


class Table(sws.Table):
    """sw_summary.Table over rows with n_anno more fields: groups[(tag, d)] = [COUNT, S x 4, NaN x 4, C, P x n_anno]"""

    def __init__(self, prefixes, actions=("gc",)):
        super().__init__(actions)
        self.prefixes = [p if isinstance(p, bytes) else p.encode() for p in prefixes]

    def add_text(self, text, tag=None):
        n = len(self.prefixes)
        for row in text.split(b"\n"):
            if not row:
                continue
            f = row.split(b"\t")
            assert len(f) == 9 + n, row
            g = self.groups.setdefault((tag, int(f[3])), [0, [0] * sws.STATS, [0] * sws.STATS, 0, [0] * n])
            g[0] += 1
            if self.gc:
                for k in range(sws.STATS):
                    m = sws.units(f[4 + k])
                    if m is None:
                        g[2][k] += 1
                    else:
                        g[1][k] += m
            if self.count:
                g[3] += int(f[8])
            for a in range(n):
                g[4][a] += prop_units(f[9 + a])
        return self

    def header(self, tagged):
        cols = ([b"tag"] if tagged else []) + [b"distance"]
        if self.gc:
            cols += [b"AVG_gc_content", b"AVG_gc_mean", b"AVG_gc_stddev", b"AVG_gc_cv"]
        cols += [b"AVG_" + p + b"Prop" for p in self.prefixes]
        if self.count:
            cols += [b"AVG_rg_count"]
        return b"\t".join(cols + [b"COUNT"]) + b"\n"

    def text(self, tagged=False):
        out = [self.header(tagged)]
        for tag, d in sorted(self.groups, key=lambda k: (b"" if k[0] is None else k[0], k[1])):
            n, s, nan, c, p = self.groups[(tag, d)]
            f = ([tag] if tagged else []) + [b"%d" % d]
            if self.gc:
                f += [b"nan" if nan[k] else sws.avg4(s[k], n) for k in range(sws.STATS)]
            f += [sws.avg4(v, n) for v in p]
            if self.count:
                f += [sws.avg4(c * 10000, n)]
            out.append(b"\t".join(f + [b"%d" % n]) + b"\n")
        return b"".join(out)

    def prop(self, mx, tags=None):
        """[slot][distance][set] as host.sw_summary_table(...)["prop"] lays the sums out"""
        slots = [None] if tags is None else sorted(set(tags))
        out = np.zeros((len(slots), mx + 1, len(self.prefixes)), np.uint64)
        for (tag, d), g in self.groups.items():
            out[slots.index(tag), d, :] = g[4]
        return out

    def prop_ties(self):
        """[(tag, distance, set)] of the groups whose P / COUNT lies exactly between two integers"""
        return [(tag, d, a) for (tag, d), g in sorted(self.groups.items(), key=lambda kv: (kv[0][0] or b"", kv[0][1]))
                for a in range(len(self.prefixes)) if 2 * (g[4][a] % g[0]) == g[0]]


def summary(texts, prefixes, tags=None, actions=("gc",)):
    """-> (the text of host.sw_summary(..., anno=), the Table) for the annotated rows of several files"""
    t = Table(prefixes, actions)
    for k, text in enumerate(texts):
        t.add_text(text, None if tags is None else tags[k])
    return t.text(tags is not None), t


def tie_units(size):
    """the q of the props k / size that are exact ties at the fourth decimal (10^4 k / size = n + 1/2): what the test at
    size 32 asserts its input to hold (1/32 -> 312, 3/32 -> 938, 5/32 -> 1562, ...)"""
    out = {}
    for k in range(1, size):
        num = 10000 * k
        if (2 * num) % size == 0 and ((2 * num) // size) % 2 == 1:
            n = num // size
            out[k] = n + (n & 1)
    return out


# ---- the synthetic input ------------------------------------------------------------------------------------------------
def runlist_json(spans):
    """{chr: (lo, hi)} -> the bytes of the runlist JSON file"""
    return json.dumps({c: ",".join("%d" % a if a == b else "%d-%d" % (a, b) for a, b in zip(lo, hi))
                       for c, (lo, hi) in spans.items()}).encode()


def synth_ctgs(seed=3, n=(20011, 19997, 20480)):
    """three ctgs of about 20 kb on two chromosomes: A holds two with a gap between them, B one"""
    rng = np.random.default_rng(seed)
    lay = [("ctg:A:1", "A", 1001, 1000 + n[0]), ("ctg:A:2", "A", 1000 + n[0] + 501, 1000 + n[0] + 500 + n[1]),
           ("ctg:B:1", "B", 1, n[2])]
    ctgs = []
    for cid, chr_id, s, e in lay:
        m = e - s + 1
        p = np.repeat(rng.uniform(0.2, 0.7, m // 300 + 1), 300)[:m]
        gc = rng.random(m) < p
        pick = rng.random(m) < 0.5
        seq = np.where(gc, np.where(pick, ord("G"), ord("c")), np.where(pick, ord("A"), ord("T"))).astype(np.uint8)
        ctgs.append(dict(id=cid, chr_id=chr_id, chr_start=s, chr_end=e, seq=seq.tobytes()))
    return ctgs


def one_ctg(n=70000, seed=5):
    rng = np.random.default_rng(seed)
    seq = rng.choice(np.frombuffer(b"ACGT", np.uint8), n)
    return [dict(id="ctg:A:1", chr_id="A", chr_start=1, chr_end=n, seq=seq.tobytes())]


def synth_features(ctgs, size=100, mx=20, seed=17, n=300):
    """about n lines of a feature file: point features, even- and odd-length ones, and features within mx * size of both
    edges of every ctg (the L and R runs are cut); the first located line of every ctg is dropped by the loader"""
    rng = np.random.default_rng(seed)
    lines = []
    for c in ctgs:
        s0, e0 = c["chr_start"], c["chr_end"]
        lines.append("%s:%d-%d" % (c["chr_id"], s0 + 50, s0 + 60))                    # (one more: a first line is dropped)
        reach = size * mx
        for k in range(n // len(ctgs)):
            kind = k % 5
            if kind == 0:                                                             # near the left edge
                s = int(rng.integers(s0 + 1, s0 + min(reach, (e0 - s0) // 3)))
            elif kind == 1:                                                           # near the right edge
                s = int(rng.integers(e0 - min(reach, (e0 - s0) // 3), e0 - 40))
            else:
                s = int(rng.integers(s0 + 1, e0 - 40))
            ln = (0, 1, 9, 10, 37)[int(rng.integers(0, 5))] if kind != 2 else 0       # points, even and odd lengths
            e = min(s + ln, e0 - 1)
            lines.append("%s:%d" % (c["chr_id"], s) if e == s else "%s:%d-%d" % (c["chr_id"], s, e))
    rng.shuffle(lines)
    return ("\n".join(lines) + "\n").encode()


def dense_set(ctgs, window_edges, seed=19):
    """The first set: on ctgs[0] a crowded stretch (spans of 1-3 bases every 4: far more than five a cell), spans that begin
    or end exactly on a window edge, one base inside it and one base outside it, and a stretch with none; ctgs[1] covered
    whole and beyond (q = 10000 everywhere); the third ctg's chromosome with scattered spans.
    window_edges: chromosome positions of ctgs[0] where windows begin (s) and end (s - 1)."""
    rng = np.random.default_rng(seed)
    a, b, c = ctgs
    sp = []
    s0 = a["chr_start"]
    x = s0 + 2000
    while x < s0 + 3500:                                                              # crowded cells
        w = int(rng.integers(1, 4))
        sp.append((x, x + w - 1))
        x += w + 1 + int(rng.integers(0, 2))
    for k, ed in enumerate(e for e in window_edges if s0 + 4000 <= e < a["chr_end"] - 6000):
        m = k % 6                                                                     # begin / end on, inside, outside the edge
        lo, hi = [(ed, ed + 6), (ed + 1, ed + 7), (ed - 1, ed + 5), (ed - 7, ed - 1), (ed - 8, ed - 2), (ed - 6, ed)][m]
        sp.append((lo, hi))
    # (nothing in the last 6000 bases of ctgs[0])
    spans = {}
    for chr_id, pairs in ((a["chr_id"], sp + [(b["chr_start"] - 100, b["chr_end"] + 100)]),
                          (c["chr_id"], [(int(x), int(x) + int(rng.integers(0, 400)))
                                         for x in rng.integers(c["chr_start"], c["chr_end"], 60)])):
        spans[chr_id] = normalise(pairs)
    return spans


def normalise(pairs):
    """sorted, overlapping and adjacent spans joined -> (lo, hi) int32 arrays"""
    out = []
    for lo, hi in sorted(pairs):
        if out and lo <= out[-1][1] + 1:
            out[-1][1] = max(out[-1][1], hi)
        else:
            out.append([lo, hi])
    return (np.array([p[0] for p in out], np.int32), np.array([p[1] for p in out], np.int32))


def sparse_set(ctgs, seed=23):
    """The second set: the first chromosome only (the other is absent -> 0), spans of 100-3000 bases, and an empty group
    under a chromosome no ctg lies on"""
    rng = np.random.default_rng(seed)
    a = ctgs[0]
    pairs, x = [], a["chr_start"] - 500
    end = max(c["chr_end"] for c in ctgs if c["chr_id"] == a["chr_id"])
    while x < end:
        w = int(rng.integers(100, 3000))
        pairs.append((x, x + w - 1))
        x += w + int(rng.integers(50, 2500))
    return {a["chr_id"]: normalise(pairs), "Z": (np.zeros(0, np.int32), np.zeros(0, np.int32))}
