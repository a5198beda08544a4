"""A pure-Python model of gams_gpu_sw_feature_text / host.sw_text (feature.rs:50-54 read_range, feature.rs:74-86 ids,
then sw.rs:132-191), and the synthetic feature file the device is held against.  tests/test_sw_text_cpu.py holds the
model to account on the CPU (golden rows, and that the synthetic input really carries the cases it is meant to);
tests/test_gpu_sw_text.py compares the device with it byte for byte.

The model: BufRead::lines(), the WHOLE line through Range::from_str and the ctg lookup (the rg loader's model,
tests/test_rg_text_cpu.py), drop-first per ctg, the kept lines of a ctg in file order numbered from 1, and the oracle's
sw.rs:141-191 (ora.sw_proc_ctg) per ctg, the ctgs in id byte order."""
import numpy as np

import peak_text as pt
from oracle import oracle as ora
from test_rg_text_cpu import locate_one, locator_order, parse_line, rust_lines


class ModelError(Exception):
    """what the entry answers GAMS_EINVAL to"""


def buckets(ctgs, data):
    """-> per ctg of `ctgs`: (located lines, [(start, end, line)] kept, in file order)"""
    located = [0] * len(ctgs)
    kept = [[] for _ in ctgs]
    for k, ln in enumerate(rust_lines(data)):
        r = parse_line(ln)                              # utils.rs:50: the line, not its first field
        if r is None:
            continue
        i = locate_one(ctgs, *r)
        if i is None:
            continue
        if located[i]:                                  # utils.rs:60-63: the first one only creates the bucket
            kept[i].append((r[1], r[2], k))
        located[i] += 1
    return located, kept


def middle_inside(c, s, e):
    """window.rs:98-110: the middle pair of the feature must be members of the ctg span"""
    flen = e - s + 1
    half = flen // 2
    mid_l, mid_r = (s, s) if half == 0 else (s + half - 1, s + half)
    return flen >= 1 and mid_l >= c["chr_start"] and mid_r <= c["chr_end"]


def features(ctgs, data):
    """-> per ctg of `ctgs`: [(feature id, start, end)], "feature:{ctg id}:{k}" from 1 in file order (feature.rs:74-86);
    ModelError for a kept feature whose middle leaves its ctg"""
    _, kept = buckets(ctgs, data)
    out = []
    for c, b in zip(ctgs, kept):
        for s, e, line in b:
            if not middle_inside(c, s, e):
                raise ModelError("line %d: the middle leaves the ctg" % (line + 1))
        out.append([("feature:%s:%d" % (c["id"], k + 1), s, e) for k, (s, e, _) in enumerate(b)])
    return out


def slices(ctgs, data, size=100, mx=20, resize=500):
    """-> per ctg of `ctgs`: its rows (-a gc), as bytes"""
    out = []
    for c, feats in zip(ctgs, features(ctgs, data)):
        if feats and c.get("seq") is None:
            raise ModelError("no sequence")
        out.append(ora.sw_proc_ctg(c["chr_id"], c["chr_start"], c["chr_end"], c["seq"], feats, size, mx, resize)
                   .encode("latin-1") if feats else b"")
    return out


def id_order(ctgs):
    return sorted(range(len(ctgs)), key=lambda i: ctgs[i]["id"].encode())


def model(ctgs, data, size=100, mx=20, resize=500):
    """-> the text of host.sw_text(eng, ctgs, data, size, mx, resize), as bytes: the ctgs in id byte order (sw.rs:97)"""
    parts = slices(ctgs, data, size, mx, resize)
    return b"".join(parts[i] for i in id_order(ctgs))


def interval_text(ctgs, data, size=100, mx=20, resize=500):
    """the same rows laid out as the entry lays them out: by interval of the ctg index (the Locator's order)"""
    parts = dict(zip((c["id"] for c in ctgs), slices(ctgs, data, size, mx, resize)))
    return b"".join(parts[c["id"]] for c in locator_order(ctgs))


# ---- the synthetic input --------------------------------------------------------------------------------------------
LONG_ID = "ctg:III:2_" + "y" * 70                       # 80 bytes
ONE_LINE, TWO_LINES, CROWDED = pt.ONE_LINE, pt.TWO_LINES, "ctg:I:1"   # exactly one / two located lines; >= 1000 kept
assert len(LONG_ID) == 80


def synth_ctgs():
    """the six ctgs of peak_text.synth_ctgs(), 20-60 kb each on three chromosomes, the last under an 80-byte id"""
    ctgs = pt.synth_ctgs()
    assert ctgs[5]["id"] == pt.LONG_ID
    ctgs[5] = dict(ctgs[5], id=LONG_ID)
    return ctgs


def edge_lines(ctgs):
    """the lines the cases of the issue are pinned on (each its own list, so that the CPU test can look for them)"""
    by = {c["id"]: c for c in ctgs}
    a, b, c2, lg = by["ctg:I:1"], by["ctg:I:2"], by["ctg:II:1"], by[LONG_ID]
    return dict(
        first_bases=["I:%d" % (a["chr_start"] + 5), "II:%d-%d" % (c2["chr_start"] + 20, c2["chr_start"] + 40),
                     "III:%d" % (lg["chr_start"] + 99)],                              # n_l = 0
        last_bases=["I:%d" % (a["chr_end"] - 5), "I:%d-%d" % (b["chr_end"] - 60, b["chr_end"] - 10),
                    "III:%d" % (lg["chr_end"] - 98)],                                 # n_r = 0
        over_edge=["I:%d-%d" % (a["chr_end"] - 100, a["chr_end"] + 50),               # into the gap behind ctg:I:1
                   "II:%d-%d" % (c2["chr_start"] - 101, c2["chr_start"] + 199),       # from before ctg:II:1
                   "I:%d-%d" % (b["chr_start"] - 30, b["chr_start"] + 400)],
        long=["I:%d-%d" % (a["chr_start"] + 5000, a["chr_start"] + 6499), "II:%d-%d" % (c2["chr_start"] + 900, c2["chr_start"] + 1100)],
        seam=["II:%d-%d" % (c2["chr_end"] - 20, c2["chr_end"] + 10)],                 # ctg:II:1 | ctg:II:2: goes to the first
    )


def synth_lines(ctgs, seed=23, n=4000):
    """about n lines of a range file over `ctgs`, shuffled behind a comment line: strands, name. prefixes, reprinted
    numbers (leading zeros, '_' and '--' between them), point ranges, the edge lines above, a ctg with exactly one located
    line and one with exactly two, invalid lines, unknown chromosomes, unlocated ranges"""
    rng = np.random.default_rng(seed)
    by_id = {c["id"]: c for c in ctgs}
    lines = []

    def line(c, s, e, k):
        head = c["chr_id"]
        if rng.random() < 0.15:
            head = "nm%d." % k + head
        if rng.random() < 0.3:
            head += "(+)" if rng.random() < 0.5 else "(-)"
        start = ("0%d" % s) if rng.random() < 0.05 else str(s)
        if e == s and rng.random() < 0.5:
            return "%s:%s" % (head, start)
        return "%s:%s%s%d" % (head, start, ("-", "_", "--")[int(rng.integers(0, 3)) if rng.random() < 0.1 else 0], e)

    weights = {CROWDED: 0.3, "ctg:I:2": 0.3, "ctg:II:1": 0.25, LONG_ID: 0.15}
    ids = list(weights)
    for k in range(n):
        c = by_id[ids[int(rng.choice(len(ids), p=list(weights.values())))]]
        s = int(rng.integers(c["chr_start"] + 1, c["chr_end"] - 400))
        e = s if rng.random() < 0.1 else s + int(rng.integers(1, 300))
        lines.append(line(c, s, e, k))
    for group in edge_lines(ctgs).values():
        lines += group
    c = by_id[ONE_LINE]
    lines.append(line(c, c["chr_start"] + 10, c["chr_start"] + 90, 1))
    c = by_id[TWO_LINES]
    lines.append(line(c, c["chr_start"] + 500, c["chr_start"] + 600, 2))
    lines.append(line(c, c["chr_start"] + 2000, c["chr_start"] + 2100, 3))
    lines += ["II:1001",                                   # the point range on a ctg start: not located
              "I:30050-30060",                             # between two ctgs
              "IV:100-200", "Mito:5",                      # unknown chromosomes
              "garbage", "", "I:1-", "I:a-b", "I :1-2", "I:12345678901", "I:1-100\tfoo", "\t\t"]
    rng.shuffle(lines)
    lines.insert(0, "# ranges of the features")
    return lines


def synth_data(lines, seed=29):
    """the bytes: one line in ten ends in \\r\\n, the last line has no newline"""
    return pt.synth_data(lines, seed)
