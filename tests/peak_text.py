"""A pure-Python model of gams_gpu_peak_text / host.peak_text (utils.rs:83-116 read_peak, then peak.rs:41-160), and the
synthetic wave TSV the device is held against.  tests/test_peak_text_cpu.py holds the model to account on the CPU
(golden rows, and that the synthetic input really carries the cases it is meant to); tests/test_gpu_peak_text.py
compares the device with it byte for byte.

The model: BufRead::lines(), parts[0] through Range::from_str and the ctg lookup (the rg loader's model,
tests/test_rg_text_cpu.py), the third field as the signal, drop-first per ctg, a stable sort by start, and the oracle's
peak.rs:65-158 (ora.peak_rows) per ctg, the ctgs in id byte order."""
import numpy as np

from oracle import oracle as ora
from test_rg_text_cpu import locate_one, parse_line, rust_lines


class ModelError(Exception):
    """what the reference panics on: the device answers GAMS_EINVAL"""


def name_prefix(field):
    """the "name." that Range::to_string() prints in front of the chromosome: the head up to its FIRST dot, the
    strand cut off first; an empty name prints nothing"""
    head = field.decode("latin-1").rstrip("\r\n ")
    head = head[:head.rindex(":")]
    if head.endswith(")"):
        head = head[:head.rindex("(")]
    dot = head.find(".")
    return head[:dot + 1] if dot > 0 else ""


def buckets(ctgs, data):
    """-> per ctg of `ctgs`: (located lines, [(start, end, signal, name prefix, line)] kept, sorted by start)"""
    located = [0] * len(ctgs)
    kept = [[] for _ in ctgs]
    for k, ln in enumerate(rust_lines(data)):
        parts = ln.split(b"\t")
        r = parse_line(parts[0])                        # utils.rs:96-99
        if r is None:
            continue
        if len(parts) < 3:
            raise ModelError("no signal column")        # utils.rs:102
        i = locate_one(ctgs, *r)
        if i is None:
            continue
        if located[i]:                                  # utils.rs:109-112: the first one only creates the bucket
            kept[i].append((r[1], r[2], parts[2].decode("latin-1"), name_prefix(parts[0]), k))
        located[i] += 1
    return located, [sorted(b, key=lambda p: p[0]) for b in kept]          # peak.rs:49 (sorted() is stable)


def ctg_rows(c, pk):
    """the rows of one ctg from its sorted kept peaks"""
    for s, e, _, _, _ in pk:
        if s < c["chr_start"] or e > c["chr_end"] or e < s:
            raise ModelError("a peak leaves its ctg")   # utils.rs:155 slices the sequence
    if pk and c.get("seq") is None:
        raise ModelError("no sequence")
    text = ora.peak_rows(c["id"], c["chr_id"], c["chr_start"], c["chr_end"], c["seq"], [p[:3] for p in pk])
    rows = text.split("\n")[:-1]
    assert len(rows) == len(pk)
    out = []
    for row, p in zip(rows, pk):                        # the oracle prints "{chr}:{runlist}": the name goes in front
        f = row.split("\t")
        f[1] = p[3] + f[1]
        out.append("\t".join(f) + "\n")
    return "".join(out)


def model(ctgs, data):
    """-> the text of host.peak_text(eng, ctgs, data), as bytes"""
    _, kept = buckets(ctgs, data)
    order = sorted(range(len(ctgs)), key=lambda i: ctgs[i]["id"].encode())
    return "".join(ctg_rows(ctgs[i], kept[i]) for i in order).encode("latin-1")


def sig_digits(text):
    """significant digits of a positional decimal"""
    return len(text.replace(".", "").lstrip("0"))


# ---- the synthetic input --------------------------------------------------------------------------------------------
LONG_ID = "ctg:III:2_" + "x" * 30                      # 40 bytes
LONG_SIGNAL = "signal_" + "s" * 33                      # 40 bytes
LAYOUT = [("ctg:I:1", "I", 1, 30000), ("ctg:I:2", "I", 30101, 70100), ("ctg:II:1", "II", 1001, 61000),
          ("ctg:II:2", "II", 61001, 81000), ("ctg:III:1", "III", 1, 25000), (LONG_ID, "III", 30001, 55000)]
ONE_LINE, TWO_LINES = "ctg:II:2", "ctg:III:1"           # ctgs with exactly one / two located lines


def synth_ctgs(seed=7):
    """six ctgs of 20-60 kb on three chromosomes, G/C content changing every 400 bases"""
    rng = np.random.default_rng(seed)
    ctgs = []
    for cid, chr_id, s, e in LAYOUT:
        n = e - s + 1
        p = np.repeat(rng.uniform(0.15, 0.75, n // 400 + 1), 400)[:n]
        gc = rng.random(n) < p
        pick = rng.random(n) < 0.5
        seq = np.where(gc, np.where(pick, ord("G"), ord("C")), np.where(pick, ord("A"), ord("t"))).astype(np.uint8)
        ctgs.append(dict(id=cid, chr_id=chr_id, chr_start=s, chr_end=e, seq=seq.tobytes()))
    return ctgs


def synth_lines(ctgs, seed=11, n=3000, long_names=False):
    """about n lines of a wave TSV over `ctgs`, shuffled behind the header: name. prefixes, strands, reprinted numbers
    (leading zeros, '_' and '--' between them), point ranges (one on a ctg start), ties on start, invalid lines, unknown
    chromosomes, unlocated ranges, extra fields, the four signals.  long_names: 130-byte name prefixes."""
    rng = np.random.default_rng(seed)
    by_id = {c["id"]: c for c in ctgs}
    signals = ["1", "-1", "", LONG_SIGNAL]
    lines = []

    def line(c, s, e, k):
        head = c["chr_id"]
        u = rng.random()
        if long_names:
            head = "n" * 128 + "%d." % (k % 10) + head
        elif u < 0.15:
            head = "nm%d." % k + head
        if rng.random() < 0.3:
            head += "(+)" if rng.random() < 0.5 else "(-)"
        start = ("0%d" % s) if rng.random() < 0.05 else str(s)
        if e == s and rng.random() < 0.5:
            rg = "%s:%s" % (head, start)
        else:
            rg = "%s:%s%s%d" % (head, start, ("-", "_", "--")[int(rng.integers(0, 3)) if rng.random() < 0.1 else 0], e)
        ln = "%s\t0.%d\t%s" % (rg, rng.integers(0, 100), signals[int(rng.integers(0, 4)) if rng.random() < 0.2 else k % 2])
        if rng.random() < 0.1:
            ln += "\textra\tmore"
        return ln

    weights = {"ctg:I:1": 0.3, "ctg:I:2": 0.3, "ctg:II:1": 0.3, LONG_ID: 0.1}
    ids = list(weights)
    for k in range(n):
        c = by_id[ids[int(rng.choice(len(ids), p=list(weights.values())))]]
        s = int(rng.integers(c["chr_start"], c["chr_end"] - 400))
        e = s if rng.random() < 0.05 else s + int(rng.integers(1, 300))
        lines.append(line(c, s, e, k))
        if k % 100 == 0:                                 # a tie on start, the longer range first in the file
            lines.append(line(c, s, e + 37, k))
    c = by_id[ONE_LINE]
    lines.append(line(c, c["chr_start"] + 10, c["chr_start"] + 90, 1))
    c = by_id[TWO_LINES]
    lines.append(line(c, c["chr_start"] + 500, c["chr_start"] + 600, 2))
    lines.append(line(c, c["chr_start"], c["chr_start"] + 100, 3))
    lines += ["II:1001\t0.5\t1",                         # the point range on a ctg start: not located
              "I:30050-30060\t0.5\t1",                   # between two ctgs
              "IV:100-200\t0.5\t1", "Mito:5\t0.1\t-1",   # unknown chromosomes
              "garbage", "", "I:1-", "I:a-b\tx\ty", "I :1-2\t0.5\t1", "I:12345678901\t0.5\t1", "\t\t"]
    rng.shuffle(lines)
    lines.insert(0, "#range\tgc_content\tsignal")
    return lines


def synth_data(lines, seed=13):
    """the bytes: one line in ten ends in \\r\\n, the last line has no newline"""
    rng = np.random.default_rng(seed)
    out = [ln + ("\r\n" if rng.random() < 0.1 else "\n") for ln in lines[:-1]]
    return ("".join(out) + lines[-1]).encode()
