"""A pure-Python model of gams_gpu_locate_seq_text / host.locate_seq_text (locate.rs:124-134 over the lines of a range
file), and the synthetic ctgs and lines the device is held against.  tests/test_locate_seq_text_cpu.py holds the model to
account on the CPU (the reference's pinned answers); tests/test_gpu_locate_seq_text.py compares the device with it byte
for byte.

The model: BufRead::lines(), rg = the line up to its first tab, Range::from_str and the half-open locate of SURVEY
section 8 a-16 (both the rg loader's model, tests/test_rg_text_cpu.py), then the slice of the ctg's bytes."""
import numpy as np

from test_rg_text_cpu import locate_one, parse_line, rust_lines


class ModelError(Exception):
    """what the reference panics on (locate.rs:133) or has no sequence for: the device answers GAMS_EINVAL.  `line` is
    the 0-based line, `outside` says that the range leaves the ctg it is located to (else: the ctg has no sequence)"""

    def __init__(self, line, outside):
        super().__init__("line %d: %s" % (line, "outside its ctg" if outside else "no sequence"))
        self.line, self.outside = line, outside


def records(ctgs, data):
    """-> [(line, rg bytes, position of the ctg in `ctgs`, start, end)] of the located lines, in line order"""
    out = []
    for k, ln in enumerate(rust_lines(data)):
        rg = ln.split(b"\t")[0]                         # locate.rs:89-91
        r = parse_line(rg)
        if r is None:
            continue
        i = locate_one(ctgs, *r)                        # the strand is not part of the lookup
        if i is not None:
            out.append((k, rg, i, r[1], r[2]))
    return out


def model(ctgs, data):
    """-> the text of host.locate_seq_text(eng, ctgs, data), as bytes; ModelError for the smallest line the reference
    panics on.  c["seq"] (bytes, or None: no sequence) holds the ctg's bytes, whatever their values"""
    recs = records(ctgs, data)
    for k, _, i, s, e in recs:
        c = ctgs[i]
        if not c["chr_start"] <= s <= e <= c["chr_end"]:
            raise ModelError(k, True)
    out = []
    for k, rg, i, s, e in recs:
        c = ctgs[i]
        if c.get("seq") is None:
            raise ModelError(k, False)
        out.append(b">" + rg + b"\n" + bytes(c["seq"][s - c["chr_start"]:e - c["chr_start"] + 1]) + b"\n")   # locate.rs:134
    return b"".join(out)


# ---- the synthetic input --------------------------------------------------------------------------------------------
# 5 k - 40 k bytes a ctg; ctg:I:2 is longer than two chunks of the copy and none of them starts on a multiple of 16
LAYOUT = [("ctg:I:1", "I", 1, 30000), ("ctg:I:2", "I", 30101, 70100), ("ctg:II:1", "II", 1001, 13000),
          ("ctg:II:2", "II", 13001, 18000), ("ctg:III:1", "III", 7, 25003)]
DROPPED = [b"garbage", b"", b"I:1-", b"I:a-b\tx", b"I :1-2", b"I:12345678901", b"\t\t",       # invalid
           b"IV:100-200", b"Mito:5",                                                            # unknown chromosomes
           b"I:30050-30060", b"II:1001", b"I:1", b"III:3-6", b"II:20000-20010"]                 # unlocated (two points on a ctg start)


def synth_ctgs(seed=5, ascii_only=False):
    """the ctgs of LAYOUT with random bytes over the full range 0..255 (ascii_only: over ACGTNacgtn)"""
    rng = np.random.default_rng(seed)
    ctgs = []
    for cid, chr_id, s, e in LAYOUT:
        n = e - s + 1
        seq = (np.frombuffer(b"ACGTNacgtn", np.uint8)[rng.integers(0, 10, n)] if ascii_only
               else rng.integers(0, 256, n).astype(np.uint8))
        ctgs.append(dict(id=cid, chr_id=chr_id, chr_start=s, chr_end=e, seq=seq.tobytes()))
    return ctgs


def row_len(line):
    """bytes of the row of a located line inside its ctg"""
    rg = line.split(b"\t")[0]
    _, s, e = parse_line(rg)
    return 1 + len(rg) + 1 + (e - s + 1) + 1


def filler(nbytes):
    """lines on ctg:I:1 whose rows are exactly nbytes bytes together (0, or at least 9): the way a test moves what
    follows to a chosen byte of the text"""
    lines = []
    while nbytes:
        take = nbytes if nbytes <= 20000 else min(20000, nbytes - 9)
        for zeros in range(4):                           # a digit more in the end moves the length by two: pad the start
            head = b"I:" + b"0" * zeros + b"2-"
            n = take - 3 - len(head)                     # bases, if the end had no digits
            hit = [b for b in range(max(n - 6, 1), n) if len(head) + len(b"%d" % (b + 1)) + b + 3 == take]
            if hit:
                lines.append(head + b"%d" % (hit[0] + 1))
                break
        else:
            raise ValueError("no filler of %d bytes" % take)
        assert row_len(lines[-1]) == take
        nbytes -= take
    return lines


def synth_lines(ctgs, seed=17, n=1500):
    """about n lines over `ctgs`, shuffled: ranges of 1 - 2000 bases, point ranges, name prefixes, strands, reprinted
    numbers, extra fields, whole ctgs, the first and the last base of a ctg, and the lines of DROPPED"""
    rng = np.random.default_rng(seed)
    lines = []
    for k in range(n):
        c = ctgs[int(rng.integers(0, len(ctgs)))]
        s = int(rng.integers(c["chr_start"], c["chr_end"] + 1))
        e = s if rng.random() < 0.2 else min(c["chr_end"], s + int(rng.integers(1, 2000)))
        if s == e == c["chr_start"]:
            e += 1                                       # (the point on a ctg start is not located)
        head = c["chr_id"]
        if rng.random() < 0.15:
            head = "nm%d." % k + head
        if rng.random() < 0.3:
            head += "(+)" if rng.random() < 0.5 else "(-)"
        start = ("0%d" % s) if rng.random() < 0.05 else str(s)
        if e == s and rng.random() < 0.5:
            ln = "%s:%s" % (head, start)
        else:
            ln = "%s:%s%s%d" % (head, start, ("-", "_", "--")[int(rng.integers(0, 3)) if rng.random() < 0.1 else 0], e)
        if rng.random() < 0.2:
            ln += "\textra\tI:1-5"
        lines.append(ln.encode())
    for c in ctgs:
        lines.append(b"%s:%d-%d" % (c["chr_id"].encode(), c["chr_start"], c["chr_end"]))        # the whole ctg
        lines.append(b"%s:%d-%d" % (c["chr_id"].encode(), c["chr_start"], c["chr_start"] + 1))  # its first bases
        lines.append(b"%s:%d" % (c["chr_id"].encode(), c["chr_end"]))                           # its last base
    lines += DROPPED
    order = rng.permutation(len(lines))
    return [lines[i] for i in order]


def synth_data(lines, seed=19, crlf=0.1, final_newline=False):
    """the bytes: one line in ten ends in \\r\\n, the last line has no newline unless asked for"""
    rng = np.random.default_rng(seed)
    out = [ln + (b"\r\n" if rng.random() < crlf else b"\n") for ln in lines[:-1]]
    return b"".join(out) + lines[-1] + (b"\n" if final_newline else b"")
