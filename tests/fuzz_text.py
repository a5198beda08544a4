"""Seeded inputs and expected outcomes for the device entries that read a text file, one `case(entry, seed, size)` for
fourteen entry families over one small `world()`.  The expected outcome of every case comes from the pure-Python model
the entry already has (tests/peak_text.py, peak_records.py, sw_text.py, sw_summary.py, sw_anno_summary.py, runlist_text.py,
gen_text.py, locate_seq_text.py, test_rg_text_cpu.py, test_loader_text_cpu.py); locate, --count and anno, which had none,
get theirs here (locate.rs:84-141, utils.rs:24-36, anno.rs:95-142).  tests/test_fuzz_text_cpu.py holds this corpus to
account without a GPU; tests/test_gpu_call_sequences.py runs it, call after call, on one handle.

An outcome is a dict: "rc" and, where rc is 0, every output the ABI gives, as bytes, ints and lists.  Nothing here imports a
GPU test module."""
import functools

import numpy as np

import gen_text as gt
import locate_seq_text as lst
import peak_records as pr
import peak_text as pt
import runlist_text as rt
import sw_anno_summary as sas
import sw_summary as sws
import sw_text as swt
from gams_amd import _lib
from oracle import oracle as ora
from test_loader_text_cpu import FEATURE, RECORDS, RESP, RG, TSV, fuzz_file, model_files, model_loader
from test_rg_text_cpu import locate_one, locator_order, parse_line, rust_lines
from test_rg_text_cpu import model as rg_model
from test_text_ops_cpu import fmt4_exact

FAMILIES = ["locate", "count", "anno", "read_range", "index", "loader", "peak_text", "peak_records", "sw_text",
            "sw_summary", "sw_summary_anno", "runlist_text", "gen_text", "locate_seq"]
SIZES = ["empty", "one", "small", "seam", "large"]
SEEDS = (0, 1, 2, 3)                    # the seeds the GPU tests draw from; REFUSED is one more
REFUSED = 7                             # the seed whose cases the device refuses (all but the empty one)
LINES = dict(empty=0, one=1, small=70, seam=1300, large=2000)
SW_PARAMS = [(100, 20, 500), (50, 10, 200), (100, 5, 500), (30, 20, 100)]


# ---- the shared fuzz pieces of tests/test_gpu_text_ops.py -------------------------------------------------------------
def fuzz_ranges(rng, ctgs, n):
    """range strings of every kind the grammar and the lookups distinguish"""
    pick = rng.integers(0, len(ctgs), n)
    kind = rng.integers(0, 16, n)
    span = rng.choice([0, 1, 10, 500, 5000, 70000], n)
    off = rng.integers(-200, 60000, n)
    out = []
    for p, k, w, o in zip(pick, kind, span, off):
        c = ctgs[p]
        s = max(1, c["chr_start"] + int(o))
        e = s + int(w)
        chrom = c["chr_id"]
        if k == 0:
            out.append(f"{chrom}:{c['chr_start']}")                       # point range on a ctg start
        elif k == 1:
            out.append(f"{chrom}(+):{s}-{e}")
        elif k == 2:
            out.append(f"nm.{chrom}(-):{s}_{e}")
        elif k == 3:
            out.append(f"{chrom}:{s}--_{e}")
        elif k == 4:
            out.append(f"chrUn:{s}-{e}")                                   # unknown chromosome
        elif k == 5:
            out.append(f"{chrom}:{12345678901 if o % 2 else 3000000000}-{e}")   # 11 digits / > INT32_MAX
        elif k == 6:
            out.append(f"{chrom}-{s}-{e}")                                 # no colon
        elif k == 7:
            out.append(f"{chrom}:{c['chr_end'] - 5}-{c['chr_end'] + 4000}")  # across ctgs
        elif k == 8:
            out.append(f"{chrom}:{s}-")
        elif k == 9:
            out.append(f"{chrom}:{s} ")
        else:
            out.append(f"{chrom}:{s}-{e}" if e != s else f"{chrom}:{s}")
    return out


def assemble(rng, lines, allow_empty=True):
    """lines with \\n or \\r\\n endings, the last one without"""
    parts = []
    n = len(lines)
    crlf = rng.random(n) < 0.3
    empty = rng.random(n) < (0.02 if allow_empty else 0.0)
    for i, ln in enumerate(lines):
        if empty[i]:
            parts.append("\r\n" if crlf[i] else "\n")
        parts.append(ln)
        if i + 1 < n:
            parts.append("\r\n" if crlf[i] else "\n")
    return "".join(parts).encode()


# ---- the world --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def world():
    """Seven ctgs of 9-30 kb on three chromosomes under the ids the synth_* generators aim at: chromosome I in two ctgs
    with a gap of 100 between them, II from 1001 on in two adjacent ctgs, III in three with gaps; random ACGT (one base in
    five lower case) with a few N runs; two runlist sets (A on I and II, B on I and on a chromosome no ctg lies on); one rg
    file.  -> dict(ctgs, order, sets, rg_data, rg_records)"""
    rng = np.random.default_rng(1000)
    n = [int(rng.integers(9000, 30001)) for _ in range(7)]
    lay, pos = [], 1
    for cid, k in (("ctg:I:1", 0), ("ctg:I:2", 1)):
        lay.append((cid, "I", pos, pos + n[k] - 1))
        pos += n[k] + 100
    pos = 1001
    for cid, k in (("ctg:II:1", 2), ("ctg:II:2", 3)):
        lay.append((cid, "II", pos, pos + n[k] - 1))
        pos += n[k]
    pos = 1
    for cid, k in (("ctg:III:1", 4), (pt.LONG_ID, 5), (swt.LONG_ID, 6)):
        lay.append((cid, "III", pos, pos + n[k] - 1))
        pos += n[k] + 5000
    ctgs = []
    for cid, chr_id, s, e in lay:
        m = e - s + 1
        p = np.repeat(rng.uniform(0.15, 0.75, m // 400 + 1), 400)[:m]
        gc = rng.random(m) < p
        pick = rng.random(m) < 0.5
        seq = np.where(gc, np.where(pick, ord("G"), ord("C")), np.where(pick, ord("A"), ord("T"))).astype(np.uint8)
        seq = np.where(rng.random(m) < 0.2, seq | 0x20, seq).astype(np.uint8)
        for _ in range(3):
            at = int(rng.integers(0, m - 200))
            seq[at:at + int(rng.integers(1, 120))] = ord("N")
        ctgs.append(dict(id=cid, chr_id=chr_id, chr_start=s, chr_end=e, seq=seq.tobytes()))
    assert len(ctgs) <= 8 and all(c["chr_end"] - c["chr_start"] < 30000 for c in ctgs)

    def spans(chr_id, lo_w, hi_w, gap):
        end = max(c["chr_end"] for c in ctgs if c["chr_id"] == chr_id)
        pairs, x = [], 1
        while x < end + 500:
            w = int(rng.integers(lo_w, hi_w))
            pairs.append((x, x + w - 1))
            x += w + int(rng.integers(1, gap))
        return sas.normalise(pairs)

    sets = [{"I": spans("I", 1, 40, 60), "II": spans("II", 100, 3000, 2500)},
            {"I": spans("I", 100, 3000, 2500), "Z": (np.zeros(0, np.int32), np.zeros(0, np.int32))}]
    order = locator_order(ctgs)
    rg_data = fuzz_file(rng, ctgs, 700)
    m = rg_model(order, rg_data)
    rg_records = [(c["id"], "%s:%d-%d" % (c["chr_id"], s, e)) for c, b in zip(order, m["buckets"]) for s, e, _ in b]
    return dict(ctgs=ctgs, order=order, sets=sets, rg_data=rg_data, rg_records=rg_records)


def rg_groups(w):
    """per ctg of w["order"]: (sorted starts, sorted stops) of its rg records, the intervals [start, end + 1)"""
    by = {c["id"]: [] for c in w["order"]}
    for cid, r in w["rg_records"]:
        _, s, e = parse_line(r.encode())
        by[cid].append((s, e + 1))
    return [(np.sort(np.array([p[0] for p in by[c["id"]]], np.int64)), np.sort(np.array([p[1] for p in by[c["id"]]], np.int64)))
            for c in w["order"]]


def lapper_count(starts, stops, qs, qe):
    """Lapper::count (rust-lapper 1.1.0): #{start < qe} - #{stop <= qs} over the separately sorted starts and stops"""
    return int(np.searchsorted(starts, qe, "left")) - int(np.searchsorted(stops, qs, "right"))


# ---- the models locate, --count and anno lacked -------------------------------------------------------------------------
def locate_model(order, data, groups=None):
    """locate.rs:84-141: per line its first field through Range::from_str and find_one_idx; "{rg}\\t{ctg id}\\n", or with
    groups (--count, utils.rs:24-36) "{rg}\\t{Lapper::count(start, end) over the ctg's rg index}\\n" """
    out = []
    for _, rg, i, s, e in lst.records(order, data):
        tail = order[i]["id"].encode("latin-1") if groups is None else b"%d" % lapper_count(*groups[i], s, e)
        out.append(rg + b"\t" + tail + b"\n")
    return b"".join(out)


def anno_model(order, spans, data, header=False, prefix=""):
    """anno.rs:95-142 with the id in field 1 and the range in field 2: every line gains "\\t{prop:.4}", prop = |set[chr] n
    [ctg] n range| as f32 / |range| as f32, 0 where the set lacks the chromosome; -H echoes the first line with
    "\\t{prefix}Prop" """
    by_id = {c["id"]: c for c in order}
    lines = rust_lines(data)
    out = []
    if header and lines:
        out.append(lines[0] + b"\t" + prefix.encode() + b"Prop\n")
        lines = lines[1:]
    for ln in lines:
        f = ln.split(b"\t")
        m = sas.CTG_ID.search(f[0].decode("latin-1"))
        chr_id, s, e = parse_line(f[1])
        prop = 0.0
        if chr_id in spans:
            c = by_id[m.group(0)]
            prop = ora.anno_prop(spans[chr_id][0], spans[chr_id][1], c["chr_start"], c["chr_end"], s, e)
        out.append(ln + b"\t" + fmt4_exact(prop).encode() + b"\n")
    return b"".join(out)


# ---- the pieces every generator mixes in ------------------------------------------------------------------------------
def finish(rng, lines, crlf=None, final_newline=None, blank=0.02):
    """the bytes of str lines: a share of CRLF ends, blank lines between, the last line with or without its newline"""
    crlf = (0.0, 0.1, 0.5)[int(rng.integers(0, 3))] if crlf is None else crlf
    final_newline = bool(rng.integers(0, 2)) if final_newline is None else final_newline
    out = []
    for k, ln in enumerate(lines):
        if k and rng.random() < blank:
            out.append("\n")
        out.append(ln + ("\r\n" if rng.random() < crlf else "\n"))
    data = "".join(out)
    if not final_newline and data:
        data = data[:-2] if data.endswith("\r\n") else data[:-1]
    return data.encode("latin-1")


def with_line(rng, data, line):
    """`data` with one more line put in front of a line picked at random"""
    starts = [0] + [i + 1 for i in range(len(data)) if data[i:i + 1] == b"\n" and i + 1 < len(data)]
    at = starts[int(rng.integers(0, len(starts)))]
    return data[:at] + line + b"\n" + data[at:]


HIGH = "nonsense é".encode()       # a byte >= 0x80 anywhere in the input: GAMS_EUNSUPPORTED


def inside(rng, c, longest=300):
    s = int(rng.integers(c["chr_start"] + 1, c["chr_end"] - longest - 1))
    return s, s + int(rng.integers(0, longest))


def inside_only(order, lines, whole_line, ok):
    """`lines` without those that are located to a ctg and fail ok(ctg, start, end): what the entry would refuse"""
    out = []
    for ln in lines:
        b = ln.encode("latin-1")
        r = parse_line(b if whole_line else b.split(b"\t")[0])
        i = None if r is None else locate_one(order, *r)
        if i is None or ok(order[i], r[1], r[2]):
            out.append(ln)
    return out


def within(c, s, e):
    return c["chr_start"] <= s <= e <= c["chr_end"]


def one_chr_lines(rng, c, n, cols=""):
    """n + 1 located lines on one ctg: the first opens the bucket, n are kept"""
    return ["%s:%d-%d%s" % ((c["chr_id"],) + inside(rng, c) + (cols,)) for _ in range(n + 1)]


# ---- the fourteen families --------------------------------------------------------------------------------------------
def _rng(entry, seed, size):
    return np.random.default_rng([FAMILIES.index(entry), seed, SIZES.index(size)])


def _range_lines(rng, w, size, tails=True):
    """the lines of the locate / --count fuzz; seam: enough of them for 16 KiB"""
    n = LINES[size]
    rgs = fuzz_ranges(rng, w["ctgs"], n)
    t = rng.integers(0, 4, n) if tails else np.zeros(n, int)
    return [r if k == 0 else r + "\tx" * int(k) for r, k in zip(rgs, t)]


def _case_locate(entry, seed, size, refuse):
    rng, w = _rng(entry, seed, size), world()
    lines = _range_lines(rng, w, size)
    if size == "one" and seed % 2:                                 # one line and no row: the point on a ctg start is not located
        lines[0] = "II:1001\tx"
    elif size != "empty":                                          # inside a ctg whatever the draw
        lines[0] = "%s:%d-%d" % ((w["ctgs"][seed % 7]["chr_id"],) + inside(rng, w["ctgs"][seed % 7]))
    data = assemble(rng, lines) if seed % 2 else finish(rng, lines)
    if refuse:
        return dict(data=with_line(rng, data, HIGH), want=dict(rc=_lib.EUNSUPPORTED))
    text = locate_model(w["order"], data, rg_groups(w) if entry == "count" else None)
    return dict(data=data, want=dict(rc=0, text=text, n_rows=text.count(b"\n")))


def _case_anno(entry, seed, size, refuse):
    rng, w = _rng(entry, seed, size), world()
    header, prefix, which = bool(seed & 1), ("", "fz", "a b")[seed % 3], (seed >> 1) & 1
    lines = []
    for k in range(700 if size == "seam" else LINES[size]):
        c = w["ctgs"][int(rng.integers(0, 7))]
        s = max(1, c["chr_start"] + int(rng.integers(-300, c["chr_end"] - c["chr_start"] + 300)))
        e = s + int(rng.choice([0, 1, 10, 500, 5000]))
        r = "%s%s:%s" % (c["chr_id"], ("", "", "(+)", "(-)")[int(rng.integers(0, 4))], "%d" % s if e == s and k % 2 else "%d-%d" % (s, e))
        cid = (c["id"], "rg:%s:%d" % (c["id"], k), "x%s_y" % c["id"])[int(rng.integers(0, 3))]
        lines.append(cid + "\t" + r + "\tmore\t%d" % k * int(rng.integers(0, 2)))
    if header and size != "empty":
        lines.insert(0, "ID\trange")
    data = finish(rng, lines, blank=0.0)
    if refuse:
        return dict(data=with_line(rng, data, b"ctg:I:1\tI:5-9\t" + HIGH), params=dict(header=header, prefix=prefix, which=which),
                    want=dict(rc=_lib.EUNSUPPORTED))
    text = anno_model(w["order"], w["sets"][which], data, header, prefix)
    return dict(data=data, params=dict(header=header, prefix=prefix, which=which),
                want=dict(rc=0, text=text, n_rows=text.count(b"\n")))


def _loader_file(rng, w, size, n_files=1, last=True):
    """one file of a load of n_files; seam: the files share its 1000 lines, and the last one ends in one long bucket"""
    data = fuzz_file(rng, w["ctgs"], 1000 // n_files if size == "seam" else LINES[size])
    if size == "seam" and last:                                             # one bucket of 300 behind the mixed lines
        data += finish(rng, one_chr_lines(rng, w["ctgs"][int(rng.integers(0, 7))], 300), final_newline=True)
    return data


def _case_read_range(entry, seed, size, refuse):
    rng, w = _rng(entry, seed, size), world()
    data = _loader_file(rng, w, size)
    if refuse:
        return dict(data=with_line(rng, data, HIGH), want=dict(rc=_lib.EUNSUPPORTED))
    m = rg_model(w["order"], data)
    flat = [r for b in m["buckets"] for r in b]
    return dict(data=data, want=dict(rc=0, off=np.cumsum([0] + [len(b) for b in m["buckets"]]).tolist(),
                                     seen=[int(x) for x in m["seen"]], start=[r[0] for r in flat], end=[r[1] for r in flat],
                                     line=[r[2] for r in flat]))


def index_queries(per):
    """the queries every index is asked: each kept range's own span, its neighbourhood, and the whole group"""
    n = len(per)
    flat = [(i, s, e) for i, b in enumerate(per) for s, e in b if s <= e]
    g, st, en = [q[0] for q in flat], [q[1] for q in flat], [q[2] for q in flat]
    return (g + g + list(range(n)), st + [max(s - 3, 0) for s in st] + [0] * n, en + [e + 3 for e in en] + [0x7fffffff] * n)


def _case_index(entry, seed, size, refuse):
    """gams_index_create_range_text (even seeds, one file) / gams_index_create_range_files (odd seeds, 1-3 files)"""
    rng, w = _rng(entry, seed, size), world()
    nf = 1 if seed % 2 == 0 else int(rng.integers(1, 4))
    files = [_loader_file(rng, w, size, nf, k == nf - 1) for k in range(nf)]
    if refuse:
        files[-1] = with_line(rng, files[-1], HIGH)
        return dict(data=files, params=dict(files=seed % 2 == 1), want=dict(rc=_lib.EUNSUPPORTED))
    m = model_files(w["order"], files)
    per = [[(p[3], p[4]) for f in range(len(files)) for p, _ in m["kept"][f][i]] for i in range(len(w["order"]))]
    qg, qs, qe = index_queries(per)
    groups = [(np.sort(np.array([s for s, _ in b], np.int64)), np.sort(np.array([e + 1 for _, e in b], np.int64))) for b in per]
    counts = [lapper_count(*groups[g], s, e) for g, s, e in zip(qg, qs, qe)]
    grp = [i if seen else 0xffffffff for i, seen in enumerate(m["seen"])]
    return dict(data=files, params=dict(files=seed % 2 == 1, queries=(qg, qs, qe)),
                want=dict(rc=0, kept=sum(len(b) for b in per), grp=grp, counts=counts))


def _case_loader(entry, seed, size, refuse):
    rng, w = _rng(entry, seed, size), world()
    nf = int(rng.integers(1, 4))
    files = [_loader_file(rng, w, size, nf, k == nf - 1) for k in range(nf)]
    kind, fmt, tag = (RG, FEATURE)[seed % 2], (RECORDS, TSV, RESP)[seed % 3], ('t"a\\g', "", "peak")[seed % 3]
    base = [int(rng.choice([0, 0, 8, 99, 12345])) for _ in w["order"]]
    if size == "large" and seed == 3:                              # one kept row of 20 kB: its block is beyond the writer's stage
        c = w["ctgs"][3]
        files[0] = ("\n".join("n" * 20000 + ".%s:%d-%d" % ((c["chr_id"],) + inside(rng, c)) for _ in range(2)) + "\n").encode() + files[0]
    params = dict(kind=kind, fmt=fmt, tag=tag, base=base)
    if refuse:
        files[0] = with_line(rng, files[0], HIGH)
        return dict(data=files, params=params, want=dict(rc=_lib.EUNSUPPORTED))
    ml = model_loader(w["order"], files, kind, tag, fmt, base)
    return dict(data=files, params=params, want=dict(rc=0, text=ml["text"], off=ml["off"], next=ml["next"],
                                                     per_file=ml["per_file"], n_rows=ml["n_rows"]))


def _peak_data(rng, w, seed, size):
    ctgs = w["ctgs"]
    if size == "empty":
        return b""
    if size == "one":                                              # one kept line: two located ones on a ctg; odd seeds: one
        return finish(rng, one_chr_lines(rng, ctgs[0], 1 - seed % 2, "\t0.5\t1"))      # located line, its bucket stays empty
    long_names = size == "large" and seed == 2                     # 256 rows of ~250 bytes: a block beyond the writers' stages
    lines = pt.synth_lines(ctgs, seed=int(rng.integers(0, 1 << 30)), n=600 if long_names else LINES[size], long_names=long_names)
    lines = inside_only(w["order"], lines, False, within)
    if size == "small":
        lines += ['q"uo\\te.%s:%d-%d\t0.3\ts"g\\' % ((ctgs[1]["chr_id"],) + inside(rng, ctgs[1])) for _ in range(3)]
    return finish(rng, lines)


def _peak_refusal(rng, w, data, size, json):
    """-> (bytes, code): a byte >= 0x80; a peak that leaves its ctg; for the JSON formats a control byte in a kept field"""
    c = w["ctgs"][0]
    if size in ("small", "large"):
        leaving = "I:%d-%d\t0.5\t1" % (c["chr_end"] - 50, c["chr_end"] + 20)
        return data + b"\n" + ("\n".join(["I:%d-%d\t0.5\t1" % (c["chr_start"] + 5, c["chr_start"] + 9), leaving])).encode() + b"\n", _lib.EINVAL
    if size == "seam" and json:
        lines = one_chr_lines(rng, c, 2, "\t0.5\ts\x01g")
        return data + b"\n" + "\n".join(lines).encode() + b"\n", _lib.EUNSUPPORTED
    return with_line(rng, data, HIGH), _lib.EUNSUPPORTED


def _peak_parts(order, data):
    _, kept = pt.buckets(order, data)
    return kept, [pt.ctg_rows(c, pk).encode("latin-1") for c, pk in zip(order, kept)]


def _case_peak_text(entry, seed, size, refuse):
    rng, w = _rng(entry, seed, size), world()
    data = _peak_data(rng, w, seed, size)
    if refuse:
        data, code = _peak_refusal(rng, w, data, size, False)
        return dict(data=data, want=dict(rc=code))
    kept, parts = _peak_parts(w["order"], data)
    return dict(data=data, want=dict(rc=0, text=b"".join(parts), off=np.cumsum([0] + [len(p) for p in parts]).tolist(),
                                     n_rows=sum(len(k) for k in kept)))


def _case_peak_records(entry, seed, size, refuse):
    rng, w = _rng(entry, seed, size), world()
    order = w["order"]
    fmt = ("records", "tsv", "resp")[seed % 3]
    base = {c["id"]: int(rng.choice([0, 0, 8, 99, 12345])) for c in order}
    data = _peak_data(rng, w, seed, size)
    params = dict(fmt=fmt, base=base)
    if refuse:
        fmt = params["fmt"] = "resp"
        data, code = _peak_refusal(rng, w, data, size, True)
        return dict(data=data, params=params, want=dict(rc=code))
    _, kept = pt.buckets(order, data)
    parts = [pr.ctg_records(c, pk, fmt, base[c["id"]]).encode("latin-1") for c, pk in zip(order, kept)]
    return dict(data=data, params=params,
                want=dict(rc=0, text=b"".join(parts), off=np.cumsum([0] + [len(p) for p in parts]).tolist(),
                          next=[base[c["id"]] + len(k) for c, k in zip(order, kept)], n_rows=sum(len(k) for k in kept)))


def _sw_data(rng, w, seed, size):
    ctgs = w["ctgs"]
    if size == "empty":
        return b""
    if size == "one":                                              # odd seeds: one located line, its bucket stays empty
        return finish(rng, one_chr_lines(rng, ctgs[2], 1 - seed % 2))
    lines = swt.synth_lines(ctgs, seed=int(rng.integers(0, 1 << 30)), n=LINES[size])
    return finish(rng, inside_only(w["order"], lines, True, swt.middle_inside))


def _sw_rows(w, data, prm):
    parts = swt.slices(w["order"], data, *prm)
    feats = sum(len(b) for b in swt.buckets(w["order"], data)[1])
    return parts, feats


def _sw_refusal(rng, w, data, size):
    if size in ("small", "large"):                                 # a kept feature whose middle leaves its ctg
        c = w["ctgs"][0]
        two = ["I:%d-%d" % (c["chr_start"] + 5, c["chr_start"] + 9), "I:%d-%d" % (c["chr_end"] - 10, c["chr_end"] + 90)]
        return data + b"\n" + "\n".join(two).encode() + b"\n", _lib.EINVAL
    return with_line(rng, data, HIGH), _lib.EUNSUPPORTED


def sw_input(entry, seed, size, refuse=None):
    """-> (input bytes, params, the refusal's code or 0) of a case of the three sw families, without running the model"""
    refuse = (seed == REFUSED and size != "empty") if refuse is None else refuse
    rng, w = _rng(entry, seed, size), world()
    prm = SW_PARAMS[seed % 4]
    params = dict(size=prm[0], mx=prm[1], resize=prm[2])
    if entry != "sw_text":
        params["n_sets"] = 0 if entry == "sw_summary" else 1 + (seed + SIZES.index(size)) % 4
        params["count"] = entry == "sw_summary" and seed % 2 == 1     # -a gc,count over the world's rg index
    data, code = _sw_data(rng, w, seed, size), 0
    if refuse:
        data, code = _sw_refusal(rng, w, data, size)
    return data, params, code


def _case_sw_text(entry, seed, size, refuse):
    w = world()
    data, params, code = sw_input(entry, seed, size, refuse)
    if code:
        return dict(data=data, params=params, want=dict(rc=code))
    parts, feats = _sw_rows(w, data, SW_PARAMS[seed % 4])
    text = b"".join(parts)
    return dict(data=data, params=params, want=dict(rc=0, text=text, off=np.cumsum([0] + [len(p) for p in parts]).tolist(),
                                                    n_features=feats, n_rows=text.count(b"\n")))


def _with_rg_count(rows, group):
    """the rows of one ctg with their ninth field: count_rg over the window (utils.rs:24-36: Lapper::count(window start,
    window end) over the rg index of its ctg)"""
    out = []
    for row in rows.split(b"\n")[:-1]:
        f = row.split(b"\t")
        _, s, e = parse_line(f[1])
        f[8] = b"%d" % lapper_count(*group, s, e)
        out.append(b"\t".join(f) + b"\n")
    return b"".join(out)


def _case_sw_summary(entry, seed, size, refuse):
    w = world()
    data, params, code = sw_input(entry, seed, size, refuse)
    if code:
        return dict(data=data, params=params, want=dict(rc=code))
    prm, n_sets = SW_PARAMS[seed % 4], params["n_sets"]
    parts, feats = _sw_rows(w, data, prm)
    if params["count"]:
        parts = [_with_rg_count(p, g) for p, g in zip(parts, rg_groups(w))]
    rows = b"".join(parts)
    want = dict(rc=0, n_features=feats, n_rows=rows.count(b"\n"))
    if n_sets:
        cols = [[r.rsplit(b"\t", 1)[1] for r in sas.annotate(rows, w["order"], s).split(b"\n")[:-1]] for s in w["sets"][:n_sets]]
        rows = b"".join(b"\t".join((r,) + tuple(cols[k % 2][i] for k in range(n_sets))) + b"\n"      # set k is sets[k % 2]
                        for i, r in enumerate(rows.split(b"\n")[:-1]))
        table = sas.Table(["s%d" % k for k in range(n_sets)]).add_text(rows)
        want["prop"] = table.prop(prm[1])[0].tolist()
    else:
        table = sws.Table(("gc", "count") if params["count"] else ("gc",)).add_text(rows)
    arr = table.arrays(prm[1])
    want.update(count=arr["count"][0], sum=arr["sum"][0], nan=arr["nan"][0], rg_count=arr["rg_count"][0])
    return dict(data=data, params=params, want=want)


def _runlist_value(rng, n, top):
    """a runlist of n tokens: unsorted, overlapping and adjacent spans, single positions"""
    lo = rng.integers(1, top, n)
    ln = rng.choice([0, 0, 1, 5, 40, 2000], n)
    toks = [(int(a), int(min(a + b, rt.I32_MAX))) for a, b in zip(lo, ln)]
    toks += [(b + 1, b + 3) for _, b in toks[:n // 10] if b + 3 <= rt.I32_MAX]         # adjacent: joins lo == hi + 1
    order = rng.permutation(len(toks))
    return rt.runlist_of([toks[i] for i in order])


def _case_runlist(entry, seed, size, refuse):
    rng = _rng(entry, seed, size)
    pretty, crlf = bool(seed & 1), seed == 3
    n = dict(empty=0, one=1, small=70, seam=1500, large=6000)[size]
    if size == "empty":
        pairs = []
    elif size == "one":                                            # odd seeds: groups and no span
        pairs = [("none", ""), ("dash", "-")] if seed % 2 else [("I", _runlist_value(rng, 1, 10 ** 6))]
    else:
        share = [0.4, 0.33, 0.27] if size == "seam" else rng.dirichlet([3, 1, 1])      # seam: 257-700 spans in a group
        top = 10 ** int(rng.integers(8 if size == "seam" else 5, 10))      # seam: too sparse to join into few spans
        pairs = [("I", _runlist_value(rng, max(int(n * share[0]), 1), top)), ("none", ""),
                 ("II", _runlist_value(rng, max(int(n * share[1]), 1), 2 * 10 ** 9)), ("dash", "-"),
                 ("chr III", _runlist_value(rng, max(int(n * share[2]), 1), 50000))]
        pairs = [pairs[i] for i in rng.permutation(len(pairs))]
    data = rt.doc(pairs, pretty=pretty, crlf=crlf)
    if refuse and size != "empty":
        bad = [('a\\"b', "1-5"), ("neg", "-5--1"), ("I", "7"), ("e", ",1-2")][SIZES.index(size) - 1]     # I: a key twice
        data = rt.doc(pairs + [bad], pretty=pretty, crlf=crlf)
    if not rt.device_takes(data):
        return dict(data=data, want=dict(rc=_lib.EUNSUPPORTED))
    sets = rt.model(data)
    return dict(data=data, want=dict(rc=0, names=list(sets), n_spans=sum(v[0].size for v in sets.values()),
                                     lo=[v[0].tolist() for v in sets.values()], hi=[v[1].tolist() for v in sets.values()]))


def _case_gen(entry, seed, size, refuse):
    rng = _rng(entry, seed, size)
    width, eol = (60, 61, 17, 256)[seed % 4], (b"\n", b"\r\n")[seed == 1 or seed == REFUSED]
    total = dict(empty=0, one=40, small=4000, seam=24000, large=100000)[size]
    piece, fill, min_len = ((700, 5, 20), (60, 3, 10), (3000, 50, 100), (97, 1, 1))[(seed + SIZES.index(size)) % 4]
    if size == "seam":
        piece, fill, min_len = 40, 3, 10                           # more than 256 ctgs in one chromosome
    recs = []
    if size != "empty":
        k = 1 if size == "one" else 2 if size == "seam" else int(rng.integers(2, 6))
        cuts = np.sort(rng.integers(0, total, k - 1)).tolist()
        for j, (a, b) in enumerate(zip([0] + cuts, cuts + [total])):
            runs = [(int(rng.integers(0, max(b - a, 1))), int(rng.choice([1, 2, 3, 5, 49, 50, 200]))) for _ in range((b - a) // 900 + 1)]
            recs.append(("c%d" % j + (" desc" if j % 2 else ""), gt.with_runs(b - a, int(rng.integers(0, 1 << 30)), runs)))
    data = gt.fasta(recs, width, eol)
    if size not in ("empty", "one") and seed % 2 == 0:
        data = data[:-len(eol)]                                    # no final newline
    params = dict(piece=piece, fill=fill, min_len=min_len)
    if refuse and size != "empty":
        k = SIZES.index(size)
        data = (b"x" + data, data.replace(b"c0", b"c\xe9", 1), data + b">c0 again\nACGT\n", data.replace(eol, b" " + eol, 2))[k - 1]
    code = gt.refusal(data)
    if code:
        return dict(data=data, params=params, want=dict(rc=getattr(_lib, code)))
    ctgs, chr_len = gt.model(data, piece, fill, min_len)
    return dict(data=data, params=params, want=dict(rc=0, chrs=list(chr_len), chr_len=chr_len, table=gt.table(ctgs),
                                                    seqs=[c["seq"] for c in ctgs]))


def _case_locate_seq(entry, seed, size, refuse):
    rng, w = _rng(entry, seed, size), world()
    ctgs = w["ctgs"]
    if size == "empty":
        lines = []
    elif size == "one":                                            # odd seeds: the point on a ctg start, not located
        lines = ["II:1001"] if seed % 2 else ["%s:%d-%d" % ((ctgs[4]["chr_id"],) + inside(rng, ctgs[4]))]
    elif size == "large":                                          # one whole-ctg row among 2000: text beyond one granule
        lines = [ln.decode() for ln in lst.synth_lines(ctgs, seed=int(rng.integers(0, 1 << 30)), n=LINES[size])]
    else:
        lines = [ln.decode() for ln in lst.synth_lines(ctgs[:2], seed=int(rng.integers(0, 1 << 30)), n=LINES[size])]
    data = finish(rng, inside_only(w["order"], lines, False, within))
    if refuse:
        if size in ("small", "large"):                             # a range that leaves the ctg it is located to
            c = ctgs[1]
            data += b"\n" + b"I:%d-%d\n" % (c["chr_end"] - 5, c["chr_end"] + 5)
            code = _lib.EINVAL
        else:
            data, code = with_line(rng, data, HIGH), _lib.EUNSUPPORTED
        return dict(data=data, want=dict(rc=code))
    text = lst.model(w["order"], data)
    return dict(data=data, want=dict(rc=0, text=text, n_rows=len(lst.records(w["order"], data))))


_CASES = dict(locate=_case_locate, count=_case_locate, anno=_case_anno, read_range=_case_read_range, index=_case_index,
              loader=_case_loader, peak_text=_case_peak_text, peak_records=_case_peak_records, sw_text=_case_sw_text,
              sw_summary=_case_sw_summary, sw_summary_anno=_case_sw_summary, runlist_text=_case_runlist, gen_text=_case_gen,
              locate_seq=_case_locate_seq)


def build(entry, seed, size):
    """the case, computed afresh (case() caches it)"""
    c = _CASES[entry](entry, seed, size, seed == REFUSED and size != "empty")
    c.setdefault("params", {})
    c.update(entry=entry, seed=seed, size=size)
    return c


@functools.lru_cache(maxsize=None)
def case(entry, seed, size):
    """-> dict(entry, seed, size, data = the input bytes (a list of files for index and loader), params, want = the
    expected outcome); the model runs once per (entry, seed, size)"""
    return build(entry, seed, size)


def corpus():
    """every (entry, seed, size) the GPU tests may draw"""
    return [(e, s, z) for e in FAMILIES for s in SEEDS + (REFUSED,) for z in SIZES]


def input_bytes(c):
    return b"".join(c["data"]) if isinstance(c["data"], list) else c["data"]


# ---- comparing outcomes -----------------------------------------------------------------------------------------------
def first_difference(got, exp):
    """where two byte strings part, with the bytes around it"""
    n = next((i for i, (a, b) in enumerate(zip(got, exp)) if a != b), min(len(got), len(exp)))
    return "lengths %d / %d, first difference at byte %d: got %r, expected %r" % (len(got), len(exp), n, got[max(n - 40, 0):n + 40],
                                                                                 exp[max(n - 40, 0):n + 40])


def difference(got, want):
    """None where two outcomes are equal, else a line that says where they part"""
    if got.get("rc") != want["rc"]:
        return "rc %r, expected %r" % (got.get("rc"), want["rc"])
    for k, v in want.items():
        g = got.get(k)
        if isinstance(v, bytes):
            if g != v:
                return "%s: %s" % (k, first_difference(g or b"", v))
        elif isinstance(v, list) and v and isinstance(v[0], bytes):
            for i, (a, b) in enumerate(zip(g, v)):
                if a != b:
                    return "%s[%d]: %s" % (k, i, first_difference(a, b))
            if len(g) != len(v):
                return "%s: %d items, expected %d" % (k, len(g), len(v))
        elif g != v:
            if isinstance(v, list) and isinstance(g, list):
                i = next((i for i, (a, b) in enumerate(zip(g, v)) if a != b), min(len(g), len(v)))
                return "%s: lengths %d / %d, first difference at [%d]: got %r, expected %r" % (k, len(g), len(v), i, g[i:i + 4], v[i:i + 4])
            return "%s: got %r, expected %r" % (k, g, v)
    return None
