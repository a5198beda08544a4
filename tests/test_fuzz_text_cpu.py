"""The corpus of tests/fuzz_text.py held to account without a GPU: every (entry, seed, size) the call-sequence tests of
tests/test_gpu_call_sequences.py may draw is built the same twice, its model answers or names the refusal's code, the
host's CPU-only routes (read_fasta, read_runlist_json, the peak record formatter) agree with the models, the corpus holds
the shapes the kernels can go wrong at, and for every family two planted near-miss variants of its rule change the
expected outcome of at least one case: a corpus that cannot tell the variant from the rule would be blind there."""
import contextlib

import numpy as np
import pytest

import fuzz_text as ft
import gen_text as gt
import helpers
import locate_seq_text as lst
import peak_records as pr
import peak_text as pt
import runlist_text as rt
import sw_summary as sws
import sw_text as swt
import test_loader_text_cpu as tlc
import test_rg_text_cpu as trc
from gams_amd import _lib, host
from oracle import oracle as ora

KIB16 = 16 * 1024
SW = ("sw_text", "sw_summary", "sw_summary_anno")
# bytes a block of rows may have for its writer to stage it in LDS (csrc/text.hip: kPeakStage, GAMS_PEAK_REC_STAGE /
# GAMS_PEAK_REC_TSV_STAGE in include/gams_gpu_diag.h, kRecStage; csrc/sw.hip: kSwTextStage), and the rows of a block (256;
# kSwTextBlock = 512 for the sw rows)
STAGE = dict(peak_text=32768, peak_records=dict(records=98304, resp=98304, tsv=32768), loader=49152, sw_text=49152)
BLOCK_ROWS = dict(sw_text=512)
# the entries that put their kept rows into buckets (per ctg, per group, per chromosome); the others print one stream of rows
BUCKETED = ("read_range", "index", "loader", "peak_text", "peak_records", "sw_text", "sw_summary", "sw_summary_anno",
            "runlist_text", "gen_text")


def cases(entry):
    return [ft.case(entry, s, z) for s in ft.SEEDS + (ft.REFUSED,) for z in ft.SIZES]


# ---- 1. the cases themselves ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ft.FAMILIES)
def test_same_arguments_same_bytes_and_the_model_answers(entry):
    for c in cases(entry):
        again = ft.sw_input(entry, c["seed"], c["size"])[:2] if entry in SW else [ft.build(entry, c["seed"], c["size"])[k] for k in ("data", "params")]
        assert again[0] == c["data"] and repr(again[1]) == repr(c["params"]), (entry, c["seed"], c["size"])
        rc = c["want"]["rc"]
        if c["seed"] == ft.REFUSED and c["size"] != "empty":
            assert rc in (_lib.EINVAL, _lib.EUNSUPPORTED) and list(c["want"]) == ["rc"]
        else:
            assert rc == 0 and len(c["want"]) > 1
        assert len(ft.input_bytes(c)) < 128 * 1024
    if entry not in SW:
        c = cases(entry)[8]
        assert ft.difference(ft.build(entry, c["seed"], c["size"])["want"], c["want"]) is None


def test_the_world():
    w = ft.world()
    ctgs = w["ctgs"]
    assert len(ctgs) <= 8 and len({c["chr_id"] for c in ctgs}) == 3
    assert all(len(c["seq"]) == c["chr_end"] - c["chr_start"] + 1 <= 30000 for c in ctgs)
    one = [c for c in ctgs if c["chr_id"] == "I"]
    assert len(one) == 2 and one[1]["chr_start"] > one[0]["chr_end"] + 1                 # two ctgs with a gap
    assert min(c["chr_start"] for c in ctgs if c["chr_id"] == "II") == 1001
    assert all(set(c["seq"]) <= set(b"ACGTacgtN") and b"N" in c["seq"] for c in ctgs)
    assert len(w["sets"]) == 2 and len(w["rg_records"]) > 100
    assert ft.world() is w


# ---- 2. the host's CPU-only routes ------------------------------------------------------------------------------------
def test_host_readers_and_formatter_agree_with_the_models():
    for c in cases("gen_text"):
        if c["want"]["rc"] != _lib.EINVAL:
            assert host.read_fasta(c["data"]) == gt.records(c["data"])
    for c in cases("runlist_text"):
        want = rt.verdict(c["data"])
        if want is not None:
            assert rt.same_sets(host.read_runlist_json(c["data"]), want)
        assert want is not None or c["want"]["rc"]
    order = ft.world()["order"]
    for c in cases("peak_records"):
        if c["want"]["rc"] == 0:
            base = c["params"]["base"]
            _, kept = pt.buckets(order, c["data"])
            tsv = "".join(pr.ctg_records(k, pk, "tsv", base[k["id"]]) for k, pk in zip(order, kept)).encode("latin-1")
            assert host.peak_rows_records(tsv, c["params"]["fmt"]) == c["want"]["text"]


# ---- 3. what the corpus must hold -------------------------------------------------------------------------------------
def records_of(text, resp):
    return [b"*3\r\n" + r for r in text.split(b"*3\r\n")[1:]] if resp else [r + b"\n" for r in text.split(b"\n")[:-1]]


def slices(w):
    return [w["text"][a:b] for a, b in zip(w["off"], w["off"][1:])]


def largest_bucket(c):
    """the most kept rows one bucket of the case holds (for an entry without buckets: its rows)"""
    e, w = c["entry"], c["want"]
    if e in ("locate", "count", "anno", "locate_seq"):
        return w["n_rows"]
    if e == "read_range":
        return max(np.diff(w["off"]))
    if e == "index":
        return max(w["counts"][-len(w["grp"]):])
    if e == "loader":
        return max(len(records_of(s, c["params"]["fmt"] == tlc.RESP)) for s in slices(w))
    if e == "peak_text":
        return max(s.count(b"\n") for s in slices(w))
    if e == "peak_records":
        return max(n - c["params"]["base"][k["id"]] for n, k in zip(w["next"], ft.world()["order"]))
    if e in SW:
        return max(len(b) for b in swt.buckets(ft.world()["order"], c["data"])[1])
    if e == "runlist_text":
        return max([len(lo) for lo in w["lo"]] + [0])
    assert e == "gen_text"
    return max([sum(t[1] == k for t in w["table"]) for k in w["chrs"]] + [0])


def block_bytes(c):
    """the bytes of every block of rows the writer sees (256 rows, 512 for the sw rows), in the entry's order"""
    n = BLOCK_ROWS.get(c["entry"], 256)
    recs = records_of(c["want"]["text"], c["params"].get("fmt") in ("resp", tlc.RESP) and c["entry"] != "peak_text")
    return [sum(map(len, recs[b:b + n])) for b in range(0, len(recs), n)]


@pytest.mark.parametrize("entry", ft.FAMILIES)
def test_corpus_conditions(entry):
    """A seam case holds 257 to 700 kept rows in one bucket.  locate, --count, anno and locate --seq have no buckets: their
    rows are one stream, cut into blocks of 256 wherever it stands, so for them only the lower bound is asked (more than one
    block) and the input's 16-48 KiB decide the size.  anno prints a row for every line, so it alone has no input with lines
    and without rows."""
    cs = cases(entry)
    refused = [c for c in cs if c["want"]["rc"]]
    assert 0 < len(refused) <= len(cs) / 4
    assert {c["size"] for c in cs if c["want"]["rc"] == 0} == set(ft.SIZES)
    good = [c for c in cs if c["want"]["rc"] == 0]
    assert any(largest_bucket(c) == 0 for c in good), "no case without a kept row"
    if entry != "anno":                                            # lines that are located (or groups, or bases) and nothing kept
        assert any(largest_bucket(c) == 0 and ft.input_bytes(c) for c in good), "no input with lines and without a kept row"
    assert any(largest_bucket(c) > 256 for c in good), "no bucket beyond 256 rows"
    inputs = [ft.input_bytes(c) for c in good]
    assert any(len(d) > KIB16 for d in inputs) and any(b"\r\n" in d for d in inputs)
    assert any(d and not d.endswith(b"\n") for d in inputs)
    for c in good:
        if c["size"] == "seam":
            assert KIB16 < len(ft.input_bytes(c)) < 3 * KIB16, (c["seed"], len(ft.input_bytes(c)))
            assert largest_bucket(c) > 256, (c["seed"], largest_bucket(c))
            assert largest_bucket(c) <= 700 or entry not in BUCKETED, (c["seed"], largest_bucket(c))
    if entry in STAGE:
        sizes = [(b, STAGE[entry][c["params"]["fmt"]] if entry == "peak_records" else STAGE[entry]) for c in good for b in block_bytes(c)]
        assert any(b > st for b, st in sizes) and any(0 < b <= st for b, st in sizes)


# ---- 4. discrimination ------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def patched(obj, name, new):
    old = getattr(obj, name)
    setattr(obj, name, new)
    try:
        yield
    finally:
        setattr(obj, name, old)


def locate_last(ctgs, chr_id, s, e):
    """locate_one, but the LAST ctg in (start, stop) order that the range touches"""
    hits = [(c["chr_start"], c["chr_end"] + 1, i) for i, c in enumerate(ctgs) if c["chr_id"] == chr_id and c["chr_start"] < e and c["chr_end"] + 1 > s]
    return max(hits)[2] if hits else None


def locate_closed(ctgs, chr_id, s, e):
    """locate_one with a closed query: a point range on a ctg start is located"""
    hits = [(c["chr_start"], c["chr_end"] + 1, i) for i, c in enumerate(ctgs) if c["chr_id"] == chr_id and c["chr_start"] <= e and c["chr_end"] + 1 > s]
    return min(hits)[2] if hits else None


def count_stop_exclusive(starts, stops, qs, qe):
    """Lapper::count with #{stop < qs}: an interval that ends on the query's first base is missed... and counted"""
    return int(np.searchsorted(starts, qe, "left")) - int(np.searchsorted(stops, qs, "left"))


def count_end_inclusive(starts, stops, qs, qe):
    """Lapper::count with #{start <= qe}"""
    return int(np.searchsorted(starts, qe, "right")) - int(np.searchsorted(stops, qs, "right"))


def prop_variant(clip=True, hi_exclusive=False):
    def prop(lo, hi, cs, ce, s, e):
        lo, hi = np.asarray(lo, np.int64), np.asarray(hi, np.int64) - int(hi_exclusive)
        a, b = (max(s, cs), min(e, ce)) if clip else (s, e)
        card = int(np.maximum(np.minimum(hi, b) - np.maximum(lo, a) + 1, 0).sum())
        return float(np.float32(card) / np.float32(e - s + 1))
    return prop


def rg_model_variant(keep_first=False, per_chr=False):
    def model(ctgs, data):
        seen, buckets, done = [False] * len(ctgs), [[] for _ in ctgs], set()
        for k, ln in enumerate(trc.rust_lines(data)):
            r = trc.parse_line(ln)
            i = None if r is None else trc.locate_one(ctgs, *r)
            if i is None:
                continue
            key = ctgs[i]["chr_id"] if per_chr else i
            if keep_first or key in done:
                buckets[i].append((r[1], r[2], k))
            done.add(key)
            seen[i] = True
        return dict(seen=seen, buckets=buckets)
    return model


def parse_untrimmed(line):
    """parse_line without the trim of trailing spaces"""
    return None if line.endswith(b" ") else PARSE(line)


PARSE = trc.parse_line


def model_files_per_load(ctgs, files):
    """model_files with the first located line of a ctg dropped once per LOAD, not once per file"""
    m = MODEL_FILES(ctgs, [b"".join(f if f.endswith(b"\n") or not f else f + b"\n" for f in files)])
    cuts = np.cumsum([0] + [len(trc.rust_lines(f)) for f in files])
    kept = [[[(p, k - cuts[f]) for p, k in m["kept"][0][i] if cuts[f] <= k < cuts[f + 1]] for i in range(len(ctgs))] for f in range(len(files))]
    return dict(seen=m["seen"], kept=kept, lines=[len(trc.rust_lines(f)) for f in files])


MODEL_FILES = tlc.model_files


def canonical_always_a_pair(parts):
    """Range::to_string() that prints start-end for a point range too"""
    name, chr_id, strand, s, e = parts
    return (name + "." if name else "") + chr_id + (f"({strand})" if strand else "") + ":" + f"{s}-{e}"


def peak_buckets_variant(keep_first=False, by_line=False):
    def buckets(ctgs, data):
        located, kept = [0] * len(ctgs), [[] for _ in ctgs]
        for k, ln in enumerate(trc.rust_lines(data)):
            parts = ln.split(b"\t")
            r = trc.parse_line(parts[0])
            i = None if r is None else trc.locate_one(ctgs, *r)
            if i is None:
                continue
            if located[i] or keep_first:
                kept[i].append((r[1], r[2], parts[2].decode("latin-1"), pt.name_prefix(parts[0]), k))
            located[i] += 1
        return located, [b if by_line else sorted(b, key=lambda p: p[0]) for b in kept]
    return buckets


def sw_buckets_keep_first(ctgs, data):
    located, kept = [0] * len(ctgs), [[] for _ in ctgs]
    for k, ln in enumerate(trc.rust_lines(data)):
        r = trc.parse_line(ln)
        i = None if r is None else trc.locate_one(ctgs, *r)
        if i is not None:
            kept[i].append((r[1], r[2], k))
            located[i] += 1
    return located, kept


def sw_features_from_zero(ctgs, data):
    return [[(fid.rsplit(":", 1)[0] + ":%d" % k, s, e) for k, (fid, s, e) in enumerate(f)] for f in FEATURES(ctgs, data)]


FEATURES = swt.features
UNITS = sws.units


def units_three_places(field):
    m = UNITS(field)
    return None if m is None else m - m % 10


def normalise_no_adjacent_join(spans):
    lo, hi = [], []
    for a, b in sorted(spans):
        if lo and a <= hi[-1]:
            hi[-1] = max(hi[-1], b)
        else:
            lo.append(a)
            hi.append(b)
    return np.array(lo, np.int32), np.array(hi, np.int32)


def normalise_first_wins(spans):
    """joins a span only into the one in front of it IN FILE ORDER, then sorts"""
    lo, hi = [], []
    for a, b in spans:
        if lo and lo[-1] <= a <= hi[-1] + 1:
            hi[-1] = max(hi[-1], b)
        else:
            lo.append(a)
            hi.append(b)
    order = np.argsort(lo, kind="stable") if lo else []
    return np.array([lo[i] for i in order], np.int32), np.array([hi[i] for i in order], np.int32)


GEN_CTGS = helpers.gen_ctgs


def gen_variant(piece=0, fill=0):
    return lambda chr_id, seq, p=500000, f=50, m=5000: GEN_CTGS(chr_id, seq, p + piece, f + fill, m)


def seq_model_variant(whole_line=False, end_exclusive=False):
    def model(ctgs, data):
        out = []
        lines = trc.rust_lines(data)
        for k, rg, i, s, e in lst.records(ctgs, data):
            c = ctgs[i]
            out.append(b">" + (lines[k] if whole_line else rg) + b"\n" + bytes(c["seq"][s - c["chr_start"]:e - c["chr_start"] + 1 - int(end_exclusive)]) + b"\n")
        return b"".join(out)
    return model


def ctg_records_from_one(c, pk, fmt, base):
    return CTG_RECORDS(c, pk, fmt, 0)


CTG_RECORDS = pr.ctg_records

# family -> [(what the variant gets wrong, the patches that plant it, the (seed, size) of a corpus case that tells)]
VARIANTS = {
    "locate": [("the last ctg a range touches, not the first", [(lst, "locate_one", locate_last)], (0, "small")),
               ("a point range on a ctg start is located", [(lst, "locate_one", locate_closed)], (0, "small"))],
    "count": [("#{stop < qs} instead of #{stop <= qs}", [(ft, "lapper_count", count_stop_exclusive)], (0, "seam")),
              ("#{start <= qe} instead of #{start < qe}", [(ft, "lapper_count", count_end_inclusive)], (1, "seam"))],
    "anno": [("the range is not cut to its ctg", [(ora, "anno_prop", prop_variant(clip=False))], (0, "small")),
             ("a span's last base is not counted", [(ora, "anno_prop", prop_variant(hi_exclusive=True))], (2, "one"))],
    "read_range": [("the first located line of a ctg is kept", [(ft, "rg_model", rg_model_variant(keep_first=True))], (0, "one")),
                   ("drop-first per chromosome instead of per ctg", [(ft, "rg_model", rg_model_variant(per_chr=True))], (0, "small"))],
    "index": [("drop-first per load instead of per file", [(ft, "model_files", model_files_per_load)], (1, "small")),
              ("#{stop < qs} instead of #{stop <= qs}", [(ft, "lapper_count", count_stop_exclusive)], (0, "seam"))],
    "loader": [("drop-first per load instead of per file", [(tlc, "model_files", model_files_per_load)], (1, "small")),
               ("a point range printed as start-end", [(tlc, "canonical", canonical_always_a_pair)], (0, "small"))],
    "peak_text": [("the first located line of a ctg is kept", [(pt, "buckets", peak_buckets_variant(keep_first=True))], (0, "one")),
                  ("peaks sorted by line instead of start", [(pt, "buckets", peak_buckets_variant(by_line=True))], (0, "small"))],
    "peak_records": [("serials from 1 instead of behind serial_base", [(pr, "ctg_records", ctg_records_from_one)], (0, "one")),
                     ("strings not escaped in the JSON", [(pr, "escape", lambda s: s)], (0, "small"))],
    "sw_text": [("the first located line of a ctg is kept", [(swt, "buckets", sw_buckets_keep_first)], (0, "one")),
                ("features numbered from 0", [(swt, "features", sw_features_from_zero)], (0, "one"))],
    "sw_summary": [("the first located line of a ctg is kept", [(swt, "buckets", sw_buckets_keep_first)], (0, "one")),
                   ("a statistic summed at three decimal places", [(sws, "units", units_three_places)], (0, "one"))],
    "sw_summary_anno": [("a span's last base is not counted", [(ora, "anno_prop", prop_variant(hi_exclusive=True))], (0, "one")),
                        ("the first located line of a ctg is kept", [(swt, "buckets", sw_buckets_keep_first)], (0, "one"))],
    "runlist_text": [("lo == hi + 1 is not joined", [(rt, "normalise", normalise_no_adjacent_join)], (0, "small")),
                     ("joined in file order, not in sorted order", [(rt, "normalise", normalise_first_wins)], (0, "small"))],
    "gen_text": [("fill off by one", [(helpers, "gen_ctgs", gen_variant(fill=1))], (1, "small")),
                 ("piece off by one", [(helpers, "gen_ctgs", gen_variant(piece=1))], (1, "small"))],
    "locate_seq": [("the header echoes the whole line", [(lst, "model", seq_model_variant(whole_line=True))], (0, "small")),
                   ("the range's last base is not copied", [(lst, "model", seq_model_variant(end_exclusive=True))], (0, "one"))],
}


def expected_with(entry, seed, size, patches):
    """the expected outcome of a case under the planted variant"""
    with contextlib.ExitStack() as st:
        for obj, name, new in patches:
            st.enter_context(patched(obj, name, new))
        return ft.build(entry, seed, size)["want"]


@pytest.mark.parametrize("entry", ft.FAMILIES)
def test_planted_variants_change_an_expected_outcome(entry):
    assert len(VARIANTS[entry]) >= 2
    for what, patches, (seed, size) in VARIANTS[entry]:
        want = ft.case(entry, seed, size)["want"]
        other = expected_with(entry, seed, size, patches)
        assert want["rc"] == 0 and other["rc"] == 0 and ft.difference(other, want) is not None, \
            "case (%d, %s) of %s does not tell: %s" % (seed, size, entry, what)
        assert ft.difference(ft.build(entry, seed, size)["want"], want) is None                # the patches are gone
