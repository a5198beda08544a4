"""CPU checks of the rg loader on the device (the bytes of a .rg file -> the rg index): the library and the host layer
declare and export it, the binding refuses two rg sources at once, and a pure-Python model of its semantics
(utils.rs:39-67 read_range with the drop-first quirk, then redis.rs:288-299) reproduces the reference's
79 -> 71 -> 69 on spo11_hot.rg.  tests/test_gpu_rg_text.py checks the device against this model."""
import ctypes as C
import os
import re

import pytest

import helpers
from gams_amd import _lib, host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GPU_RG = ("gams_gpu_read_range_text", "gams_index_create_range_text")
HOST_RG = ("gams_host_locate_rg", "gams_host_locate_text_rg", "gams_host_read_range_text",
           "gams_host_read_range_text_get", "gams_host_sw_actions_rg", "gams_host_sw_multi_actions_rg",
           "gams_host_rg_load")


# ---- the model ------------------------------------------------------------------------------------
def rust_lines(data):
    """BufRead::lines(): split on \\n, one \\r before it dropped, a last line without \\n kept as it is"""
    segs = data.split(b"\n")
    last = segs.pop()
    out = [s[:-1] if s.endswith(b"\r") else s for s in segs]
    if last:
        out.append(last)
    return out


# intspan Range::from_str over the whole line: [name.]chr[(strand)]:start[-end]; the name ends at the FIRST dot, the
# strand's text is not looked at, the numbers have 1-10 digits and runs of '-' / '_' between them
RANGE = re.compile(r"^(?:[^.]*\.)?([\w/-]+)(?:\([^)]*\))?:(\d{1,10})(?:[-_]+(\d{1,10}))?$", re.A)


def parse_line(line):
    """(chr, start, end) of a line, or None: the trailing '\\r', '\\n' and spaces trimmed, values <= INT32_MAX"""
    m = RANGE.match(line.decode("latin-1").rstrip("\r\n "))
    if not m:
        return None
    s = int(m.group(2))
    e = int(m.group(3)) if m.group(3) else s
    if s > 0x7fffffff or e > 0x7fffffff:
        return None
    return m.group(1), s, e


def locator_order(ctgs):
    """the ctgs as gams::Locator orders them: by chromosome (byte order), the caller's order inside one"""
    by_chr = {}
    for c in ctgs:
        by_chr.setdefault(c["chr_id"], []).append(c)
    return [c for k in sorted(by_chr, key=lambda k: k.encode()) for c in by_chr[k]]


def locate_one(ctgs, chr_id, s, e):
    """Lapper::find(s, e).next() over the chromosome's [chr_start, chr_end + 1): the first ctg in (start, stop) order
    with start < e and stop > s (the half-open query: a point range on a ctg start is not located); its position in
    `ctgs`, or None"""
    hits = [(c["chr_start"], c["chr_end"] + 1, i) for i, c in enumerate(ctgs)
            if c["chr_id"] == chr_id and c["chr_start"] < e and c["chr_end"] + 1 > s]
    return min(hits)[2] if hits else None


def model(ctgs, data):
    """read_range over the bytes of ONE file.  -> dict(lines, valid, located = the counts; seen[i] = ctg i of `ctgs`
    had a located line; buckets[i] = [(start, end, line)] kept for ctg i in file order, the first located line of
    every ctg dropped)"""
    n_valid = n_located = 0
    seen = [False] * len(ctgs)
    buckets = [[] for _ in ctgs]
    lines = rust_lines(data)
    for k, ln in enumerate(lines):
        r = parse_line(ln)
        if r is None:
            continue
        n_valid += 1
        i = locate_one(ctgs, *r)
        if i is None:
            continue
        n_located += 1
        if seen[i]:
            buckets[i].append((r[1], r[2], k))           # and_modify(push)
        seen[i] = True                                   # or_default(): the first range only creates the bucket
    return dict(lines=len(lines), valid=n_valid, located=n_located, seen=seen, buckets=buckets)


# ---- tests ----------------------------------------------------------------------------------------
def test_new_entries_are_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "gams_gpu.h")).read()
    lib = C.CDLL(_lib.SO_PATH)
    for name in GPU_RG:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert name in _lib.PROTOTYPES, name
        assert hasattr(lib, name), name
    diag = open(os.path.join(ROOT, "include", "gams_gpu_diag.h")).read()
    assert "gams_gpu_last_stage_ms" in diag and "gams_gpu_last_stage_ms" in _lib.PROTOTYPES
    hl = C.CDLL(host.SO_PATH)
    for name in HOST_RG:
        assert hasattr(hl, name), name


def test_null_arguments_are_einval():
    lib = _lib.load()
    n = C.c_uint64()
    ix = C.c_void_p()
    assert lib.gams_gpu_read_range_text(None, None, None, b"I:1-2\n", 6, None, None, None, None, None, 0,
                                        C.byref(n)) == _lib.EINVAL
    assert lib.gams_index_create_range_text(None, None, None, b"I:1-2\n", 6, C.byref(ix), None, C.byref(n)) == _lib.EINVAL


class _NoDevice:
    h = None


def test_two_rg_sources_raise_value_error():
    ctg = dict(id="ctg:I:1", chr_id="I", chr_start=1, chr_end=1000, seq=b"A" * 1000)
    recs, data = [("ctg:I:1", "I:5-8")], b"I:5-8\n"
    with pytest.raises(ValueError):
        host.locate(_NoDevice(), [ctg], ["I:1-10"], count=True, rg_records=recs, rg_data=data)
    with pytest.raises(ValueError):
        host.locate_text(_NoDevice(), [ctg], b"I:1-10\n", count=True, rg_records=recs, rg_data=data)
    with pytest.raises(ValueError):
        host.sw(_NoDevice(), ctg, [("feature:ctg:I:1:1", 100, 200)], actions=("gc", "count"), rg_records=recs, rg_data=data)
    with pytest.raises(ValueError):
        host.sw_multi([_NoDevice()], [ctg], [[("feature:ctg:I:1:1", 100, 200)]], actions=("count",), rg_records=recs,
                      rg_data=data)


def test_model_parses_like_range_from_str():
    ok = {b"I:1-100": ("I", 1, 100), b"I(+):5-9": ("I", 5, 9), b"name.I:5-9": ("I", 5, 9), b"I:7": ("I", 7, 7),
          b"I:5__-9 \r": ("I", 5, 9), b"a.b.c:1-2": None, b"chr-1/x:2147483647": ("chr-1/x", 2147483647, 2147483647)}
    for ln, want in ok.items():
        assert parse_line(ln) == want, ln
    for ln in (b"", b"I", b"I:", b":5", b"I:1-100\tfoo", b"I:12345678901", b"I:2147483648", b"I:1-", b"I:a-b",
               b"I:1-2-", b"I(+:1-2", b"I :1-2"):
        assert parse_line(ln) is None, ln


def test_model_reproduces_the_reference_counts(s288c):
    """tests/cli.rs:235-253: spo11_hot.rg has 79 lines, 71 of them are located and 69 kept (one dropped per ctg; the
    ctg table is the one test_oracle_golden.py and test_gpu_host.py pin the same figures on)"""
    ctgs = []
    for chr_id in ("I", "Mito"):
        ctgs += helpers.gen_ctgs(chr_id, s288c[chr_id], piece=100000)
    with open(os.path.join(helpers.S288C, "spo11_hot.rg"), "rb") as fh:
        m = model(ctgs, fh.read())
    assert (m["lines"], m["located"], sum(len(b) for b in m["buckets"])) == (79, 71, 69)
    assert sum(m["seen"]) == 2
