"""CPU checks of `sw` from the bytes of a feature file (gams_gpu_sw_feature_text / host.sw_text): the header, the
ctypes stub and both libraries declare and export the entries, the binding refuses two rg sources at once, the
pure-Python model of tests/sw_text.py reproduces the oracle's rows on spo11_hot.rg, and the synthetic input really
carries the cases tests/test_gpu_sw_text.py holds the device against."""
import ctypes as C
import os
import re

import pytest

import helpers
import sw_text as swt
from gams_amd import _lib, host
from oracle import oracle as ora
from test_oracle_golden import _all_ctgs, _read_range
from test_rg_text_cpu import locator_order, parse_line

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOCK, STAGE = 512, 49152                 # kSwTextBlock, kSwTextStage of gams_amd/csrc/sw.hip


def test_new_entries_are_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "gams_gpu.h")).read()
    assert re.search(r"\bint\s+gams_gpu_sw_feature_text\s*\(", hdr)
    assert "gams_gpu_sw_feature_text" in _lib.PROTOTYPES
    assert hasattr(C.CDLL(_lib.SO_PATH), "gams_gpu_sw_feature_text")
    assert hasattr(C.CDLL(host.SO_PATH), "gams_host_sw_text")
    assert callable(host.sw_text)
    src = open(os.path.join(ROOT, "gams_amd", "csrc", "sw.hip")).read()
    assert "kSwTextBlock = %d" % BLOCK in src and "kSwTextStage = %d" % STAGE in src


def test_null_arguments_are_einval():
    lib = _lib.load()
    n = C.c_uint64()
    assert lib.gams_gpu_sw_feature_text(None, None, None, None, None, None, None, None, b"I:1-2\n", 6, 100, 20, 500, 1, None,
                                        None, None, C.byref(n), None, C.byref(n), C.byref(n)) == _lib.EINVAL
    # the batch entries and the range gc: no handle, no seqset or no outputs, refused before anything touches a device
    # (tests/test_gpu_sw_refusals.py holds the refusals that need a handle)
    assert lib.gams_gpu_sw_batch(None, None, 0, None, None, None, None, None, 100, 20, 500, None, 0, None, C.byref(n)) == _lib.EINVAL
    assert lib.gams_gpu_sw_batch(None, None, 0, None, None, None, None, None, 100, 20, 500, None, 0, None, None) == _lib.EINVAL
    assert lib.gams_gpu_sw_count_batch(None, None, 0, None, None, None, None, None, 100, 20, None, None, None, 0, None,
                                       C.byref(n)) == _lib.EINVAL
    text, nb = C.c_void_p(), C.c_uint64()
    assert lib.gams_gpu_sw_text_actions(None, None, 0, None, None, None, None, None, None, None, 100, 20, 500, 1, None, None,
                                        C.byref(text), C.byref(nb), None, C.byref(n)) == _lib.EINVAL
    assert lib.gams_gpu_sw_text(None, None, 0, None, None, None, None, None, None, None, 100, 20, 500, None, None, None,
                                None) == _lib.EINVAL
    assert lib.gams_gpu_range_gc_batch(None, None, 0, None, None, None, None, None, None) == _lib.EINVAL
    assert lib.gams_gpu_range_gc(None, None, 0, 1, None, None, 0, None) == _lib.EINVAL
    assert lib.gams_gpu_sw(None, None, 0, 1, None, None, 0, 100, 20, 500, None, 0, None) == _lib.EINVAL


class _NoDevice:
    h = None


def test_two_rg_sources_raise_value_error():
    ctg = dict(id="ctg:I:1", chr_id="I", chr_start=1, chr_end=1000, seq=b"A" * 1000)
    with pytest.raises(ValueError):
        host.sw_text(_NoDevice(), [ctg], b"I:5-8\nI:9-20\n", actions=("gc", "count"), rg_records=[("ctg:I:1", "I:5-8")],
                     rg_data=b"I:5-8\n")
    with pytest.raises(ValueError):
        host.sw_text(_NoDevice(), [ctg], b"I:5-8\n", actions=("nonsense",))


def test_model_on_the_golden_rg_file(s288c):
    """the model's text = the oracle loop of tests/test_oracle_golden.py::test_sw_structure"""
    ctgs = _all_ctgs(s288c)
    with open(os.path.join(helpers.S288C, "spo11_hot.rg"), "rb") as fh:
        data = fh.read()
    got = swt.model(ctgs, data)
    buckets = _read_range(helpers.read_lines("spo11_hot.rg"), helpers.ctg_index(ctgs))
    want = ""
    for c in sorted(ctgs, key=lambda c: c["id"]):
        feats = [(f"feature:{c['id']}:{i + 1}", r[1], r[2]) for i, r in enumerate(buckets.get(c["id"], []))]
        want += ora.sw_proc_ctg(c["chr_id"], c["chr_start"], c["chr_end"], c["seq"], feats)
    assert got == want.encode()
    assert sum(len(f) for f in swt.features(ctgs, data)) == 69
    rows = got.split(b"\n")[:-1]
    assert len(rows) > 2000
    assert any(r.startswith(b"sw:feature:ctg:I:2:32:1\t") for r in rows)


def test_model_refuses_a_kept_middle_outside_its_ctg():
    ctgs = swt.synth_ctgs()
    first, bad = b"I:100-200\n", b"I:29990-30099\n"                    # overlaps ctg:I:1 (.. 30000), the middle at 30044
    with pytest.raises(swt.ModelError):
        swt.features(ctgs, first + bad)
    assert sum(len(f) for f in swt.features(ctgs, bad + first)) == 1   # the same line as the dropped first line


@pytest.fixture(scope="module")
def synth():
    ctgs = swt.synth_ctgs()
    lines = swt.synth_lines(ctgs)
    data = swt.synth_data(lines)
    return ctgs, lines, data, swt.interval_text(ctgs, data)


def _rows_of(text, ctgs, data, rng_line):
    """the rows of the feature a line became (the line is kept: it is not the first of its ctg)"""
    r = parse_line(rng_line.encode())
    for c, feats in zip(ctgs, swt.features(ctgs, data)):
        for fid, s, e in feats:
            if c["chr_id"] == r[0] and (s, e) == (r[1], r[2]):
                return [row for row in text.split(b"\n") if row.startswith(b"sw:" + fid.encode() + b":")]
    raise AssertionError("not kept: " + rng_line)


def test_synthetic_input_carries_its_cases(synth):
    ctgs, lines, data, text = synth
    assert lines[0].startswith("#") and 4000 < len(lines) < 4100
    assert b"\r\n" in data and not data.endswith(b"\n")
    heads = [ln.split(":")[0] for ln in lines]
    assert any("(+)" in h for h in heads) and any("(-)" in h for h in heads) and any("." in h for h in heads)
    assert any(re.search(r":0\d", ln) for ln in lines) and any(re.fullmatch(r"[\w.()+-]+:\d+", ln) for ln in lines)
    assert any("_" in ln.split(":")[-1] for ln in lines) and any("--" in ln for ln in lines)
    located, kept = swt.buckets(ctgs, data)
    by = {c["id"]: i for i, c in enumerate(ctgs)}
    assert located[by[swt.ONE_LINE]] == 1 and kept[by[swt.ONE_LINE]] == []
    assert located[by[swt.TWO_LINES]] == 2 and len(kept[by[swt.TWO_LINES]]) == 1
    assert len(kept[by[swt.CROWDED]]) >= 1000
    assert len(swt.LONG_ID) == 80 and len(kept[by[swt.LONG_ID]]) > 0
    for c, b in zip(ctgs, kept):                                       # every kept feature has its middle inside its ctg
        assert all(swt.middle_inside(c, s, e) for s, e, _ in b)
    # invalid lines, unknown chromosomes, unlocated ranges
    parsed = [parse_line(ln.encode()) for ln in lines]
    assert sum(p is None for p in parsed) >= 8
    assert any(p and p[0] in ("IV", "Mito") for p in parsed)
    assert sum(located) < sum(p is not None for p in parsed) - 2
    edge = swt.edge_lines(ctgs)
    rows = text.split(b"\n")[:-1]
    types = lambda rr: {r.split(b"\t")[2] for r in rr}
    for ln in edge["first_bases"]:
        assert b"L" not in types(_rows_of(text, ctgs, data, ln)), ln
    for ln in edge["last_bases"]:
        assert b"R" not in types(_rows_of(text, ctgs, data, ln)), ln
    for ln in edge["over_edge"] + edge["seam"]:
        _, s, e = parse_line(ln.encode())
        c = ctgs[swt.locate_one(ctgs, *parse_line(ln.encode()))]
        assert s < c["chr_start"] or e > c["chr_end"], ln
        assert _rows_of(text, ctgs, data, ln), ln
    seam_ctg = ctgs[swt.locate_one(ctgs, *parse_line(edge["seam"][0].encode()))]
    assert seam_ctg["id"] == "ctg:II:1"
    for ln in edge["long"]:
        _, s, e = parse_line(ln.encode())
        assert e - s + 1 > 100 and _rows_of(text, ctgs, data, ln), ln
    # the text kernels' paths: rows in interval order, 512 to a block, a block staged in LDS up to 49152 bytes
    assert len(rows) > 2 * BLOCK
    sizes = [sum(len(r) + 1 for r in rows[k:k + BLOCK]) for k in range(0, len(rows) - BLOCK + 1, BLOCK)]
    assert max(sizes) > STAGE and min(sizes) < STAGE
    # serials cross 9 -> 10, 99 -> 100, 999 -> 1000
    for k in (9, 10, 99, 100, 999, 1000):
        assert any(r.startswith(b"sw:feature:%s:%d:1\t" % (swt.CROWDED.encode(), k)) for r in rows), k
    # the slices in id order are the model's text
    assert sorted(rows) == sorted(swt.model(ctgs, data).split(b"\n")[:-1])
    assert [c["id"] for c in locator_order(ctgs)] == [c["id"] for c in ctgs]
