"""CPU checks of the sw summary's Prop columns: gams_prop4_units against the text of every fraction, the
pure-Python model of tests/sw_anno_summary.py against a table written out by hand, the host's summariser with props=
against it, the same path alone behind the stand-alone driver tests/sw_anno_summary_main.cpp (host compiler with the
address and undefined-behaviour sanitizers, no HIP, no device), the declared entries, and that the synthetic inputs of
tests/test_gpu_sw_anno_summary.py really carry the cases they are meant to."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import sw_anno_summary as sas
import sw_text as swt
from gams_amd import _lib, host
from test_sw_summary_cpu import HAND_ROWS, HAND_TABLE, rows_of_text, without_column

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

# the dozen rows of tests/test_sw_summary_cpu.py after `gams anno cds.json stdin | gams anno rep.json stdin`: in cdsProp the
# average ties 5 / 2 (distance 0) and 7 / 2 (distance 3), an average of exactly 1 (distance 1); repProp is 0 everywhere
HAND_PROPS = [(b"0.0002", b"0.0000"), (b"0.0003", b"0.0000"),                          # distance 0
              (b"1.0000", b"0.0000"), (b"1.0000", b"0.0000"), (b"1.0000", b"0.0000"),  # 1
              (b"0.5000", b"0.0000"),                                                  # 2
              (b"0.0003", b"0.0000"), (b"0.0004", b"0.0000"),                          # 3
              (b"0.1000", b"0.0000"), (b"0.2000", b"0.0000"),                          # 4
              (b"0.0000", b"0.0000"), (b"1.0000", b"0.0000")]                          # 5
HAND_ANNO_ROWS = b"".join(row + b"\t" + p[0] + b"\t" + p[1] + b"\n" for row, p in zip(HAND_ROWS.split(b"\n")[:-1], HAND_PROPS))
HAND_ANNO_TABLE = b"""\
distance\tAVG_gc_content\tAVG_gc_mean\tAVG_gc_stddev\tAVG_gc_cv\tAVG_cdsProp\tAVG_repProp\tAVG_rg_count\tCOUNT
0\t0.0002\t0.0004\t0.15\tnan\t0.0002\t0\t0.5\t2
1\t0.5\t0.3812\t0.0001\t1.6667\t1\t0\t1\t3
2\t1\t0\t0.25\t0\t0.5\t0\t0\t1
3\t0.3334\t0.5\t0.01\t0.02\t0.0004\t0\t5\t2
4\t0.1234\t0.2\t0.3\t0.4\t0.15\t0\t2\t2
5\t1\t0.1\t0.1\t0.1\t0.5\t0\t2.5\t2
"""
PREFIXES = ("cds", "rep")


def columns(table, keep):
    return b"".join(b"\t".join(ln.split(b"\t")[i] for i in keep) + b"\n" for ln in table.split(b"\n")[:-1])


def f32_div(card, ln):
    return np.float32(card) / np.float32(ln)


def test_prop4_units_against_the_text_of_every_fraction():
    """every (card, len) with 1 <= len <= 600, 0 <= card <= len: the q of the summary is the digits of the text"""
    seen = {}
    for ln in range(1, 601):
        for card in range(ln + 1):
            v = f32_div(card, ln)
            seen.setdefault(v.tobytes(), v)
    assert len(seen) > 100000
    for v in seen.values():
        text = "%.4f" % float(v)
        q = host.prop4_units(float(v))
        assert "%d.%04d" % divmod(q, 10000) == text == host.fmt_prop4(float(v)), (float(v), q, text)
    # the exact ties of size 32: the f32 is k / 32 exactly, 10^4 k / 32 ends in .5 and goes to the even neighbour
    assert host.prop4_units(float(f32_div(1, 32))) == 312
    assert host.prop4_units(float(f32_div(3, 32))) == 938
    assert host.prop4_units(float(f32_div(5, 32))) == 1562
    assert host.prop4_units(0.0) == 0 and host.prop4_units(1.0) == 10000
    assert sas.tie_units(32)[1] == 312 and sas.tie_units(32)[3] == 938 and sas.tie_units(32)[5] == 1562
    for bad in (-0.5, 1.5, float("nan")):
        with pytest.raises(host.HostError) as ei:
            host.prop4_units(bad)
        assert ei.value.code == _lib.EINVAL


def test_hand_written_table():
    assert without_column(without_column(HAND_ANNO_TABLE, 5), 5) == HAND_TABLE        # the Prop columns stand behind gc_cv
    text, table = sas.summary([HAND_ANNO_ROWS], PREFIXES, actions=("gc", "count"))
    assert text == HAND_ANNO_TABLE
    # the header names and the column order of every action set
    assert sas.summary([HAND_ANNO_ROWS], PREFIXES)[0] == without_column(HAND_ANNO_TABLE, 7)
    assert sas.summary([HAND_ANNO_ROWS], PREFIXES, actions=("count",))[0] == columns(HAND_ANNO_TABLE, (0, 5, 6, 7, 8))
    no_gc = sas.summary([HAND_ANNO_ROWS], PREFIXES, actions=())[0]
    assert no_gc == columns(HAND_ANNO_TABLE, (0, 5, 6, 8))
    assert no_gc.split(b"\n")[0] == b"distance\tAVG_cdsProp\tAVG_repProp\tCOUNT"
    assert text.split(b"\n")[0].split(b"\t")[5:8] == [b"AVG_cdsProp", b"AVG_repProp", b"AVG_rg_count"]
    # the ties, the all-zero column, the average of exactly 1
    assert (None, 0, 0) in table.prop_ties() and (None, 3, 0) in table.prop_ties()
    assert table.groups[(None, 0)][4] == [5, 0] and table.groups[(None, 3)][4] == [7, 0]
    body = [ln.split(b"\t") for ln in text.split(b"\n")[1:-1]]
    assert [ln[5] for ln in body] == [b"0.0002", b"1", b"0.5", b"0.0004", b"0.15", b"0.5"]
    assert all(ln[6] == b"0" for ln in body)
    # tags: ordered by tag bytes, then distance
    tagged = sas.summary([HAND_ANNO_ROWS, HAND_ANNO_ROWS], PREFIXES, [b"b", b"a"], actions=("gc", "count"))[0].split(b"\n")
    rows = HAND_ANNO_TABLE.split(b"\n")[1:-1]
    assert tagged[0] == b"tag\t" + HAND_ANNO_TABLE.split(b"\n")[0]
    assert tagged[1:-1] == [b"a\t" + ln for ln in rows] + [b"b\t" + ln for ln in rows]
    # without sets the model is the one of tests/sw_summary.py
    assert sas.summary([HAND_ROWS], (), actions=("gc", "count"))[0] == HAND_TABLE


def hand_props():
    return [np.array([sas.prop_units(p[a]) for p in HAND_PROPS], np.uint32) for a in range(2)]


def test_host_summariser_with_props():
    rows, cnt = rows_of_text(HAND_ROWS)
    props = hand_props()
    assert host.sw_summarise_rows(rows, cnt, mx=5, actions=("gc", "count"), props=props, prefixes=PREFIXES) == HAND_ANNO_TABLE
    assert host.sw_summarise_rows(rows, mx=5, props=props, prefixes=PREFIXES) == without_column(HAND_ANNO_TABLE, 7)
    assert host.sw_summarise_rows(rows, cnt, mx=7, actions=("count",), props=props, prefixes=PREFIXES) == columns(
        HAND_ANNO_TABLE, (0, 5, 6, 7, 8))
    assert host.sw_summarise_rows(rows, mx=5, actions=("gibbs",), props=props, prefixes=PREFIXES) == columns(
        HAND_ANNO_TABLE, (0, 5, 6, 8))
    assert host.sw_summarise_rows(rows, mx=5, actions=(), props=props[:1], prefixes=["cds"]) == columns(HAND_ANNO_TABLE, (0, 5, 8))
    tab = host.sw_summarise_rows(rows, cnt, mx=5, actions=("gc", "count"), table=True, props=props, prefixes=PREFIXES)
    model = sas.summary([HAND_ANNO_ROWS], PREFIXES, actions=("gc", "count"))[1]
    assert np.array_equal(tab["prop"], model.prop(5)) and tab["prop"].shape == (1, 6, 2)
    want = model.arrays(5)
    assert all(np.array_equal(tab[k], np.asarray(want[k], np.uint64)) for k in ("count", "sum", "nan", "rg_count"))
    # without props: today's bytes, and no "prop" in the table
    assert host.sw_summarise_rows(rows, cnt, mx=5, actions=("gc", "count")) == HAND_TABLE
    assert host.sw_summarise_rows(rows, cnt, mx=5, actions=("gc", "count"), props=None, prefixes=None) == HAND_TABLE
    assert "prop" not in host.sw_summarise_rows(rows, cnt, mx=5, actions=("gc", "count"), table=True)
    empty = host.sw_summarise_rows(np.zeros(0, _lib.SW_ROW_DTYPE), mx=3, props=[[], []], prefixes=PREFIXES)
    assert empty == sas.Table(PREFIXES).header(False)
    with pytest.raises(ValueError):
        host.sw_summarise_rows(rows, mx=5, props=props, prefixes=["cds"])             # one prefix per column
    with pytest.raises(ValueError):
        host.sw_summarise_rows(rows, mx=5, props=[props[0][:3]], prefixes=["cds"])    # one unit per row
    with pytest.raises(host.HostError) as ei:
        host.sw_summarise_rows(rows, mx=5, props=[np.full(rows.size, 10001, np.uint32)], prefixes=["cds"])
    assert ei.value.code == _lib.EINVAL


# ---- the host summariser's translation unit and text_fmt.hpp alone, under the sanitizers --------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("sw_anno_summary") / "sw_anno_summary_main"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-ffp-contract=off", os.path.join(HERE, "sw_anno_summary_main.cpp"),
                           os.path.join(ROOT, "gams_amd", "host", "gams_sw_summary.cpp"), "-o", str(exe)])
    return str(exe)


def driver_input(mx, actions, prefixes, props):
    lines = ["%d %d %d %s" % (mx, host.sw_actions(actions), len(prefixes), " ".join(prefixes))]
    for r, row in enumerate(HAND_ROWS.split(b"\n")[:-1]):
        f = row.decode().split("\t")
        lines.append(" ".join([f[3]] + [x.lower() for x in f[4:8]] + [f[8]] + [str(int(p[r])) for p in props]))
    return "\n".join(lines) + "\n"


def test_driver_on_the_hand_written_case(driver, tmp_path):
    props = hand_props()
    cases = [(5, ("gc", "count"), PREFIXES, props, HAND_ANNO_TABLE),
             (5, ("gc",), PREFIXES, props, without_column(HAND_ANNO_TABLE, 7)),
             (9, (), PREFIXES, props, columns(HAND_ANNO_TABLE, (0, 5, 6, 8))),
             (5, ("gc", "count"), (), [], HAND_TABLE),
             (4, ("gc",), PREFIXES, props, b"error %d\n" % _lib.EINVAL)]                  # a distance beyond max
    for k, (mx, actions, prefixes, cols, want) in enumerate(cases):
        path = tmp_path / ("case%d.txt" % k)
        path.write_text(driver_input(mx, actions, prefixes, cols))
        res = subprocess.run([driver, str(path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert res.returncode == 0 and res.stderr == b"", res.stderr[-2000:]
        head, _, body = res.stdout.partition(b"\n")
        assert head == b"units %d" % sum(ln + 1 for ln in range(1, 601))
        assert body == want, (k, body)


def test_entries_are_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "gams_gpu.h")).read()
    lib = C.CDLL(_lib.SO_PATH)
    for name in ("gams_sw_summary_create_anno", "gams_sw_summary_read_anno", "gams_gpu_sw_summary_batch_anno",
                 "gams_gpu_sw_feature_summary_anno"):
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert name in _lib.PROTOTYPES and hasattr(lib, name), name
    assert int(re.search(r"#define\s+GAMS_SW_SUMMARY_MAX_ANNO\s+(\d+)u", hdr).group(1)) == _lib.SW_SUMMARY_MAX_ANNO == 4
    hl = C.CDLL(host.SO_PATH)
    assert all(hasattr(hl, n) for n in ("gams_host_sw_summary_anno", "gams_host_sw_summarise_rows_props",
                                        "gams_host_sw_summary_text_props", "gams_host_prop4_units"))
    # the LDS rule of the summary with sets: both tables in the 2560 words of the table without sets
    src = open(os.path.join(ROOT, "gams_amd", "csrc", "sw.hip")).read()
    assert "kSumLdsWords = kSumLdsGroups * kSumWords" in src
    L = _lib.load()
    p = C.c_void_p()
    assert L.gams_sw_summary_create_anno(None, 20, 1, 1, 100, 500, 2, C.byref(p)) == _lib.EINVAL
    assert L.gams_sw_summary_read_anno(None, None, None) == _lib.EINVAL
    assert L.gams_gpu_sw_summary_batch_anno(None, None, 0, None, None, None, None, None, 100, 20, 500, 1, None, None, None, 0,
                                            0, None, None, None) == _lib.EINVAL
    assert L.gams_gpu_sw_feature_summary_anno(None, None, None, None, None, None, None, None, b"I:1-2\n", 6, 100, 20, 500, 1,
                                              None, None, None, 0, 0, None, None, None, None) == _lib.EINVAL


def lds_limit(n_anno):
    """the largest max a call with n_anno sets reduces in LDS: (max + 1) * (10 + n_anno) <= 2560"""
    return 2560 // (10 + n_anno) - 1


def test_synthetic_input_carries_its_cases():
    """what tests/test_gpu_sw_anno_summary.py leans on, shown with the oracle's rows and cover"""
    assert [lds_limit(n) for n in range(5)] == [255, 231, 212, 195, 181]
    ctgs = sas.synth_ctgs()
    data = sas.synth_features(ctgs)
    rows = swt.model(ctgs, data)
    per = {}
    for row in rows.split(b"\n")[:-1]:
        f = row.split(b"\t")
        per.setdefault(f[0].rsplit(b":", 1)[0], {b"M": [], b"L": 0, b"R": 0})
        if f[2] == b"M":
            per[f[0].rsplit(b":", 1)[0]][b"M"].append(f[1])
        else:
            per[f[0].rsplit(b":", 1)[0]][f[2]] += 1
    assert 280 <= len(per) <= 300
    assert any(v[b"L"] < 20 and v[b"R"] == 20 for v in per.values()) and any(v[b"R"] < 20 and v[b"L"] == 20 for v in per.values())
    widths = set()
    for v in per.values():
        r = sas.RANGE.match(v[b"M"][0])
        widths.add(int(r.group(3) or r.group(2)) - int(r.group(2)) + 1)
    assert 99 in widths and 100 in widths                       # point and odd features: 99-bp M windows; even ones: 100
    edges = sorted({int(sas.RANGE.match(r.split(b"\t")[1]).group(2)) for r in rows.split(b"\n")[:-1]
                    if r.split(b"\t")[0].startswith(b"sw:feature:ctg:A:1:")})
    dense, sparse = sas.dense_set(ctgs, edges), sas.sparse_set(ctgs)
    lo, hi = dense["A"]
    assert np.all(lo[1:] > hi[:-1] + 1)                         # normalised: disjoint, not adjacent
    # a crowded stretch: the grid has about one span a cell, so 300 spans inside 1500 bases next to 20 kb with few
    # put far more than five into the cells there
    assert int(((lo >= ctgs[0]["chr_start"] + 2000) & (lo < ctgs[0]["chr_start"] + 3500)).sum()) > 250
    for s in (dense, sparse):
        back = host.read_runlist_json(sas.runlist_json(s))          # the JSON says the spans
        assert list(back) == list(s) and all(np.array_equal(back[k][0], s[k][0]) and np.array_equal(back[k][1], s[k][1]) for k in s)
    both = sas.annotate(sas.annotate(rows, ctgs, dense), ctgs, sparse)
    qs = [(r.split(b"\t")[0], sas.prop_units(r.split(b"\t")[9]), sas.prop_units(r.split(b"\t")[10])) for r in both.split(b"\n")[:-1]]
    assert all(q[1] == 10000 for q in qs if q[0].startswith(b"sw:feature:ctg:A:2:"))       # the span over the whole ctg
    assert all(q[2] == 0 for q in qs if q[0].startswith(b"sw:feature:ctg:B:1:"))           # the absent chromosome
    assert any(q[1] == 0 for q in qs if q[0].startswith(b"sw:feature:ctg:A:1:"))           # the stretch with no span
    assert any(0 < q[1] < 1000 for q in qs) and any(0 < q[2] < 10000 for q in qs) and any(q[2] == 10000 for q in qs)
    # at size 32 the props are k / 32: the input holds rows whose q comes from a tie
    rows32 = swt.model(ctgs, data, 32, 20, 160)
    ties = set(sas.tie_units(32).values())
    q32 = [sas.prop_units(r.split(b"\t")[9]) for r in sas.annotate(rows32, ctgs, dense).split(b"\n")[:-1]
           if sas.RANGE.match(r.split(b"\t")[1]).group(3) and
           int(sas.RANGE.match(r.split(b"\t")[1]).group(3)) - int(sas.RANGE.match(r.split(b"\t")[1]).group(2)) == 31]
    assert any(q in ties for q in q32)
