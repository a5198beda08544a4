"""CPU checks of the sw summary: the pure-Python model of tests/sw_summary.py against a table written
out by hand, the host's summariser (host.sw_summarise_rows, no engine) against the model on crafted rows, the declared
entries, and that the synthetic inputs of tests/test_gpu_sw_summary.py really carry the cases they are meant to."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import sw_summary as sws
import sw_text as swt
from gams_amd import _lib, host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROW = _lib.SW_ROW_DTYPE

# a dozen rows as `gams sw -a gc -a count` prints them: an exact tie in gc_content (5 / 2) and gc_mean (7 / 2) at
# distance 0, a NaN cv there, a -0 at distance 1, distance 2 and 3 only as L, distance 4 only as R
HAND_ROWS = b"""\
sw:feature:ctg:I:1:1:1\tI:951-1050\tM\t0\t0.0002\t0.0003\t0.1\tNaN\t0
sw:feature:ctg:I:1:2:1\tI:2951-3050\tM\t0\t0.0003\t0.0004\t0.2\t0.5\t1
sw:feature:ctg:I:1:1:2\tI:851-950\tL\t1\t0.4\t0.3812\t-0\t1.5\t2
sw:feature:ctg:I:1:1:3\tI:1051-1150\tR\t1\t0.5\t0.3812\t0\t2.5\t0
sw:feature:ctg:I:1:2:2\tI:2851-2950\tL\t1\t0.6\t0.3812\t0.0003\t1\t1
sw:feature:ctg:I:1:2:3\tI:2751-2850\tL\t2\t1\t0\t0.25\t0\t0
sw:feature:ctg:I:1:1:4\tI:651-750\tL\t3\t0.3333\t0.5\t0.01\t0.02\t7
sw:feature:ctg:I:1:2:4\tI:2651-2750\tL\t3\t0.3334\t0.5\t0.01\t0.02\t3
sw:feature:ctg:I:1:1:5\tI:1351-1450\tR\t4\t0.1234\t0.2\t0.3\t0.4\t4
sw:feature:ctg:I:1:2:5\tI:3351-3450\tR\t4\t0.1235\t0.2\t0.3\t0.4\t0
sw:feature:ctg:I:1:1:6\tI:451-550\tL\t5\t0.9999\t0.1\t0.1\t0.1\t0
sw:feature:ctg:I:1:2:6\tI:3451-3550\tR\t5\t1\t0.1\t0.1\t0.1\t5
"""
HAND_TABLE = b"""\
distance\tAVG_gc_content\tAVG_gc_mean\tAVG_gc_stddev\tAVG_gc_cv\tAVG_rg_count\tCOUNT
0\t0.0002\t0.0004\t0.15\tnan\t0.5\t2
1\t0.5\t0.3812\t0.0001\t1.6667\t1\t3
2\t1\t0\t0.25\t0\t0\t1
3\t0.3334\t0.5\t0.01\t0.02\t5\t2
4\t0.1234\t0.2\t0.3\t0.4\t2\t2
5\t1\t0.1\t0.1\t0.1\t2.5\t2
"""


def without_column(table, k):
    return b"".join(b"\t".join(f for i, f in enumerate(ln.split(b"\t")) if i != k) + b"\n" for ln in table.split(b"\n")[:-1])


def rows_of_text(text):
    """the rows' text as the arrays of gams_gpu_sw_batch: every statistic the f32 nearest to what is printed"""
    lines = text.split(b"\n")[:-1]
    rows = np.zeros(len(lines), ROW)
    cnt = np.zeros(len(lines), np.int32)
    for r, ln in enumerate(lines):
        f = ln.split(b"\t")
        rows[r]["type"] = b"MLR".index(f[2])
        rows[r]["distance"] = int(f[3])
        for k, name in enumerate(("gc_content", "gc_mean", "gc_stddev", "gc_cv")):
            rows[r][name] = np.float32(f[4 + k].decode())
        cnt[r] = int(f[8]) if f[8] else 0
    return rows, cnt


def test_hand_written_table():
    text, table = sws.summary([HAND_ROWS], actions=("gc", "count"))
    assert text == HAND_TABLE
    assert sws.summary([HAND_ROWS])[0] == without_column(HAND_TABLE, 5)
    assert sws.summary([HAND_ROWS], actions=("count",))[0] == b"".join(
        b"\t".join(ln.split(b"\t")[i] for i in (0, 5, 6)) + b"\n" for ln in HAND_TABLE.split(b"\n")[:-1])
    assert (None, 0, 0) in sws.ties(table) and (None, 0, 1) in sws.ties(table)
    # with tags: ordered by tag bytes, then distance
    tagged = sws.summary([HAND_ROWS, HAND_ROWS], [b"b", b"a"], actions=("gc", "count"))[0].split(b"\n")
    body = HAND_TABLE.split(b"\n")[1:-1]
    assert tagged[0] == b"tag\t" + HAND_TABLE.split(b"\n")[0]
    assert tagged[1:-1] == [b"a\t" + ln for ln in body] + [b"b\t" + ln for ln in body]
    assert sws.avg4(5, 2) == b"0.0002" and sws.avg4(7, 2) == b"0.0004" and sws.avg4(0, 3) == b"0" and sws.avg4(4000, 1) == b"0.4"


def test_host_summariser_on_the_hand_written_rows():
    rows, cnt = rows_of_text(HAND_ROWS)
    assert host.sw_summarise_rows(rows, cnt, mx=5, actions=("gc", "count")) == HAND_TABLE
    assert host.sw_summarise_rows(rows, mx=5) == without_column(HAND_TABLE, 5)
    assert host.sw_summarise_rows(rows, mx=9) == without_column(HAND_TABLE, 5)        # groups without rows are not printed
    tab = host.sw_summarise_rows(rows, cnt, mx=5, actions=("gc", "count"), table=True)
    want = sws.summary([HAND_ROWS], actions=("gc", "count"))[1].arrays(5)
    assert all(np.array_equal(tab[k], np.asarray(want[k], np.uint64)) for k in ("count", "sum", "nan", "rg_count"))
    assert host.sw_summarise_rows(np.zeros(0, ROW), mx=3) == sws.Table().header(False)
    with pytest.raises(host.HostError) as ei:
        host.sw_summarise_rows(rows, mx=4)                                            # a distance beyond max
    assert ei.value.code == _lib.EINVAL
    with pytest.raises(host.HostError):
        host.sw_summarise_rows(rows, None, mx=5, actions=("count",))                  # count without the counts


def test_host_summariser_on_crafted_rows():
    """2000 rows of round4 values -- the f32 nearest to m / 10^4 --, NaN, -0 and, as only the host's route meets them,
    values of 1000 and more; their text is made with the project's `{}` of an f32 (host.fmt_f32) and read by the model"""
    rng = np.random.default_rng(5)
    n, mx = 2000, 40
    rows = np.zeros(n, ROW)
    rows["distance"] = rng.integers(0, mx + 1, n)
    rows["type"] = np.where(rows["distance"] == 0, 0, rng.integers(1, 3, n))
    special = np.array([np.nan, -0.0, 0.0, 1.0, 999.9999, 1000.0, 1500.25, 2000.0, 0.0001, 0.5], np.float32)
    for name in ("gc_content", "gc_mean", "gc_stddev", "gc_cv"):
        m = rng.integers(0, 10 ** 7, n)
        m[rng.random(n) < 0.7] %= 10000                                               # most values lie below 1
        v = (m / 10000.0).astype(np.float32)
        pick = rng.random(n) < 0.1
        v[pick] = special[rng.integers(0, special.size, int(pick.sum()))]
        rows[name] = v
    cnt = rng.integers(0, 2 ** 31 - 1, n).astype(np.int32)
    shown = {}

    def show(v):
        key = np.float32(v).tobytes()
        if key not in shown:
            shown[key] = host.fmt_f32(float(v)).encode()
        return shown[key]

    text = b"".join(b"sw:f:1\tI:1-2\t%c\t%d\t%s\t%s\t%s\t%s\t%d\n" % (b"MLR"[r["type"]], r["distance"], show(r["gc_content"]),
                    show(r["gc_mean"]), show(r["gc_stddev"]), show(r["gc_cv"]), c) for r, c in zip(rows, cnt))
    assert b"\tNaN\t" in text and b"\t-0\t" in text and b"\t1500.25\t" in text
    for actions in (("gc",), ("gc", "count"), ("count",), ()):
        want, model = sws.summary([text], actions=actions)
        assert host.sw_summarise_rows(rows, cnt, mx=mx, actions=actions) == want
        tab = host.sw_summarise_rows(rows, cnt, mx=mx, actions=actions, table=True)
        arr = model.arrays(mx)
        assert all(np.array_equal(tab[k], np.asarray(arr[k], np.uint64)) for k in ("count", "sum", "nan", "rg_count"))
    bad = rows[:1].copy()
    bad["gc_cv"] = -0.5
    with pytest.raises(host.HostError) as ei:
        host.sw_summarise_rows(bad, mx=mx)
    assert ei.value.code == _lib.EUNSUPPORTED


def test_entries_are_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "gams_gpu.h")).read()
    lib = C.CDLL(_lib.SO_PATH)
    assert all(hasattr(C.CDLL(host.SO_PATH), n) for n in ("gams_host_sw_summary", "gams_host_sw_summarise_rows", "gams_host_sw_summary_text"))
    src = open(os.path.join(ROOT, "gams_amd", "csrc", "sw.hip")).read()
    assert "kSumLdsGroups = 256" in src                        # the LDS budget tests/test_gpu_sw_summary.py names its paths by
    for name in ("gams_gpu_sw_feature_summary", "gams_gpu_sw_summary_batch", "gams_sw_summary_create", "gams_sw_summary_reset",
                 "gams_sw_summary_read", "gams_sw_summary_destroy"):
        assert re.search(r"\b(int|void)\s+%s\s*\(" % name, hdr), name
        assert name in _lib.PROTOTYPES and hasattr(lib, name), name
    assert int(re.search(r"#define\s+GAMS_SW_SUMMARY_WORDS\s+(\d+)u", hdr).group(1)) == _lib.SW_SUMMARY_WORDS
    # null arguments are refused before anything touches a device
    L = _lib.load()
    assert L.gams_sw_summary_create(None, 20, 1, 1, 100, 500, None) == _lib.EINVAL
    assert L.gams_gpu_sw_feature_summary(None, None, None, None, None, None, None, None, b"I:1-2\n", 6, 100, 20, 500, 1, None,
                                         None, None, 0, None, None) == _lib.EINVAL
    assert L.gams_gpu_sw_summary_batch(None, None, 0, None, None, None, None, None, 100, 20, 500, 1, None, None, None, 0,
                                       None) == _lib.EINVAL


def test_synthetic_input_carries_its_cases():
    """What the GPU tests lean on.  "A distance with only L rows" is read per feature: 4000 features spread over six ctgs
    fill every distance from both sides, so no distance of the whole file is L-only; what reaches the kernel is a
    feature whose rows at some distance exist on one side only (n_r < n_l, down to n_r = 0, and the reverse), and the
    hand-written table above has whole groups of one side.  An exact tie does not arise by chance in groups of
    thousands of rows; tie_data() constructs one in a group of two."""
    ctgs = swt.synth_ctgs()
    data = swt.synth_data(swt.synth_lines(ctgs))
    text = swt.model(ctgs, data)
    per = {}
    for row in text.split(b"\n")[:-1]:
        f = row.split(b"\t")
        fid = f[0].rsplit(b":", 1)[0]
        per.setdefault(fid, {b"M": 0, b"L": 0, b"R": 0})[f[2]] += 1
    assert all(v[b"M"] == 1 for v in per.values()) and len(per) > 3500
    assert any(v[b"L"] == 0 and v[b"R"] > 0 for v in per.values())                    # n_l = 0
    assert any(v[b"R"] == 0 and v[b"L"] > 0 for v in per.values())                    # n_r = 0
    assert any(0 < v[b"R"] < v[b"L"] for v in per.values()) and any(0 < v[b"L"] < v[b"R"] for v in per.values())
    table = sws.summary([text])[1]
    assert sorted(d for _, d in table.groups) == list(range(21)) and table.rows() == text.count(b"\n") > 100000
    assert (41 * len(per)) % 256 != 0
    # the constructed tie
    tie = sws.tie_data(ctgs, lambda d: swt.model(ctgs, d))
    t = sws.summary([swt.model(ctgs, tie)])[1]
    assert (None, 0, 0) in sws.ties(t) and t.groups[(None, 0)][0] == 2
    # the flank cases: one tile gives NaN deviations beside a finite mean, no tile a NaN mean beside a -0 deviation
    small = swt.synth_data(swt.synth_lines(ctgs, seed=37, n=600))
    one_tile = sws.summary([swt.model(ctgs, small, 100, 20, 100)])[1]
    assert all(g[2][2] == g[0] and g[2][3] == g[0] and g[2][1] == 0 for (_, d), g in one_tile.groups.items() if d)
    assert 0 < one_tile.groups[(None, 0)][2][1] < one_tile.groups[(None, 0)][2][2]     # (an M window cut short at an edge: no tile)
    no_tile = swt.model(ctgs, small, 100, 20, 50)
    assert b"\tNaN\t-0\tNaN\t" in no_tile
