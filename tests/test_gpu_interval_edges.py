"""The interval index at its edges, through the C ABI: the tie order of every sort path (gams_gpu_locate returns the
index of the earliest of equal (start, stop) pairs in the caller's order), the packed one-word sort key at its
limits, count cells and cover cells of exact occupancy around their inline capacities, degenerate intervals and
extreme queries, and the same tie order through the text path.  Inputs and models: interval_edges.py, proved on the
CPU by test_interval_edges_cpu.py.  Expected values: the CPU twins gams_ref_count / gams_ref_locate /
gams_ref_cover on every query, compared exactly (integers equal, floats bit for bit), and the numpy closed form of
Lapper::count."""
import ctypes as C

import numpy as np
import pytest

import interval_edges as ie
from gams_amd import engine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = engine.Engine(0)
    yield e
    e.close()


def run_index(eng, c):
    """(count, hit) of gams_gpu_count and gams_gpu_locate on every query of the case, one call each"""
    ix = C.c_void_p()
    eng.check(eng.lib.gams_index_create(eng.h, c.n_groups, c.off.ctypes.data, c.starts.ctypes.data, c.stops.ctypes.data,
                                        C.byref(ix)))
    cnt = np.full(c.qg.size, -99, np.int32)
    hit = np.full(c.qg.size, -99, np.int64)
    try:
        eng.check(eng.lib.gams_gpu_count(eng.h, ix, c.qg.ctypes.data, c.qs.ctypes.data, c.qe.ctypes.data, c.qg.size,
                                         cnt.ctypes.data))
        eng.check(eng.lib.gams_gpu_locate(eng.h, ix, c.qg.ctypes.data, c.qs.ctypes.data, c.qe.ctypes.data, c.qg.size,
                                          hit.ctypes.data))
    finally:
        eng.lib.gams_index_destroy(eng.h, ix)
    return cnt, hit


def same(c, got, exp, what):
    """exact equality on every query; the first few that differ named by their group"""
    bad = np.flatnonzero(got != exp)
    assert bad.size == 0, (f"{what}: {bad.size} of {got.size} queries differ; "
                           + "; ".join(f"{c.describe(q)}: got {got[q]}, expected {exp[q]}" for q in bad[:5]))


def check_case(eng, name):
    c = ie.CASES[name]()
    exp_cnt, exp_hit = ie.twin_answers(name)
    cnt, hit = run_index(eng, c)
    same(c, cnt, exp_cnt, "count against gams_ref_count")
    same(c, cnt.astype(np.int64), ie.closed_form_count(c), "count against the closed form")
    same(c, hit, exp_hit, "locate against gams_ref_locate")
    return c, cnt, hit


def test_tie_order_of_the_workgroup_sorts(eng):
    """groups of every size around the LDS build's capacities, once with narrow coordinates (the packed one-word
    key) and once spanning nearly 2^32 (the two-word network), about eight scattered copies of every pair: the hit
    is the copy that comes first in the caller's order"""
    c, _, hit = check_case(eng, "ties")
    same(c, hit, ie.first_of_equal_pairs(c, hit), "the hit is not the first of its equal pairs")


def test_tie_order_through_the_radix_sort(eng):
    """the same groups plus 8,193 and 20,000 intervals: the whole index, the small groups included, goes through
    the segmented radix sort and the table kernels"""
    c, _, hit = check_case(eng, "ties_radix")
    same(c, hit, ie.first_of_equal_pairs(c, hit), "the hit is not the first of its equal pairs")


def test_packed_key_at_its_limits(eng):
    """bs + bt + bp of exactly 64 and 65, bt == 32 over narrow starts, bs == 32 over narrow stops (reversed
    intervals among them), each without pads (n == N == 1,024) and with 1,023 of them (n == 1,025)"""
    check_case(eng, "packed")


def test_count_cells_of_exact_occupancy(eng):
    """a first, a middle and a last cell of the count grid holding 1 .. 20 and 31 .. 33 keys: the seven inline keys,
    the batch of eight behind them, its early exits and the search inside a larger cell, and the group's end"""
    check_case(eng, "cells")


def test_degenerate_intervals_and_extreme_queries(eng):
    """stop == start, stop < start, starts of 0 and 2^32 - 1, stops of 2^32 - 1 (the pad value of a cell record), one
    long interval over many short ones; queries with qs == 2^32 - 1, qe == 0, qs == qe and qe < qs.  The twin defines
    the answers: count is last - first as a signed difference, locate the scan for start < qe && stop > qs."""
    c, cnt, _ = check_case(eng, "degenerate")
    assert cnt.min() < 0 < cnt.max()


def test_cover_cells_of_exact_occupancy_and_the_walk(eng):
    """1 .. 12 spans in a first, a middle and a last cell of the span grid (five inline, then covered_upto), every
    range across them, so that covered_upto_below walks 0 .. 12 records (six before it searches), each clipped by
    itself, by a window one base shorter on each side and by a far-away one; negative coordinates, s == INT32_MIN
    and e == INT32_MAX - 1"""
    c = ie.cover_case()
    exp = ie.twin_cover()
    sp = C.c_void_p()
    eng.check(eng.lib.gams_spans_create(eng.h, c.n_groups, c.off.ctypes.data, c.lo.ctypes.data, c.hi.ctypes.data,
                                        C.byref(sp)))
    prop = np.full(c.g.size, -1, np.float32)
    try:
        eng.check(eng.lib.gams_gpu_cover(eng.h, sp, c.g.ctypes.data, c.cl.ctypes.data, c.ch.ctypes.data, c.s.ctypes.data,
                                         c.e.ctypes.data, c.g.size, prop.ctypes.data))
    finally:
        eng.lib.gams_spans_destroy(eng.h, sp)
    same(c, prop.view(np.uint32), exp.view(np.uint32), "prop, bit for bit, against gams_ref_cover")


def test_locate_text_prints_the_earlier_of_two_equal_ctgs(eng):
    """two ctgs of one chromosome with the same interval and different ids: every located line prints the id of
    the one that comes first in the caller's order, on the device text path and through host.locate"""
    from gams_amd import host
    from oracle import oracle as ora
    from test_gpu_text_ops import LocTables, abi_locate

    def ctg(cid, chr_id, s, e):
        return dict(id=cid, chr_id=chr_id, chr_start=s, chr_end=e)

    # the ids sort against the caller's order, so that no sort by name gives the right answer by accident
    ctgs = [ctg("ctg:I:9", "I", 1, 1000), ctg("ctg:I:2", "I", 1, 1000), ctg("ctg:II:5", "II", 1, 500),
            ctg("ctg:I:8", "I", 2001, 3000), ctg("ctg:I:7", "I", 1001, 2000), ctg("ctg:I:1", "I", 2001, 3000),
            ctg("ctg:II:4", "II", 1, 500), ctg("ctg:I:0", "I", 1, 1000)]
    earlier = {"ctg:I:2": "ctg:I:9", "ctg:I:0": "ctg:I:9", "ctg:I:1": "ctg:I:8", "ctg:II:4": "ctg:II:5"}
    rgs = [("I", 5, 10), ("I", 1000, 1000), ("I", 1, 1000), ("I", 2500, 2600), ("I", 900, 1100), ("I", 2001, 2002),
           ("I", 3000, 3000), ("II", 7, 9), ("II", 500, 500), ("I", 1500, 2500), ("I", 1, 1), ("II", 400, 900)]
    lines = [f"{c}:{s}-{e}" if e != s else f"{c}:{s}" for c, s, e in rgs]
    # expected: gams_ref_locate over the tables as LocTables lays them out (chromosomes by name, the caller's order inside)
    chrs = sorted({c["chr_id"] for c in ctgs})
    ordered = [c for k in chrs for c in ctgs if c["chr_id"] == k]
    off = np.cumsum([0] + [sum(c["chr_id"] == k for c in ctgs) for k in chrs]).astype(np.uint64)
    st = np.array([c["chr_start"] for c in ordered], np.uint32)
    sp = np.array([c["chr_end"] + 1 for c in ordered], np.uint32)
    qg = np.array([chrs.index(c) for c, _, _ in rgs], np.uint32)
    qs = np.array([s for _, s, _ in rgs], np.uint32)
    qe = np.array([e for _, _, e in rgs], np.uint32)                      # Lapper::find(start, end), utils.rs:16
    hit = np.full(len(rgs), -9, np.int64)
    assert ora.ref().gams_ref_locate(len(chrs), off.ctypes.data, st.ctypes.data, sp.ctypes.data, qg.ctypes.data,
                                     qs.ctypes.data, qe.ctypes.data, len(rgs), hit.ctypes.data) == 0
    want = [(ln, ordered[h]["id"]) for ln, h in zip(lines, hit) if h >= 0]
    assert len(want) >= 9 and not any(cid in earlier for _, cid in want)
    assert {cid for _, cid in want} >= set(earlier.values())
    exp = "".join(f"{ln}\t{cid}\n" for ln, cid in want)
    data = ("\n".join(lines) + "\n").encode()
    T = LocTables(eng, ctgs)
    try:
        rc, text, rows = abi_locate(eng, T, data)
    finally:
        T.close()
    assert rc == 0 and rows == len(want) and text.decode() == exp
    assert host.locate(eng, ctgs, lines) == exp
    assert host.locate_text(eng, ctgs, data).decode() == exp and host.last_operator_device() == 1
