"""The builders of interval_edges.py land where they aim, and the CPU twins agree with the closed forms on them: the
tie groups take the sort network they are meant for, the packed-key variants hit their bit sums, the cell sweeps
produce every occupancy around the inline capacities under a mirror of the grid rule, and the constants all of
that rests on are still the ones in the C text.  No GPU; test_gpu_interval_edges.py runs the kernels on the same
inputs."""
import os
import re

import numpy as np

import interval_edges as ie

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _src(name):
    with open(os.path.join(ROOT, "gams_amd", "csrc", name)) as fh:
        return fh.read()


def test_constants_follow_the_source():
    """a change of any of these must bring the sweeps of interval_edges.py up for review"""
    hpp, hip = _src("interval_kernels.hpp"), _src("interval.hip")
    m = re.search(r"#ifndef GAMS_CELL_SHIFT\s*\n#define GAMS_CELL_SHIFT (\d+)\s*\n#endif", hpp)
    assert m and int(m.group(1)) == ie.CELL_SHIFT == 1
    assert "GAMS_CELL_SHIFT" not in _src("Makefile")                     # nothing overrides the default
    bk = re.search(r"struct BkRec \{(.*?)\};", hpp, flags=re.S).group(1)
    assert re.findall(r"uint32_t k\[(\d+)\];", bk) == [str(ie.BK_INLINE)] == ["7"]
    cell = re.search(r"struct SpanCell \{(.*?)\};", hpp, flags=re.S).group(1)
    assert re.findall(r"int32_t lo\[(\d+)\], hi\[(\d+)\];", cell) == [(str(ie.SPAN_INLINE),) * 2] == [("5", "5")]
    walk = re.search(r"uint64_t covered_upto_below\(.*?\n\}", hpp, flags=re.S).group(0)
    assert re.findall(r"for \(int step = 0; step < (\d+); \+\+step\)", walk) == [str(ie.WALK_STEPS)] == ["6"]
    assert re.findall(r"constexpr uint32_t kBuildCap = (\d+);", hip) == [str(ie.BUILD_CAP)]
    # the grid of the count cells: (n >> kCellShift) + 1 slots over min(first start, first stop) .. max(last, last)
    assert hip.count("(n >> kCellShift) + 1u") == 2


def test_dir_params_mirror():
    assert ie.dir_params(0, 0, 1) == (0, 0, 1)
    assert ie.dir_params(5, 5 + 2**31, 1) == (5, 32, 1)                  # a one-cell grid wider than 2^31: shift 32
    assert ie.dir_params(10, 19, 10) == (10, 0, 10)
    assert ie.dir_params(10, 20, 10) == (10, 1, 6)
    assert ie.dir_params(0, 0, 0) == (0, 0, 0)
    occ = ie.cell_occupancy([10, 11, 12, 20], ie.dir_params(10, 20, 3))
    assert occ.tolist() == [3, 0, 1]


def test_tie_groups_take_both_networks_and_the_twin_returns_the_first_of_equal_pairs():
    for radix in (False, True):
        c = ie.tie_case(radix)
        sizes = ie.TIE_SIZES_RADIX if radix else ie.TIE_SIZES
        assert [g[0].size for g in c.groups] == [n for n in sizes for _ in (0, 1)]
        assert (max(sizes) > ie.BUILD_CAP) == radix
        for label, (st, sp) in zip(c.labels, c.groups):
            assert (sum(ie.pack_bits(st, sp)) <= 64) == ("narrow" in label), label
            assert np.all(sp > st)
            pairs, copies = np.unique(np.stack([st, sp], 1), axis=0, return_counts=True)
            assert copies.max() >= 2 and len(pairs) >= 2, label         # equal pairs, and more than one pair
            assert len(np.unique(st)) < len(pairs) or len(pairs) == 2, label   # equal starts with different stops
    c = ie.tie_case(True)
    cnt, hit = ie.twin_answers("ties_radix")
    assert np.array_equal(cnt, ie.closed_form_count(c))
    assert np.array_equal(hit >= 0, cnt > 0)                             # stop > start everywhere: a count is a hit
    # the twin's hit is the first of its equal pairs in the caller's order, and that is a real choice: most hits have
    # a later twin that an unstable sort could return instead
    assert np.array_equal(hit, ie.first_of_equal_pairs(c, hit))
    k = np.flatnonzero(hit >= 0)
    key = (c.starts.astype(np.uint64) << np.uint64(32)) | c.stops
    later = np.zeros(c.starts.size, bool)
    for g in range(c.n_groups):
        a, b = int(c.off[g]), int(c.off[g + 1])
        _, first, copies = np.unique(key[a:b], return_index=True, return_counts=True)
        later[a + first[copies > 1]] = True
    assert later[hit[k]].mean() > 0.8
    for g in range(c.n_groups):                                          # ... in every group
        assert later[hit[k[c.qg[k] == g]]].any(), c.labels[g]
    assert np.array_equal(ie.twin_answers("ties")[0], ie.closed_form_count(ie.tie_case(False)))


def test_packed_variants_land_on_their_bit_sums():
    c = ie.packed_case()
    it = iter(zip(c.labels, c.groups))
    for n in ie.PACKED_SIZES:
        for kind in ie.PACKED_KINDS:
            label, (st, sp) = next(it)
            bs, bt, bp = ie.pack_bits(st, sp)
            assert st.size == n and bp == (10 if n == 1024 else 11), label
            assert bs + bt + bp == ie.packed_sum(n, kind), (label, bs, bt, bp)
            if kind == "bt32":
                assert bt == 32 and int(st.max()) - int(st.min()) < 2**10 and int(sp.max()) == ie.U32_MAX
            if kind == "bs32":
                assert bs == 32 and np.count_nonzero(sp < st) > n // 4   # reversed intervals, legal input
            if kind == "sum64":                                          # the all-ones key, at the last slot
                assert (st[n - 1], sp[n - 1]) == (st.max(), sp.max())
                assert int(st.max()) - int(st.min()) == 2**bs - 1 and int(sp.max()) - int(sp.min()) == 2**bt - 1
            assert np.unique(np.stack([st, sp], 1), axis=0).shape[0] < n                # equal pairs here too
    cnt, hit = ie.twin_answers("packed")
    assert np.array_equal(cnt, ie.closed_form_count(c))
    assert np.array_equal(hit, ie.first_of_equal_pairs(c, hit))
    assert np.count_nonzero(hit >= 0) > hit.size // 4 and np.count_nonzero(hit < 0) > 100


def test_count_sweep_fills_cells_to_every_occupancy():
    c = ie.cell_case()
    want = set(range(5, 19))
    seen = {(arr, pos): set() for arr in ("starts", "stops") for pos in range(3)}
    it = iter(zip(c.labels, c.groups))
    for recipe in ie.CELL_RECIPES:
        for equal_starts in (False, True):
            for k in ie.CELL_C:
                label, (st, sp) = next(it)
                grid = ie.count_grid(st, sp)
                assert grid[2] >= 2, label
                cells_s = (st[:k].astype(np.int64) - grid[0]) >> grid[1]
                cells_t = (sp[:k].astype(np.int64) - grid[0]) >> grid[1]
                if recipe != "middle" or k >= 4:                         # all c keys share one cell, starts and stops
                    assert len(set(cells_s) | set(cells_t)) == 1, label
                    b = int(cells_s[0])
                    where = {"first": b == 0, "last": b == grid[2] - 1, "middle": 0 < b < grid[2] - 1}[recipe]
                    assert where, (label, b, grid)
                    pos = list(ie.CELL_RECIPES).index(recipe)
                    seen["starts", pos].add(int(ie.cell_occupancy(st, grid)[b]))
                    seen["stops", pos].add(int(ie.cell_occupancy(sp, grid)[b]))
    for key, occ in seen.items():
        assert want <= occ, (key, sorted(want - occ))
        assert {31, 32, 33} <= occ, key
    cnt, hit = ie.twin_answers("cells")
    assert np.array_equal(cnt, ie.closed_form_count(c))                  # the reference alone
    assert np.array_equal(hit, ie.first_of_equal_pairs(c, hit))
    per_group = np.bincount(c.qg, minlength=c.n_groups)
    assert per_group.min() > 50 and per_group.max() < 1500


def test_cover_sweep_fills_cells_and_crosses_the_walk():
    c = ie.cover_case()
    seen = [set(), set(), set()]
    for label, (lo, hi) in zip(c.labels, c.sets):
        assert np.all(hi >= lo) and np.all(lo[1:] > hi[:-1]), label      # what gams_spans_create demands
        if lo.size < 3:
            continue
        grid = ie.span_grid(lo)
        if grid[2] < 3:
            continue
        for pos, occ in zip(seen, ie.by_position(ie.cell_occupancy(lo.astype(np.int64) + 2**31, grid))):
            pos |= occ
    for pos in seen:
        assert {4, 5, 6} <= pos, seen
    # the crowded cells send queries to the walk, with 4 .. 8 spans between the two ends and spans below them
    g = c.labels.index("first c=12")
    sel = np.flatnonzero((c.g == g) & ~c.far)
    L = np.maximum(c.s[sel], c.cl[sel]).astype(np.int64)
    H = np.minimum(c.e[sel], c.ch[sel]).astype(np.int64)
    k = H >= L
    fallback, between, below = ie.cover_model(c.sets[g][0], L[k], H[k])
    assert set(range(0, 10)) <= set(between[fallback])
    assert {ie.WALK_STEPS - 1, ie.WALK_STEPS, ie.WALK_STEPS + 1} <= set(between[fallback & (below >= 1)])
    assert np.count_nonzero(~fallback) > 100
    prop = ie.twin_cover()
    assert np.all(prop[c.far] == 0)                                      # a far-away window
    assert np.count_nonzero(prop > 0) > prop.size // 4
    assert np.count_nonzero(c.s == ie.I32_MIN) > 100 and np.count_nonzero(c.e == ie.I32_MAX - 1) > 100
    assert np.all(c.e >= c.s)


def test_degenerate_case_holds_what_it_names():
    c = ie.degenerate_case()
    st, sp = c.starts, c.stops
    assert np.any(sp == st) and np.any(sp < st) and np.any(sp == ie.U32_MAX) and np.any(st == ie.U32_MAX) and np.any(st == 0)
    assert np.any(c.qs == ie.U32_MAX) and np.any(c.qe == 0) and np.any(c.qs == c.qe) and np.any(c.qe < c.qs)
    cnt, hit = ie.twin_answers("degenerate")
    assert np.array_equal(cnt, ie.closed_form_count(c))                  # last - first, a signed difference
    assert cnt.min() < 0 < cnt.max()
    # locate is the scan for start < qe && stop > qs over the (start, stop, caller's index) order
    rng = np.random.default_rng(5)
    for q in rng.choice(hit.size, 3000, replace=False):
        g = int(c.qg[q])
        s, t = c.groups[g]
        order = np.lexsort((np.arange(s.size), t, s))
        ok = (s[order] < c.qe[q]) & (t[order] > c.qs[q])
        exp = int(order[np.argmax(ok)]) + int(c.off[g]) if ok.any() else -1
        assert hit[q] == exp, c.describe(q)
    # the long interval lying over many short ones is the first hit of a query far inside it
    g = c.labels.index("one long interval over many short ones")
    q = np.flatnonzero((c.qg == g) & (c.qs > 1000) & (c.qe > c.qs) & (c.qe < 5000))
    assert q.size > 100 and np.all(hit[q] == int(c.off[g]) + 200)
