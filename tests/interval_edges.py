"""Input builders and CPU models for the edges of the interval index (gams_amd/csrc/interval.hip,
interval_kernels.hpp): the tie order of the three sort paths, the packed one-word sort key at its limits, count
cells and span cells of exact occupancy, degenerate intervals and extreme queries.  test_interval_edges_cpu.py
proves the builders on the CPU, test_gpu_interval_edges.py runs the kernels on them.

Expected values are the CPU twins (oracle/gams_ref.c), computed once per case and shared.  Nothing here imports
the GPU package, and the oracle is imported inside the functions that need it.
"""
import functools

import numpy as np

U32_MAX = 2**32 - 1
I32_MIN, I32_MAX = -2**31, 2**31 - 1

# what the sweeps below rest on; test_interval_edges_cpu.py reads the same numbers out of the C text
CELL_SHIFT = 1          # GAMS_CELL_SHIFT: about 2^CELL_SHIFT keys per cell of the count path's grid
BK_INLINE = 7           # BkRec::k: keys inline in a count cell's record
SPAN_INLINE = 5         # SpanCell::lo / hi: spans inline in a cover cell's record
WALK_STEPS = 6          # covered_upto_below: records walked before it searches
BUILD_CAP = 8192        # kBuildCap: the largest group sorted in a workgroup's LDS


# ---- mirrors of the builders' arithmetic ---------------------------------------------------------------------------
def dir_params(first, last, n):
    """dir_params / build_dir: (key0, shift, nb) of a grid of at most n buckets over [first, last]"""
    if n == 0:
        return 0, 0, 0
    rng = int(last) - int(first)
    shift = 0
    while (rng >> shift) >= n:
        shift += 1
    return int(first), shift, (rng >> shift) + 1


def count_grid(st, sp):
    """the ONE grid of cells the count path lays over a group's starts and stops (index_group_kernel)"""
    n = st.size
    return dir_params(min(int(st.min()), int(sp.min())), max(int(st.max()), int(sp.max())), (n >> CELL_SHIFT) + 1)


def cell_occupancy(keys, grid):
    """keys per cell of the grid, cell 0 first"""
    key0, shift, nb = grid
    return np.bincount((np.asarray(keys, np.int64) - key0) >> shift, minlength=nb)


def span_grid(lo):
    """build_dir over the biased lows of one group's spans (gams_spans_create)"""
    key = np.asarray(lo, np.int64) + 2**31
    return dir_params(key[0], key[-1], key.size)


def by_position(occ):
    """occupancies of the first cell, of the cells in the middle and of the last cell (a grid of at least 3 cells)"""
    return {int(occ[0])}, {int(x) for x in occ[1:-1]}, {int(occ[-1])}


def pack_bits(st, sp):
    """(bs, bt, bp) of index_build_kernel's packed key: the bit length of (max - min) | 1 of the starts and of the
    stops, and of the slot number among N = 2^ceil(log2 n) >= 4 slots.  One word when the sum is at most 64."""
    n = st.size
    N = 4
    while N < n:
        N <<= 1
    bs = ((int(st.max()) - int(st.min())) | 1).bit_length()
    bt = ((int(sp.max()) - int(sp.min())) | 1).bit_length()
    return bs, bt, ((N - 1) | 1).bit_length()


# ---- cases: one index and its queries --------------------------------------------------------------------------------
class IndexCase:
    """groups: [(label, starts, stops)] in the caller's order; queries: per group (qs, qe)"""

    def __init__(self, groups, queries):
        self.labels = [g[0] for g in groups]
        self.groups = [(np.asarray(g[1], np.uint32), np.asarray(g[2], np.uint32)) for g in groups]
        self.off = np.cumsum([0] + [g[0].size for g in self.groups]).astype(np.uint64)
        self.starts = np.ascontiguousarray(np.concatenate([g[0] for g in self.groups]), np.uint32)
        self.stops = np.ascontiguousarray(np.concatenate([g[1] for g in self.groups]), np.uint32)
        self.qg = np.ascontiguousarray(np.concatenate([np.full(q[0].size, g) for g, q in enumerate(queries)]), np.uint32)
        self.qs = np.ascontiguousarray(np.concatenate([q[0] for q in queries]), np.uint32)
        self.qe = np.ascontiguousarray(np.concatenate([q[1] for q in queries]), np.uint32)
        for a in (self.off, self.starts, self.stops, self.qg, self.qs, self.qe):
            a.setflags(write=False)

    @property
    def n_groups(self):
        return len(self.groups)

    def describe(self, q):
        g = int(self.qg[q])
        return f"query {q}: group {g} ({self.labels[g]}), qs {int(self.qs[q])}, qe {int(self.qe[q])}"


def _u32(x):
    return np.clip(np.asarray(x, np.int64), 0, U32_MAX)


# 1. tie order ----------------------------------------------------------------------------------------------------------
TIE_SIZES = (3, 4, 5, 255, 256, 257, 1024, 1025, 2048, 2049, 4096, 4097, 8192)
TIE_SIZES_RADIX = TIE_SIZES + (8193, 20000)


def tie_group(n, wide, seed):
    """n intervals made of about n / 8 distinct (start, stop) pairs, each repeated, shuffled: equal pairs sit at
    scattered positions of the caller's order.  wide: starts and stops both span nearly 2^32 (the two-word network);
    else coordinates of a few bits (the packed key).  -> (starts, stops, the distinct pairs)"""
    rng = np.random.default_rng(seed)
    d = max(2, n // 8)
    if wide:
        base = rng.integers(1000, 2**32 - 2000, (d + 1) // 2)
        st = rng.choice(base, d)                               # equal starts with different stops among them
        st[0], st[1] = 3, 2**32 - 900
        sp = st + rng.integers(1, 200, d)
    else:
        st = rng.integers(0, max(2, d // 2), d) * 5 + 10
        sp = st + rng.integers(1, 6, d)
    pairs = np.unique(np.stack([st, sp], 1), axis=0)
    reps = pairs[np.arange(n) % len(pairs)][rng.permutation(n)]
    return reps[:, 0].astype(np.uint32), reps[:, 1].astype(np.uint32), pairs


def tie_queries(pairs, wide):
    """every distinct pair exactly, from its first and from its last base, and ranges that cover several pairs"""
    a, b = pairs[:, 0], pairs[:, 1]
    qs = [a, b - 1, a, a, a - 3]
    qe = [a + 1, b, a + 7, a + 40, b + 1000]
    if wide:
        qs.append(a)
        qe.append(a + 2**30)
    return _u32(np.concatenate(qs)), _u32(np.concatenate(qe))


@functools.lru_cache(maxsize=None)
def tie_case(radix):
    """radix False: every group fits a workgroup (index_build_kernel); True: groups of 8,193 and 20,000 intervals send
    the whole index through the segmented radix sort and the table kernels"""
    groups, queries = [], []
    for n in (TIE_SIZES_RADIX if radix else TIE_SIZES):
        for wide in (False, True):
            st, sp, pairs = tie_group(n, wide, 1000 + 2 * n + wide)
            groups.append((f"n={n} {'wide' if wide else 'narrow'}", st, sp))
            queries.append(tie_queries(pairs, wide))
    return IndexCase(groups, queries)


# 2. the packed key at its limits ----------------------------------------------------------------------------------------
PACKED_SIZES = (1024, 1025)        # N = 1,024 with bp = 10 and no pads; N = 2,048 with bp = 11 and 1,023 pads
PACKED_KINDS = ("sum64", "sum65", "bt32", "bs32")


def packed_sum(n, kind):
    """bs + bt + bp the variant is built for"""
    bp = 10 if n <= 1024 else 11
    return {"sum64": 64, "sum65": 65, "bt32": 10 + 32 + bp, "bs32": 32 + 10 + bp}[kind]


def packed_group(n, kind, seed):
    rng = np.random.default_rng(seed)
    bp = 10 if n <= 1024 else 11
    d = n // 2 + 1

    def band(lo, bits):
        """d values in [lo, lo + 2^bits - 1], both ends among them"""
        v = lo + rng.integers(0, 2**bits, d)
        v[0], v[1] = lo, lo + 2**bits - 1
        return v

    if kind in ("sum64", "sum65"):
        bs = 27 if kind == "sum64" else 28
        bt = 64 - bp - 27
        st = band(1000, bs)
        sp = band(2**28 + 5000, bt)                            # beyond every start
    elif kind == "bt32":
        st = band(100, 10)
        sp = band(7, 32)[:d]
        sp[1] = U32_MAX
        sp = np.minimum(sp, U32_MAX)
    else:
        st = np.minimum(band(0, 32), U32_MAX)
        st[1] = U32_MAX
        sp = band(2**31, 10)                                   # many of these intervals are reversed
    # the largest start with the largest stop: with bs + bt + bp == 64 and n == N its key at the last slot is all ones
    st[2], sp[2] = st.max(), sp.max()
    st[3], sp[3] = st.min(), sp.min()
    idx = np.arange(n) % d
    idx = idx[rng.permutation(n)]
    idx[n - 1] = 2
    return st[idx].astype(np.uint32), sp[idx].astype(np.uint32)


def packed_queries(st, sp, seed):
    """from every stored start and stop, each also shifted by +-1"""
    rng = np.random.default_rng(seed)
    v = np.concatenate([st, sp]).astype(np.int64)
    v = np.unique(_u32(np.concatenate([v - 1, v, v + 1])))
    a, b = rng.choice(v, 2 * v.size), rng.choice(v, 2 * v.size)
    return np.concatenate([v, np.minimum(a, b)]), np.concatenate([_u32(v + 1), np.maximum(a, b)])


@functools.lru_cache(maxsize=None)
def packed_case():
    groups, queries = [], []
    for n in PACKED_SIZES:
        for k, kind in enumerate(PACKED_KINDS):
            st, sp = packed_group(n, kind, 2000 + 10 * n + k)
            groups.append((f"n={n} {kind}", st, sp))
            queries.append(packed_queries(st, sp, 3000 + 10 * n + k))
    return IndexCase(groups, queries)


# 3. count cells of exact occupancy ------------------------------------------------------------------------------------
CELL_C = tuple(range(1, 21)) + (31, 32, 33)
CELL_RECIPES = {"first": (1000, (4_000_000_000,)), "last": (4_000_000_000, (5,)),
                "middle": (2_000_000_000, (5, 4_000_000_000))}


def cell_group(recipe, c, equal_starts):
    """c keys in one cell of the count grid plus the outliers that stretch the grid.  equal_starts: c equal starts
    with different stops; else c consecutive starts, stop = start + 1."""
    base, outliers = CELL_RECIPES[recipe]
    k = np.arange(c, dtype=np.int64)
    st = np.full(c, base, np.int64) if equal_starts else base + k
    sp = base + 1 + k
    o = np.array(outliers, np.int64)
    return np.concatenate([st, o]).astype(np.uint32), np.concatenate([sp, o + 1]).astype(np.uint32)


def _pairs_in(lo, hi):
    """every (qs, qe) with qs <= qe + 1 in [lo, hi]"""
    v = np.arange(lo, hi + 1, dtype=np.int64)
    a, b = np.meshgrid(v, v, indexing="ij")
    k = a <= b + 1
    return a[k], b[k]


def cell_queries(recipe, c):
    base, outliers = CELL_RECIPES[recipe]
    qs, qe = [], []
    a, b = _pairs_in(base - 2, base + c + 3)
    qs.append(a)
    qe.append(b)
    w = np.arange(base - 2, base + c + 4, dtype=np.int64)
    for o in outliers:
        a, b = _pairs_in(o - 2, o + 1 + 3)
        qs.append(a)
        qe.append(b)
        for far in range(o - 1, o + 3):                        # from the cluster to the outlier or back
            qs.append(np.minimum(w, far))
            qe.append(np.maximum(w, far))
    return _u32(np.concatenate(qs)), _u32(np.concatenate(qe))


@functools.lru_cache(maxsize=None)
def cell_case():
    groups, queries = [], []
    for recipe in CELL_RECIPES:
        for equal_starts in (False, True):
            for c in CELL_C:
                st, sp = cell_group(recipe, c, equal_starts)
                groups.append((f"{recipe} c={c} {'equal starts' if equal_starts else 'consecutive'}", st, sp))
                queries.append(cell_queries(recipe, c))
    return IndexCase(groups, queries)


# 5. degenerate intervals and extreme queries ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def degenerate_case():
    M = U32_MAX
    k = np.arange(30, dtype=np.int64)
    mixed = [(10, 10), (20, 20), (30, 25), (40, 0), (0, 5), (0, 0), (0, M), (100, M), (M, M), (M, 0), (M - 1, M),
             (7, 7), (7, 7), (9, 3)] + [(50 + 2 * i, 51 + 2 * i) for i in range(12)]
    long_over = [(1000 + 10 * i, 1003 + 10 * i) for i in range(200)] + [(5, 5000), (2000, 2000), (2500, 2400)]
    groups = [
        ("mixed", [p[0] for p in mixed], [p[1] for p in mixed]),
        ("one long interval over many short ones", [p[0] for p in long_over], [p[1] for p in long_over]),
        ("stop == start", 100 + 3 * k, 100 + 3 * k),
        ("stop < start", 1000 + 5 * k, 998 + 3 * k),
        ("one interval at the top", [M], [M]),
        ("stops at the pad value", [M - 15, 0, M - 2], [M, M, M - 1]),
        ("starts of 0", [0, 0, 0, 0, 0], [0, 1, M, 2, 1]),
    ]
    queries = []
    for _, st, sp in groups:
        v = np.concatenate([np.asarray(st, np.int64), np.asarray(sp, np.int64)])
        if v.size > 100:
            v = np.concatenate([v[::10], v[-8:]])
        v = np.unique(_u32(np.concatenate([v - 1, v, v + 1, [0, 1, 2, M - 1, M]])))
        a, b = np.meshgrid(v, v, indexing="ij")                # every order: qs == qe and qe < qs among them
        queries.append((a.ravel(), b.ravel()))
    return IndexCase(groups, queries)


CASES = {"ties": lambda: tie_case(False), "ties_radix": lambda: tie_case(True), "packed": packed_case,
         "cells": cell_case, "degenerate": degenerate_case}


@functools.lru_cache(maxsize=None)
def twin_answers(name):
    """(count, hit) of gams_ref_count and gams_ref_locate on every query of the case"""
    from oracle import oracle as ora

    R = ora.ref()
    c = CASES[name]()
    cnt = np.full(c.qg.size, -99, np.int32)
    hit = np.full(c.qg.size, -99, np.int64)
    args = (c.n_groups, c.off.ctypes.data, c.starts.ctypes.data, c.stops.ctypes.data, c.qg.ctypes.data, c.qs.ctypes.data,
            c.qe.ctypes.data, c.qg.size)
    assert R.gams_ref_count(*args, cnt.ctypes.data) == 0
    assert R.gams_ref_locate(*args, hit.ctypes.data) == 0
    cnt.setflags(write=False)
    hit.setflags(write=False)
    return cnt, hit


def closed_form_count(c):
    """Lapper::count in numpy: #{start < qe} - #{stop <= qs}, the signed difference of the two lower bounds"""
    out = np.empty(c.qg.size, np.int64)
    for g, (st, sp) in enumerate(c.groups):
        sel = np.flatnonzero(c.qg == g)
        out[sel] = (np.searchsorted(np.sort(st), c.qe[sel], "left").astype(np.int64)
                    - np.searchsorted(np.sort(sp), c.qs[sel].astype(np.uint64) + 1, "left"))
    return out


def first_of_equal_pairs(c, hit):
    """for every hit: the smallest index in the caller's order among the group's intervals equal to the one found"""
    out = np.full(hit.size, -1, np.int64)
    for g, (st, sp) in enumerate(c.groups):
        sel = np.flatnonzero((c.qg == g) & (hit >= 0))
        if not sel.size:
            continue
        key = (st.astype(np.uint64) << np.uint64(32)) | sp.astype(np.uint64)
        order = np.argsort(key, kind="stable")
        first = order[np.searchsorted(key[order], key[hit[sel] - int(c.off[g])], "left")]
        out[sel] = first + int(c.off[g])
    return out


# 4. cover cells of exact occupancy, and the walk ---------------------------------------------------------------------
SPAN_C = tuple(range(1, 13))
# (cluster base, outliers before, outliers behind): c disjoint spans [base + 3k, base + 3k + 1]
SPAN_RECIPES = {"first": (100, (), (2_000_000_000,)), "last": (1_900_000_000, (5,), ()),
                "middle": (1_000_000_000, (5,), (2_000_000_000,)),
                "first, negative": (-2_000_000_000, (), (2_000_000_000,)),
                "last, across zero": (-20, (-2_000_000_000,), ())}


def span_group(recipe, c):
    base, before, behind = SPAN_RECIPES[recipe]
    lo = base + 3 * np.arange(c, dtype=np.int64)
    b, a = np.array(before, np.int64), np.array(behind, np.int64)
    return (np.concatenate([b, lo, a]).astype(np.int32), np.concatenate([b + 4, lo + 1, a + 100]).astype(np.int32))


def span_queries(recipe, c):
    """(s, e, clip_lo, clip_hi): every s <= e across the cluster, each clipped by itself, by a window one base
    shorter on each side and by a far-away window; some around the outliers; s = INT32_MIN and e = INT32_MAX - 1"""
    base, before, behind = SPAN_RECIPES[recipe]
    first, last = base, base + 3 * (c - 1) + 1
    v = np.arange(first - 2, last + 3, dtype=np.int64)
    a, b = np.meshgrid(v, v, indexing="ij")
    k = a <= b
    s, e = [a[k]], [b[k]]
    for o, width in [(x, 4) for x in before] + [(x, 100) for x in behind]:
        w = np.array([o - 1, o, o + 1, o + width - 1, o + width, o + width + 1], np.int64)
        a, b = np.meshgrid(w, w, indexing="ij")
        k = a <= b
        s.append(a[k])
        e.append(b[k])
    inner = np.array([first - 1, first, first + 3 * (c // 2), last, last + 2], np.int64)
    s.append(np.full(inner.size + 2, I32_MIN, np.int64))       # the L > INT32_MIN branch
    e.append(np.concatenate([inner, [I32_MIN, I32_MAX - 1]]))
    s.append(np.concatenate([inner, [I32_MAX - 1]]))
    e.append(np.full(inner.size + 1, I32_MAX - 1, np.int64))
    s, e = np.concatenate(s), np.concatenate(e)
    far_lo = np.where(e < I32_MAX - 3000, e + 1000, np.where(s > I32_MIN + 3000, s - 2000, 5))
    far_hi = np.where(e < I32_MAX - 3000, e + 2000, np.where(s > I32_MIN + 3000, s - 1000, 4))
    cl = np.concatenate([s, np.minimum(s + 1, I32_MAX), far_lo])
    ch = np.concatenate([e, np.maximum(e - 1, I32_MIN), far_hi])
    return np.tile(s, 3), np.tile(e, 3), cl, ch


class CoverCase:
    def __init__(self):
        self.labels, self.sets, q = [], [], []
        for recipe in SPAN_RECIPES:
            for c in SPAN_C:
                self.labels.append(f"{recipe} c={c}")
                self.sets.append(span_group(recipe, c))
                q.append(span_queries(recipe, c))
        self.off = np.cumsum([0] + [s[0].size for s in self.sets]).astype(np.uint64)
        self.lo = np.ascontiguousarray(np.concatenate([s[0] for s in self.sets]), np.int32)
        self.hi = np.ascontiguousarray(np.concatenate([s[1] for s in self.sets]), np.int32)
        self.g = np.ascontiguousarray(np.concatenate([np.full(x[0].size, g) for g, x in enumerate(q)]), np.uint32)
        self.s, self.e, self.cl, self.ch = (np.ascontiguousarray(np.concatenate([x[k] for x in q]), np.int32)
                                            for k in range(4))
        self.far = np.concatenate([np.arange(x[0].size) >= 2 * (x[0].size // 3) for x in q])   # the far-away clips
        for a in (self.off, self.lo, self.hi, self.g, self.s, self.e, self.cl, self.ch):
            a.setflags(write=False)

    @property
    def n_groups(self):
        return len(self.sets)

    def describe(self, q):
        g = int(self.g[q])
        return (f"query {q}: group {g} ({self.labels[g]}), range {int(self.s[q])}..{int(self.e[q])}, "
                f"clip {int(self.cl[q])}..{int(self.ch[q])}")


@functools.lru_cache(maxsize=None)
def cover_case():
    return CoverCase()


@functools.lru_cache(maxsize=None)
def twin_cover():
    from oracle import oracle as ora

    R = ora.ref()
    c = cover_case()
    prop = np.full(c.g.size, -1, np.float32)
    assert R.gams_ref_cover(c.n_groups, c.off.ctypes.data, c.lo.ctypes.data, c.hi.ctypes.data, c.g.ctypes.data,
                            c.cl.ctypes.data, c.ch.ctypes.data, c.s.ctypes.data, c.e.ctypes.data, c.g.size,
                            prop.ctypes.data) == 0
    prop.setflags(write=False)
    return prop


def cover_model(lo, L, H):
    """span_cover_kernel's choice for clipped ranges [L, H] (H >= L, int64 arrays) against one group of spans:
    -> (fallback, between, below): whether a crowded cell sends the query to covered_upto + covered_upto_below, the
    spans with L - 1 < lo <= H that the walk passes, and the spans with lo <= L - 1 (none: the answer below is 0)"""
    key = np.asarray(lo, np.int64) + 2**31
    n = key.size
    key0, shift, nb = span_grid(lo)
    rank_edge = np.searchsorted(key, key0 + (np.arange(nb, dtype=np.int64) << shift), "left")

    def crowded(x):
        kx = x + 2**31
        has = kx >= key0
        b = np.minimum((np.maximum(kx, key0) - key0) >> shift, nb - 1)
        r = rank_edge[b]
        t = np.minimum(np.searchsorted(key, kx, "right") - r, SPAN_INLINE)
        return has & (t == SPAN_INLINE) & (r + SPAN_INLINE < n)

    fallback = crowded(H) | ((L > I32_MIN) & crowded(L - 1))
    below = np.searchsorted(key, L - 1 + 2**31, "right")
    return fallback, np.searchsorted(key, H + 2**31, "right") - below, below
