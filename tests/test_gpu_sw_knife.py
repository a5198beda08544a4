"""sw.hip where the f32 rounding order decides the printed value: sw_kernel, range_gc_kernel and range_gc_cols_kernel
on the batteries and the range grid of tests/sw_knife.py.  The rows of gams_gpu_sw_batch against the CPU twin
gams_ref_sw as bytes, per parameter set (the default, flanks of 7, 8 = kKeep, 9 and 16 tiles, tile values that are
ties at size 32, 64 and 128, the stddev-sensitive size 7), once as one selected ctg and once with the ctg selected
twice; gams_gpu_sw_text against the oracle's text over the same rows and over ctgs too short for a tile (NaN, -0);
the sets at 7, 8 and 9 tiles against each other where the ctg clips a flank to the same tiles; every (G/C count,
length) pair up to 4096 bases through gams_gpu_range_gc_batch against the model, bit for bit; the ties and the pairs
a wrong formula changes through gams_gpu_peak_text, on a ctg in the first 64-KiB segment of the seqset buffer and on
one behind it.  test_sw_knife_cpu.py proves on the CPU that a tree sum, f64 accumulation, a fused d * d, a one-pass
variance, half-even rounding and a reciprocal multiply each change rows these inputs hold."""
import ctypes as C

import numpy as np
import pytest

import peak_text as pt
import sw_knife as sk
from gams_amd import _lib, engine
from test_gpu_peak_text import PeakTables, abi_peak
from test_gpu_peak_text import in_id_order as peak_in_id_order
from test_gpu_text_edges import first_difference
from test_sw_knife_cpu import first_row_difference, oracle_text, twin_rows

pytestmark = pytest.mark.gpu

SETS = list(sk.SETS)
FILLER = 70_000          # bases of a ctg that pushes the next slot behind the first 64-KiB segment of the buffer


@pytest.fixture(scope="module")
def eng():
    e = engine.Engine(0)
    yield e
    e.close()


def seq_of(c):
    return np.frombuffer(c["seq"], np.uint8)


def gpu_rows(eng, ss, sel, ctgs, feats, params):
    """gams_gpu_sw_batch over the selected slots `sel` of the seqset (ctgs[k] and its features feats[k] = (fs, fe) for
    selected ctg k) -> (rows, row_off)"""
    sel = np.array(sel, np.uint32)
    cst = np.array([c["chr_start"] for c in ctgs], np.int32)
    foff = np.concatenate(([0], np.cumsum([f[0].size for f in feats]))).astype(np.uint64)
    fs = np.ascontiguousarray(np.concatenate([f[0] for f in feats]), np.int32)
    fe = np.ascontiguousarray(np.concatenate([f[1] for f in feats]), np.int32)
    n, roff = C.c_uint64(), np.zeros(sel.size + 1, np.uint64)
    args = (eng.h, ss.p, sel.size, sel.ctypes.data, cst.ctypes.data, foff.ctypes.data, fs.ctypes.data, fe.ctypes.data, *params)
    eng.check(eng.lib.gams_gpu_sw_batch(*args, None, 0, roff.ctypes.data, C.byref(n)))          # size query
    rows = np.zeros(n.value, _lib.SW_ROW_DTYPE)
    eng.check(eng.lib.gams_gpu_sw_batch(*args, rows.ctypes.data, rows.size, roff.ctypes.data, C.byref(n)))
    assert n.value == rows.size
    return rows, roff


def gpu_text(eng, ss, sel, ctgs, feats, params):
    """gams_gpu_sw_text over the same arguments -> (text, ctg_off, n_rows)"""
    sel = np.array(sel, np.uint32)
    cst = np.array([c["chr_start"] for c in ctgs], np.int32)
    foff = np.concatenate(([0], np.cumsum([f[0].size for f in feats]))).astype(np.uint64)
    fs = np.ascontiguousarray(np.concatenate([f[0] for f in feats]), np.int32)
    fe = np.ascontiguousarray(np.concatenate([f[1] for f in feats]), np.int32)
    ids = [i.encode() for c, f in zip(ctgs, feats) for i in sk.feature_ids(c, f[0].size)]
    id_arr = (C.c_char_p * len(ids))(*ids)
    chr_arr = (C.c_char_p * len(ctgs))(*[c["chr_id"].encode() for c in ctgs])
    txt, tb, toff, nr = C.c_void_p(), C.c_uint64(), C.c_void_p(), C.c_uint64()
    eng.check(eng.lib.gams_gpu_sw_text(eng.h, ss.p, sel.size, sel.ctypes.data, chr_arr, cst.ctypes.data, foff.ctypes.data,
                                       fs.ctypes.data, fe.ctypes.data, id_arr, *params, C.byref(txt), C.byref(tb), C.byref(toff),
                                       C.byref(nr)))
    off = np.frombuffer((C.c_uint64 * (sel.size + 1)).from_address(toff.value), np.uint64).copy()
    return (C.string_at(txt.value, tb.value) if tb.value else b""), off, nr.value


@pytest.mark.parametrize("params", SETS)
def test_rows_equal_the_twin(eng, params):
    """every field of every row of the battery, the floats bit for bit: alone, and with the ctg selected twice in one
    batch (the second time from a slot behind the first 64-KiB segment of the buffer)"""
    c, fs, fe, _ = sk.battery(params)
    want = twin_rows(c, fs, fe, params)
    ss = engine.SeqSet(eng, [seq_of(c), seq_of(c)])
    try:
        got, roff = gpu_rows(eng, ss, [0], [c], [(fs, fe)], params)
        assert first_row_difference(got, want) is None, first_row_difference(got, want)
        assert roff.tolist() == [0, want.size]
        got, roff = gpu_rows(eng, ss, [0, 1], [c, c], [(fs, fe), (fs, fe)], params)
        assert roff.tolist() == [0, want.size, 2 * want.size]
        for k in (0, 1):
            part = got[k * want.size:(k + 1) * want.size]
            assert first_row_difference(part, want) is None, (k, first_row_difference(part, want))
    finally:
        ss.close()


@pytest.mark.parametrize("params", SETS)
def test_rows_of_short_ctgs_equal_the_twin(eng, params):
    """ctgs of size - 1 .. 3 * size + 1 bases: flanks of no tile (NaN, -0, NaN) and of one (NaN stddev).  Every field
    bit for bit, -0 included, but a NaN is any NaN: which sign and payload an operation hands on is the processor's
    choice (0 / 0 is the negative quiet NaN on x86 and stays so through the twin's arithmetic; the device's division
    returns the positive one), and the reference prints `NaN` for all of them"""
    ctgs = sk.short_ctgs(params)
    feats = [sk.short_features(c) for c in ctgs]
    want = np.concatenate([twin_rows(c, *f, params) for c, f in zip(ctgs, feats)])
    assert np.isnan(want["gc_mean"]).any() and np.isnan(want["gc_stddev"]).any() and np.signbit(want["gc_stddev"]).any()
    ss = engine.SeqSet(eng, [seq_of(c) for c in ctgs])
    try:
        got, _ = gpu_rows(eng, ss, list(range(len(ctgs))), ctgs, feats, params)
        for r in (got, want):
            for f in sk.FIELDS:
                r[f][np.isnan(r[f])] = np.float32(np.nan)
        assert first_row_difference(got, want) is None, first_row_difference(got, want)
    finally:
        ss.close()


@pytest.mark.parametrize("params", SETS)
def test_text_equals_the_oracle(eng, params):
    """the device formatter over the same rows: values next to ties, and the NaN and -0 of the short ctgs"""
    c, fs, fe, _ = sk.battery(params)
    ctgs = [c] + sk.short_ctgs(params)
    feats = [(fs, fe)] + [sk.short_features(x) for x in ctgs[1:]]
    parts = [oracle_text(x, *f, params).encode() for x, f in zip(ctgs, feats)]
    want = b"".join(parts)
    assert b"\tNaN\t-0\tNaN\t\n" in want
    ss = engine.SeqSet(eng, [seq_of(x) for x in ctgs])
    try:
        got, off, n_rows = gpu_text(eng, ss, list(range(len(ctgs))), ctgs, feats, params)
        assert got == want, first_difference(got, want)
        assert n_rows == want.count(b"\n")
        assert off.tolist() == np.concatenate(([0], np.cumsum([len(p) for p in parts]))).tolist()
    finally:
        ss.close()


def test_keep_sets_agree_where_the_flank_is_the_same_tiles(eng):
    """flanks of 7, 8 (kept in registers) and 9 tiles (the ninth recomputed through range_gc) over one ctg: where the
    ctg clips the flank of a window to the same tiles under two resizes, the device gives the same row -- the value of
    a tile does not depend on the pass that computed it"""
    c, fs, fe = sk.keep_features()
    ss = engine.SeqSet(eng, [seq_of(c)])
    try:
        got = {p: gpu_rows(eng, ss, [0], [c], [(fs, fe)], p)[0] for p in sk.KEEP_SETS}
    finally:
        ss.close()
    compared = 0
    for a, b, same in sk.keep_pairs():
        assert same.size == got[a].size == got[b].size
        d = first_row_difference(got[a][same], got[b][same])
        assert d is None, (a, b, d)
        compared += int(same.sum())
    assert compared > 1000
    for p in sk.KEEP_SETS:
        want = twin_rows(c, fs, fe, p)
        assert first_row_difference(got[p], want) is None, (p, first_row_difference(got[p], want))


def test_range_gc_over_the_whole_grid(eng):
    """all 4,198,400 (G/C count, length) pairs in one gams_gpu_range_gc_batch call against the model, bit for bit; then
    the ties and the pairs a wrong formula changes once more on the same bases in a slot behind the first 64-KiB
    segment, at another chr_start"""
    g, c = sk.grid(), sk.grid_ctg()
    ss = engine.SeqSet(eng, [seq_of(c), np.full(FILLER, ord("C"), np.uint8), seq_of(c)])
    try:
        n = g["c"].size
        sel, cst, roff = np.zeros(1, np.uint32), np.ones(1, np.int32), np.array([0, n], np.uint64)
        rs, re = np.ascontiguousarray(g["start"]), np.ascontiguousarray(g["end"])
        gc = np.full(n, -1.0, np.float32)
        eng.check(eng.lib.gams_gpu_range_gc_batch(eng.h, ss.p, 1, sel.ctypes.data, cst.ctypes.data, roff.ctypes.data,
                                                  rs.ctypes.data, re.ctypes.data, gc.ctypes.data))
        bad = np.flatnonzero(gc.view(np.uint32) != g["gc"].view(np.uint32))
        first = [(int(g["c"][q]), int(g["len"][q]), "%08x" % gc[q:q + 1].view(np.uint32)[0], "%08x" % g["gc"][q:q + 1].view(np.uint32)[0])
                 for q in bad[:5]]
        print("range gc grid: %d mismatches of %d" % (bad.size, n), first)
        assert bad.size == 0, first
        idx = sk.grid_edges()
        sel, cst, roff = np.array([2], np.uint32), np.array([5001], np.int32), np.array([0, idx.size], np.uint64)
        rs, re = np.ascontiguousarray(g["start"][idx] + 5000), np.ascontiguousarray(g["end"][idx] + 5000)
        gc = np.full(idx.size, -1.0, np.float32)
        eng.check(eng.lib.gams_gpu_range_gc_batch(eng.h, ss.p, 1, sel.ctypes.data, cst.ctypes.data, roff.ctypes.data,
                                                  rs.ctypes.data, re.ctypes.data, gc.ctypes.data))
        bad = np.flatnonzero(gc.view(np.uint32) != g["gc"][idx].view(np.uint32))
        assert bad.size == 0, [(int(g["c"][idx[q]]), int(g["len"][idx[q]]), "%08x" % gc[q:q + 1].view(np.uint32)[0]) for q in bad[:5]]
    finally:
        ss.close()


def test_peak_text_over_the_ties_and_the_changed_pairs(eng):
    """range_gc_cols_kernel: the ties and the pairs a wrong formula changes as the lines of a wave TSV, against the
    model of tests/peak_text.py; chromosome II holds the same bases in a slot behind the first 64-KiB segment"""
    ctgs, data, idx = sk.grid_peak_case()
    want = pt.model(ctgs, data)
    assert want.count(b"\n") == 2 * idx.size
    ss = engine.SeqSet(eng, [seq_of(ctgs[0]), np.full(FILLER, ord("C"), np.uint8), seq_of(ctgs[1])])
    T = PeakTables(eng, ctgs, slots=[0, 2])
    try:
        rc, text, off, n_rows = abi_peak(eng, T, ss, data)
        assert rc == 0, eng.lib.gams_gpu_last_error(eng.h)
        got = peak_in_id_order(T, text, off)
        assert got == want, first_difference(got, want)
        assert n_rows == 2 * idx.size
    finally:
        T.close()
        ss.close()
