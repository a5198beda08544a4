"""The branches of the two scan kernels that ordinary sequence never takes, against the CPU twins and the oracle:
gen_scan_kernel / gams_gpu_valid_spans (gen.hip) on sequences of at most a 16-B chunk, on full last chunks that end
valid, on every byte value at every position of a chunk and with more boundaries than the flip list holds (the grow-
and-rescan); the gc index of sw.hip (gc_index_build, gc_before) on all-G/C ctgs longer than a 64-KiB segment, whose
segment-local prefixes use all 16 bits of their field."""
import ctypes as C

import numpy as np
import pytest

from helpers import synth
from gams_amd import _lib, engine
from oracle import oracle as ora

pytestmark = pytest.mark.gpu

R = ora.ref()


@pytest.fixture(scope="module")
def eng():
    e = engine.Engine(0)
    yield e
    e.close()


def gpu_spans(eng, seq, fill, min_len, cap):
    lo, hi = np.full(cap + 1, -7, np.int32), np.full(cap + 1, -7, np.int32)     # entry `cap` is a sentinel
    n = C.c_uint64()
    eng.check(eng.lib.gams_gpu_valid_spans(eng.h, seq.ctypes.data, seq.size, fill, min_len, lo.ctypes.data, hi.ctypes.data,
                                           cap, C.byref(n)))
    assert lo[cap] == -7 and hi[cap] == -7
    return n.value, lo[:cap], hi[:cap]


def ref_spans(seq, fill, min_len, cap):
    lo, hi = np.full(cap + 1, -7, np.int32), np.full(cap + 1, -7, np.int32)
    n = C.c_uint64()
    assert R.gams_ref_valid_spans(seq.ctypes.data, seq.size, fill, min_len, lo.ctypes.data, hi.ctypes.data, cap, C.byref(n)) == 0
    return n.value, lo[:cap], hi[:cap]


def numpy_runs(seq):
    """maximal runs of ACGTacgt, 1-based inclusive (what fill 1 / min 1 leaves untouched)"""
    ok = np.isin(seq, np.frombuffer(b"ACGTacgt", np.uint8))
    d = np.diff(np.concatenate(([0], ok.view(np.int8), [0])))
    return np.flatnonzero(d == 1) + 1, np.flatnonzero(d == -1)


def pattern(name, n):
    if name == "A":
        return np.full(n, ord("A"), np.uint8)
    if name == "N":
        return np.full(n, ord("N"), np.uint8)
    if name in ("AN", "NA"):
        return np.resize(np.frombuffer(name.encode(), np.uint8), n).copy()
    s = np.full(n, ord("A"), np.uint8)               # "ends": valid except the first and the last base
    s[0] = s[-1] = ord("N")
    return s


@pytest.mark.parametrize("name", ["A", "N", "AN", "NA", "ends"])
def test_valid_spans_of_short_and_chunk_aligned_sequences(eng, name):
    """Lengths within one 16-B chunk (a single partial chunk), on both sides of one and two chunks and of a workgroup's
    4096 bases; the lengths that are multiples of 16 and end valid take the close-the-open-run branch of a full last
    chunk.  n_spans, lo, hi against the CPU twin for three (fill, min) pairs; with fill 1 / min 1 also against numpy."""
    for n in (1, 2, 15, 16, 17, 31, 32, 33, 4095, 4096, 4097):
        seq = pattern(name, n)
        for fill, mn in ((1, 1), (2, 1), (50, 1)):
            cap = n + 1
            na, lo_a, hi_a = gpu_spans(eng, seq, fill, mn, cap)
            nb, lo_b, hi_b = ref_spans(seq, fill, mn, cap)
            assert na == nb, (name, n, fill, na, nb)
            assert np.array_equal(lo_a[:na], lo_b[:nb]) and np.array_equal(hi_a[:na], hi_b[:nb]), (name, n, fill)
            if fill == 1:
                lo_n, hi_n = numpy_runs(seq)
                assert na == lo_n.size and np.array_equal(lo_a[:na], lo_n) and np.array_equal(hi_a[:na], hi_n), (name, n)
        if name in ("A", "NA") and n % 16 == 0:
            assert seq[-1] == ord("A")               # (the branch this length is here for: a full last chunk, open run)


def test_valid_spans_every_byte_value_at_every_chunk_position(eng):
    """Byte b (0..255) at offset 16 + j (j = 0..15) of a 48-byte block of A, all 4096 blocks in one sequence: only
    ACGTacgt may be valid -- the bytes that differ from a valid one in bit 5 or bit 7 alone included (the SWAR test
    clears the case bit; the look-back at the previous chunk's last base is a separate scalar test, j = 15)."""
    blocks = np.full((256, 16, 48), ord("A"), np.uint8)
    for j in range(16):
        blocks[:, j, 16 + j] = np.arange(256, dtype=np.uint8)
    seq = np.ascontiguousarray(blocks.reshape(-1))
    assert seq.size == 196_608
    valid = set(b"ACGTacgt")
    lo_n, hi_n = numpy_runs(seq)
    assert lo_n.size == 1 + 16 * (256 - len(valid))                    # every other byte cuts the run of A once
    na, lo_a, hi_a = gpu_spans(eng, seq, 1, 1, lo_n.size + 8)
    nb, lo_b, hi_b = ref_spans(seq, 1, 1, lo_n.size + 8)
    assert na == nb == lo_n.size
    assert np.array_equal(lo_a[:na], lo_n) and np.array_equal(hi_a[:na], hi_n)
    assert np.array_equal(lo_b[:nb], lo_n) and np.array_equal(hi_b[:nb], hi_n)


@pytest.mark.parametrize("n", [65_536, 65_538, 140_000])
def test_valid_spans_flip_list_exactly_full_and_regrown(eng, n):
    """`AN` repeated: a run boundary at every base, n flips.  65,536 fill the list of 2^16 entries exactly (no rescan),
    65,538 and 140,000 take the grow-and-rescan.  fill 1: a span per A; fill 2: the single span 1 .. n - 1."""
    seq = pattern("AN", n)
    na, lo_a, hi_a = gpu_spans(eng, seq, 1, 1, n // 2 + 4)
    nb, lo_b, hi_b = ref_spans(seq, 1, 1, n // 2 + 4)
    assert na == nb == n // 2
    each = np.arange(1, n, 2, dtype=np.int32)
    assert np.array_equal(lo_a[:na], each) and np.array_equal(hi_a[:na], each)
    assert np.array_equal(lo_b[:nb], each) and np.array_equal(hi_b[:nb], each)
    na, lo_a, hi_a = gpu_spans(eng, seq, 2, 1, 4)
    assert na == 1 and lo_a[0] == 1 and hi_a[0] == n - 1
    assert ref_spans(seq, 2, 1, 4)[0] == 1
    if n == 140_000:
        # fewer output entries than spans: the full count, the first `cap` spans, nothing behind them (the sentinel)
        na, lo_a, hi_a = gpu_spans(eng, seq, 1, 1, 10)
        assert na == n // 2
        assert np.array_equal(lo_a, each[:10]) and np.array_equal(hi_a, each[:10])


# ---- the gc index with saturated segment-local prefixes -----------------------------------------------------------
SEG = 65_536
DELTAS = (-17, -16, -15, -1, 0, 1, 15, 16, 17)


@pytest.fixture(scope="module")
def gc_ctgs():
    return [np.full(200_000, ord("G"), np.uint8), np.full(65_552, ord("c"), np.uint8), synth(70_000, 5)]


def edge_points(n, buf_off):
    """1-based coordinates around the multiples of 64 KiB of the ctg, and around the segment boundaries of the seqset
    buffer if the ctg begins at byte `buf_off` of it (ctgs are 256-B aligned)"""
    pts = {SEG * k + d for k in (1, 2, 3) for d in DELTAS}
    pts |= {SEG * m - buf_off + d for m in range(1, 8) for d in DELTAS}
    return sorted(p for p in pts if 1 <= p <= n)


def test_range_gc_across_segments_of_an_all_gc_ctg(eng, gc_ctgs):
    """gams_gpu_range_gc_batch against the oracle, bit for bit: the whole ctg, single bases, and every range between two
    coordinates around a 64-KiB boundary.  On the all-G and all-c ctgs a segment's local prefix runs up to 65,520 (bit 15
    of the 16-bit field set from the middle of the segment on) and every answer is exactly 1."""
    ss = engine.SeqSet(eng, gc_ctgs)
    rs_all, re_all, exp, roff = [], [], [], [0]
    buf_off = 0
    for c, seq in enumerate(gc_ctgs):
        n = seq.size
        pts = edge_points(n, buf_off)
        buf_off += (n + 255) // 256 * 256
        pairs = [(1, n)] + [(p, p) for p in pts] + [(1, 1), (n, n)] + [(s, e) for s in pts for e in pts if s < e]
        rs_all += [s for s, _ in pairs]
        re_all += [e for _, e in pairs]
        exp += [ora.range_gc_content(seq, 1, s, e) for s, e in pairs]
        roff.append(len(rs_all))
    rs, re_ = np.array(rs_all, np.int32), np.array(re_all, np.int32)
    sel, cst = np.arange(3, dtype=np.uint32), np.ones(3, np.int32)
    roff = np.array(roff, np.uint64)
    gc = np.full(rs.size, -1.0, np.float32)
    eng.check(eng.lib.gams_gpu_range_gc_batch(eng.h, ss.p, 3, sel.ctypes.data, cst.ctypes.data, roff.ctypes.data, rs.ctypes.data,
                                              re_.ctypes.data, gc.ctypes.data))
    exp = np.array(exp, np.float32)
    bad = np.flatnonzero(gc.view(np.uint32) != exp.view(np.uint32))
    assert bad.size == 0, [(int(rs[q]), int(re_[q]), float(gc[q]), float(exp[q])) for q in bad[:5]]
    assert (gc[:int(roff[2])] == 1.0).all()
    assert rs.size > 600 and int(roff[1]) > 350
    ss.close()


def test_sw_rows_across_segments_of_an_all_gc_ctg(eng, gc_ctgs):
    """gams_gpu_sw against its CPU twin, every field (floats bit for bit), for features at the same coordinates: the
    windows and the resized flanks of a feature straddle the boundaries where the local prefix wraps to the next segment."""
    ss = engine.SeqSet(eng, gc_ctgs)
    buf_off = 0
    for c, seq in enumerate(gc_ctgs):
        n = seq.size
        pts = edge_points(n, buf_off)
        buf_off += (n + 255) // 256 * 256
        feats = sorted({(p, min(p + w, n)) for p in pts for w in (0, 1, 30, 99)})
        fs, fe = np.array([f[0] for f in feats], np.int32), np.array([f[1] for f in feats], np.int32)
        cap = fs.size * 41
        a_rows, b_rows = np.zeros(cap, _lib.SW_ROW_DTYPE), np.zeros(cap, _lib.SW_ROW_DTYPE)
        na, nb = C.c_uint64(), C.c_uint64()
        eng.check(eng.lib.gams_gpu_sw(eng.h, ss.p, c, 1, fs.ctypes.data, fe.ctypes.data, fs.size, 100, 20, 500,
                                      a_rows.ctypes.data, cap, C.byref(na)))
        assert R.gams_ref_sw(seq.ctypes.data, seq.size, 1, fs.ctypes.data, fe.ctypes.data, fs.size, 100, 20, 500,
                             b_rows.ctypes.data, cap, C.byref(nb)) == 0
        assert na.value == nb.value > 20 * fs.size
        a, b = a_rows[:na.value], b_rows[:nb.value]
        if a.tobytes() != b.tobytes():
            q = next(i for i in range(a.size) if a[i:i + 1].tobytes() != b[i:i + 1].tobytes())
            raise AssertionError((c, q, a[q], b[q]))
        if c < 2:
            assert (a["gc_content"] == 1.0).all()
    ss.close()
