"""What the query entries do with their pooled scratch on every exit: after a call that fails halfway and after one that
succeeds, every block the call took is back in the handle's pools -- once.  gams_gpu_release_cached empties the pools
and reports the bytes they held, so a leaked block shows as fewer bytes than expected, a block returned twice as more
(or as a crash), and a request of another size as another count of 2-MiB pool granules.

Each scenario: empty the pools; the call; its return code; the held bytes; the same call and the same held bytes again
(nothing grows); a succeeding call of the same entry against the reference twin (oracle/gams_ref.h), the host operator
or the model its own tests compare it with; the held bytes after that one.

The HELD literals were recorded by running this file against the build of the commit BEFORE the entries' scratch moved
to PoolBlock / Carver / GAMS_TRY (each exit releasing by hand), never from the code under test."""
import ctypes as C

import numpy as np
import pytest

from gams_amd import _lib, engine, host
from oracle import oracle as ora
from test_gpu_rg_text import abi_read_range, model_arrays, same
from test_gpu_text_ops import AnnoTables, LocTables, abi_anno, abi_locate, first_fields, rust_lines

pytestmark = pytest.mark.gpu

L = _lib.load()
R = ora.ref()
MIB = 1 << 20
SIZE, MAX, RESIZE = 100, 2, 100
CTG = dict(id="ctg:I:1", chr_id="I", chr_start=1, chr_end=1000, seq=b"")
RUNLISTS = {"I": "1-100,300-400,950-1000"}
BAD_BYTE = b"I:100-200\nI:3\xff0-400\n"
RG_OK = b"I:100-200\nI:300-400\nI:5-9\nII:1-5\nI:990-1000\n"

# held bytes (after the failing call, after the succeeding call), from the parent commit's build
HELD = {
    "sw_batch": (2 * MIB, 4 * MIB),
    "range_gc_batch": (2 * MIB, 4 * MIB),
    "sw_text": (8 * MIB, 8 * MIB),
    "anno_text": (4 * MIB, 6 * MIB),
    "locate_text": (2 * MIB, 6 * MIB),
    "read_range_text": (2 * MIB, 10 * MIB),
    "count": (None, 2 * MIB),
    "valid_spans": (None, 4 * MIB),
}


@pytest.fixture(scope="module")
def eng():
    e = engine.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def seq():
    a = np.frombuffer(b"ACGT", np.uint8)[np.random.default_rng(11).integers(0, 4, 1000)].copy()
    a[400:420] = ord("N")
    return a


def held(eng):
    v = C.c_uint64()
    eng.check(L.gams_gpu_release_cached(eng.h, C.byref(v)))
    return v.value


def run_scenario(eng, name, fail, code, ok):
    """`fail` -> the return code of the failing call (None: the entry has no failing scenario); `ok` runs the succeeding
    call and checks its result"""
    held(eng)
    got = [None, None, None]
    if fail is not None:
        for k in range(2):
            rc = fail()
            assert rc == code, (name, rc, L.gams_gpu_last_error(eng.h))
            got[k] = held(eng)
    ok()
    got[2] = held(eng)
    print(f"HELD {name}: after the failing call {got[0]} and {got[1]}, after the succeeding call {got[2]}")
    want_fail, want_ok = HELD[name]
    assert got[0] == got[1] == want_fail, (name, got)
    assert got[2] == want_ok, (name, got)


def sw_arrays(feats, chr_start):
    fs = np.array([f[0] for f in feats], np.int32)
    fe = np.array([f[1] for f in feats], np.int32)
    return np.zeros(1, np.uint32), np.array([chr_start], np.int32), np.array([0, fs.size], np.uint64), fs, fe


def test_sw_batch(eng, seq):
    """(a) the second feature has its middle outside the ctg: EINVAL after the pinned staging was taken"""
    ss = engine.SeqSet(eng, [seq])
    rows = np.zeros(64, _lib.SW_ROW_DTYPE)
    n = C.c_uint64()

    def call(feats):
        sel, cst, foff, fs, fe = sw_arrays(feats, 1)
        return L.gams_gpu_sw_batch(eng.h, ss.p, 1, sel.ctypes.data, cst.ctypes.data, foff.ctypes.data, fs.ctypes.data,
                                   fe.ctypes.data, SIZE, MAX, RESIZE, rows.ctypes.data, rows.size, None, C.byref(n))

    def ok():
        feats = [(100, 200), (800, 900)]
        assert call(feats) == 0
        _, _, _, fs, fe = sw_arrays(feats, 1)
        exp = np.zeros(64, _lib.SW_ROW_DTYPE)
        m = C.c_uint64()
        assert R.gams_ref_sw(seq.ctypes.data, seq.size, 1, fs.ctypes.data, fe.ctypes.data, fs.size, SIZE, MAX, RESIZE,
                             exp.ctypes.data, exp.size, C.byref(m)) == 0
        assert n.value == m.value > 2 and rows[:n.value].tobytes() == exp[:m.value].tobytes()

    try:
        run_scenario(eng, "sw_batch", lambda: call([(100, 200), (990, 1200)]), _lib.EINVAL, ok)
    finally:
        ss.close()


def test_range_gc_batch(eng, seq):
    """(b) a range that leaves the ctg: EINVAL after the pinned staging was taken"""
    ss = engine.SeqSet(eng, [seq])
    gc = np.zeros(4, np.float32)

    def call(ranges):
        sel, cst, roff, rs, re_ = sw_arrays(ranges, 1)
        return L.gams_gpu_range_gc_batch(eng.h, ss.p, 1, sel.ctypes.data, cst.ctypes.data, roff.ctypes.data, rs.ctypes.data,
                                         re_.ctypes.data, gc.ctypes.data)

    def ok():
        ranges = [(100, 200), (900, 1000), (7, 7)]
        assert call(ranges) == 0
        _, _, _, rs, re_ = sw_arrays(ranges, 1)
        exp = np.zeros(4, np.float32)
        assert R.gams_ref_range_gc(seq.ctypes.data, seq.size, 1, rs.ctypes.data, re_.ctypes.data, rs.size, exp.ctypes.data) == 0
        assert gc[:3].tobytes() == exp[:3].tobytes()

    try:
        run_scenario(eng, "range_gc_batch", lambda: call([(900, 1100)]), _lib.EINVAL, ok)
    finally:
        ss.close()


def test_sw_text(eng, seq):
    """(c) rows with a negative coordinate: EUNSUPPORTED once the text kernels have run, with both staging blocks and
    both text blocks taken"""
    ss = engine.SeqSet(eng, [seq])
    chr_arr = (C.c_char_p * 1)(b"I")

    def call(feats, chr_start):
        sel, cst, foff, fs, fe = sw_arrays(feats, chr_start)
        ids = (C.c_char_p * fs.size)(*[f"feature:ctg:I:1:{j + 1}".encode() for j in range(fs.size)])
        txt, tb, toff, nr = C.c_void_p(), C.c_uint64(), C.c_void_p(), C.c_uint64()
        rc = L.gams_gpu_sw_text(eng.h, ss.p, 1, sel.ctypes.data, chr_arr, cst.ctypes.data, foff.ctypes.data, fs.ctypes.data,
                                fe.ctypes.data, ids, SIZE, MAX, RESIZE, C.byref(txt), C.byref(tb), C.byref(toff), C.byref(nr))
        return rc, (C.string_at(txt.value, tb.value) if rc == 0 and tb.value else b""), ids, fs, fe

    def ok():
        rc, text, ids, fs, fe = call([(100, 200), (800, 900)], 1)
        assert rc == 0
        rt, rb = C.c_void_p(), C.c_uint64()
        assert R.gams_ref_sw_text(b"I", seq.ctypes.data, seq.size, 1, fs.ctypes.data, fe.ctypes.data, ids, fs.size, SIZE, MAX,
                                  RESIZE, C.byref(rt), C.byref(rb)) == 0
        exp = C.string_at(rt.value, rb.value)
        R.gams_ref_free(rt)
        assert text == exp and text.count(b"\n") > 2

    try:
        run_scenario(eng, "sw_text", lambda: call([(-400, -300)], -500)[0], _lib.EUNSUPPORTED, ok)
    finally:
        ss.close()


def test_anno_text(eng):
    """(d) a field index beyond the line's fields: EINVAL once the parse has run, with both scratch blocks taken"""
    data = b"ctg:I:1\tI:50-350\nctg:I:1\tI:900-1000\n"
    exp = host.anno(eng, [CTG], RUNLISTS, [ln.decode() for ln in rust_lines(data)], idx_id=1, idx_range=2).encode()
    T = AnnoTables(eng, [CTG], RUNLISTS)

    def ok():
        rc, text, rows = abi_anno(eng, T, data)
        assert rc == 0 and rows == 2 and text == exp

    try:
        run_scenario(eng, "anno_text", lambda: abi_anno(eng, T, data, idx_range=5)[0], _lib.EINVAL, ok)
    finally:
        T.close()


def test_locate_text(eng):
    """(e) a byte >= 0x80 in the input: EUNSUPPORTED inside the front both text paths share"""
    data = b"I:100-200\nI:2000-2100\nI:999\n"
    exp = host.locate(eng, [CTG], first_fields(data)).encode()
    T = LocTables(eng, [CTG])

    def ok():
        rc, text, rows = abi_locate(eng, T, data)
        assert rc == 0 and rows == 2 and text == exp

    try:
        run_scenario(eng, "locate_text", lambda: abi_locate(eng, T, BAD_BYTE)[0], _lib.EUNSUPPORTED, ok)
    finally:
        T.close()


def test_read_range_text(eng):
    """(f) the rg loader on the same input: EUNSUPPORTED; the succeeding call takes its page-locked block too"""
    T = LocTables(eng, [CTG])

    def ok():
        rc, got = abi_read_range(eng, T, RG_OK, 1)
        want = model_arrays([CTG], RG_OK)
        assert rc == 0 and want["start"].size == 3 and same(got, want), (got, want)

    try:
        run_scenario(eng, "read_range_text", lambda: abi_read_range(eng, T, BAD_BYTE, 1)[0], _lib.EUNSUPPORTED, ok)
    finally:
        T.close()


def test_count(eng):
    """(g) gams_gpu_count on an index of two groups"""
    off = np.array([0, 3, 5], np.uint64)
    st, sp = np.array([10, 50, 50, 5, 900], np.uint32), np.array([20, 60, 300, 6, 1001], np.uint32)
    g, qs, qe = np.array([0, 0, 1, 1, 2], np.uint32), np.array([1, 55, 1, 950, 1], np.uint32), np.array([1000, 55, 4, 950, 9], np.uint32)
    ix = C.c_void_p()
    eng.check(L.gams_index_create(eng.h, 2, off.ctypes.data, st.ctypes.data, sp.ctypes.data, C.byref(ix)))

    def ok():
        got, exp = np.full(5, -7, np.int32), np.full(5, -8, np.int32)
        assert L.gams_gpu_count(eng.h, ix, g.ctypes.data, qs.ctypes.data, qe.ctypes.data, 5, got.ctypes.data) == 0
        assert R.gams_ref_count(2, off.ctypes.data, st.ctypes.data, sp.ctypes.data, g.ctypes.data, qs.ctypes.data,
                                qe.ctypes.data, 5, exp.ctypes.data) == 0
        assert np.array_equal(got, exp) and got[0] > 0

    try:
        run_scenario(eng, "count", None, None, ok)
    finally:
        L.gams_index_destroy(eng.h, ix)


def test_valid_spans(eng, seq):
    """(g) gams_gpu_valid_spans on the ctg's bases (one run of N inside)"""

    def ok():
        lo_a, hi_a, lo_b, hi_b = (np.zeros(8, np.int32) for _ in range(4))
        na, nb = C.c_uint64(), C.c_uint64()
        assert L.gams_gpu_valid_spans(eng.h, seq.ctypes.data, seq.size, 10, 50, lo_a.ctypes.data, hi_a.ctypes.data, 8, C.byref(na)) == 0
        assert R.gams_ref_valid_spans(seq.ctypes.data, seq.size, 10, 50, lo_b.ctypes.data, hi_b.ctypes.data, 8, C.byref(nb)) == 0
        assert na.value == nb.value == 2 and np.array_equal(lo_a, lo_b) and np.array_equal(hi_a, hi_b)

    run_scenario(eng, "valid_spans", None, None, ok)
