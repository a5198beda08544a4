"""The nearest-neighbour ΔG on the device, through the C ABI: gams_gpu_range_dg_batch, gams_gpu_sw_dg_batch,
gams_gpu_sw_text_dg and the host operators above them.  Every expected value is gams_dg_polymer_host -- the twin, held to
the model and to the reference's answers by test_dg_cpu.py -- on the same table over the bytes the test uploaded, and
every comparison is bit for bit (NaN as NaN)."""
import ctypes as C

import numpy as np
import pytest

import dg_model
import helpers
from gams_amd import _lib, engine, host

pytestmark = pytest.mark.gpu

CS = _lib.DG_STAGE_BASES
TABLE = dg_model.table(37.0, 1.0)


@pytest.fixture(scope="module")
def eng():
    e = engine.Engine(0)
    yield e
    e.close()


def twin(seq, table=TABLE):
    t = _lib.DgTable.from_buffer_copy(np.ascontiguousarray(table, np.float32).tobytes())
    a = np.frombuffer(bytes(seq), np.uint8)
    out = C.c_float()
    assert _lib.load().gams_dg_polymer_host(C.byref(t), a.ctypes.data if a.size else None, a.size, C.byref(out)) == _lib.OK
    return np.float32(out.value)


def assert_same_bits(got, exp, what=""):
    got, exp = np.asarray(got, np.float32), np.asarray(exp, np.float32)
    assert got.shape == exp.shape, what
    bad = np.flatnonzero(~((got.view(np.uint32) == exp.view(np.uint32)) | (np.isnan(got) & np.isnan(exp))))
    assert bad.size == 0, (what, bad[:8], got[bad[:8]], exp[bad[:8]])


# ---- one seqset: 5,000 + 300 + 140,000 bases ------------------------------------------------------------------------------
N_AT, AT_LEN, PAL_AT, PAL2_AT, N_ONE = 110001, 4000, 120000, 121000, 90000
N_HIGH = 95007                  # an invalid byte on the last base of its 16-B piece (95007 % 16 == 15)
CHR_START = (1, 10001, 500001)


def make_ctgs():
    rng = np.random.default_rng(42)
    ctgs = [bytearray(dg_model.random_seq(rng, n)) for n in (5000, 300, 140000)]
    c = ctgs[2]
    c[N_ONE] = ord("N")
    c[N_HIGH] = ord("N")
    for p in (100000, 100003, 130000):
        c[p] = ord("n")
    c[N_AT:N_AT + AT_LEN] = b"AT" * (AT_LEN // 2)
    comp = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")
    half = dg_model.random_seq(rng, 20)
    pal = half + half.translate(comp)[::-1]
    c[PAL_AT:PAL_AT + 40] = pal
    miss = bytearray(pal)
    miss[31] = ord("A") if pal[31] not in b"Aa" else ord("C")
    c[PAL2_AT:PAL2_AT + 40] = miss
    ctgs[0][4000] = ord("N")
    return [bytes(x) for x in ctgs]


@pytest.fixture(scope="module")
def case(eng):
    ctgs = make_ctgs()
    ss = engine.SeqSet(eng, ctgs)
    yield ctgs, ss
    ss.close()


def run(eng, ss, ctgs, sel, ranges, table=TABLE):
    """ranges[k] = [(0-based start, length)] inside selected ctg k -> (got, expected)"""
    cst = [CHR_START[i] for i in sel]
    off = np.concatenate([[0], np.cumsum([len(r) for r in ranges])]).astype(np.uint64)
    rs = [cs + s for cs, rl in zip(cst, ranges) for s, _ in rl]
    re_ = [cs + s + n - 1 for cs, rl in zip(cst, ranges) for s, n in rl]
    rc, got = engine.range_dg_batch(eng, ss, sel, cst, off, rs, re_, table)
    assert rc == _lib.OK, eng.lib.gams_gpu_last_error(eng.h)
    exp = np.array([twin(ctgs[i][s:s + n], table) for i, rl in zip(sel, ranges) for s, n in rl], np.float32)
    return got, exp


LENGTHS = [1, 2, 3, 4, 15, 16, 17, 31, 32, 33, 63, 64, 65, 99, 100, 101, CS - 1, CS, CS + 1, 2 * CS, 2 * CS + 1, 65535]


def edge_ranges():
    """the crossed list on ctg 2 and the planted cases (docstring of the test)"""
    r = [(2048 + o, n) for o in range(16) for n in LENGTHS]                  # every start offset x every length
    r += [(0, 50), (0, 3), (140000 - 50, 50), (140000 - 3, 3), (140000 - 65535, 65535)]   # first and last base
    r += [(40000, 65535)]                                                    # a long one over the planted n's
    # one N: at index 0, at len - 1, at C - 1, at C, at 16-B piece edges; and just outside a range
    r += [(N_ONE, 40), (N_ONE - 39, 40), (N_ONE - (CS - 1), CS + 5), (N_ONE - CS, CS + 5), (N_ONE - 2 * CS, 2 * CS + 1)]
    r += [(N_ONE - d, 40) for d in (15, 16, 17, 31, 32)] + [(N_ONE + 1, 40), (N_ONE - 40, 40), (N_ONE - 16, 16), (N_ONE - 15, 15)]
    # one N on the last base of a piece: just behind a range's tail, just in front of its head, first, last and inside;
    # and on the last base a stage holds (the piece of the range's first base + C - 1) of ranges that go on, end there,
    # or end one base in front
    base = N_HIGH - 15 - (CS - 16)                                           # the piece that begins stage 0 of such a range
    r += [(N_HIGH - 40, 40), (N_HIGH - 15, 15), (N_HIGH - 1, 1), (N_HIGH + 1, 40), (N_HIGH, 1), (N_HIGH, 40), (N_HIGH - 39, 40),
          (N_HIGH - 15, 16), (N_HIGH - 20, 40)]
    r += [(base + h, n) for h in (0, 4, 15) for n in (N_HIGH - base - h + 89, N_HIGH - base - h + 1, N_HIGH - base - h)]
    # (AT)n, its own reverse complement from A and from T, over one and two stage seams; odd: (AT)n + A
    for start in (N_AT, N_AT + 1, N_AT + 14, N_AT + 15):
        r += [(start, 600), (start, 1200), (start, 3000), (start, 601), (start, 4), (start, 16)]
    r += [(N_AT + AT_LEN - 600, 600), (N_AT + AT_LEN - 599, 600), (N_AT - 1, 600)]   # the last: one base in front breaks it
    r += [(PAL_AT, 40), (PAL2_AT, 40), (PAL_AT + 1, 38), (PAL_AT, 39)]
    return r


def test_range_dg_edges(eng, case):
    """every start offset modulo 16 x every length around the piece and stage sizes up to 65,535; ranges on a ctg's
    first and last base; an invalid byte at index 0, len - 1, C - 1, C and at piece edges; (AT)n from A and from T over
    stage seams and (AT)n + A; the palindrome whole and with one base changed; then one group of 64 holding a
    65,535-base range and 63 ranges of 3 bases"""
    ctgs, ss = case
    r0 = [(0, 100), (4900, 100), (3990, 11), (3990, 10), (4001, 99), (0, 5000)]
    r1 = [(0, 300), (0, 3), (297, 3), (1, 298)]
    r2 = edge_ranges()
    r2 += [(5000 + i, 3) for i in range(-(len(r0) + len(r1) + len(r2)) % 64)]   # the planted group is one wave of the launch:
    assert (len(r0) + len(r1) + len(r2)) % 64 == 0                            # it starts on a multiple of 64 of the whole list
    r2 += [(3000 + 5 * i, 3) for i in range(20)] + [(1000, 65535)] + [(3000 + 5 * i, 3) for i in range(20, 63)]
    got, exp = run(eng, ss, ctgs, [0, 1, 2], [r0, r1, r2])
    assert_same_bits(got, exp)
    assert np.isnan(exp).sum() > 20 and (~np.isnan(exp)).sum() > 300
    # the symmetry term is in where it belongs
    t = TABLE
    at = dict(zip(r2, exp[len(r0) + len(r1):]))
    assert at[(PAL_AT, 40)] != at[(PAL2_AT, 40)]
    assert at[(N_AT, 600)] == dg_model.polymer(t, b"AT" * 300) and at[(N_AT + 1, 600)] == dg_model.polymer(t, b"TA" * 300)


def test_range_dg_ctg_selected_twice(eng, case):
    ctgs, ss = case
    rng = np.random.default_rng(3)
    a = [(int(s), int(n)) for s, n in zip(rng.integers(0, 139000, 70), rng.integers(1, 700, 70))]
    b = [(int(s), int(n)) for s, n in zip(rng.integers(0, 139000, 70), rng.integers(1, 700, 70))]
    got, exp = run(eng, ss, ctgs, [2, 2], [a, b])
    assert_same_bits(got, exp)
    got, exp = run(eng, ss, ctgs, [2, 0, 2], [b, [(0, 100)], []])
    assert_same_bits(got, exp)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 4097])
def test_range_dg_list_sizes(eng, case, n):
    ctgs, ss = case
    rng = np.random.default_rng(n)
    lens = [5000, 300, 140000]
    ranges = [[], [], []]
    for _ in range(n):
        k = int(rng.integers(0, 3))
        ln = int(rng.integers(1, 131))
        ranges[k].append((int(rng.integers(0, lens[k] - ln + 1)), ln))
    got, exp = run(eng, ss, ctgs, [0, 1, 2], ranges)
    assert got.size == n
    assert_same_bits(got, exp)


def test_range_dg_other_tables(eng, case):
    """the answer is a function of (table, bytes): the (30, 0.1) terms, the register-resident table, a table of the caller"""
    ctgs, ss = case
    r = [(2048 + o, n) for o in (0, 7, 15) for n in (3, 100, CS + 1, 2 * CS + 1)] + [(N_AT, 600), (PAL_AT, 40), (N_ONE, 5)]
    for table in (dg_model.table(30.0, 0.1), np.arange(1, 22, dtype=np.float32) / np.float32(7)):
        got, exp = run(eng, ss, ctgs, [2], [r], table)
        assert_same_bits(got, exp)
    assert eng.lib.gams_gpu_dg_set_table(eng.h, _lib.DG_TABLE_BPERMUTE) == _lib.OK
    try:
        got, exp = run(eng, ss, ctgs, [0, 1, 2], [[(0, 100), (3990, 11)], [(0, 300)], edge_ranges()])
        assert_same_bits(got, exp)
    finally:
        assert eng.lib.gams_gpu_dg_set_table(eng.h, _lib.DG_TABLE_LDS) == _lib.OK
    assert eng.lib.gams_gpu_dg_set_table(eng.h, 2) == _lib.EINVAL


# ---- refusals, each followed by a good call on the same handle ----------------------------------------------------------
def test_range_dg_refusals(eng, case):
    ctgs, ss = case
    good = [[(10, 100)], [(0, 300)], [(N_AT, 600), (N_ONE, 3)]]

    def call(sel, cst, off, rs, re_, table, seqset=ss):
        rc, _ = engine.range_dg_batch(eng, seqset, sel, cst, off, rs, re_, table)
        return rc, eng.lib.gams_gpu_last_error(eng.h).decode()

    def still_good():
        got, exp = run(eng, ss, ctgs, [0, 1, 2], good)
        assert_same_bits(got, exp)

    rc, msg = call([2], [500001], [0, 1], [500001], [500100], None)
    assert rc == _lib.EINVAL and msg.startswith("gpu_range_dg")
    still_good()
    for bad in (np.nan, np.inf, -np.inf):
        for slot in (0, 15, 16, 19, 20):
            t = TABLE.copy()
            t[slot] = bad
            rc, msg = call([2], [500001], [0, 1], [500001], [500100], t)
            assert rc == _lib.EINVAL and "non-finite" in msg
    still_good()
    # a range outside its ctg: code and message as gpu_range_gc gives them, under the new entry's name
    for rs, re_ in ((500000, 500100), (500001, 640001), (500100, 500099)):
        rc, msg = call([2], [500001], [0, 1], [rs], [re_], TABLE)
        assert rc == _lib.EINVAL and msg == "gpu_range_dg: range 0 is not inside the ctg", msg
        gc = np.zeros(1, np.float32)
        a = [np.array(x, t) for x, t in (([2], np.uint32), ([500001], np.int32), ([0, 1], np.uint64), ([rs], np.int32), ([re_], np.int32))]
        assert eng.lib.gams_gpu_range_gc_batch(eng.h, ss.p, 1, *[x.ctypes.data for x in a], gc.ctypes.data) == _lib.EINVAL
        assert eng.lib.gams_gpu_last_error(eng.h).decode() == msg.replace("range_dg", "range_gc")
    rc, msg = call([0, 2], [1, 500001], [0, 1, 2], [1, 499999], [100, 500100], TABLE)
    assert rc == _lib.EINVAL and msg == "gpu_range_dg: range 0 of selected ctg 1 is not inside the ctg"
    rc, msg = call([3], [1], [0, 1], [1], [100], TABLE)
    assert rc == _lib.EINVAL and msg == "gpu_range_dg: ctg index out of range"
    still_good()
    rc, msg = call([2], [500001], [0, 1], [500001], [500001 + 65535], TABLE)       # 65,536 bases
    assert rc == _lib.EUNSUPPORTED and msg.startswith("gpu_range_dg: range 0")
    rc, _ = call([2], [500001], [0, 1], [500001], [500001 + 65534], TABLE)
    assert rc == _lib.OK
    still_good()
    # a plane-only seqset
    po = engine.SeqSet(eng, ctgs, upload=False)
    off, nb = po.layout()
    plane = np.zeros(nb // 8 + 1, np.uint8)
    po.upload_ranges(None, plane, 0, int(off[2]) + 140000)   # a plane without bytes
    rc, msg = call([2], [500001], [0, 1], [500001], [500100], TABLE, seqset=po)
    assert rc == _lib.ESTATE
    n = C.c_uint64()
    a = [np.array(x, t) for x, t in (([2], np.uint32), ([500001], np.int32), ([0, 1], np.uint64), ([500100], np.int32), ([500100], np.int32))]
    dg = np.zeros(64, np.float32)
    t = engine._dg_table(TABLE)
    assert eng.lib.gams_gpu_sw_dg_batch(eng.h, po.p, 1, *[x.ctypes.data for x in a], 100, 2, C.byref(t), dg.ctypes.data, 64,
                                        None, C.byref(n)) == _lib.ESTATE
    po.close()
    still_good()


# ---- the sw entries ----------------------------------------------------------------------------------------------------------
def sel_arrays(ctgs, feats, sel):
    cst = [ctgs[i]["chr_start"] for i in sel]
    foff = np.concatenate([[0], np.cumsum([len(feats[i]) for i in sel])])
    fs = [f[1] for i in sel for f in feats[i]]
    fe = [f[2] for i in sel for f in feats[i]]
    ids = [f[0] for i in sel for f in feats[i]]
    return cst, foff, fs, fe, ids


def sw_rows(eng, ss, sel, cst, foff, fs, fe, size, mx):
    n = C.c_uint64()
    a = [np.ascontiguousarray(x, t) for x, t in ((sel, np.uint32), (cst, np.int32), (foff, np.uint64), (fs, np.int32), (fe, np.int32))]
    roff = np.zeros(len(sel) + 1, np.uint64)
    args = (eng.h, ss.p, len(sel), *[x.ctypes.data for x in a], size, mx, 500)
    eng.check(eng.lib.gams_gpu_sw_batch(*args, None, 0, roff.ctypes.data, C.byref(n)))
    rows = np.zeros(max(n.value, 1), _lib.SW_ROW_DTYPE)
    eng.check(eng.lib.gams_gpu_sw_batch(*args, rows.ctypes.data, rows.size, roff.ctypes.data, C.byref(n)))
    return rows[:n.value], roff


@pytest.fixture(scope="module")
def sw_case(eng, s288c):
    rng = np.random.default_rng(8)
    ctgs = helpers.gen_ctgs("I", s288c["I"], piece=30000)[:4]
    syn = bytearray(dg_model.random_seq(rng, 9000))
    syn[4000] = ord("N")
    ctgs.append(dict(id="ctg:syn:1", chr_id="syn", chr_start=1001, chr_end=10000, seq=bytes(syn)))
    feats = []
    for k, c in enumerate(ctgs):
        n = 0 if k == 2 else 40
        a = rng.integers(c["chr_start"], c["chr_end"] + 1, n)
        b = np.minimum(a + rng.choice([0, 1, 50, 999], n), c["chr_end"])
        f = [(int(x), int(y)) for x, y in zip(a, b)]
        if k == 4:   # windows that clip at both ctg ends, and around the N
            f += [(1001, 1001), (1002, 1003), (1050, 1060), (10000, 10000), (9990, 10000), (9940, 9950), (5000, 5002), (1001, 10000)]
        feats.append([(f"feature:{c['id']}:{j + 1}", x, y) for j, (x, y) in enumerate(f)])
    ss = engine.SeqSet(eng, [c["seq"] for c in ctgs])
    yield ctgs, feats, ss
    ss.close()


def expected_sw_dg(eng, ss, ctgs, feats, sel, size, mx, table=TABLE):
    cst, foff, fs, fe, _ = sel_arrays(ctgs, feats, sel)
    rows, roff = sw_rows(eng, ss, sel, cst, foff, fs, fe, size, mx)
    exp = np.zeros(rows.size, np.float32)
    for k, i in enumerate(sel):
        c = ctgs[i]
        for r in range(int(roff[k]), int(roff[k + 1])):
            exp[r] = twin(c["seq"][rows["start"][r] - c["chr_start"]:rows["end"][r] - c["chr_start"] + 1], table)
    return exp, roff, rows


@pytest.mark.parametrize("size,mx", [(100, 20), (7, 2), (3, 1), (2, 1), (1500, 2)])
def test_sw_dg_batch(eng, sw_case, size, mx):
    """dg[r] is the twin over row r's (start, end) of gams_gpu_sw_batch; n_rows, row_off and the size query are that
    entry's.  At size 2 every L / R window is None; at size 1500 the M windows are longer than two stages."""
    ctgs, feats, ss = sw_case
    for sel in ([0, 1, 2, 3, 4], [4, 1, 1]):
        exp, roff, rows = expected_sw_dg(eng, ss, ctgs, feats, sel, size, mx)
        cst, foff, fs, fe, _ = sel_arrays(ctgs, feats, sel)
        got, got_off = engine.sw_dg_batch(eng, ss, sel, cst, foff, fs, fe, size, mx, TABLE)   # (size query inside)
        assert np.array_equal(got_off, roff) and got.size == rows.size
        assert_same_bits(got, exp, (size, mx, sel))
        lens = rows["end"] - rows["start"] + 1
        if size == 2:
            assert np.isnan(got[rows["type"] != 0]).all() and lens.max() <= 2
        if size == 1500:
            assert lens.max() > 2 * CS and (~np.isnan(got)).sum() > 10
        if size == 100:
            assert (~np.isnan(got)).mean() > 0.9 and np.isnan(got).any()
    # a cap below the rows: the first `cap` values
    cst, foff, fs, fe, _ = sel_arrays(ctgs, feats, [0, 4])
    exp, _, _ = expected_sw_dg(eng, ss, ctgs, feats, [0, 4], size, mx)
    a = [np.ascontiguousarray(x, t) for x, t in (([0, 4], np.uint32), (cst, np.int32), (foff, np.uint64), (fs, np.int32), (fe, np.int32))]
    n, t = C.c_uint64(), engine._dg_table(TABLE)
    part = np.full(70, 7.0, np.float32)
    eng.check(eng.lib.gams_gpu_sw_dg_batch(eng.h, ss.p, 2, *[x.ctypes.data for x in a], size, mx, C.byref(t), part.ctypes.data,
                                           65, None, C.byref(n)))
    assert n.value == exp.size
    assert_same_bits(part[:min(65, exp.size)], exp[:65])
    assert (part[65:] == 7.0).all()


def with_column(text, dg):
    rows = text.decode().split("\n")[:-1]
    assert len(rows) == len(dg)
    return "".join(r + "\t" + dg_model.fmt(v) + "\n" for r, v in zip(rows, dg)).encode()


def test_sw_text_dg(eng, sw_case):
    """byte for byte the text of gams_gpu_sw_text_actions with "\\t" + the "%.4f" of the row's ΔG (or nothing) in front of
    every "\\n", for the action sets gc, count, gc + count and none; the per-ctg offsets follow"""
    ctgs, feats, ss = sw_case
    rng = np.random.default_rng(2)
    rgs = [[(int(x), int(x) + int(rng.choice([0, 5, 300]))) for x in rng.integers(c["chr_start"], c["chr_end"], 300)] for c in ctgs]
    off = np.concatenate([[0], np.cumsum([len(g) for g in rgs])]).astype(np.uint64)
    ix = engine.Index(eng, off, np.array([s for g in rgs for s, _ in g], np.uint32), np.array([e + 1 for g in rgs for _, e in g], np.uint32))
    sel = [0, 1, 2, 3, 4]
    cst, foff, fs, fe, ids = sel_arrays(ctgs, feats, sel)
    names = [ctgs[i]["chr_id"] for i in sel]
    for size, mx in ((100, 20), (3, 1)):
        dg, roff = engine.sw_dg_batch(eng, ss, sel, cst, foff, fs, fe, size, mx, TABLE)
        for actions in (_lib.SW_GC, _lib.SW_COUNT, _lib.SW_GC | _lib.SW_COUNT, 0):
            rc, old, old_off = engine.sw_text_actions(eng, ss, sel, names, cst, foff, fs, fe, ids, size, mx, 500, actions, ix, sel)
            assert rc == _lib.OK
            rc, new, new_off = engine.sw_text_dg(eng, ss, sel, names, cst, foff, fs, fe, ids, size, mx, 500, actions, TABLE, ix, sel)
            assert rc == _lib.OK
            assert new == with_column(old, dg), (size, actions)
            for k in range(len(sel)):
                part = with_column(old[int(old_off[k]):int(old_off[k + 1])], dg[int(roff[k]):int(roff[k + 1])])
                assert new[int(new_off[k]):int(new_off[k + 1])] == part
    assert b"\t\n" in new and b"\t-" in new                  # None rows and values
    # unknown action bits and a NULL table stay GAMS_EINVAL
    for bad in (4, 8):
        assert engine.sw_text_dg(eng, ss, sel, names, cst, foff, fs, fe, ids, 100, 20, 500, bad, TABLE, ix, sel)[0] == _lib.EINVAL
    assert engine.sw_text_dg(eng, ss, sel, names, cst, foff, fs, fe, ids, 100, 20, 500, _lib.SW_GC, None)[0] == _lib.EINVAL
    # a caller's table scaled so that a row reaches 2^20: refused, and the handle's next call is right
    big = (TABLE * np.float32(2.0 ** 20 / 100.0)).astype(np.float32)
    vals, _ = engine.sw_dg_batch(eng, ss, sel, cst, foff, fs, fe, 100, 20, big)
    assert np.nanmax(np.abs(vals)) >= 2 ** 20
    assert engine.sw_text_dg(eng, ss, sel, names, cst, foff, fs, fe, ids, 100, 20, 500, _lib.SW_GC, big)[0] == _lib.EUNSUPPORTED
    rc, again, _ = engine.sw_text_dg(eng, ss, sel, names, cst, foff, fs, fe, ids, 3, 1, 500, 0, TABLE, ix, sel)
    assert rc == _lib.OK and again == new
    ix.close()


def test_sw_text_dg_long_names_leave_the_stage(eng, sw_case):
    """a ctg with a 100-byte name and 100-byte feature ids: a 512-row block is beyond the 49,152-B stage"""
    ctgs, feats, ss = sw_case
    c = ctgs[0]
    pts = np.linspace(c["chr_start"] + 3000, c["chr_end"] - 3000, 40).astype(int)
    fl = [("f" * 90 + f"{j:010d}", int(p), int(p)) for j, p in enumerate(pts)]
    name = "chr" + "x" * 97
    cst, foff, fs, fe, ids = [c["chr_start"]], [0, len(fl)], [f[1] for f in fl], [f[2] for f in fl], [f[0] for f in fl]
    dg, _ = engine.sw_dg_batch(eng, ss, [0], cst, foff, fs, fe, 100, 20, TABLE)
    assert dg.size > 1024
    rc, old, _ = engine.sw_text_actions(eng, ss, [0], [name], cst, foff, fs, fe, ids, 100, 20, 500, _lib.SW_GC)
    assert rc == _lib.OK and 512 * (len(old) / dg.size) > 2 * 49152       # a block of 512 rows is far beyond the stage
    rc, new, _ = engine.sw_text_dg(eng, ss, [0], [name], cst, foff, fs, fe, ids, 100, 20, 500, _lib.SW_GC, TABLE)
    assert rc == _lib.OK and new == with_column(old, dg)


# ---- one handle, nothing released -----------------------------------------------------------------------------------------
def test_call_sequence_on_one_handle(case, sw_case):
    """a 4,097-range call, a 3-range call, the sw text call, the 3-range call again: every answer as on a fresh handle"""
    ctgs, _ = case
    sctgs, feats, _ = sw_case
    e = engine.Engine(0)
    try:
        ss = engine.SeqSet(e, ctgs)
        s2 = engine.SeqSet(e, [c["seq"] for c in sctgs])
        rng = np.random.default_rng(77)
        many = [(int(s), int(n)) for s, n in zip(rng.integers(0, 138000, 4097), rng.integers(1, 1200, 4097))]
        three = [(N_AT, 600), (N_ONE - 5, 10), (2050, 2 * CS + 1)]
        got, exp = run(e, ss, ctgs, [2], [many])
        assert_same_bits(got, exp)
        got3, exp3 = run(e, ss, ctgs, [2], [three])
        assert_same_bits(got3, exp3)
        sel = [0, 1, 3, 4]
        cst, foff, fs, fe, ids = sel_arrays(sctgs, feats, sel)
        names = [sctgs[i]["chr_id"] for i in sel]
        rc, text, _ = engine.sw_text_dg(e, s2, sel, names, cst, foff, fs, fe, ids, 100, 20, 500, _lib.SW_GC, TABLE)
        assert rc == _lib.OK
        dg, _ = engine.sw_dg_batch(e, s2, sel, cst, foff, fs, fe, 100, 20, TABLE)
        exp_dg, _, _ = expected_sw_dg(e, s2, sctgs, feats, sel, 100, 20)
        assert_same_bits(dg, exp_dg)
        rc, old, _ = engine.sw_text_actions(e, s2, sel, names, cst, foff, fs, fe, ids, 100, 20, 500, _lib.SW_GC)
        assert rc == _lib.OK and text == with_column(old, exp_dg)
        again, _ = run(e, ss, ctgs, [2], [three])
        assert_same_bits(again, exp3)
        ss.close()
        s2.close()
    finally:
        e.close()


# ---- the operators -----------------------------------------------------------------------------------------------------------
def test_host_operators(eng, sw_case, case):
    ctgs, feats, ss = sw_case
    d = host.DeltaG()
    assert bytes(d.table) == TABLE.tobytes()
    rng = np.random.default_rng(4)
    recs = [(c["id"], f"{c['chr_id']}:{int(x)}-{int(x) + 3}") for c in ctgs for x in rng.integers(c["chr_start"], c["chr_end"] - 3, 200)]
    sel = list(range(len(ctgs)))
    cst, foff, fs, fe, _ = sel_arrays(ctgs, feats, sel)
    dg, roff = engine.sw_dg_batch(eng, ss, sel, cst, foff, fs, fe, 100, 20, TABLE)
    rg_file = "".join(r + "\n" for _, r in recs).encode()                # the bytes of an rg file over the same ranges
    for kw in (dict(actions=("gc",)), dict(actions=("gc", "count"), rg_data=rg_file), dict(actions=("count",), rg_data=rg_file)):
        old = host.sw_multi([eng], ctgs, feats, 100, 20, 500, **kw)
        exp = with_column(old.encode(), dg).decode()
        assert host.sw_gibbs(eng, ctgs, feats, 100, 20, 500, dg=d, **kw) == exp            # host sequences
        assert host.sw_gibbs(eng, ctgs, feats, 100, 20, 500, seqset=ss, **kw) == exp      # resident bases, default DeltaG
    counts = [int(r.split("\t")[8]) for r in exp.splitlines()]
    assert sum(c > 0 for c in counts) > 20                                # the rg file's ranges do land in windows
    # without an rg file every count is 0, as sw_multi without records
    assert host.sw_gibbs(eng, ctgs, feats, 100, 20, 500, actions=("count",), seqset=ss) == with_column(
        host.sw_multi([eng], ctgs, feats, 100, 20, 500, actions=("count",)).encode(), dg).decode()
    # a table scaled so that rows reach 2^20: the device text refuses, the operator formats the rows on the host
    big = host.DeltaG()
    big.table = engine._dg_table((TABLE * np.float32(2.0 ** 20 / 100.0)).astype(np.float32))
    vals, _ = engine.sw_dg_batch(eng, ss, sel, cst, foff, fs, fe, 100, 20, big.table)
    assert np.nanmax(np.abs(vals)) >= 2 ** 20 and np.isnan(vals).any()
    for kw in (dict(actions=("gc",)), dict(actions=("gc", "count"), rg_data=rg_file)):
        exp = with_column(host.sw_multi([eng], ctgs, feats, 100, 20, 500, **kw).encode(), vals).decode()
        assert host.sw_gibbs(eng, ctgs, feats, 100, 20, 500, dg=big, **kw) == exp
        assert host.sw_gibbs(eng, ctgs, feats, 100, 20, 500, dg=big, seqset=ss, **kw) == exp
    with pytest.raises(ValueError):
        host.sw_gibbs(eng, ctgs, feats, rg_data=[rg_file, rg_file])
    # actions=("gibbs",) of the old operators still prints nothing in its place
    assert all(r.endswith("\t") for r in host.sw_multi([eng], ctgs, feats, actions=("gibbs",)).splitlines())
    # range_dg against DeltaG.polymer per range
    bctgs, bss = case
    ranges = [[(1, 100), (4001, 4001), (3990, 4001)], [(10001, 10300)], [(500001 + N_AT, 500001 + N_AT + 599), (500001 + PAL_AT, 500001 + PAL_AT + 39)]]
    got = host.range_dg(eng, bss, [0, 1, 2], list(CHR_START), ranges, d)
    k = 0
    for i, rl in enumerate(ranges):
        for s, e in rl:
            want = d.polymer(bctgs[i][s - CHR_START[i]:e - CHR_START[i] + 1])
            assert (want is None and np.isnan(got[k])) or np.float32(want) == got[k]
            k += 1
    assert k == got.size == 6 and np.isnan(got).sum() == 2
