"""The rg loader on the device: gams_gpu_read_range_text / gams_index_create_range_text through the C ABI and the host
operators above them (Locator::set_rg_index_text, gams::read_range_text, the rg_data= forms of locate / sw), against
the pinned host path (host.read_range, rg_records=) and the pure-Python model of tests/test_rg_text_cpu.py."""
import ctypes as C

import numpy as np
import pytest

import helpers
from gams_amd import _lib, engine, host
from test_gpu_sw_count import bucket_features, features_of
from test_gpu_text_ops import LocTables, _ok, abi_locate, all_ctgs, read_bytes
from test_rg_text_cpu import locator_order, model, parse_line, rust_lines

pytestmark = pytest.mark.gpu

L = _lib.load()
NONE = 0xffffffff


@pytest.fixture(scope="module")
def eng():
    e = engine.Engine(0)
    yield e
    e.close()


def ctg(chr_id, serial, start, end):
    return dict(id=f"ctg:{chr_id}:{serial}", chr_id=chr_id, chr_start=start, chr_end=end, seq=b"")


# three ctgs of one chromosome and one of another; the gap 2001..2999 belongs to no ctg
SMALL = [ctg("I", 1, 1, 1000), ctg("I", 2, 1001, 2000), ctg("I", 3, 3000, 9000), ctg("II", 1, 1, 5000)]


def abi_read_range(eng, T, data, n_ctg):
    """(rc, dict(off, seen, start, end, line)) of gams_gpu_read_range_text: the size query, then the arrays"""
    off, seen = np.full(n_ctg + 1, 77, np.uint64), np.full(max(n_ctg, 1), 77, np.uint8)
    n = C.c_uint64(123)
    rc = L.gams_gpu_read_range_text(eng.h, T.ix, T.chr, data, len(data), off.ctypes.data, seen.ctypes.data, None, None, None,
                                    0, C.byref(n))
    if rc:
        return rc, None
    k = n.value
    st, en, ln = (np.full(max(k, 1), -5, t) for t in (np.int32, np.int32, np.int64))
    ln = ln.astype(np.uint32)
    if k:
        off2, seen2 = off.copy(), seen.copy()
        rc = L.gams_gpu_read_range_text(eng.h, T.ix, T.chr, data, len(data), off2.ctypes.data, seen2.ctypes.data,
                                        st.ctypes.data, en.ctypes.data, ln.ctypes.data, k, C.byref(n))
        assert rc == 0 and n.value == k and np.array_equal(off, off2) and np.array_equal(seen, seen2)
    return rc, dict(off=off, seen=seen[:n_ctg], start=st[:k], end=en[:k], line=ln[:k])


def model_arrays(ctgs, data):
    """the model's buckets in the layout of gams_gpu_read_range_text (ctgs in Locator order)"""
    m = model(ctgs, data)
    off = np.cumsum([0] + [len(b) for b in m["buckets"]]).astype(np.uint64)
    flat = [r for b in m["buckets"] for r in b]
    col = lambda j, t: np.array([r[j] for r in flat], t)
    return dict(off=off, seen=np.array(m["seen"], np.uint8), start=col(0, np.int32), end=col(1, np.int32),
                line=col(2, np.uint32))


def same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("off", "seen", "start", "end", "line"))


def abi_index(eng, T, data, n_ctg):
    """(rc, index, rg_group, n_kept) of gams_index_create_range_text"""
    ix, n = C.c_void_p(), C.c_uint64(123)
    grp = np.full(max(n_ctg, 1), 7, np.uint32)
    rc = L.gams_index_create_range_text(eng.h, T.ix, T.chr, data, len(data), C.byref(ix), grp.ctypes.data, C.byref(n))
    return rc, ix, grp[:n_ctg], n.value


def index_destroy(eng, ix):
    L.gams_index_destroy(eng.h, ix)


def index_of(eng, off, start, end):
    """gams_index_create over buckets given as arrays: intervals [start, end + 1)"""
    ix = C.c_void_p()
    off = np.ascontiguousarray(off, np.uint64)
    st = np.ascontiguousarray(start if len(start) else [0], np.uint32)
    sp = np.ascontiguousarray(np.asarray(end, np.int64) + 1 if len(end) else [0], np.uint32)
    _ok(eng, L.gams_index_create(eng.h, off.size - 1, off.ctypes.data, st.ctypes.data, sp.ctypes.data, C.byref(ix)))
    return ix


def abi_count(eng, ix, group, qs, qe):
    group, qs, qe = (np.ascontiguousarray(x, np.uint32) for x in (group, qs, qe))
    out = np.full(max(qs.size, 1), -9, np.int32)
    _ok(eng, L.gams_gpu_count(eng.h, ix, group.ctypes.data, qs.ctypes.data, qe.ctypes.data, qs.size, out.ctypes.data))
    return out[:qs.size]


def check_against_model(eng, ctgs, data):
    """both entries on `data` against the model; returns the model's arrays"""
    order = locator_order(ctgs)
    want = model_arrays(order, data)
    T = LocTables(eng, ctgs)
    try:
        rc, got = abi_read_range(eng, T, data, len(order))
        assert rc == 0 and same(got, want), (got, want)
        rc, ix, grp, kept = abi_index(eng, T, data, len(order))
        assert rc == 0 and kept == want["start"].size
        assert np.array_equal(grp, np.where(want["seen"] != 0, np.arange(len(order)), NONE).astype(np.uint32))
        # the index answers as gams_index_create over the model's buckets: every range's own span and its neighbours
        ref = index_of(eng, want["off"], want["start"], want["end"])
        try:
            g = np.repeat(np.arange(len(order)), np.diff(want["off"]).astype(np.int64))
            qg = np.concatenate([g, g, np.arange(len(order))]).astype(np.uint32)
            qs = np.concatenate([want["start"], np.maximum(want["start"] - 3, 0), np.zeros(len(order))]).astype(np.uint32)
            qe = np.concatenate([want["end"], want["end"] + 3, np.full(len(order), 0x7fffffff)]).astype(np.uint32)
            a, b = abi_count(eng, ix, qg, qs, qe), abi_count(eng, ref, qg, qs, qe)
            assert np.array_equal(a, b)
            assert np.array_equal(a[2 * g.size:], np.diff(want["off"]).astype(np.int32))     # the whole group
        finally:
            L.gams_index_destroy(eng.h, ref)
            L.gams_index_destroy(eng.h, ix)
    finally:
        T.close()
    return want


def flat_records(b):
    """host.read_range_text's buckets as (ctg id, start, end) in bucket order"""
    out = []
    for k, cid in enumerate(b["ids"]):
        lo, hi = int(b["off"][k]), int(b["off"][k + 1])
        out += [(cid, int(s), int(e)) for s, e in zip(b["start"][lo:hi], b["end"][lo:hi])]
    return out


def triples(records):
    """host.read_range's (ctg id, Range::to_string) records as (ctg id, start, end)"""
    return [(cid,) + parse_line(r.encode())[1:] for cid, r in records]


def model_triples(ctgs, data):
    m = model(ctgs, data)
    return [(ctgs[i]["id"], s, e) for i in sorted(range(len(ctgs)), key=lambda i: ctgs[i]["id"].encode())
            for s, e, _ in m["buckets"][i]]


# ---- goldens --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["spo11_hot.rg", "SK1.snp.rg"])
def test_goldens_equal_read_range(eng, s288c, name):
    ctgs = all_ctgs(s288c)
    data = read_bytes(name)
    want = host.read_range(eng, ctgs, helpers.read_lines(name))
    got = host.read_range_text(eng, ctgs, data)
    assert host.last_operator_device() == 1
    assert flat_records(got) == triples(want) == model_triples(ctgs, data)
    assert got["ids"] == sorted(got["ids"]) and {c for c, _ in want} <= set(got["ids"])
    for k in range(len(got["ids"])):                                  # file order inside every bucket
        assert np.all(np.diff(got["line"][int(got["off"][k]):int(got["off"][k + 1])].astype(np.int64)) > 0)
    check_against_model(eng, ctgs, data)


def test_spo11_is_79_71_69(eng, s288c):
    got = host.read_range_text(eng, all_ctgs(s288c), read_bytes("spo11_hot.rg"))
    assert got["start"].size == 69 and len(got["ids"]) == 2


@pytest.mark.parametrize("rg_name", ["spo11_hot.rg", "SK1.snp.rg"])
def test_locate_count_golden_rg_data(eng, s288c, rg_name):
    ctgs = all_ctgs(s288c)
    recs = host.read_range(eng, ctgs, helpers.read_lines(rg_name))
    rg_data = read_bytes(rg_name)
    for q in ("spo11_hot.rg", "SK1.snp.rg"):
        data = read_bytes(q)
        want = host.locate_text(eng, ctgs, data, count=True, rg_records=recs)
        assert want.count(b"\n") > 50
        assert host.locate_text(eng, ctgs, data, count=True, rg_data=rg_data) == want
        assert host.locate(eng, ctgs, helpers.read_lines(q), count=True, rg_data=rg_data).encode() == want


def test_sw_count_golden_rg_data(eng, s288c):
    ctgs = sorted(all_ctgs(s288c), key=lambda c: c["id"])
    buckets = bucket_features(ctgs)
    recs = host.read_range(eng, ctgs, helpers.read_lines("SK1.snp.rg"))
    rg_data = read_bytes("SK1.snp.rg")
    flist = [features_of(c, buckets) for c in ctgs]
    acts = ("gc", "count")
    want = host.sw_multi([eng], ctgs, flist, actions=acts, rg_records=recs)
    assert sum(int(r.split("\t")[8]) > 0 for r in want.splitlines()) > 100
    assert host.sw_multi([eng], ctgs, flist, actions=acts, rg_data=rg_data) == want
    second = engine.Engine(0)                 # a handle is not thread-safe: two handles for two host threads
    try:
        assert host.sw_multi([eng, second], ctgs, flist, actions=acts, rg_data=rg_data) == want
    finally:
        second.close()
    for c, feats in zip(ctgs, flist):
        if feats:
            assert host.sw(eng, c, feats, actions=acts, rg_data=rg_data) == host.sw(eng, c, feats, actions=acts, rg_records=recs)


def test_count_answers_like_index_create(eng, s288c):
    """a few hundred queries per ctg against the text-built index and gams_index_create over the same buckets"""
    ctgs = all_ctgs(s288c)
    order = locator_order(ctgs)
    rng = np.random.default_rng(11)
    for name in ("spo11_hot.rg", "SK1.snp.rg"):
        data = read_bytes(name)
        T = LocTables(eng, ctgs)
        try:
            rc, b = abi_read_range(eng, T, data, len(order))
            rc2, ix, grp, kept = abi_index(eng, T, data, len(order))
            assert rc == 0 and rc2 == 0 and kept == b["start"].size
            ref = index_of(eng, b["off"], b["start"], b["end"])
            for i, c in enumerate(order):
                qs = rng.integers(max(c["chr_start"] - 50, 0), c["chr_end"] + 50, 300)
                qe = qs + rng.integers(0, 3000, 300)
                g = np.full(300, i)
                assert np.array_equal(abi_count(eng, ix, g, qs, qe), abi_count(eng, ref, g, qs, qe))
            L.gams_index_destroy(eng.h, ref)
            L.gams_index_destroy(eng.h, ix)
        finally:
            T.close()


# ---- line edges -----------------------------------------------------------------------------------
EDGES = {
    "one line, no newline": b"I:5-9",
    "two on a ctg, no newline": b"I:5-9\nI:20-30",
    "crlf": b"I:5-9\r\nI:20-30\r\nI:40-50\r\n",
    "last line keeps its cr": b"I:5-9\nI:20-30\r",
    "blank lines": b"\n\nI:5-9\n\nI:20-30\n\n\nI:40\n",
    "strand and name": b"I:1-3\nI(+):5-9\nname.I:15-19\nname.I(-):25-29\n",
    "eleven digits": b"I:1-3\nI:12345678901\nI:5-12345678901\nI:2147483648\nI:7-2147483647\nI:8\n",
    "unknown chromosome": b"I:1-3\nIII:5-9\nI:5-9\nX:1\n",
    "point on a ctg start": b"I:1-3\nI:1001\nI:1001-1002\nI:3000\nI:1\nI:2\n",
    "spans two ctgs": b"I:1-3\nI:990-1010\nI:1990-3010\nI:1001-1002\nI:1500-1600\nI:2500-2600\n",
    "reversed": b"I:1-3\nI:500-100\nI:1500-900\nI:100-500\n",
    "trailing spaces": b"I:1-3  \nI:5-9 \n I:5-9\nI :5-9\n",
    "separators": b"I:1-3\nI:5_9\nI:5--9\nI:5-_-9\nI:5-\nI:-9\nI:5-9-\n",
}


@pytest.mark.parametrize("name", sorted(EDGES))
def test_line_edges(eng, name):
    data = EDGES[name]
    want = check_against_model(eng, SMALL, data)
    lines = [ln.decode() for ln in rust_lines(data)]
    got = host.read_range_text(eng, SMALL, data)
    assert host.last_operator_device() == 1
    assert flat_records(got) == triples(host.read_range(eng, SMALL, lines)) == model_triples(SMALL, data)
    assert got["start"].size == want["start"].size


def test_zero_bytes(eng):
    want = check_against_model(eng, SMALL, b"")
    assert want["start"].size == 0 and not want["seen"].any()
    got = host.read_range_text(eng, SMALL, b"")
    assert got["ids"] == [] and got["off"].tolist() == [0]
    assert host.locate_text(eng, SMALL, b"I:5-9\n", count=True, rg_data=b"") == \
        host.locate_text(eng, SMALL, b"I:5-9\n", count=True, rg_records=[])
    check_against_model(eng, SMALL, b"\n")


def test_second_field_is_not_cut(eng):
    """read_range parses the whole line (utils.rs:50): a tab makes it invalid here, while locate -f cuts at it"""
    data = b"I:1-3\nI:5-9\tfoo\nI:20-30\n"
    want = check_against_model(eng, SMALL, data)
    assert want["line"].tolist() == [2]
    T = LocTables(eng, SMALL)
    try:
        rc, text, rows = abi_locate(eng, T, data)
        assert rc == 0 and rows == 3 and b"I:5-9\tctg:I:1\n" in text
    finally:
        T.close()


def test_high_byte_is_refused_and_the_host_answers(eng):
    data = b"I:1-3\nI:5-9\ncaf\x80:1-2\nI:20-30\n"
    T = LocTables(eng, SMALL)
    try:
        assert abi_read_range(eng, T, data, len(SMALL))[0] == _lib.EUNSUPPORTED
        assert abi_index(eng, T, data, len(SMALL))[0] == _lib.EUNSUPPORTED
        assert abi_read_range(eng, T, b"I:1-3\n\0I:5-9\n", len(SMALL))[0] == _lib.EUNSUPPORTED
    finally:
        T.close()
    got = host.read_range_text(eng, SMALL, data)
    assert host.last_operator_device() == 0
    m = model_arrays(locator_order(SMALL), data)
    assert (got["start"].tolist(), got["end"].tolist(), got["line"].tolist()) == ([5, 20], [9, 30], [1, 3])
    assert np.array_equal(got["line"], m["line"])
    assert host.rg_load(eng, SMALL, data, text_path=True) == 1 and host.last_operator_device() == 0
    q = b"I:1-100\nI:1500-1600\n"
    assert host.locate_text(eng, SMALL, q, count=True, rg_data=data) == b"I:1-100\t2\nI:1500-1600\t0\n"


# ---- quirk edges ----------------------------------------------------------------------------------
def test_a_ctg_with_one_located_line_has_an_empty_group(eng):
    data = b"I:5-9\nI:20-30\nI:1500-1600\n"          # ctg 1: two lines, ctg 2: one, ctg 3 and II: none
    want = check_against_model(eng, SMALL, data)
    assert want["seen"].tolist() == [1, 1, 0, 0] and want["off"].tolist() == [0, 1, 1, 1, 1]
    T = LocTables(eng, SMALL)
    try:
        rc, ix, grp, kept = abi_index(eng, T, data, 4)
        assert rc == 0 and kept == 1 and grp.tolist() == [0, 1, NONE, NONE]
        q = b"I:1-100\nI:1500-1600\n"
        text, nb, rows = C.c_void_p(), C.c_uint64(), C.c_uint64()
        rc = L.gams_gpu_count_text(eng.h, T.ix, T.chr, ix, grp.ctypes.data, q, len(q), C.byref(text), C.byref(nb),
                                   C.byref(rows))
        assert rc == 0 and C.string_at(text, nb.value) == b"I:1-100\t1\nI:1500-1600\t0\n"
        q = b"I:4000-4100\n"                          # located to a ctg without a group: refused, as documented
        rc = L.gams_gpu_count_text(eng.h, T.ix, T.chr, ix, grp.ctypes.data, q, len(q), C.byref(text), C.byref(nb),
                                   C.byref(rows))
        assert rc == _lib.EUNSUPPORTED
        L.gams_index_destroy(eng.h, ix)
    finally:
        T.close()
    assert host.locate_text(eng, SMALL, b"I:1-100\nI:1500-1600\n", count=True, rg_data=data) == b"I:1-100\t1\nI:1500-1600\t0\n"
    assert host.last_operator_device() == 1
    got = host.read_range_text(eng, SMALL, data)
    assert got["ids"] == ["ctg:I:1", "ctg:I:2"] and got["off"].tolist() == [0, 1, 1]


def test_the_same_line_twice(eng):
    want = check_against_model(eng, SMALL, b"I:5-9\nI:5-9\nII:7\nII:7\nII:7\n")
    assert want["line"].tolist() == [1, 3, 4] and want["start"].tolist() == [5, 7, 7]


# ---- block edges of the new kernels ---------------------------------------------------------------
def three_ctg_file(n, second_at=None, alternate=False, seed=0):
    """n lines over ctgs 1..3 of SMALL: sorted by position with the first line of ctg 2 at `second_at`, or alternating"""
    rng = np.random.default_rng(seed)
    lo = {0: 1, 1: 1001, 2: 3000}
    if alternate:
        which = np.arange(n) % 3
    else:
        a = n // 3 if second_at is None else second_at
        b = a + max((n - a) // 2, 1)
        which = np.where(np.arange(n) < a, 0, np.where(np.arange(n) < b, 1, 2))
    out = []
    for k, w in enumerate(which):
        s = lo[int(w)] + int(rng.integers(1, 900))
        out.append(f"I:{s}-{s + int(rng.integers(0, 50))}")
    return ("\n".join(out) + "\n").encode()


@pytest.mark.parametrize("n", [255, 256, 257, 513])
def test_block_edges_sorted(eng, n):
    check_against_model(eng, SMALL, three_ctg_file(n, seed=n))


@pytest.mark.parametrize("at", [255, 256, 63, 64])
def test_first_line_of_a_ctg_on_a_block_edge(eng, at):
    data = three_ctg_file(513, second_at=at, seed=at)
    want = check_against_model(eng, SMALL, data)
    assert at not in want["line"].tolist() and at + 1 in want["line"].tolist()     # the line at the edge is the dropped one


@pytest.mark.parametrize("n", [255, 256, 257, 513])
def test_alternating_ctgs_twice(eng, n):
    """no run longer than 1, bucket order differs from file order: equal to the model, order and `line` included, on
    two consecutive calls"""
    data = three_ctg_file(n, alternate=True, seed=n)
    order = locator_order(SMALL)
    want = model_arrays(order, data)
    assert not np.all(np.diff(want["line"].astype(np.int64)) > 0)
    T = LocTables(eng, SMALL)
    try:
        for _ in range(2):
            rc, got = abi_read_range(eng, T, data, len(order))
            assert rc == 0 and same(got, want)
    finally:
        T.close()
    check_against_model(eng, SMALL, data)


# ---- index capacity -------------------------------------------------------------------------------
@pytest.mark.parametrize("located", [8193, 8194])
def test_index_capacity(eng, located):
    """8,192 kept: the workgroup builder at its cap; 8,193: the segmented radix sort behind it"""
    rng = np.random.default_rng(located)
    big = [ctg("I", 1, 1, 1_000_000), ctg("II", 1, 1, 1000)]
    s = rng.integers(1, 990_000, located)
    e = s + rng.integers(0, 5000, located)
    data = ("\n".join(f"I:{a}-{b}" for a, b in zip(s, e)) + "\nII:5-6\nII:7-8\n").encode()
    T = LocTables(eng, big)
    try:
        rc, ix, grp, kept = abi_index(eng, T, data, 2)
        assert rc == 0 and kept == located and grp.tolist() == [0, 1]
        qs = rng.integers(0, 1_000_000, 1000)
        qe = qs + rng.integers(0, 20000, 1000)
        starts, stops = np.sort(s[1:]), np.sort(e[1:] + 1)
        want = np.searchsorted(starts, qe, "left") - np.searchsorted(stops, qs + 1, "left")
        assert np.array_equal(abi_count(eng, ix, np.zeros(1000), qs, qe), want.astype(np.int32))
        assert abi_count(eng, ix, [1], [0], [100]).tolist() == [1]
        L.gams_index_destroy(eng.h, ix)
    finally:
        T.close()


# ---- reuse of the handle's cached buffers ---------------------------------------------------------
def test_loads_around_a_locate_text_and_a_shorter_file_after_a_longer(eng):
    long_ = three_ctg_file(513, alternate=True, seed=5)
    short = b"I:5-9\nI:20-30\nI:1500-1600"                   # no final newline: the longer file's tail lies behind it
    order = locator_order(SMALL)
    T = LocTables(eng, SMALL)
    try:
        rc, a = abi_read_range(eng, T, long_, len(order))
        assert rc == 0 and same(a, model_arrays(order, long_))
        rc, text, rows = abi_locate(eng, T, b"I:5-9\nII:7\n")
        assert rc == 0 and rows == 2
        rc, b = abi_read_range(eng, T, long_, len(order))
        assert rc == 0 and same(a, b)
        rc, c = abi_read_range(eng, T, short, len(order))
        assert rc == 0 and same(c, model_arrays(order, short)) and c["line"].tolist() == [1]
        rc, ix, grp, kept = abi_index(eng, T, short, len(order))
        assert rc == 0 and kept == 1 and grp.tolist() == [0, 1, NONE, NONE]
        L.gams_index_destroy(eng.h, ix)
    finally:
        T.close()


def test_stage_stopwatch(eng):
    data = three_ctg_file(513, seed=9)
    T = LocTables(eng, SMALL)
    try:
        rc, ix, grp, kept = abi_index(eng, T, data, len(SMALL))
        assert rc == 0
        ms, n = (C.c_float * 16)(), C.c_uint32()
        _ok(eng, L.gams_gpu_last_stage_ms(eng.h, ms, 16, C.byref(n)))
        assert n.value == 9 and all(0.0 <= ms[k] < 1000.0 for k in range(9))
        L.gams_index_destroy(eng.h, ix)
    finally:
        T.close()
