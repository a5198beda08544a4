"""gams_spans_create_runlist_text on the device: the bytes of a runlist JSON file to a resident span set, held against
the model of tests/runlist_text.py -- the golden intergenic.json, a document pushed across every 16-B / 64-B / 4-KiB /
16-KiB boundary, unsorted / overlapping / adjacent / duplicate spans, the directory at its extremes (through
gams_gpu_cover, bit for bit against a set from gams_spans_create), every refusal with the host's fallback behind it,
and one AnnoSet shared by several input files."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import helpers
import runlist_text as rt
from gams_amd import _lib, engine, host

pytestmark = pytest.mark.gpu
L = _lib.load()
I32_MAX = rt.I32_MAX


@pytest.fixture(scope="module")
def eng():
    e = engine.Engine(0)
    yield e
    e.close()


def create(eng, data):
    """the raw entry: (rc, sp, names, n_groups, n_spans)"""
    sp, nm = C.c_void_p(1), C.c_void_p(1)
    ng, ns = C.c_uint32(), C.c_uint64()
    rc = L.gams_spans_create_runlist_text(eng.h, data, len(data), C.byref(sp), C.byref(nm), C.byref(ng), C.byref(ns))
    return rc, sp, nm, ng.value, ns.value


def read_set(eng, sp, nm):
    """(names, [lo per group], [hi per group]) of a set and its name table, through gams_names_read and gams_spans_read"""
    n, nb, ns = C.c_uint32(), C.c_uint64(), C.c_uint64()
    eng.check(L.gams_names_read(eng.h, nm, C.byref(n), C.byref(nb), None, None))
    flat, noff = C.create_string_buffer(max(nb.value, 1)), np.zeros(n.value + 1, np.uint64)
    eng.check(L.gams_names_read(eng.h, nm, C.byref(n), C.byref(nb), flat, noff.ctypes.data))
    names = [flat.raw[int(noff[g]):int(noff[g + 1])].decode() for g in range(n.value)]
    off = np.zeros(n.value + 1, np.uint64)
    eng.check(L.gams_spans_read(eng.h, sp, off.ctypes.data, None, None, 0, C.byref(ns)))
    lo, hi = np.zeros(max(ns.value, 1), np.int32), np.zeros(max(ns.value, 1), np.int32)
    if ns.value:
        eng.check(L.gams_spans_read(eng.h, sp, off.ctypes.data, lo.ctypes.data, hi.ctypes.data, ns.value, C.byref(ns)))
    cut = lambda a: [a[int(off[g]):int(off[g + 1])].tolist() for g in range(n.value)]
    return names, cut(lo), cut(hi)


def destroy_set(eng, sp, nm):
    L.gams_spans_destroy(eng.h, sp)
    L.gams_names_destroy(eng.h, nm)


def spans_from_arrays(eng, sets):
    off, lo, hi = rt.as_arrays(sets)
    lo, hi = np.append(lo, np.int32(0)), np.append(hi, np.int32(0))       # (never an empty buffer)
    sp = C.c_void_p()
    eng.check(L.gams_spans_create(eng.h, len(sets), off.ctypes.data, lo.ctypes.data, hi.ctypes.data, C.byref(sp)))
    return sp


def cover(eng, sp, q):
    grp, cl, ch, qs, qe = q
    prop = np.zeros(grp.size, np.float32)
    eng.check(L.gams_gpu_cover(eng.h, sp, grp.ctypes.data, cl.ctypes.data, ch.ctypes.data, qs.ctypes.data, qe.ctypes.data,
                               grp.size, prop.ctypes.data))
    return prop


def queries(sets, n, seed):
    """n queries over the groups of `sets`: point ranges, whole-group ranges, ranges that touch a span's end from either
    side, random ranges; clips wide and narrow; a group beyond the set now and then"""
    rng = np.random.default_rng(seed)
    groups = [g for g, v in enumerate(sets.values()) if v[0].size]
    vals = list(sets.values())
    grp, cl, ch, qs, qe = (np.zeros(n, np.uint32), np.ones(n, np.int32), np.full(n, I32_MAX, np.int32), np.ones(n, np.int32),
                           np.ones(n, np.int32))
    kind = rng.integers(0, 6, n)
    for i in range(n):
        g = groups[int(rng.integers(0, len(groups)))] if groups else 0
        lo, hi = vals[g] if groups else (np.array([5], np.int32), np.array([9], np.int32))
        k = int(rng.integers(0, lo.size))
        a, b = int(lo[k]), int(hi[k])
        if kind[i] == 0:                                       # a point: on an end, one beside it
            s = e = min(max((a, b, a - 1, b + 1)[int(rng.integers(0, 4))], 1), I32_MAX)
        elif kind[i] == 1:                                     # the whole group, and beyond
            s, e = max(int(lo[0]) - int(rng.integers(0, 3)), 1), min(int(hi[-1]) + int(rng.integers(0, 3)), I32_MAX)
        elif kind[i] == 2:                                     # ends on a span's first base, or one before it
            e = max(a - int(rng.integers(0, 2)), 1)
            s = max(e - int(rng.integers(0, 1000)), 1)
        elif kind[i] == 3:                                     # begins on a span's last base, or one behind it
            s = min(b + int(rng.integers(0, 2)), I32_MAX)
            e = min(s + int(rng.integers(0, 1000)), I32_MAX)
        else:                                                  # across a few spans
            k2 = min(k + int(rng.integers(0, 8)), lo.size - 1)
            s, e = max(a - int(rng.integers(0, 5)), 1), min(int(hi[k2]) + int(rng.integers(0, 5)), I32_MAX)
        grp[i], qs[i], qe[i] = g, s, e
        if rng.integers(0, 4) == 0:                            # a clip that cuts into the range
            cl[i] = min(max(s + int(rng.integers(-3, 4)), 1), I32_MAX)
            ch[i] = min(max(e + int(rng.integers(-3, 4)), 1), I32_MAX)
        if rng.integers(0, 50) == 0:
            grp[i] = len(sets) + int(rng.integers(0, 3))
    return grp, cl, ch, qs, qe


def check_document(eng, data, n_queries=0, seed=1):
    """the device's set of `data` equals the model: names, spans, and (n_queries > 0) gams_gpu_cover bit for bit against a
    set from gams_spans_create of the model's spans"""
    want = rt.model(data)
    assert rt.device_takes(data)
    got = host.read_runlist_text(eng, data)
    assert rt.same_sets(got, want)
    if n_queries:
        rc, sp, nm, ng, ns = create(eng, data)
        assert rc == 0 and ng == len(want) and ns == sum(v[0].size for v in want.values())
        ref = spans_from_arrays(eng, want)
        try:
            q = queries(want, n_queries, seed)
            a, b = cover(eng, sp, q), cover(eng, ref, q)
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
            assert (a > 0).sum() > n_queries // 4 and (a < 1).sum() > n_queries // 20
        finally:
            L.gams_spans_destroy(eng.h, sp)
            L.gams_names_destroy(eng.h, nm)
            L.gams_spans_destroy(eng.h, ref)
    return want


def all_ctgs(s288c, piece=100000):
    ctgs = []
    for chr_id in ("I", "Mito"):
        ctgs += helpers.gen_ctgs(chr_id, s288c[chr_id], piece=piece)
    return ctgs


def golden(name):
    with open(os.path.join(helpers.S288C, name), "rb") as fh:
        return fh.read()


# ---- golden ------------------------------------------------------------------------------------------------------------
def test_golden(eng, s288c):
    js = golden("intergenic.json")
    want = check_document(eng, js, n_queries=20000)
    assert [v[0].size for v in want.values()] == [25, 85, 32, 176, 47, 79, 30, 122, 62, 69, 75, 110, 99, 88, 140, 108]
    ctgs = all_ctgs(s288c)
    data = golden("ctg.range.tsv")
    kw = dict(header=True, prefix="intergenic", idx_id=1, idx_range=2)
    exp = host.anno_text(eng, ctgs, json.loads(js), data, **kw)
    got = host.anno_text(eng, ctgs, js, data, **kw)
    assert host.last_operator_device() == 1
    assert got == exp and b"85779\t0.0000" in got and b"130218\t0.1072" in got
    lines = [ln for ln in data.decode().split("\n") if ln]
    assert host.anno(eng, ctgs, js, lines, **kw).encode() == exp
    aset = host.AnnoSet(eng, js)
    try:
        assert aset.device is True and host.last_operator_device() == 1
        assert aset.n_groups == 16 and aset.n_spans == 1347 and aset.names == list(want)
        assert rt.same_sets(aset.spans(), want)
    finally:
        aset.close()


# ---- seams -------------------------------------------------------------------------------------------------------------
def test_seams(eng):
    doc = rt.seam_doc()
    want = rt.model(doc)
    assert [v[0].size for v in want.values()] == [300, 0, 1000, 1, 0, 900] and rt.device_takes(doc)
    for p in rt.SEAM_PREFIXES:
        got = host.read_runlist_text(eng, b" " * p + doc)
        assert rt.same_sets(got, want), p


# ---- normalisation -----------------------------------------------------------------------------------------------------
def disjoint_spans(n, seed, base=1000):
    rng = np.random.default_rng(seed)
    lo = base + np.cumsum(rng.integers(3, 400, n))
    ln = rng.integers(0, 2, n)                                   # (gaps of at least two: nothing joins)
    return [(int(a), int(a + b)) for a, b in zip(lo, ln)]


def shuffled(spans, seed):
    out = list(spans)
    np.random.default_rng(seed).shuffle(out)
    return out


def normalisation_documents():
    base = disjoint_spans(10000, 11)
    rng = np.random.default_rng(12)
    messy = list(base)
    for k in rng.choice(len(base) - 1, 3000, replace=False):     # 30 %: reach into the next span, or end right before it
        a, b = base[int(k)]
        nxt = base[int(k) + 1]
        messy[int(k)] = (a, nxt[0] + int(rng.integers(0, 2)) if rng.integers(0, 2) else nxt[0] - 1)
    chain = [(1_000_000_000 + 7 * i, 1_000_000_000 + 7 * i + 6) for i in range(1000)]
    return {
        "shuffled": rt.doc([("I", rt.runlist_of(shuffled(base, 1)))]),
        "overlapping and adjacent": rt.doc([("I", rt.runlist_of(shuffled(messy, 2)))]),
        "adjacent chain": rt.doc([("I", rt.runlist_of(shuffled(chain, 3)))]),
        "adjacent chain in order": rt.doc([("I", rt.runlist_of(chain))]),
        "second group unsorted": rt.doc([("I", rt.runlist_of(base[:3000])), ("II", rt.runlist_of(shuffled(base[:3000], 4)))],
                                        pretty=True),
        "duplicates": rt.doc([("I", rt.runlist_of(shuffled(base[:2000] * 3, 5))), ("II", "5,5,5-5,4-6,5")]),
    }


NORMALISATION = normalisation_documents()


@pytest.mark.parametrize("name", sorted(NORMALISATION))
def test_normalisation(eng, name):
    data = NORMALISATION[name]
    want = check_document(eng, data, n_queries=20000, seed=len(name))
    if name.startswith("adjacent chain"):
        assert want["I"][0].tolist() == [1_000_000_000] and want["I"][1].tolist() == [1_000_000_000 + 6999]
        assert len(data) > 16384                                 # the run crosses workgroups of the text passes and of the joins
    if name == "overlapping and adjacent":
        assert 6000 < want["I"][0].size < 9000
    if name == "duplicates":
        assert want["I"][0].size == 2000 and want["II"][0].tolist() == [4]


# ---- directory ---------------------------------------------------------------------------------------------------------
def directory_documents():
    rng = np.random.default_rng(21)
    spread = np.unique(np.concatenate([[1, I32_MAX - 1], rng.integers(1, I32_MAX - 1, 3000)]))
    spread = spread[np.diff(spread, append=2**40) > 2]
    spread[-1] = I32_MAX - 1
    close = [(500_000 + 3 * i, 500_000 + 3 * i + int(i % 2)) for i in range(22)]     # lows within 64 of each other
    many = disjoint_spans(8193, 22)
    return {
        "spread": rt.doc([("I", rt.runlist_of([(int(a), int(a) + 1) for a in spread]))]),
        "close": rt.doc([("I", rt.runlist_of(close))]),
        "1 span": rt.doc([("I", "77-2147483647")]),
        "2 spans": rt.doc([("I", "1,2147483647")]),
        "8193 spans": rt.doc([("I", rt.runlist_of(many))]),
    }


DIRECTORY = directory_documents()


@pytest.mark.parametrize("name", sorted(DIRECTORY))
def test_directory(eng, name):
    want = check_document(eng, DIRECTORY[name], n_queries=20000, seed=len(name))
    lo = want["I"][0]
    key0, shift, nb, d = rt.span_dir(lo)
    assert nb <= lo.size and d[-1] == lo.size
    if name == "spread":
        assert lo[0] == 1 and lo[-1] == I32_MAX - 1 and shift >= 19
    if name == "close":
        assert int(lo[-1]) - int(lo[0]) < 64 and shift == 2
    if name == "2 spans":
        assert (shift, nb) == (30, 2)                            # a range of 2^31 - 2 over two buckets
    if name == "8193 spans":
        assert lo.size == 8193


# ---- refusals ----------------------------------------------------------------------------------------------------------
REFUSED = {
    "a backslash": b'{"a\\"b": "1-5"}',
    "a byte >= 0x80": '{"chré": "1-5"}'.encode(),
    "a NUL": b'{"I\x00": "1-5"}',
    "a nested object": b'{"I": {"a": "1-5"}, "II": "3"}',
    "a number value": b'{"I": 5, "II": "3"}',
    "a space inside a runlist": b'{"I": "1-5, 7-9"}',
    "5-3": b'{"I": "1,5-3"}',
    "11 digits": b'{"I": "00000000012-00000000015"}',
    "11 digits outside i32": b'{"I": "12345678901"}',
    "2147483648": b'{"I": "1-2147483648"}',
    "-5--1": b'{"I": "-5--1,3"}',
    "a duplicate key": b'{"I": "1-5", "II": "7", "I": "9-12"}',
    "a missing brace": b'{"I": "1-5", "II": "7"',
    "text after the brace": b'{"I": "1-5"} {"II": "7"}',
    "an empty token": b'{"I": "1-5,,7"}',
    "a trailing comma in a runlist": b'{"I": "1-5,"}',
    "a leading comma in a runlist": b'{"I": ",1-5"}',
    "a control character in a key": b'{"I\tI": "1-5"}',
    "an array": b'["1-5"]',
    "null": b'{"I": null}',
    "an odd number of strings": b'{"I": "1-5", "II"}',
    "two colons": b'{"I":: "1-5", "II" "7"}',
    "nothing": b"",
}
GOOD = b'{"I": "1-5,9", "II": "3"}'


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_refusals(eng, name):
    data = REFUSED[name]
    assert not rt.device_takes(data)
    rc, sp, nm, ng, ns = create(eng, data)
    assert rc == _lib.EUNSUPPORTED and sp.value is None and nm.value is None and (ng, ns) == (0, 0)
    assert L.gams_gpu_last_error(eng.h)
    assert rt.same_sets(host.read_runlist_text(eng, GOOD), rt.model(GOOD))      # the handle stays usable
    want = rt.verdict(data)
    if want is None:
        with pytest.raises(host.HostError) as ei:
            host.AnnoSet(eng, data)
        assert ei.value.code == _lib.EINVAL
    else:
        aset = host.AnnoSet(eng, data)
        try:
            assert aset.device is False and host.last_operator_device() == 0
            assert rt.same_sets(aset.spans(), want)
        finally:
            aset.close()
    assert rt.same_sets(host.read_runlist_text(eng, GOOD), rt.model(GOOD))


def test_refusal_verdicts_cover_both_outcomes():
    ok = {k for k, v in REFUSED.items() if rt.verdict(v) is not None}
    assert ok == {"a backslash", "a byte >= 0x80", "11 digits", "-5--1", "a duplicate key", "an empty token",
                  "a trailing comma in a runlist", "a leading comma in a runlist"}


# ---- reuse -------------------------------------------------------------------------------------------------------------
def test_one_set_several_input_files(eng, s288c):
    js = golden("intergenic.json")
    runlists = json.loads(js)
    ctgs = all_ctgs(s288c)
    data = golden("ctg.range.tsv")
    rows = [r for r in data.split(b"\n") if r]
    files = [(data, True), (b"\n".join(rows[1:][::-1]), False), (b"\r\n".join(rows[1:3] * 50) + b"\r\n", False)]
    aset = host.AnnoSet(eng, js)
    try:
        assert aset.device
        for blob, header in files:
            kw = dict(header=header, prefix="intergenic", idx_id=1, idx_range=2)
            got = host.anno_text(eng, ctgs, aset, blob, **kw)
            assert host.last_operator_device() == 1
            assert got == host.anno_text(eng, ctgs, runlists, blob, **kw) and got.count(b"\n") >= 3
    finally:
        aset.close()
