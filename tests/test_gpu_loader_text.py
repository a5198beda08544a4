"""The loaders on the device over several files: gams_index_create_range_files / gams_gpu_loader_text through the C ABI,
host.loader_text and the rg_data=[...] forms of locate / sw above them, against the pure-Python model of
tests/test_loader_text_cpu.py (one read_range per file, drop-first per file, serials carried on, the canonical range) and,
for one file on fresh counters, against the host's loader_records / loader_tsv / resp_command."""
import ctypes as C

import numpy as np
import pytest

import helpers
from gams_amd import _lib, engine, host
from test_gpu_rg_text import SMALL, abi_count, abi_index, ctg, index_of, three_ctg_file
from test_gpu_text_ops import LocTables, _ok, all_ctgs, read_bytes
from test_loader_text_cpu import FEATURE, RECORDS, RESP, RG, TSV, fuzz_case, host_order_text, model_files, model_loader
from test_rg_text_cpu import locator_order, rust_lines

pytestmark = pytest.mark.gpu

L = _lib.load()
NONE = 0xffffffff
FMT = {RECORDS: "records", TSV: "tsv", RESP: "resp"}
KIND = {RG: "rg", FEATURE: "feature"}


@pytest.fixture(scope="module")
def eng():
    e = engine.Engine(0)
    yield e
    e.close()


def file_args(files):
    bufs = [np.frombuffer(bytes(f), np.uint8) for f in files]
    ptrs = (C.c_void_p * max(len(bufs), 1))(*[b.ctypes.data if b.size else None for b in bufs])
    lens = np.array([b.size for b in bufs] or [0], np.uint64)
    return len(bufs), ptrs, lens, bufs


def abi_loader(eng, T, files, n_ctg, kind=RG, tag=b"", fmt=RECORDS, base=None):
    """(rc, dict(text, off, next, per_file, n_rows)) of gams_gpu_loader_text"""
    nf, ptrs, lens, _keep = file_args(files)
    text, nb, rows = C.c_void_p(), C.c_uint64(77), C.c_uint64(77)
    off = np.full(nf * n_ctg + 1, 77, np.uint64)
    nxt = np.full(max(n_ctg, 1), -7, np.int32)
    per = np.full(max(nf, 1), 77, np.uint64)
    b = None if base is None else np.ascontiguousarray(base, np.int32)
    rc = L.gams_gpu_loader_text(eng.h, T.ix, T.chr, T.ids, nf, ptrs, lens.ctypes.data, kind, tag, len(tag), fmt,
                                None if b is None else b.ctypes.data, C.byref(text), C.byref(nb), off.ctypes.data,
                                nxt.ctypes.data, per.ctypes.data, C.byref(rows))
    if rc:
        return rc, None
    return rc, dict(text=C.string_at(text, nb.value) if nb.value else b"", off=off.tolist(), next=nxt[:n_ctg].tolist(),
                    per_file=per[:nf].tolist(), n_rows=rows.value)


def abi_index_files(eng, T, files, n_ctg):
    nf, ptrs, lens, _keep = file_args(files)
    ix, n = C.c_void_p(), C.c_uint64(123)
    grp = np.full(max(n_ctg, 1), 7, np.uint32)
    rc = L.gams_index_create_range_files(eng.h, T.ix, T.chr, nf, ptrs, lens.ctypes.data, C.byref(ix), grp.ctypes.data, C.byref(n))
    return rc, ix, grp[:n_ctg], n.value


def check_index(eng, ctgs, files):
    """gams_index_create_range_files against gams_index_create over the model's buckets, the ranges of a ctg from all
    files: every range's own span, its neighbourhood, and the whole group"""
    order = locator_order(ctgs)
    m = model_files(order, files)
    per = [[(p[3], p[4]) for f in range(len(files)) for p, _ in m["kept"][f][i]] for i in range(len(order))]
    off = np.cumsum([0] + [len(b) for b in per]).astype(np.uint64)
    st = np.array([s for b in per for s, _ in b], np.int64)
    en = np.array([e for b in per for _, e in b], np.int64)
    T = LocTables(eng, ctgs)
    try:
        rc, ix, grp, kept = abi_index_files(eng, T, files, len(order))
        assert rc == 0 and kept == st.size
        assert np.array_equal(grp, np.where(np.array(m["seen"]), np.arange(len(order)), NONE).astype(np.uint32))
        ref = index_of(eng, off, st, en)
        try:
            g = np.repeat(np.arange(len(order)), np.diff(off).astype(np.int64))
            qg = np.concatenate([g, g, np.arange(len(order))]).astype(np.uint32)
            qs = np.concatenate([st, np.maximum(st - 3, 0), np.zeros(len(order))]).astype(np.uint32)
            qe = np.concatenate([en, en + 3, np.full(len(order), 0x7fffffff)]).astype(np.uint32)
            a, b = abi_count(eng, ix, qg, qs, qe), abi_count(eng, ref, qg, qs, qe)
            assert np.array_equal(a, b)
            assert np.array_equal(a[2 * g.size:], np.diff(off).astype(np.int32))
        finally:
            L.gams_index_destroy(eng.h, ref)
            L.gams_index_destroy(eng.h, ix)
    finally:
        T.close()
    return per


def check_loader(eng, ctgs, files, kind=RG, tag="", fmt=RECORDS, base=None, device=1):
    """the ABI and host.loader_text against the model; base: {ctg id: counter}; device = 0: the ABI refuses the case and
    the host's passes answer.  Returns the model's answer."""
    order = locator_order(ctgs)
    b = None if base is None else [base.get(c["id"], 0) for c in order]
    want = model_loader(order, files, kind, tag, fmt, b)
    T = LocTables(eng, ctgs)
    try:
        if not device:
            assert abi_loader(eng, T, files, len(order), kind, tag.encode("latin-1"), fmt, b)[0] == _lib.EUNSUPPORTED
        for _ in range(2 if device else 0):                    # two calls are identical
            rc, got = abi_loader(eng, T, files, len(order), kind, tag.encode("latin-1"), fmt, b)
            assert rc == 0, L.gams_gpu_last_error(eng.h)
            assert got["text"] == want["text"]
            assert got["off"] == want["off"] and got["next"] == want["next"]
            assert got["per_file"] == want["per_file"] and got["n_rows"] == want["n_rows"]
    finally:
        T.close()
    text, nxt, per = host.loader_text(eng, ctgs, files, KIND[kind], tag, FMT[fmt], base)
    assert host.last_operator_device() == device
    assert text == host_order_text(order, want)
    assert nxt == {c["id"]: n for c, n in zip(order, want["next"])} and per == want["per_file"]
    return want


def host_one_file(eng, ctgs, data, kind, tag, fmt):
    """the host's text of one file on fresh counters: loader_records, loader_tsv without its header, resp_command"""
    lines = [ln.decode("latin-1") for ln in rust_lines(data)]
    t = tag if kind == FEATURE else None
    if fmt == TSV:
        return host.loader_tsv(eng, ctgs, lines, t).split("\n", 1)[1].encode("latin-1")
    recs = host.loader_records(eng, ctgs, lines, t)
    if fmt == RESP:
        return b"".join(host.resp_command(["SET", k.encode("latin-1"), v.encode("latin-1")]) for k, v in recs)
    return "".join(f"{k}\t{v}\n" for k, v in recs).encode("latin-1")


# ---- file seams -----------------------------------------------------------------------------------
SEAMS = {
    "no final newline, then a file": [b"I:5-9\nI:20-30", b"I:40-50\nI:60-70\nI:1500\nI:1600\n"],
    "an empty file between": [b"I:5-9\nI:20-30\n", b"", b"I:40-50\nI:60-70\n"],
    "a file of one newline": [b"I:5-9\nI:20-30\n", b"\n", b"I:40-50\nI:60-70\n"],
    "crlf": [b"I:5-9\r\nI:20-30\r\n", b"I:40-50\r\nI:60-70\r\nII:7\r\nII:8\r\n"],
    "the last file without a newline": [b"I:5-9\nI:20-30\n", b"I:40-50\nI:60-70"],
    "no newline anywhere, a cr kept": [b"I:5-9\nI:20-30\r", b"I:40-50\nI:60-70\r"],
    "empty files around": [b"", b"I:5-9\nI:20-30", b"", b""],
    "only empty files": [b"", b""],
    "no file": [],
    "a first line that would join": [b"I:5-9\nI:2", b"0-30\nI:40\nI:41\n"],
}


@pytest.mark.parametrize("name", sorted(SEAMS))
def test_file_seams(eng, name):
    files = SEAMS[name]
    for kind, fmt in ((RG, RECORDS), (FEATURE, RESP), (FEATURE, TSV)):
        check_loader(eng, SMALL, files, kind, "tg", fmt)
    check_index(eng, SMALL, files)


def test_nothing_kept_leaves_the_counters(eng):
    T = LocTables(eng, SMALL)
    try:
        for files in ([], [b"", b""], [b"I:5-9\n", b"I:7\n"]):
            rc, got = abi_loader(eng, T, files, 4, base=[3, 4, 5, 6])
            assert rc == 0 and got["text"] == b"" and got["n_rows"] == 0 and got["next"] == [3, 4, 5, 6]
            assert got["off"] == [0] * (len(files) * 4 + 1) and got["per_file"] == [0] * len(files)
    finally:
        T.close()


# ---- drop-first per file --------------------------------------------------------------------------
def test_one_located_line_in_each_of_three_files(eng):
    files = [b"I:5-9\nI:1500\nI:1600\n", b"I:20-30\nI:1700\nI:1800\n", b"I:40-50\n"]
    base = {"ctg:I:1": 11, "ctg:I:2": 5}
    want = check_loader(eng, SMALL, files, base=base)
    assert want["seen"] == [True, True, False, False] and want["next"] == [11, 7, 0, 0] and want["n_rows"] == 2
    assert b"rg:ctg:I:1:" not in want["text"] and b"rg:ctg:I:2:7\t" in want["text"]
    per = check_index(eng, SMALL, files)
    assert per[0] == [] and per[1] == [(1600, 1600), (1800, 1800)]


def test_a_ctg_located_in_the_second_file_only(eng):
    files = [b"I:5-9\nI:20-30\n", b"II:7\nII:8-9\nII:10\nI:40\n"]
    want = check_loader(eng, SMALL, files, FEATURE, "x", TSV)
    assert want["per_file"] == [1, 2] and want["next"] == [1, 0, 0, 2]
    assert want["off"][1] == want["off"][7] == len(b"feature:ctg:I:1:1\tI:20-30\t11\tx\n") and want["off"][8] == len(want["text"])
    check_index(eng, SMALL, files)


def test_two_files_are_not_their_concatenation(eng):
    a, b = b"I:5-9\nI:20-30\n", b"I:40-50\nI:60-70\n"
    two, one = check_loader(eng, SMALL, [a, b]), check_loader(eng, SMALL, [a + b])
    assert (two["n_rows"], one["n_rows"]) == (2, 3) and two["text"] != one["text"]
    assert check_index(eng, SMALL, [a, b])[0] == [(20, 30), (60, 70)]
    assert check_index(eng, SMALL, [a + b])[0] == [(20, 30), (40, 50), (60, 70)]


# ---- run leaders ----------------------------------------------------------------------------------
def split_lines(data, cuts):
    lines = data.split(b"\n")[:-1]
    edges = [0] + list(cuts) + [len(lines)]
    return [b"".join(ln + b"\n" for ln in lines[a:b]) for a, b in zip(edges, edges[1:])]


@pytest.mark.parametrize("cuts", [(64,), (65,), (256, 257), (1,), (63, 64, 65, 128, 192)])
def test_a_file_boundary_inside_a_run(eng, cuts):
    """the same ctg on both sides of the seam: the line behind it is its file's first, dropped, whatever lane it has"""
    data = three_ctg_file(400, second_at=390, seed=cuts[0])          # lines 0..389 on ctg 1: one run over every seam
    files = split_lines(data, cuts)
    want = check_loader(eng, SMALL, files)
    m = model_files(locator_order(SMALL), files)
    assert all(k != 0 for f in range(len(files)) for _, k in m["kept"][f][0]) and want["n_rows"] > 380
    check_index(eng, SMALL, files)


@pytest.mark.parametrize("n", [255, 256, 257, 513])
def test_alternating_ctgs_and_block_seams_of_the_writer(eng, n):
    """every lane a run leader; n lines in three files give n - 9 rows, around the writer's blocks of 256"""
    files = split_lines(three_ctg_file(n + 9, alternate=True, seed=n), (100, 103))
    for kind, fmt in ((RG, RECORDS), (FEATURE, RESP)):
        want = check_loader(eng, SMALL, files, kind, "alt", fmt, base={"ctg:I:2": 9})
        assert want["n_rows"] == n
    check_index(eng, SMALL, files)


# ---- serials and row lengths ----------------------------------------------------------------------
@pytest.mark.parametrize("base", [8, 9, 98, 99, 9998, 99998, 2147483643])
@pytest.mark.parametrize("fmt", [RECORDS, RESP])
def test_serial_digits(eng, base, fmt):
    files = [b"I:5\nI:6\nI:7\n", b"I:8\nI:9\nI:10\n"]                 # serials base + 1 .. base + 4: a digit more on the way
    want = check_loader(eng, SMALL, files, RG, "", fmt, base={"ctg:I:1": base})
    assert want["next"][0] == base + 4


def test_a_serial_beyond_int32_max_is_einval(eng):
    T = LocTables(eng, SMALL)
    try:
        rc, got = abi_loader(eng, T, [b"I:5\nI:6\n"], 4, base=[2147483646, 0, 0, 0])
        assert rc == 0 and got["next"][0] == 2147483647 and b"rg:ctg:I:1:2147483647\t" in got["text"]
        assert abi_loader(eng, T, [b"I:5\nI:6\n", b"I:7\nI:8\n"], 4, base=[2147483646, 0, 0, 0])[0] == _lib.EINVAL
        assert abi_loader(eng, T, [b"I:5\nI:6\n"], 4, base=[-1, 0, 0, 0])[0] == _lib.EINVAL
        rc, got = abi_loader(eng, T, [b"I:5\nI:6\n"], 4)                 # a call after a refused call works
        assert rc == 0 and got["text"] == b'rg:ctg:I:1:1\t{"id":"rg:ctg:I:1:1","range":"I:6"}\n'
    finally:
        T.close()
    with pytest.raises(host.HostError):
        host.loader_text(eng, SMALL, [b"I:5\nI:6\nI:7\n"], serial_base={"ctg:I:1": 2147483646})


def test_id_and_json_lengths_cross_a_digit(eng):
    """RESP prints both lengths: an id of 9 -> 10 and 99 -> 100 bytes, a JSON of 99 -> 100 bytes"""
    short = [dict(id="c", chr_id="I", chr_start=1, chr_end=1000, seq=b""),
             dict(id="d" * 90, chr_id="II", chr_start=1, chr_end=1000, seq=b"")]
    files = [b"I:5\nI:6\nI:7\nI:8\nII:5\nII:6\nII:7\nII:8\n"]
    want = check_loader(eng, short, files, RG, "", RESP, base={"c": 9997, "d" * 90: 99997})
    for n in (9, 10, 99, 100):
        assert b"$%d\r\nrg:" % n in want["text"]
    names = b"".join(b"n" * k + b".I:5\n" for k in range(58, 75))
    want = check_loader(eng, short, [b"I:2\n" + names], RG, "", RESP)
    assert b"$99\r\n{" in want["text"] and b"$100\r\n{" in want["text"]
    check_loader(eng, short, [b"I:2\n" + names], FEATURE, "t", RESP)


# ---- the range text -------------------------------------------------------------------------------
def test_ranges_are_canonical_not_echoed(eng):
    data = b"I:2\nI:5\nI:5-5\nI:007_9 \nI:9-5\nI:5--_9\r\n.I:5\nI():6\nnm.I:7\n"
    for kind, fmt in ((RG, RECORDS), (FEATURE, RECORDS), (FEATURE, TSV), (FEATURE, RESP)):
        want = check_loader(eng, SMALL, [data], kind, "tag", fmt)
        assert host_one_file(eng, SMALL, data, kind, "tag", fmt) == want["text"]
    rows = model_loader(locator_order(SMALL), [data], FEATURE, "tag", TSV)["text"].decode().splitlines()
    assert [r.split("\t")[1:3] for r in rows] == [["I:5", "1"], ["I:5", "1"], ["I:7-9", "3"], ["I:9-5", "-3"], ["I:5-9", "5"],
                                                   ["I:5", "1"], ["I:6", "1"], ["nm.I:7", "1"]]


def test_names_and_strands_are_escaped_in_json_only(eng):
    data = b'I:2\nq"uo\\te(.I:5\nI(+):6\nI(-):7\nI("):8\n\\".I(\\):9\n'
    for kind, fmt in ((RG, RECORDS), (RG, TSV), (FEATURE, RESP)):
        want = check_loader(eng, SMALL, [data], kind, 'a"b\\c', fmt)
        assert host_one_file(eng, SMALL, data, kind, 'a"b\\c', fmt) == want["text"]
    assert b'"range":"q\\"uo\\\\te(.I:5"' in check_loader(eng, SMALL, [data])["text"]


def test_a_tab_in_a_kept_name_is_refused_and_the_host_answers(eng):
    data = b"I:2\nna\tme.I:5-9\nI:20\n"
    T = LocTables(eng, SMALL)
    try:
        assert abi_loader(eng, T, [data], 4)[0] == _lib.EUNSUPPORTED
        assert abi_loader(eng, T, [b"na\tme.I:5-9\nI:20\n"], 4)[0] == 0          # the dropped line is never looked at
        rc, got = abi_loader(eng, T, [b"I:2\nI:20\n"], 4)                        # a call after a refused call works
        assert rc == 0 and got["n_rows"] == 1
    finally:
        T.close()
    order = locator_order(SMALL)
    ml = model_loader(order, [data, b"I:30\nI:31\n"], FEATURE, "t", RESP, [7, 0, 0, 0])
    text, nxt, per = host.loader_text(eng, SMALL, [data, b"I:30\nI:31\n"], "feature", "t", "resp", {"ctg:I:1": 7})
    assert host.last_operator_device() == 0
    assert text == host_order_text(order, ml) and nxt["ctg:I:1"] == 10 and per == [2, 1]


# ---- the tag --------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["", 'q"uote', "back\\slash", "a b,c:{}"])
def test_tags(eng, tag):
    data = b"I:2\nI:5-9\nII:3\nII:4\n"
    for fmt in (RECORDS, TSV, RESP):
        want = check_loader(eng, SMALL, [data], FEATURE, tag, fmt)
        assert host_one_file(eng, SMALL, data, FEATURE, tag, fmt) == want["text"]
    assert check_loader(eng, SMALL, [data], RG, tag)["text"] == check_loader(eng, SMALL, [data], RG, "")["text"]


def test_a_tag_with_a_high_or_control_byte_is_refused(eng):
    data = b"I:2\nI:5-9\n"
    T = LocTables(eng, SMALL)
    try:
        for tag in (b"caf\xe9", b"a\tb", b"a\0b"):
            assert abi_loader(eng, T, [data], 4, FEATURE, tag)[0] == _lib.EUNSUPPORTED
            assert abi_loader(eng, T, [data], 4, RG, tag)[0] == 0               # the rg records have no tag
    finally:
        T.close()
    check_loader(eng, SMALL, [data], FEATURE, "caf\xe9", RECORDS, device=0)


# ---- the writer -----------------------------------------------------------------------------------
def test_a_row_beyond_the_lds_stage(eng):
    long_name = b"n" * 60000
    data = b"I:2\n" + b"".join(b"I:%d\n" % k for k in range(2, 300)) + long_name + b'".I(+):7-9\n' + \
        b"".join(b"I:%d\n" % k for k in range(300, 600))
    for fmt in (RECORDS, RESP):
        want = check_loader(eng, SMALL, [data, data], FEATURE, "long", fmt)
        assert want["n_rows"] == 2 * 599 and len(want["text"]) > 120000


def test_text_off_where_the_callers_order_is_not_id_order(eng):
    ctgs = [ctg("II", 1, 1, 5000), ctg("I", 3, 3000, 9000), ctg("I", 1, 1, 1000), ctg("I", 2, 1001, 2000)]
    order = locator_order(ctgs)
    assert [c["id"] for c in order] == ["ctg:I:3", "ctg:I:1", "ctg:I:2", "ctg:II:1"]
    files = [b"II:2\nI:3001\nI:5\nI:1500\nII:7\nI:3500\nI:6\nI:1600\nI:1700\n", b"I:7\nI:8\nII:9\nII:10\nII:11\n"]
    want = check_loader(eng, ctgs, files, base={"ctg:I:2": 40})
    assert np.diff(want["off"]).tolist() == [len(r) for f in want["rows"] for r in f]
    assert [r.count(b"\n") for f in want["rows"] for r in f] == [1, 1, 2, 1, 0, 1, 0, 2]
    text = host.loader_text(eng, ctgs, files, serial_base={"ctg:I:2": 40})[0].decode()
    assert [ln.split("\t")[0] for ln in text.splitlines()] == [
        "rg:ctg:I:1:1", "rg:ctg:I:2:41", "rg:ctg:I:2:42", "rg:ctg:I:3:1", "rg:ctg:II:1:1", "rg:ctg:I:1:2", "rg:ctg:II:1:2",
        "rg:ctg:II:1:3"]


# ---- the index ------------------------------------------------------------------------------------
def test_index_of_one_file_is_the_one_file_entry(eng, s288c):
    ctgs = all_ctgs(s288c)
    order = locator_order(ctgs)
    data = read_bytes("spo11_hot.rg")
    T = LocTables(eng, ctgs)
    try:
        rc1, ix1, grp1, kept1 = abi_index(eng, T, data, len(order))
        rc2, ix2, grp2, kept2 = abi_index_files(eng, T, [data], len(order))
        assert rc1 == 0 and rc2 == 0 and kept1 == kept2 == 69 and np.array_equal(grp1, grp2)
        ms, n = (C.c_float * 16)(), C.c_uint32()
        _ok(eng, L.gams_gpu_last_stage_ms(eng.h, ms, 16, C.byref(n)))
        assert n.value == 9
        rng = np.random.default_rng(3)
        g = rng.integers(0, len(order), 2000)
        qs = rng.integers(0, 250000, 2000)
        qe = qs + rng.integers(0, 20000, 2000)
        assert np.array_equal(abi_count(eng, ix1, g, qs, qe), abi_count(eng, ix2, g, qs, qe))
        L.gams_index_destroy(eng.h, ix1)
        L.gams_index_destroy(eng.h, ix2)
    finally:
        T.close()


def test_index_over_two_and_three_golden_files(eng, s288c):
    ctgs = all_ctgs(s288c)
    a, b = read_bytes("spo11_hot.rg"), read_bytes("SK1.snp.rg")
    per2 = check_index(eng, ctgs, [a, b])
    per3 = check_index(eng, ctgs, [b, a[:-1], b])
    assert sum(map(len, per3)) == sum(map(len, per2)) + sum(map(len, check_index(eng, ctgs, [b])))


def test_rg_data_as_a_list_equals_rg_records_per_file(eng, s288c):
    ctgs = all_ctgs(s288c)
    a, b = read_bytes("spo11_hot.rg"), read_bytes("SK1.snp.rg")
    recs = host.read_range(eng, ctgs, helpers.read_lines("spo11_hot.rg")) + host.read_range(eng, ctgs, helpers.read_lines("SK1.snp.rg"))
    q = read_bytes("spo11_hot.rg")
    want = host.locate_text(eng, ctgs, q, count=True, rg_records=recs)
    assert want.count(b"\n") > 50
    assert host.locate_text(eng, ctgs, q, count=True, rg_data=[a, b]) == want
    assert host.locate_text(eng, ctgs, q, count=True, rg_data=(a, b"", b)) == want
    assert host.locate(eng, ctgs, helpers.read_lines("spo11_hot.rg"), count=True, rg_data=[a, b]).encode() == want
    assert host.locate_text(eng, ctgs, q, count=True, rg_data=[a]) == host.locate_text(eng, ctgs, q, count=True, rg_data=a)
    feats = b"I:1000-3000\nI:20000-24000\nI:50000-50500\nI:150000-151000\nI:152000-153000\nMito:1000-2000\nMito:3000-4000\n"
    want = host.sw_text(eng, ctgs, feats, actions=("count",), rg_records=recs)
    assert want.count(b"\n") > 100
    assert host.sw_text(eng, ctgs, feats, actions=("count",), rg_data=[a, b]) == want
    by_id = sorted(ctgs, key=lambda c: c["id"])
    flist = [[(f"feature:{c['id']}:1", c["chr_start"] + 500, c["chr_start"] + 2500)] for c in by_id]
    want = host.sw_multi([eng], by_id, flist, actions=("gc", "count"), rg_records=recs)
    assert host.sw_multi([eng], by_id, flist, actions=("gc", "count"), rg_data=[a, b]) == want
    c0 = by_id[0]
    assert host.sw(eng, c0, flist[0], actions=("gc", "count"), rg_data=[a, b]) == \
        host.sw(eng, c0, flist[0], actions=("gc", "count"), rg_records=recs)


# ---- goldens --------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [RECORDS, TSV, RESP])
@pytest.mark.parametrize("kind", [RG, FEATURE])
def test_both_goldens_in_one_load(eng, s288c, kind, fmt):
    ctgs = all_ctgs(s288c)
    a, b = read_bytes("spo11_hot.rg"), read_bytes("SK1.snp.rg")
    want = check_loader(eng, ctgs, [a, b], kind, "hot", fmt)
    assert want["per_file"][0] == 69 and want["n_rows"] > 1000
    one = check_loader(eng, ctgs, [a], kind, "hot", fmt)
    assert one["n_rows"] == 69
    text = host.loader_text(eng, ctgs, [a], KIND[kind], "hot", FMT[fmt])[0]
    assert text == host_one_file(eng, ctgs, a, kind, "hot", fmt)


def test_stage_stopwatch(eng):
    files = split_lines(three_ctg_file(513, seed=9), (200,))
    T = LocTables(eng, SMALL)
    try:
        rc, got = abi_loader(eng, T, files, 4, FEATURE, b"t", RESP)
        assert rc == 0 and got["n_rows"] == 513 - 4
        ms, n = (C.c_float * 16)(), C.c_uint32()
        _ok(eng, L.gams_gpu_last_stage_ms(eng.h, ms, 16, C.byref(n)))
        assert n.value == 10 and all(0.0 <= ms[k] < 1000.0 for k in range(10))
    finally:
        T.close()


# ---- fuzz -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(20))
def test_fuzz(eng, seed):
    """up to 4 files of up to 2,000 lines over up to 40 ctgs, no control bytes: the device answers every case"""
    ctgs, files, kind, tag, fmt, base = fuzz_case(seed)
    check_loader(eng, ctgs, files, kind, tag, fmt, base, device=1)
    check_index(eng, ctgs, files)
