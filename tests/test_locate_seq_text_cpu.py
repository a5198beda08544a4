"""CPU checks behind gams_gpu_locate_seq_text / host.locate_seq_text: the model of tests/locate_seq_text.py against the
reference's pinned answers on the golden S288c ctgs, the new entries' declarations, and the chunk / piece arithmetic of
gams_amd/csrc/seq_text_plan.hpp through the stand-alone driver tests/seq_text_plan_main.cpp (host compiler with the
address and undefined-behaviour sanitizers, no HIP, no device)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import helpers
import locate_seq_text as lst
from gams_amd import _lib, host

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GT, RG, NL_RG, BASES, NL_END = range(5)
ALL_PIECES = 31


def golden_ctgs(s288c):
    ctgs = []
    for chr_id in ("I", "Mito"):
        ctgs += helpers.gen_ctgs(chr_id, s288c[chr_id], piece=100000)
    return ctgs


# ---- the model against the reference's answers ----------------------------------------------------------------------
def test_model_pins_the_reference_answers(s288c):
    """tests/cli.rs:160-171: I:1000-1010 is ATACAATTATA"""
    ctgs = golden_ctgs(s288c)
    assert lst.model(ctgs, b"I:1000-1010\n") == b">I:1000-1010\nATACAATTATA\n"
    assert lst.model(ctgs, b"I:1000-1002\n") == b">I:1000-1002\nATA\n"
    strand = lst.model(ctgs, b"I(+):100001-100010")
    assert strand == b">I(+):100001-100010\n" + s288c["I"][100000:100010] + b"\n"
    assert lst.model(ctgs, b"I:1000-1002\tspo11\t0.5\r\n") == b">I:1000-1002\nATA\n"        # cut at the first tab
    assert lst.model(ctgs, b"II:1000-1100\ngarbage\n\nI:1000-\n") == b""                    # unknown chromosome, garbage
    assert lst.model(ctgs, b"I:100001\n") == b""                                            # a point on a ctg start
    assert lst.model(ctgs, b"I:100002\n") == b">I:100002\n" + s288c["I"][100001:100002] + b"\n"
    four = b"I:1000-1002\nI:1000-1010\nII:1000-1100\nI(+):100001-100010\n"                   # as test_gpu_host.test_locate_seq
    assert lst.model(ctgs, four).split(b"\n")[:-1] == [b">I:1000-1002", b"ATA", b">I:1000-1010", b"ATACAATTATA",
                                                       b">I(+):100001-100010", s288c["I"][100000:100010]]


def test_model_refuses_what_the_reference_panics_on(s288c):
    ctgs = golden_ctgs(s288c)
    for bad in (b"I:100000-100001", b"I:99990-100005", b"I:2000-1000"):     # ctg-spanning (located to the ctg in front), reversed
        with pytest.raises(lst.ModelError) as ei:
            lst.model(ctgs, b"I:5-9\n" + bad + b"\nI:100000-100001\n")
        assert (ei.value.line, ei.value.outside) == (1, True)
    with pytest.raises(lst.ModelError) as ei:
        lst.model([dict(c, seq=None) for c in ctgs], b"II:5\nI:5-9\n")
    assert (ei.value.line, ei.value.outside) == (1, False)


def test_synthetic_input_carries_its_cases():
    ctgs = lst.synth_ctgs()
    lines = lst.synth_lines(ctgs)
    data = lst.synth_data(lines)
    recs = lst.records(ctgs, data)
    assert len(lst.rust_lines(data)) == len(lines) and not data.endswith(b"\n") and b"\r\n" in data
    assert 1200 < len(recs) < len(lines) - len(lst.DROPPED) + 1
    located = {k for k, *_ in recs}
    for k, ln in enumerate(lst.rust_lines(data)):
        assert (ln in lst.DROPPED) == (k not in located), ln
    want = lst.model(ctgs, data)
    assert want.count(b">") >= len(recs)                 # (the sequences hold every byte value, '>' and '\n' too)
    seqs = np.concatenate([np.frombuffer(c["seq"], np.uint8) for c in ctgs])
    assert np.unique(seqs).size == 256
    assert any(e - s + 1 == len(ctgs[i]["seq"]) for _, _, i, s, e in recs)            # a whole ctg
    assert any(b"(" in rg for _, rg, *_ in recs) and any(b"." in rg for _, rg, *_ in recs)
    assert all(c["chr_start"] % 16 != 0 for c in ctgs)
    for n in list(range(9, 300)) + [9999, 10000, 10001, 20000, 20001, 20008, 20009, 50000]:
        assert sum(lst.row_len(ln) for ln in lst.filler(n)) == n
    assert lst.filler(0) == []
    assert len(lst.model(ctgs, b"\n".join(lst.filler(777)))) == 777 and len(lst.model(ctgs, b"\n".join(lst.filler(50000)))) == 50000


# ---- the new entries ------------------------------------------------------------------------------------------------
def test_new_entries_are_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "gams_gpu.h")).read()
    diag = open(os.path.join(ROOT, "include", "gams_gpu_diag.h")).read()
    assert re.search(r"\bint\s+gams_gpu_locate_seq_text\s*\(", hdr)
    assert re.search(r"\buint32_t\s+gams_gpu_locate_seq_chunk\s*\(\s*void\s*\)", diag)
    lib = C.CDLL(_lib.SO_PATH)
    vp, u64p = C.c_void_p, C.POINTER(C.c_uint64)
    assert _lib.PROTOTYPES["gams_gpu_locate_seq_text"] == (C.c_int, [vp, vp, vp, vp, vp, vp, vp, vp, C.c_uint64,
                                                                      C.POINTER(vp), u64p, u64p])
    assert _lib.PROTOTYPES["gams_gpu_locate_seq_chunk"] == (C.c_uint32, [])
    for name in ("gams_gpu_locate_seq_text", "gams_gpu_locate_seq_chunk"):
        assert hasattr(lib, name), name
    assert hasattr(C.CDLL(host.SO_PATH), "gams_host_locate_seq_text")
    assert callable(host.locate_seq_text) and "locate_seq_text" in host.last_operator_device.__doc__


def test_chunk_and_null_arguments():
    lib = _lib.load()
    c = lib.gams_gpu_locate_seq_chunk()
    assert c >= 16 and c % 16 == 0 and c & (c - 1) == 0
    text, nb, rows = C.c_void_p(), C.c_uint64(), C.c_uint64()
    assert lib.gams_gpu_locate_seq_text(None, None, None, None, None, None, None, b"I:1-2\n", 6, C.byref(text), C.byref(nb),
                                        C.byref(rows)) == _lib.EINVAL


# ---- seq_text_plan.hpp ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("seq_text_plan") / "seq_text_plan_main"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           os.path.join(HERE, "seq_text_plan_main.cpp"), "-o", str(exe)])
    return str(exe)


@pytest.fixture(scope="module")
def chunk(driver):
    c = int(subprocess.run([driver, "--chunk"], stdout=subprocess.PIPE, text=True, check=True).stdout)
    assert c == _lib.load().gams_gpu_locate_seq_chunk()
    return c


def run(driver, chunk, sets):
    """every set is a list of rows, None (a line without a row) or (rg_len, n_bases) -> [(total, chunks, runs, begin_mask,
    end_mask)]; a FAIL line of the driver fails here"""
    text = "".join(" ".join("x" if r is None else "%d:%d" % r for r in rows) + "\n" for rows in sets)
    out = subprocess.run([driver], input=text, stdout=subprocess.PIPE, text=True, check=True).stdout.split("\n")[:-1]
    assert len(out) == len(sets)
    res = []
    for rows, ln in zip(sets, out):
        f = ln.split(" ")
        assert f[0] == "ok", (ln, rows[:8])
        total = sum(r[0] + r[1] + 3 for r in rows if r is not None)
        assert int(f[1]) == total and int(f[2]) == -(-total // chunk)
        res.append(tuple(int(v) for v in f[1:]))
    return res


def one_row(total):
    """a row of exactly `total` bytes (>= 3)"""
    return (min(7, total - 3), total - 3 - min(7, total - 3))


def test_plan_random_sets(driver, chunk):
    rng = np.random.default_rng(23)
    sets = []
    for _ in range(40):
        rows = []
        for _ in range(int(rng.integers(1, 400))):
            u = rng.random()
            if u < 0.3:
                rows.append(None)
            elif u < 0.8:
                rows.append((int(rng.integers(0, 20)), int(rng.integers(0, 60))))
            else:
                rows.append((int(rng.integers(0, 40)), int(rng.integers(0, 3 * chunk))))
        sets.append(rows)
    sets.append([None] * 300 + [(5, 9)] + [None] * 700 + [(3, 2 * chunk)] + [None] * 300)      # long runs of lines without rows
    sets.append([None, None, (4, 40), None, (4, 50), None, None])                               # a first and a last row of zero length
    sets.append([None] * 5)                                                                     # no row at all
    sets.append([])
    res = run(driver, chunk, sets)
    assert res[-1][0] == res[-2][0] == 0 and res[-1][1] == 0
    assert all(r[2] >= sum(5 for row in s if row is not None and row[0] and row[1]) for r, s in zip(res, sets))


def test_plan_sizes_at_the_chunk(driver, chunk):
    sets = [[one_row(3)], [one_row(15)], [(0, 0), None, one_row(9)],                            # total < 16
            [one_row(16)], [one_row(chunk)], [one_row(chunk - 1)], [one_row(chunk + 1)],
            [one_row(2 * chunk)], [one_row(chunk - 100), one_row(100)], [one_row(4 * chunk - 50), one_row(50)],
            [one_row(3 * chunk + 5)],                                                           # one row over four chunks
            [(0, 0)] * (2 * chunk),                                                             # 2 C rows of 3 bytes
            [(0, 0)] * (2 * chunk) + [None, (1, 0)]]
    res = run(driver, chunk, sets)
    assert [r[1] for r in res[:7]] == [1, 1, 1, 1, 1, 1, 2]
    assert res[10][1] == 4 and res[10][2] == 5 + 3                   # five pieces, the bases cut three times
    assert res[11][0] == 6 * chunk and res[11][1] == 6 and res[11][2] == 6 * chunk


def test_plan_every_piece_on_a_seam(driver, chunk):
    """every piece ends on a chunk's last byte in one set and begins on a chunk's first byte in another"""
    rg, nb = 11, 40
    row = rg + nb + 3
    # the byte of the row, counted from its start, that is the last one of each piece
    last = {GT: 0, RG: rg, NL_RG: rg + 1, BASES: rg + 1 + nb, NL_END: rg + 2 + nb}
    first = {GT: 0, RG: 1, NL_RG: rg + 1, BASES: rg + 2, NL_END: rg + 2 + nb}
    ends, begins = 0, 0
    for p in range(5):
        lead = chunk - 1 - last[p]                                   # the piece's last byte is byte chunk - 1 of the text
        (r,) = run(driver, chunk, [[one_row(lead), None, (rg, nb), one_row(50)]])
        assert r[4] & (1 << p), (p, r)
        ends |= r[4]
        lead = chunk - first[p]                                      # the piece's first byte is byte `chunk` of the text
        (r,) = run(driver, chunk, [[one_row(lead), (rg, nb), None, one_row(50)]])
        assert r[3] & (1 << p), (p, r)
        begins |= r[3]
    assert ends == ALL_PIECES and begins == ALL_PIECES
