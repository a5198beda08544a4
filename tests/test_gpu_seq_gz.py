"""gams_gpu_seq_gz: the `seq:` values of a resident seqset as gzip members deflated on the device.  The expected value of
every member is the host twin (gams_seq_gz_host, held to account on the CPU by tests/test_seq_gz_cpu.py) over the bases
SeqSet.download brings back; every comparison is byte for byte.  Shapes sit around the block size, not genomes."""
import ctypes as C
import gzip
import os

import numpy as np
import pytest

import helpers
import peak_text as pt
from gams_amd import _lib, engine, host
from test_gpu_peak_text import PeakTables, abi_peak, seq_arrays
from test_gpu_wave_plane import image_of
from test_seq_gz_cpu import fib, masked_dna, member

pytestmark = pytest.mark.gpu

L = _lib.load()
B = _lib.SEQ_GZ_BLOCK
STAGES = 5          # hist, codes, sizes, pack, copy


@pytest.fixture(scope="module")
def eng():
    e = engine.Engine(0)
    yield e
    e.close()


def case_seqs():
    """the members' cases as ctgs: lengths around the block size of masked DNA (odd lengths leave the next member at an
    odd byte, and its first block at every bit of a word), one value repeated, all 256 values, Fibonacci frequencies
    (a literal code that has to be limited), random bytes, and empty ctgs at the front, inside and at the end"""
    rng = np.random.default_rng(11)
    f = fib(17)
    seqs = [b""] + [masked_dna(n, 300 + k) for k, n in enumerate((1, 2, B - 1, B, B + 1, 2 * B + 1, 4096, 4097, 16, 17, 15))]
    seqs += [b"", b"G" * 1000, b"\x00" * (B + 5), bytes(range(256)), bytes(range(256)) * 300,
             b"".join(bytes([i * 3]) * c for i, c in enumerate(f)), rng.integers(0, 256, 3 * B + 77, dtype=np.uint8).tobytes(),
             b"A" * B + b"\xff" * 10, masked_dna(5 * B + 4099, 4), b""]
    return seqs


@pytest.fixture(scope="module")
def cases(eng):
    seqs = case_seqs()
    ss = engine.SeqSet(eng, seqs)
    want = [member(s) for s in seqs]            # computed once, shared, never changed
    yield ss, seqs, want
    ss.close()


def split(data, off):
    assert off[0] == 0 and int(off[-1]) == len(data)
    return [data[int(off[i]):int(off[i + 1])] for i in range(len(off) - 1)]


def stage_ms(eng):
    ms, n = (C.c_float * 16)(), C.c_uint32()
    rc = L.gams_gpu_last_stage_ms(eng.h, ms, 16, C.byref(n))
    return rc, list(ms[:n.value])


def test_device_members_equal_the_host_twin(eng, cases):
    ss, seqs, want = cases
    data, off = engine.seq_gz(eng, ss, 0, len(seqs))
    got = split(data, off)
    for i, (g, w, s) in enumerate(zip(got, want, seqs)):
        assert ss.download(i) == s
        assert g == w, (i, len(s), len(g), len(w))
        assert gzip.decompress(g) == s
    rc, ms = stage_ms(eng)
    assert rc == 0 and len(ms) == STAGES and all(m >= 0 for m in ms)
    # two calls return identical bytes
    again, off2 = engine.seq_gz(eng, ss, 0, len(seqs))
    assert again == data and np.array_equal(off, off2)


@pytest.mark.parametrize("first,count", [(0, 1), (2, 3), (5, 4), (12, 1), (12, 2), (21, 1), (21, 0), (22, 0), (0, 0), (6, 16)])
def test_sub_ranges(eng, cases, first, count):
    ss, seqs, want = cases
    assert len(seqs) == 22
    data, off = engine.seq_gz(eng, ss, first, count)
    assert split(data, off) == want[first:first + count]
    if count == 0:
        assert stage_ms(eng)[0] == _lib.ESTATE          # nothing ran


def test_one_ctg_and_hundreds_of_tiny_ones(eng):
    one = masked_dna(2 * B + 300, 77)
    ss = engine.SeqSet(eng, [one])
    try:
        data, off = engine.seq_gz(eng, ss, 0, 1)
        assert data == member(one) and list(off) == [0, len(data)]
    finally:
        ss.close()
    rng = np.random.default_rng(3)
    tiny = [masked_dna(int(n), 500 + k) for k, n in enumerate(rng.integers(0, 70, 400))]
    assert sum(1 for t in tiny if not t) >= 2
    ss = engine.SeqSet(eng, tiny)
    try:
        data, off = engine.seq_gz(eng, ss, 0, len(tiny))
        got = split(data, off)
        assert got == [member(t) for t in tiny]
        assert [gzip.decompress(g) for g in got] == tiny
        assert host.seq_gz(eng, ss) == got and host.seq_gz(eng, ss, 390) == got[390:] and host.seq_gz(eng, ss, 7, 2) == got[7:9]
    finally:
        ss.close()


def resp_walk(buf):
    """[(key, value)] of a stream of three-argument SET commands, every length and terminator checked"""
    at, out = 0, []

    def line():
        nonlocal at
        end = buf.index(b"\r\n", at)
        s = buf[at:end]
        at = end + 2
        return s

    def bulk():
        nonlocal at
        head = line()
        assert head[:1] == b"$" and head[1:].isdigit()
        n = int(head[1:])
        s = buf[at:at + n]
        assert len(s) == n and buf[at + n:at + n + 2] == b"\r\n"
        at += n + 2
        return s

    while at < len(buf):
        assert line() == b"*3"
        assert bulk() == b"SET"
        key = bulk()
        out.append((key, bulk()))
    assert at == len(buf)
    return out


def test_resp_stream(eng, cases):
    ss, seqs, want = cases
    ids = [f"ctg:{'I' if i % 3 else 'chr2_x:y'}:{i * 37 + 1}" for i in range(len(seqs))]
    assert len(set(ids)) == len(ids)
    data, off = engine.seq_gz(eng, ss, 0, len(seqs), _lib.LOADER_RESP, ids)
    units = split(data, off)
    recs = resp_walk(data)
    assert [k for k, _ in recs] == [b"seq:" + i.encode() for i in ids]
    assert [v for _, v in recs] == want
    for u, i, w in zip(units, ids, want):               # every unit is the command of its slot
        assert resp_walk(u) == [(b"seq:" + i.encode(), w)]
        assert u == host.resp_command([b"SET", b"seq:" + i.encode(), w])
    # a sub-range takes its ids by position: entry i names slot first + i
    data, off = engine.seq_gz(eng, ss, 4, 3, _lib.LOADER_RESP, ids[4:7])
    assert resp_walk(data) == list(zip([b"seq:" + i.encode() for i in ids[4:7]], want[4:7]))
    assert host.seq_records(eng, ss, [dict(id=i) for i in ids]) == b"".join(units)


def test_round_trip_on_the_golden_genome(eng):
    with gzip.open(os.path.join(helpers.S288C, "genome.fa.gz"), "rb") as fh:
        fasta = fh.read()
    ctgs, _, ss = host.gen_text(eng, fasta, piece=100000)
    try:
        assert host.last_operator_device() == 1 and len(ctgs) == 3
        members = host.seq_gz(eng, ss)
        bases = [ss.download(i) for i in range(len(ctgs))]
        assert [gzip.decompress(m) for m in members] == bases
        assert members == [member(b) for b in bases]
        assert sum(map(len, members)) <= sum(len(host.encode_gz(b)) for b in bases)
        from_gz, _ = host.wave_gz(eng, [dict(c, gz=m) for c, m in zip(ctgs, members)])
        plain = host.wave(eng, [dict(c, seq=b) for c, b in zip(ctgs, bases)])
        assert from_gz.decode() == plain and plain.count("\n") > 100
        recs = resp_walk(host.seq_records(eng, ss, ctgs))
        assert recs == [(b"seq:" + c["id"].encode(), m) for c, m in zip(ctgs, members)]
    finally:
        ss.close()


def raw_call(eng, ss, first, count, fmt, nm=None):
    out, n = C.c_void_p(), C.c_uint64()
    off = np.zeros(count + 1 if count < 1 << 20 else 2, np.uint64)
    return L.gams_gpu_seq_gz(eng.h, ss.p if ss is not None else None, first, count, nm, fmt, C.byref(out), C.byref(n),
                             off.ctypes.data)


def test_return_codes_leave_the_handle_usable(eng, cases):
    ss, seqs, want = cases
    n = len(seqs)
    M, R = _lib.SEQ_GZ_MEMBERS, _lib.LOADER_RESP
    assert raw_call(eng, ss, n + 1, 0, M) == _lib.EINVAL
    assert raw_call(eng, ss, 0, n + 1, M) == _lib.EINVAL
    assert raw_call(eng, ss, n - 1, 2, M) == _lib.EINVAL
    assert raw_call(eng, ss, 3, 0xffffffff, M) == _lib.EINVAL        # first + count wraps
    for fmt in (_lib.LOADER_RECORDS, _lib.LOADER_TSV, 4, -1):
        assert raw_call(eng, ss, 0, 1, fmt) == _lib.EINVAL
    assert raw_call(eng, ss, 0, 2, R) == _lib.EINVAL                 # the SET stream without names
    assert raw_call(eng, None, 0, 1, M) == _lib.EINVAL
    nm = C.c_void_p()
    eng.check(L.gams_names_create(eng.h, 1, (C.c_char_p * 1)(b"ctg:I:1"), C.byref(nm)))
    try:
        assert raw_call(eng, ss, 0, 2, R, nm) == _lib.EINVAL         # fewer names than slots
        assert raw_call(eng, ss, 0, 1, R, nm) == _lib.OK
    finally:
        L.gams_names_destroy(eng.h, nm)
    arrs = [np.frombuffer(s, np.uint8) for s in (b"ACGT" * 100, b"GGCC" * 33)]
    po = engine.SeqSet(eng, arrs, upload=False)
    try:
        off, img, plane = image_of(po, arrs)
        po.upload_ranges(None, plane, 0, int(off[-1]) + arrs[-1].size)
        assert raw_call(eng, po, 0, 2, M) == _lib.ESTATE
    finally:
        po.close()
    data, off = engine.seq_gz(eng, ss, 0, n)
    assert split(data, off) == want


def test_other_entries_texts_stay_valid_across_a_call(eng, cases):
    """the bytes belong to this entry alone: a text of gams_gpu_peak_text fetched before is unchanged behind it, and
    this entry's own pointer is what its next call reuses"""
    ss, seqs, want = cases
    ctgs = pt.synth_ctgs()
    data = pt.synth_data(pt.synth_lines(ctgs))
    pss = engine.SeqSet(eng, seq_arrays(ctgs))
    T = PeakTables(eng, ctgs)
    try:
        text, nb, rows = C.c_void_p(), C.c_uint64(), C.c_uint64()
        off = np.zeros(len(T.order) + 1, np.uint64)
        eng.check(L.gams_gpu_peak_text(eng.h, pss.p, T.ix, T.chr, T.ids, T.slot.ctypes.data, T.cs.ctypes.data,
                                       T.ce.ctypes.data, data, len(data), C.byref(text), C.byref(nb), off.ctypes.data,
                                       C.byref(rows)))
        before = C.string_at(text, nb.value)
        assert rows.value > 100
        members, moff = engine.seq_gz(eng, ss, 0, len(seqs))
        assert split(members, moff) == want
        assert C.string_at(text, nb.value) == before
        assert abi_peak(eng, T, pss, data)[1] == before
        again, _ = engine.seq_gz(eng, ss, 0, len(seqs))
        assert again == members
    finally:
        T.close()
        pss.close()


def test_block_size_knob_matches_the_host_twin(eng):
    """gams_gpu_seq_gz_set_block (the measurement knob of gams_gpu_diag.h): other block sizes, the same agreement"""
    seqs = [masked_dna(70000, 8), b"", masked_dna(4096 * 3, 9), masked_dna(4096 * 3 + 1, 10)]
    e2 = engine.Engine(0)
    ss = engine.SeqSet(e2, seqs)
    try:
        assert L.gams_gpu_seq_gz_set_block(e2.h, 1000) == _lib.EINVAL
        for block in (4096, 65536):
            e2.check(L.gams_gpu_seq_gz_set_block(e2.h, block))
            data, off = engine.seq_gz(e2, ss, 0, len(seqs))
            assert split(data, off) == [member(s, block) for s in seqs]
    finally:
        ss.close()
        e2.close()
