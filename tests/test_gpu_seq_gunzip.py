"""gams_seqset_upload_gz and the indexed writer of gams_gpu_seq_gz: the indexed members equal the host twin byte for
byte; uploaded again they inflate on the device into the slots of a seqset, bases and G/C plane; whatever is not an
intact indexed member is FOREIGN and goes the host's way, and nothing outside a taken slot is written.  Every damaged
member here has been through the host twin of the decoder (tests/test_seq_gz_index_cpu.py, also under the sanitizers)."""
import ctypes as C
import gzip
import os
import zlib

import numpy as np
import pytest

import helpers
import seq_gz_index as gi
from gams_amd import _lib, engine, host
from seq_gz_index import B, CHUNK, damaged, gunzip_host, imember
from test_gpu_host import HEADER
from test_gpu_seq_gz import resp_walk, split, stage_ms
from test_gpu_wave_plane import image_of
from test_seq_gz_cpu import masked_dna, member

pytestmark = pytest.mark.gpu

L = _lib.load()
DONE, FOREIGN = _lib.SEQ_GZ_DONE, _lib.SEQ_GZ_FOREIGN
IDX = _lib.SEQ_GZ_INDEXED
STAGES = 4          # upload, tables, decode, join


@pytest.fixture(scope="module")
def eng():
    e = engine.Engine(0)
    yield e
    e.close()


def case_seqs(block):
    """the CPU list as ctgs, with empty ctgs at the front, inside and at the end"""
    seqs = [d for _, d in gi.case_inputs(block)]
    return [b""] + seqs[:9] + [b""] + seqs[9:] + [masked_dna(3 * block + 4099, 4), b""]


@pytest.fixture(scope="module")
def cases(eng):
    seqs = case_seqs(B)
    ss = engine.SeqSet(eng, seqs)
    want = [imember(s) for s in seqs]            # computed once, shared, never changed
    yield ss, seqs, want
    ss.close()


def gc_plane(s):
    a = np.frombuffer(s, np.uint8)
    out = np.zeros((a.size + 7) // 8, np.uint8)
    if a.size:
        assert L.gams_gc_plane(a.ctypes.data, a.size, out.ctypes.data) == _lib.OK
    return out.tobytes()


def upload_gz(eng, ss, first, members):
    """the raw entry -> (rc, statuses, n_foreign)"""
    n = len(members)
    bufs = [np.frombuffer(bytes(m), np.uint8) for m in members]
    ptrs = (C.c_void_p * max(n, 1))(*[b.ctypes.data if b.size else None for b in bufs])
    lens = np.array([b.size for b in bufs], np.uint64)
    st = np.full(max(n, 1), 77, np.uint8)
    nf = C.c_uint32(12345)
    rc = L.gams_seqset_upload_gz(eng.h, ss.p, first, n, ptrs, lens.ctypes.data, st.ctypes.data, C.byref(nf))
    return rc, st[:n].tolist(), nf.value


def test_indexed_writer_equals_the_host_twin(eng, cases):
    ss, seqs, want = cases
    data, off = engine.seq_gz(eng, ss, 0, len(seqs), _lib.SEQ_GZ_MEMBERS | IDX)
    got = split(data, off)
    for i, (g, w, s) in enumerate(zip(got, want, seqs)):
        assert g == w, (i, len(s), len(g), len(w))
        assert gzip.decompress(g) == s
    for first, count in [(0, 1), (3, 4), (10, 2), (len(seqs) - 1, 1), (len(seqs), 0), (5, len(seqs) - 5)]:
        data, off = engine.seq_gz(eng, ss, first, count, _lib.SEQ_GZ_MEMBERS | IDX)
        assert split(data, off) == want[first:first + count]
    # without the bit every byte is what it was
    data, off = engine.seq_gz(eng, ss, 0, len(seqs))
    assert split(data, off) == [member(s) for s in seqs]
    assert host.seq_gz(eng, ss, 2, 5, indexed=True) == want[2:7]
    # the SET stream frames the same members
    ids = ["ctg:I:%d" % (i * 7 + 1) for i in range(len(seqs))]
    data, off = engine.seq_gz(eng, ss, 0, len(seqs), _lib.LOADER_RESP | IDX, ids)
    assert resp_walk(data) == [(b"seq:" + i.encode(), w) for i, w in zip(ids, want)]
    assert host.seq_records(eng, ss, [dict(id=i) for i in ids], indexed=True) == data


def test_indexed_writer_at_block_4096_and_other_chunks():
    seqs = case_seqs(4096)
    e2 = engine.Engine(0)
    ss = engine.SeqSet(e2, seqs)
    try:
        e2.check(L.gams_gpu_seq_gz_set_block(e2.h, 4096))
        data, off = engine.seq_gz(e2, ss, 0, len(seqs), _lib.SEQ_GZ_MEMBERS | IDX)
        members = split(data, off)
        assert members == [imember(s, 4096) for s in seqs]
        data, off = engine.seq_gz(e2, ss, 4, 9, _lib.SEQ_GZ_MEMBERS | IDX)
        assert split(data, off) == members[4:13]
        assert L.gams_gpu_seq_gz_set_chunk(e2.h, 100) == _lib.EINVAL
        for block, chunk in ((8192, 512), (65536, 1024), (32768, 4096)):
            e2.check(L.gams_gpu_seq_gz_set_block(e2.h, block))
            e2.check(L.gams_gpu_seq_gz_set_chunk(e2.h, chunk))
            data, off = engine.seq_gz(e2, ss, 0, len(seqs), _lib.SEQ_GZ_MEMBERS | IDX)
            other = split(data, off)
            assert other == [imember(s, block, chunk) for s in seqs]
            # ... and the decoder reads block and chunk from the member
            back = engine.SeqSet(e2, seqs, upload=False)
            try:
                rc, st, nf = upload_gz(e2, back, 0, other)
                assert (rc, nf) == (_lib.OK, 0) and st == [DONE] * len(seqs)
                assert [back.download(i) for i in range(len(seqs))] == seqs
            finally:
                back.close()
    finally:
        ss.close()
        e2.close()


def test_round_trip_into_a_fresh_seqset(eng, cases):
    ss, seqs, want = cases
    back = engine.SeqSet(eng, seqs, upload=False)
    try:
        rc, st, nf = upload_gz(eng, back, 0, want)
        assert (rc, nf) == (_lib.OK, 0) and st == [DONE] * len(seqs)
        rc, ms = stage_ms(eng)
        assert rc == 0 and len(ms) == STAGES and all(m >= 0 for m in ms)
        for i, s in enumerate(seqs):
            assert back.download(i) == s, i
            assert back.download(i, plane=True) == gc_plane(s), i
        data, off = engine.seq_gz(eng, back, 0, len(seqs), _lib.SEQ_GZ_MEMBERS | IDX)
        assert split(data, off) == want
        # a sub-range of slots
        rc, st, nf = upload_gz(eng, back, 3, want[3:8])
        assert (rc, st, nf) == (_lib.OK, [DONE] * 5, 0)
        assert [back.download(i) for i in range(len(seqs))] == seqs
    finally:
        back.close()


def test_wave_on_the_golden_chromosome_from_gz(eng):
    genome = helpers.load_s288c()
    ctgs = helpers.gen_ctgs("I", genome["I"])
    golden = "\n".join(helpers.read_lines("I.peaks.tsv")) + "\n"
    members = [host.encode_gz_fast(c["seq"], indexed=True) for c in ctgs]
    ss = engine.SeqSet.from_gz(eng, members)
    try:
        assert ss.went == (len(ctgs), 0) and list(ss.lengths) == [len(c["seq"]) for c in ctgs]
        bases = [ss.download(i) for i in range(len(ctgs))]
        assert bases == [bytes(c["seq"]) for c in ctgs]
        assert HEADER + host.wave(eng, [dict(c, seq=b) for c, b in zip(ctgs, bases)]) == golden
    finally:
        ss.close()
    by_device, _ = host.wave_gz(eng, [dict(c, gz=m) for c, m in zip(ctgs, members)], inflate="device")
    by_host, _ = host.wave_gz(eng, [dict(c, gz=m) for c, m in zip(ctgs, members)])
    assert HEADER + by_device.decode() == golden and by_host == by_device


def zlib_gives(v):
    try:
        d = zlib.decompressobj(31)
        out = d.decompress(v) + d.flush()
        return out if d.eof else None
    except zlib.error:
        return None


def pattern(n, k):
    return bytes((np.arange(n, dtype=np.uint32) * 7 + k).astype(np.uint8) | 0x80)


def test_mixed_batch_keeps_what_it_does_not_take(eng):
    data = masked_dna(2 * B + 5000, 21)
    good, bad = damaged(data)
    for name, v in bad:                                   # only what the CPU twin has refused goes to the device
        assert gunzip_host(v)[:2] == (_lib.OK, FOREIGN), name
    # behind every damaged member a slot whose content is checked: in turn an intact indexed member (DONE) and a plain
    # one (refused on the host: its slot keeps the pattern), so that every device-refused slot has checked neighbours
    small = [masked_dna(n, 40 + n) for n in (5000, 1, 70000)]
    members, truth = [imember(small[0]), good], [small[0], data]
    for k, (name, v) in enumerate(bad):
        between = masked_dna(300 + 17 * k, 60 + k)
        members += [v, imember(between) if k % 2 == 0 else member(between)]
        truth += [data, between]
    members += [imember(small[1]), member(small[2]), imember(small[2])]
    truth += [small[1], small[2], small[2]]
    host_refused = [gunzip_host(v)[3] == 0 for v in members]          # the O(1) checks already fail: n_out = 0
    twin = [gunzip_host(v)[1] for v in members]
    refused = [i for i in range(len(truth)) if twin[i] == FOREIGN and not host_refused[i]]
    assert sum(host_refused) >= 10 and twin.count(DONE) == 10 and len(refused) == 6
    ss = engine.SeqSet(eng, truth, upload=False)
    try:
        fill = [pattern(len(t), i) for i, t in enumerate(truth)]
        for i, f in enumerate(fill):
            ss.upload(i, f)
        planes = [ss.download(i, plane=True) for i in range(len(truth))]
        rc, st, nf = upload_gz(eng, ss, 0, members)
        assert rc == _lib.OK and st == twin and nf == twin.count(FOREIGN)
        checked = set()
        for i, t in enumerate(truth):
            if st[i] == DONE:
                assert ss.download(i) == t and ss.download(i, plane=True) == gc_plane(t), i
                checked.add(i)
            elif host_refused[i]:
                assert ss.download(i) == fill[i] and ss.download(i, plane=True) == planes[i], i
                checked.add(i)
        for i in refused:                                 # both neighbours of every device-refused slot are intact
            assert i - 1 in checked and i + 1 in checked, i
    finally:
        ss.close()
    # the host level takes the same batch -- but for what no inflater takes: those values are its error -- and ends with
    # every slot right, by either route
    readable = [i for i, v in enumerate(members) if zlib_gives(v) == truth[i]]
    on_device = [twin[i] for i in readable].count(DONE)
    assert len(readable) == len(members) - 5 and on_device == 10 and len(readable) - on_device >= 10
    ss = engine.SeqSet.from_gz(eng, [members[i] for i in readable])
    try:
        assert ss.went == (on_device, len(readable) - on_device)
        assert [ss.download(k) for k in range(len(readable))] == [truth[i] for i in readable]
        assert [ss.download(k, plane=True) for k in range(len(readable))] == [gc_plane(truth[i]) for i in readable]
    finally:
        ss.close()
    with pytest.raises(host.HostError):
        engine.SeqSet.from_gz(eng, [members[0], dict(bad)["body_bit"]]).close()


def test_argument_checks(eng, cases):
    ss, seqs, want = cases
    n = len(seqs)
    back = engine.SeqSet(eng, seqs, upload=False)
    try:
        assert upload_gz(eng, back, 0, want)[0] == _lib.OK
        wrong = list(want)
        wrong[5] = want[6]                                # an intact member of another length
        assert len(seqs[5]) != len(seqs[6])
        rc, _, _ = upload_gz(eng, back, 0, wrong)
        assert rc == _lib.EINVAL and b"slot 5" in L.gams_gpu_last_error(eng.h)
        assert [back.download(i) for i in range(n)] == seqs
        assert upload_gz(eng, back, n, want[:1])[0] == _lib.EINVAL
        assert upload_gz(eng, back, 1, want)[0] == _lib.EINVAL
        st, nf = np.zeros(1, np.uint8), C.c_uint32()
        assert L.gams_seqset_upload_gz(eng.h, back.p, 3, 0xffffffff, None, None, st.ctypes.data, C.byref(nf)) == _lib.EINVAL
        assert L.gams_seqset_upload_gz(eng.h, back.p, 0, 1, None, None, st.ctypes.data, C.byref(nf)) == _lib.EINVAL
        nf.value = 9
        assert L.gams_seqset_upload_gz(eng.h, back.p, 2, 0, None, None, None, C.byref(nf)) == _lib.OK and nf.value == 0
        assert upload_gz(eng, back, n, [])[0] == _lib.OK
    finally:
        back.close()
    arrs = [np.frombuffer(s, np.uint8) for s in (b"ACGT" * 100, b"GGCC" * 33)]
    po = engine.SeqSet(eng, arrs, upload=False)
    try:
        off, img, plane = image_of(po, arrs)
        po.upload_ranges(None, plane, 0, int(off[-1]) + arrs[-1].size)
        assert upload_gz(eng, po, 0, [imember(a.tobytes()) for a in arrs])[0] == _lib.ESTATE
    finally:
        po.close()


def test_two_calls_with_a_pass_between_them(eng):
    """the second call queues behind the pass that reads what the first one wrote"""
    genome = helpers.load_s288c()
    ctgs = helpers.gen_ctgs("I", genome["I"])
    first = [bytes(c["seq"]) for c in ctgs]
    second = [s[::-1] for s in first]
    ss = engine.SeqSet(eng, first, upload=False)
    try:
        assert upload_gz(eng, ss, 0, [imember(s) for s in first])[:2] == (_lib.OK, [DONE] * len(first))
        plan = engine.WavePlan(eng, ss, 100, 10, 100, 3.0, 1.0)
        try:
            plan.run()                                    # queued, not waited for
            assert upload_gz(eng, ss, 0, [imember(s) for s in second])[:2] == (_lib.OK, [DONE] * len(first))
            peaks_first = plan.peaks().copy()
            assert [ss.download(i) for i in range(len(first))] == second
            plan.run()
            peaks_second = plan.peaks().copy()
        finally:
            plan.close()
    finally:
        ss.close()
    ref = engine.SeqSet(eng, first)
    try:
        plan = engine.WavePlan(eng, ref, 100, 10, 100, 3.0, 1.0)
        try:
            plan.run()
            assert np.array_equal(plan.peaks(), peaks_first) and peaks_first.size > 10
            for i, s in enumerate(second):
                ref.upload(i, s)
            plan.run()
            assert np.array_equal(plan.peaks(), peaks_second)
        finally:
            plan.close()
    finally:
        ref.close()


def test_hundreds_of_tiny_ctgs(eng):
    rng = np.random.default_rng(3)
    tiny = [masked_dna(int(n), 500 + k) for k, n in enumerate(rng.integers(0, 70, 400))]
    assert sum(1 for t in tiny if not t) >= 2
    ss = engine.SeqSet.from_gz(eng, [imember(t) for t in tiny])
    try:
        assert ss.went == (400, 0)
        assert [ss.download(i) for i in range(400)] == tiny
        assert [ss.download(i, plane=True) for i in range(400)] == [gc_plane(t) for t in tiny]
    finally:
        ss.close()
