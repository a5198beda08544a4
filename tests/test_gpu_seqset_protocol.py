"""The seqset protocol (common.hpp: gams_seqset_write_begin / write_end / read_begin) through the C ABI: the state every
writer hands to every reader.  One seqset of two ctgs (4,097 and 40,000 bases) holds content A; a writer brings content
B; a reader before and behind it answers for A and for B, bit for bit against its oracle or host twin.  That pins the drop
of the G/C index and the hand-over of `dirty` for every pair.  These are state transitions, which are deterministic: nothing
here tries to catch a race (test_reupload_is_ordered_behind_queued_passes is the ordering test)."""
import ctypes as C
import zlib

import numpy as np
import pytest

import dg_model
import locate_seq_text as lst
from gams_amd import _lib, engine
from oracle import oracle as ora
from test_gpu_dg import TABLE, assert_same_bits, twin
from test_gpu_locate_seq_text import SeqTables, abi_seq
from test_gpu_seq_gunzip import DONE, IDX, upload_gz
from test_gpu_seq_gz import split
from test_gpu_wave_plane import image_of

pytestmark = pytest.mark.gpu

L = _lib.load()
LENS = (4097, 40000)
CHR_START = (1, 50001)
# 1-based (start, end) inside each ctg: first and last base, one base, ranges over 16-B pieces, a long one
RANGES = ([(1, 1), (1, 4097), (4097, 4097), (17, 48), (100, 3000), (4000, 4097)],
          [(1, 40000 - 1), (40000, 40000), (1, 3), (13333, 13340), (13300, 26700), (26600, 26800), (39000, 40000)])


def content(seed):
    rng = np.random.default_rng(seed)
    seqs = [bytearray(dg_model.random_seq(rng, n)) for n in LENS]
    seqs[1][20000] = ord("N")
    return [bytes(s) for s in seqs]


A, B = content(1), content(2)


def ctgs_of(seqs):
    return [dict(id=f"ctg:{c}:1", chr_id=c, chr_start=cs, chr_end=cs + n - 1, seq=s) for c, cs, n, s in zip("ab", CHR_START, LENS, seqs)]


LINES = b"".join(b"%s:%d-%d\n" % (c.encode(), cs + s - 1, cs + e - 1) for c, cs, rl in zip("ab", CHR_START, RANGES) for s, e in rl)


@pytest.fixture(scope="module")
def world():
    eng = engine.Engine(0)
    ss = engine.SeqSet(eng, A)
    other = engine.SeqSet(eng, B)                                          # the source of the indexed members of B
    data, off = engine.seq_gz(eng, other, 0, 2, _lib.SEQ_GZ_MEMBERS | IDX)
    T = SeqTables(eng, ctgs_of(A))
    # every expected answer, computed once and shared: per content, per reader
    want = {}
    for name, seqs in (("A", A), ("B", B)):
        want[name] = dict(
            gc=np.array([ora.range_gc_content(s, cs, cs + a - 1, cs + b - 1) for s, cs, rl in zip(seqs, CHR_START, RANGES) for a, b in rl], np.float32),
            dg=np.array([twin(s[a - 1:b]) for s, rl in zip(seqs, RANGES) for a, b in rl], np.float32),
            gz=list(seqs), seq=lst.model(ctgs_of(seqs), LINES))
    yield dict(eng=eng, ss=ss, members_b=split(data, off), T=T, want=want)
    T.close()
    other.close()
    ss.close()
    eng.close()


def batch_arrays():
    off = np.concatenate([[0], np.cumsum([len(r) for r in RANGES])]).astype(np.uint64)
    rs = np.array([cs + a - 1 for cs, rl in zip(CHR_START, RANGES) for a, _ in rl], np.int32)
    re_ = np.array([cs + b - 1 for cs, rl in zip(CHR_START, RANGES) for _, b in rl], np.int32)
    return np.array([0, 1], np.uint32), np.array(CHR_START, np.int32), off, rs, re_


def read_gc(w, ss=None):
    """-> (rc, values): gams_gpu_range_gc_batch, which builds the G/C index"""
    sel, cst, off, rs, re_ = batch_arrays()
    gc = np.zeros(rs.size, np.float32)
    rc = L.gams_gpu_range_gc_batch(w["eng"].h, (ss or w["ss"]).p, 2, sel.ctypes.data, cst.ctypes.data, off.ctypes.data, rs.ctypes.data,
                                   re_.ctypes.data, gc.ctypes.data)
    return rc, gc


def read_dg(w, ss=None):
    sel, cst, off, rs, re_ = batch_arrays()
    return engine.range_dg_batch(w["eng"], ss or w["ss"], sel, cst, off, rs, re_, TABLE)


def read_gz(w, ss=None):
    """-> (rc, the members of both slots inflated with zlib)"""
    out, n, off = C.c_void_p(), C.c_uint64(), np.zeros(3, np.uint64)
    rc = L.gams_gpu_seq_gz(w["eng"].h, (ss or w["ss"]).p, 0, 2, None, _lib.SEQ_GZ_MEMBERS, C.byref(out), C.byref(n), off.ctypes.data)
    if rc != _lib.OK:
        return rc, None
    return rc, [zlib.decompress(m, 31) for m in split(C.string_at(out, n.value), off)]


def read_seq(w, ss=None):
    rc, text, _ = abi_seq(w["eng"], w["T"], ss or w["ss"], LINES)
    return rc, text


READERS = dict(gc=read_gc, dg=read_dg, gz=read_gz, seq=read_seq)


def check_read(w, reader, name):
    rc, got = READERS[reader](w)
    assert rc == _lib.OK, L.gams_gpu_last_error(w["eng"].h)
    exp = w["want"][name][reader]
    if reader in ("gc", "dg"):
        assert_same_bits(got, exp, (reader, name))
    else:
        assert got == exp, (reader, name)


def upload_all(w, seqs, ss=None):
    arrs = [np.frombuffer(s, np.uint8) for s in seqs]
    ptrs = (C.c_void_p * 2)(*[a.ctypes.data for a in arrs])
    w["eng"].check(L.gams_seqset_upload_all(w["eng"].h, (ss or w["ss"]).p, ptrs))


def write_upload(w):
    """slot 0 through gams_seqset_upload, and slot 1 the same way: the whole content is B behind the writer"""
    w["ss"].upload(0, B[0])
    w["ss"].upload(1, B[1])


def write_upload_image(w):
    off, img, _ = image_of(w["ss"], [np.frombuffer(s, np.uint8) for s in B])
    w["ss"].upload_image(img, 0, int(off[1]) + LENS[1])
    w["eng"].sync()                                                       # the image may go


def write_upload_gz(w):
    rc, st, nf = upload_gz(w["eng"], w["ss"], 0, w["members_b"])
    assert (rc, st, nf) == (_lib.OK, [DONE, DONE], 0)


WRITERS = dict(upload=write_upload, upload_all=lambda w: upload_all(w, B), upload_image=write_upload_image, upload_gz=write_upload_gz)


@pytest.mark.parametrize("reader", list(READERS))
@pytest.mark.parametrize("writer", list(WRITERS))
def test_writer_hands_over_to_reader(world, writer, reader):
    """A is read, the writer brings B, B is read: by the same reader, which has left its own state behind (the G/C index
    of range_gc, a clean `dirty`)"""
    w = world
    upload_all(w, A)
    check_read(w, reader, "A")
    WRITERS[writer](w)
    check_read(w, reader, "B")


def test_upload_ranges_burst(world):
    """three gams_seqset_upload_ranges calls back to back over disjoint thirds of the layout, no reader between them (the
    second and third take the once-per-epoch path), then one range_dg over ranges that straddle the seams"""
    w = world
    eng, ss = w["eng"], w["ss"]
    upload_all(w, A)
    check_read(w, "dg", "A")                                              # a reader: the burst's first call orders itself
    off, img, plane = image_of(ss, [np.frombuffer(s, np.uint8) for s in B])
    end = int(off[1]) + LENS[1]
    cuts = [0, (end // 3) & ~7, (2 * end // 3) & ~7, end]
    assert int(off[1]) < cuts[1] < cuts[2]                                # both seams lie inside ctg 1
    for lo, hi in zip(cuts, cuts[1:]):
        ss.upload_ranges(img, plane, lo, hi)
    seams = [c - int(off[1]) for c in cuts[1:3]]                          # 0-based positions in ctg 1
    r1 = [(p - d, n) for p in seams for d, n in ((2, 4), (8, 16), (100, 200), (3000, 6000), (0, 50), (50, 50))]
    r1 += [(0, 3), (LENS[1] - 3, 3)]
    cst = np.array(CHR_START, np.int32)
    roff = np.array([0, 1, 1 + len(r1)], np.uint64)
    rs = np.array([1] + [CHR_START[1] + p for p, _ in r1], np.int32)
    re_ = np.array([LENS[0]] + [CHR_START[1] + p + n - 1 for p, n in r1], np.int32)
    rc, got = engine.range_dg_batch(eng, ss, [0, 1], cst, roff, rs, re_, TABLE)
    assert rc == _lib.OK, L.gams_gpu_last_error(eng.h)
    exp = np.array([twin(B[0])] + [twin(B[1][p:p + n]) for p, n in r1], np.float32)
    assert_same_bits(got, exp)
    assert not np.isnan(exp).any()                                        # every range has a value to be wrong about
    eng.sync()                                                            # the images may go


def test_plane_only_and_back(world):
    """after gams_seqset_upload_ranges with a plane image only the readers of bytes and the device inflate answer
    GAMS_ESTATE; after a gams_seqset_upload_all they all answer again, and for what that call brought"""
    w = world
    eng = w["eng"]
    po = engine.SeqSet(eng, B)
    try:
        off, _, plane = image_of(po, [np.frombuffer(s, np.uint8) for s in B])
        po.upload_ranges(None, plane, 0, int(off[1]) + LENS[1])
        eng.sync()                                                        # the image may go
        # The refusals are asserted where each entry is tested -- range_dg: test_gpu_dg.py::test_range_dg_refusals; seq_gz:
        # test_gpu_seq_gz.py::test_return_codes_leave_the_handle_usable; gams_seqset_upload_gz:
        # test_gpu_seq_gunzip.py::test_argument_checks; range_gc: test_gpu_wave_plane.py::test_plane_only_seqset -- and are
        # not repeated.  One of them says here that the state is reached:
        assert read_gz(w, po)[0] == _lib.ESTATE
        upload_all(w, A, po)
        for reader in READERS:
            rc, got = READERS[reader](w, po)
            assert rc == _lib.OK, (reader, L.gams_gpu_last_error(eng.h))
            exp = w["want"]["A"][reader]
            if reader in ("gc", "dg"):
                assert_same_bits(got, exp, reader)
            else:
                assert got == exp, reader
        rc, st, nf = upload_gz(eng, po, 0, w["members_b"])                # the device inflate takes the seqset again
        assert (rc, st, nf) == (_lib.OK, [DONE, DONE], 0)
        assert read_gz(w, po) == (_lib.OK, list(B))
    finally:
        po.close()
