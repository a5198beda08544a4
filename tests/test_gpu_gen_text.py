"""`gams gen` from the bytes of a FASTA file on the device: gams_gpu_gen_text through the C ABI and host.gen_text above
it.  The pure-Python model of tests/gen_text.py is the expected value everywhere; every comparison is exact."""
import ctypes as C
import gzip
import os

import numpy as np
import pytest

import gen_text as gt
import helpers
from gams_amd import _lib, engine, host

pytestmark = pytest.mark.gpu

L = _lib.load()


@pytest.fixture(scope="module")
def eng():
    e = engine.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def genome():
    with gzip.open(os.path.join(helpers.S288C, "genome.fa.gz"), "rb") as fh:
        return fh.read()


class Gen:
    """one gams_gpu_gen_text call: rc, and on success the chromosomes, the ctg table and the adopted seqset"""

    def __init__(self, eng, data, piece=500000, fill=50, min_len=5000):
        self.eng, self.g, self.seqset = eng, C.c_void_p(), None
        prm = _lib.GenParams(piece, fill, min_len)
        self.rc = L.gams_gpu_gen_text(eng.h, bytes(data), len(data), C.byref(prm), C.byref(self.g))
        if self.rc != _lib.OK:
            assert not self.g.value
            return
        n_chr, n_ctg, nb = C.c_uint32(), C.c_uint32(), C.c_uint64()
        eng.check(L.gams_gen_counts(eng.h, self.g, C.byref(n_chr), C.byref(n_ctg), C.byref(nb)))
        names = np.zeros(max(nb.value, 1), np.uint8)
        off = np.zeros(n_chr.value + 1, np.uint64)
        clen = np.zeros(max(n_chr.value, 1), np.uint32)
        self.tab = np.zeros(max(n_ctg.value, 1), _lib.GEN_CTG_DTYPE)
        eng.check(L.gams_gen_chrs(eng.h, self.g, names.ctypes.data, off.ctypes.data, clen.ctypes.data))
        eng.check(L.gams_gen_ctgs(eng.h, self.g, self.tab.ctypes.data))
        self.tab = self.tab[:n_ctg.value]
        raw = names.tobytes()
        self.chrs = [raw[int(off[i]):int(off[i + 1])].decode() for i in range(n_chr.value)]
        self.chr_len = dict(zip(self.chrs, clen[:n_chr.value].tolist()))
        assert len(self.chr_len) == len(self.chrs)
        p = C.c_void_p()
        eng.check(L.gams_gen_seqset(eng.h, self.g, C.byref(p)))
        self.seqset = engine.SeqSet.adopt(eng, p.value, (self.tab["chr_end"] - self.tab["chr_start"] + 1).astype(np.uint32))

    def table(self):
        return [(f"ctg:{self.chrs[t['chr']]}:{t['serial']}", self.chrs[t["chr"]], int(t["chr_start"]), int(t["chr_end"]),
                 int(t["chr_end"]) - int(t["chr_start"]) + 1) for t in self.tab]

    def close(self):
        if self.seqset is not None:
            self.seqset.close()
            self.seqset = None
        if self.g.value:
            L.gams_gen_destroy(self.eng.h, self.g)
            self.g = C.c_void_p()


def plane_of(seq):
    out = np.zeros((len(seq) + 7) // 8, np.uint8)
    a = np.frombuffer(seq, np.uint8)
    assert L.gams_gc_plane(a.ctypes.data if a.size else None, a.size, out.ctypes.data) == 0
    return out.tobytes()


def check_case(eng, case):
    """the three checks of every case: the table and the chromosome lengths, the bases of every slot, their plane"""
    ctgs, chr_len = gt.model(case.data, case.piece, case.fill, case.min_len)
    g = Gen(eng, case.data, case.piece, case.fill, case.min_len)
    try:
        assert g.rc == _lib.OK, eng.lib.gams_gpu_last_error(eng.h)
        assert g.chrs == list(chr_len) and g.chr_len == chr_len
        assert g.table() == gt.table(ctgs)
        for i, c in enumerate(ctgs):
            assert g.seqset.download(i) == c["seq"], (case.name, c["id"])
            assert g.seqset.download(i, plane=True) == plane_of(c["seq"]), (case.name, c["id"])
    finally:
        g.close()
    return ctgs


@pytest.mark.parametrize("case", gt.line_cases(), ids=lambda c: c.name)
def test_line_geometry(eng, case):
    check_case(eng, case)


@pytest.mark.parametrize("case", gt.span_cases(), ids=lambda c: c.name)
def test_span_geometry(eng, case):
    ctgs = check_case(eng, case)
    if case.name == "lead_n":      # every misalignment of a ctg's first base against the stream's 16-B units
        assert sorted(320 * int(c["chr_id"][1:]) + c["chr_start"] - 1 & 15 for c in ctgs) == list(range(16))
    if case.name == "run_over_chromosomes_short":
        assert ctgs == []


def test_size(eng):
    case = gt.size_case()
    assert len(case.data) > 180 * gt.BLK and sum(len(s) for _, s in gt.records(case.data)) % 16 == 0
    ctgs = check_case(eng, case)
    assert len(ctgs) > 20
    ms, n = (C.c_float * 16)(), C.c_uint32()
    Gen(eng, case.data, case.piece, case.fill, case.min_len).close()
    eng.check(L.gams_gpu_last_stage_ms(eng.h, ms, 16, C.byref(n)))
    assert n.value == 5 and all(m >= 0 for m in ms[:5])


@pytest.mark.parametrize("piece", [100000, 500000])
def test_golden_genome_and_wave_on_the_seqset(eng, genome, piece):
    case = gt.Case("S288c", genome, piece, 50, 5000)
    ctgs = check_case(eng, case)
    if piece == 100000:
        assert [c["id"] for c in ctgs] == ["ctg:I:1", "ctg:I:2", "ctg:Mito:1"]
    g = Gen(eng, genome, piece)
    up = engine.SeqSet(eng, [c["seq"] for c in ctgs])
    try:
        peaks = []
        for ss in (g.seqset, up):
            plan = engine.WavePlan(eng, ss)
            plan.run()
            peaks.append(plan.peaks())
            assert plan.last_input() == _lib.WAVE_INPUT_PLANE
            plan.set_input(_lib.WAVE_INPUT_BYTES)
            plan.run()
            assert np.array_equal(plan.peaks(), peaks[-1]) and plan.last_input() == _lib.WAVE_INPUT_BYTES
            plan.close()
        assert peaks[0].size > 0 and np.array_equal(peaks[0], peaks[1])
        # a reader of the bytes: range gc inside the first ctg
        rs, re_ = np.array([1, 777, 5000], np.int32), np.array([100, 4000, 99999], np.int32)
        gcs = []
        for ss in (g.seqset, up):
            gc = np.zeros(3, np.float32)
            eng.check(L.gams_gpu_range_gc(eng.h, ss.p, 0, 1, rs.ctypes.data, re_.ctypes.data, 3, gc.ctypes.data))
            gcs.append(gc)
        assert np.array_equal(gcs[0], gcs[1]) and gcs[0].min() > 0
    finally:
        up.close()
        g.close()


def test_return_codes(eng):
    E = _lib
    g = Gen(eng, b"")
    assert g.rc == E.OK and g.chrs == [] and g.table() == [] and g.seqset.lengths.size == 0
    g.close()
    s = gt.bases(300, 9)
    ok = b">a\n" + s + b"\n"
    assert Gen(eng, s + b"\n").rc == E.EINVAL
    assert Gen(eng, b"\n" + ok).rc == E.EINVAL
    for piece, fill, min_len in ((0, 50, 5000), (500000, 0, 5000), (500000, 50, 0), (-1, 50, 5000)):
        assert Gen(eng, ok, piece, fill, min_len).rc == E.EINVAL
    assert Gen(eng, b"", 0, 50, 5000).rc == E.EINVAL
    assert Gen(eng, b">a\n" + s[:100] + b"\xc3" + s[100:] + b"\n").rc == E.EUNSUPPORTED
    assert Gen(eng, b">a \x80\n" + s + b"\n").rc == E.EUNSUPPORTED
    assert Gen(eng, b">a\n" + s[:100] + b"\x00" + s[100:] + b"\n").rc == E.EUNSUPPORTED
    for case in gt.refused_cases():
        assert Gen(eng, case.data, case.piece, case.fill, case.min_len).rc == E.EUNSUPPORTED, case.name
    # the seqset is handed out once
    g, p = Gen(eng, ok, 1000, 5, 20), C.c_void_p()
    assert g.rc == E.OK and g.table() == [("ctg:a:1", "a", 1, 300, 300)]
    assert L.gams_gen_seqset(eng.h, g.g, C.byref(p)) == E.ESTATE
    # download: its own errors
    assert L.gams_seqset_download(eng.h, g.seqset.p, 1, None, None) == E.EINVAL
    assert L.gams_seqset_download(eng.h, g.seqset.p, 0, None, None) == E.OK
    g.close()


def test_download_of_an_uploaded_seqset_and_its_states(eng):
    seqs = [gt.bases(1000, 1, 1e-2), gt.bases(257, 2), gt.bases(5, 3)]
    ss = engine.SeqSet(eng, seqs)
    try:
        for i, s in enumerate(seqs):
            assert ss.download(i) == s and ss.download(i, plane=True) == plane_of(s)
        off, nb = ss.layout()
        image = np.zeros(nb, np.uint8)
        for o, s in zip(off.tolist(), seqs):
            image[o:o + len(s)] = np.frombuffer(s[::-1], np.uint8)
        ss.upload_image(image, 0, int(off[-1]) + 8)              # bytes without their plane: the plane is stale
        eng.sync()
        assert ss.download(0) == seqs[0][::-1]
        buf = np.zeros(1000, np.uint8)
        assert L.gams_seqset_download(eng.h, ss.p, 0, None, buf.ctypes.data) == _lib.ESTATE
        plane = np.zeros(nb // 8 + 1, np.uint8)
        ss.upload_ranges(None, plane, 0, int(off[-1]) + 8)       # a plane without bytes: plane-only
        eng.sync()
        assert L.gams_seqset_download(eng.h, ss.p, 0, buf.ctypes.data, None) == _lib.ESTATE
    finally:
        ss.close()


def test_two_runs_are_identical(eng):
    case = next(c for c in gt.line_cases() if c.name == "all_geometries_one_file")
    runs = []
    for _ in range(2):
        g = Gen(eng, case.data, case.piece, case.fill, case.min_len)
        assert g.rc == _lib.OK
        runs.append((g.chrs, g.chr_len, g.table(), [g.seqset.download(i) for i in range(len(g.tab))],
                     [g.seqset.download(i, plane=True) for i in range(len(g.tab))]))
        g.close()
    assert runs[0] == runs[1]


def test_host_gen_text(eng, genome):
    want, want_len = gt.model(genome, piece=100000)
    ctgs, chr_len, ss = host.gen_text(eng, genome, piece=100000)
    try:
        assert host.last_operator_device() == 1
        assert gt.table(ctgs) == gt.table(want) and chr_len == want_len
        assert [c["range"] for c in ctgs] == [c["range"] for c in want]
        assert host.tsv_ctgs(ctgs) == host.tsv_ctgs(want)
        assert all(ss.download(i) == c["seq"] for i, c in enumerate(want))
    finally:
        ss.close()
    # where the device refuses, the host's passes answer
    for case in gt.refused_cases():
        want, want_len = gt.model(case.data, case.piece, case.fill, case.min_len)
        ctgs, chr_len, ss = host.gen_text(eng, case.data, case.piece, case.fill, case.min_len)
        try:
            assert host.last_operator_device() == 0, case.name
            assert gt.table(ctgs) == gt.table(want) and chr_len == want_len, case.name
            for i, c in enumerate(want):
                assert ss.download(i) == c["seq"] and ss.download(i, plane=True) == plane_of(c["seq"]), (case.name, c["id"])
        finally:
            ss.close()
    with pytest.raises(host.HostError) as err:
        host.gen_text(eng, b"ACGT\n")
    assert err.value.code == _lib.EINVAL
