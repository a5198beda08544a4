"""`gams peak` on the device: gams_gpu_peak_text through the C ABI and host.peak_text above it, against the pinned host
path (host.peak) where the input is position-sorted and the pure-Python model of tests/peak_text.py everywhere."""
import ctypes as C

import numpy as np
import pytest

import helpers
import peak_text as pt
from gams_amd import _lib, engine, host
from test_gpu_text_ops import LocTables, all_ctgs, read_bytes
from test_gpu_wave_plane import image_of
from test_rg_text_cpu import locator_order, parse_line

pytestmark = pytest.mark.gpu

L = _lib.load()
NONE = 0xffffffff


@pytest.fixture(scope="module")
def eng():
    e = engine.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def synth():
    """the synthetic ctgs, the bytes of their wave TSV and the model's text, made once"""
    ctgs = pt.synth_ctgs()
    data = pt.synth_data(pt.synth_lines(ctgs))
    return ctgs, data, pt.model(ctgs, data)


def seq_arrays(ctgs):
    return [np.frombuffer(c["seq"], np.uint8) for c in ctgs]


class PeakTables(LocTables):
    """LocTables and, per interval of the ctg index (the Locator's order), the seqset slot and the ctg's place"""

    def __init__(self, eng, ctgs, slots=None):
        super().__init__(eng, ctgs)
        self.order = locator_order(ctgs)
        slot_of = {c["id"]: (i if slots is None else slots[i]) for i, c in enumerate(ctgs)}
        self.slot = np.array([slot_of[c["id"]] for c in self.order], np.uint32)
        self.cs = np.array([c["chr_start"] for c in self.order], np.int32)
        self.ce = np.array([c["chr_end"] for c in self.order], np.int32)


def abi_peak(eng, T, ss, data):
    """(rc, text, text_off, n_rows) of gams_gpu_peak_text"""
    text, nb, rows = C.c_void_p(), C.c_uint64(), C.c_uint64()
    off = np.full(len(T.order) + 1, 77, np.uint64)
    rc = L.gams_gpu_peak_text(eng.h, ss.p, T.ix, T.chr, T.ids, T.slot.ctypes.data, T.cs.ctypes.data, T.ce.ctypes.data,
                              data, len(data), C.byref(text), C.byref(nb), off.ctypes.data, C.byref(rows))
    return rc, (C.string_at(text, nb.value) if rc == 0 and nb.value else b""), off, rows.value


def in_id_order(T, text, off):
    """the slices of the entry's text, the ctgs in id byte order: what host.peak_text returns"""
    ids = sorted(range(len(T.order)), key=lambda i: T.order[i]["id"].encode())
    return b"".join(text[int(off[i]):int(off[i + 1])] for i in ids)


def test_golden_I_peaks(eng, s288c):
    ctgs = helpers.gen_ctgs("I", s288c["I"], piece=500000)
    data = read_bytes("I.peaks.tsv")
    got = host.peak_text(eng, ctgs, data)
    assert host.last_operator_device() == 1
    assert got.decode() == host.peak(eng, ctgs, helpers.read_lines("I.peaks.tsv"))     # position-sorted: all agree
    assert got == pt.model(ctgs, data)
    assert got.count(b"\n") == 115
    with pytest.raises(host.HostError) as ei:                  # piece 100000: a peak leaves its ctg
        host.peak_text(eng, all_ctgs(s288c), data)
    assert ei.value.code == _lib.EINVAL


def test_synthetic_input_equals_the_model(eng, synth):
    ctgs, data, want = synth
    got = host.peak_text(eng, ctgs, data)
    assert host.last_operator_device() == 1
    assert got == want


def test_entry_slices_determinism_and_refusals(eng, synth):
    ctgs, data, want = synth
    ss = engine.SeqSet(eng, seq_arrays(ctgs))
    T = PeakTables(eng, ctgs)
    try:
        rc, text, off, rows = abi_peak(eng, T, ss, data)
        assert rc == 0 and rows == want.count(b"\n") == text.count(b"\n")
        assert off[0] == 0 and off[-1] == len(text) and np.all(np.diff(off.astype(np.int64)) >= 0)
        for i, c in enumerate(T.order):                        # every slice holds its ctg's rows, and only those
            part = text[int(off[i]):int(off[i + 1])]
            assert all(r.startswith(b"peak:" + c["id"].encode() + b":") for r in part.split(b"\n")[:-1]), c["id"]
        assert in_id_order(T, text, off) == want
        rc2, text2, off2, rows2 = abi_peak(eng, T, ss, data)
        assert (rc2, text2, rows2) == (0, text, rows) and np.array_equal(off, off2)
        # the stages of the call
        ms = (C.c_float * 16)()
        n = C.c_uint32()
        assert L.gams_gpu_last_stage_ms(eng.h, ms, 16, C.byref(n)) == 0 and n.value == 10
        assert all(ms[k] >= 0 for k in range(10))
        rc, text, off, rows = abi_peak(eng, T, ss, b"")
        assert (rc, text, rows) == (0, b"", 0) and not off.any()
        rc, text, off, rows = abi_peak(eng, T, ss, b"#range\tgc_content\tsignal\nI:5-9\t0.1\t1\n")   # one located line
        assert (rc, text, rows) == (0, b"", 0) and not off.any()
        # a valid range with two fields, located or not
        assert abi_peak(eng, T, ss, data + b"\nI:5-9\t0.1\n")[0] == _lib.EINVAL
        assert abi_peak(eng, T, ss, b"IV:5-9\t0.1\n")[0] == _lib.EINVAL
        # a refused byte: the entry says so, the operator falls back to the host's passes and prints the same text
        bad = data + b"\nnonsense \xc3\xa9\n"
        assert abi_peak(eng, T, ss, bad)[0] == _lib.EUNSUPPORTED
        assert host.peak_text(eng, ctgs, bad) == want and host.last_operator_device() == 0
        assert host.peak_text(eng, ctgs, bad, seqset=ss) == want and host.last_operator_device() == 0
    finally:
        T.close()
        ss.close()


def test_early_ends_and_the_row_without_a_signal(eng, synth):
    """An input without lines, and one whose every located line is the first of its ctg (nothing kept): GAMS_OK, no text,
    no rows, and the stopwatch of the call invalid (a full call in front of each leaves ten stages to forget).  A valid
    range without a signal column is refused with its message, in front of every later check."""
    ctgs, data, _ = synth
    ss = engine.SeqSet(eng, seq_arrays(ctgs))
    T = PeakTables(eng, ctgs)
    ms, n = (C.c_float * 16)(), C.c_uint32()
    try:
        for early in (b"", b"I:5-9\t0.1\t1\nII:2000-2004\t0.2\t1\n"):       # two ctgs, one line in each
            assert abi_peak(eng, T, ss, data)[0] == 0
            assert L.gams_gpu_last_stage_ms(eng.h, ms, 16, C.byref(n)) == 0 and n.value == 10
            rc, text, off, rows = abi_peak(eng, T, ss, early)
            assert (rc, text, rows) == (0, b"", 0) and not off.any()
            assert L.gams_gpu_last_stage_ms(eng.h, ms, 16, C.byref(n)) == _lib.ESTATE
        # (the second line alone would end as above: nothing kept)
        assert abi_peak(eng, T, ss, b"I:5-9\t0.1\nII:2000-2004\t0.2\t1\n")[0] == _lib.EINVAL
        assert L.gams_gpu_last_error(eng.h) == b"gpu_peak_text: a row has no signal column (the reference panics, utils.rs:102)"
    finally:
        T.close()
        ss.close()


def test_missing_sequence_and_plane_only_seqset(eng, synth):
    ctgs, data, _ = synth
    seqs = seq_arrays(ctgs)
    # ctg:I:2 has kept peaks and no sequence: a seqset of the other five
    slots = [0, None, 1, 2, 3, 4]
    ss = engine.SeqSet(eng, [s for s, k in zip(seqs, slots) if k is not None])
    T = PeakTables(eng, ctgs, [NONE if k is None else k for k in slots])
    try:
        assert abi_peak(eng, T, ss, data)[0] == _lib.EINVAL
        # ... and none for a ctg without kept peaks is fine: the ctg with one located line
        lines = [ln for ln in data.split(b"\n") if (parse_line(ln.split(b"\t")[0]) or ("",))[0] != "I"]
        rc, text, off, rows = abi_peak(eng, T, ss, b"\n".join(lines))
        assert rc == 0 and rows > 0 and off[1] == off[2]
        with pytest.raises(host.HostError) as ei:
            host.peak_text(eng, [dict(c, slot=k) for c, k in zip(ctgs, slots)], data, seqset=ss)
        assert ei.value.code == _lib.EINVAL
    finally:
        T.close()
        ss.close()
    ss = engine.SeqSet(eng, seqs, upload=False)
    T = PeakTables(eng, ctgs)
    try:
        off, img, plane = image_of(ss, seqs)
        ss.upload_ranges(None, plane, 0, int(off[-1]) + seqs[-1].size)
        assert abi_peak(eng, T, ss, data)[0] == _lib.ESTATE
    finally:
        T.close()
        ss.close()


def test_resident_seqset_gives_the_same_text(eng, synth):
    ctgs, data, want = synth
    ss = engine.SeqSet(eng, seq_arrays(ctgs))
    try:
        assert host.peak_text(eng, ctgs, data, seqset=ss) == want and host.last_operator_device() == 1
        # the slots named explicitly: the seqset in another order than the ctgs
        perm = [3, 0, 5, 1, 4, 2]
        seqs = seq_arrays(ctgs)
        ss2 = engine.SeqSet(eng, [seqs[perm.index(k)] for k in range(6)])
        try:
            assert host.peak_text(eng, [dict(c, slot=perm[i]) for i, c in enumerate(ctgs)], data, seqset=ss2) == want
        finally:
            ss2.close()
    finally:
        ss.close()


def test_long_name_prefixes(eng):
    """130-byte name. prefixes in front of every range: rows of ~250 bytes, so a block of 256 rows is ~64 KB, beyond the
    32-KB LDS stage of the row writer (every other case here is staged)"""
    ctgs = pt.synth_ctgs()
    data = pt.synth_data(pt.synth_lines(ctgs, seed=17, n=700, long_names=True))
    want = pt.model(ctgs, data)
    assert want.count(b"\n") > 512 and b"n" * 128 in want
    assert host.peak_text(eng, ctgs, data) == want and host.last_operator_device() == 1
