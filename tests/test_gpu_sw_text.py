"""`gams sw` from the bytes of a feature file on the device: gams_gpu_sw_feature_text through the C ABI and host.sw_text
above it, against the pure-Python model of tests/sw_text.py (the oracle's rows over the model's features), the pinned
per-ctg path (host.sw) on the golden rg file, and host.sw_multi over the model's features for the count actions."""
import ctypes as C

import numpy as np
import pytest

import helpers
import sw_text as swt
from gams_amd import _lib, engine, host
from test_gpu_text_ops import LocTables, all_ctgs, read_bytes
from test_gpu_wave_plane import image_of
from test_rg_text_cpu import locator_order

pytestmark = pytest.mark.gpu

L = _lib.load()
NONE = 0xffffffff
STAGES = 12                # lines parse locate first keep offsets order | gather geometry rows text-lengths text-write
GC, COUNT = _lib.SW_GC, _lib.SW_COUNT


@pytest.fixture(scope="module")
def eng():
    e = engine.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def synth():
    """the synthetic ctgs, the bytes of their feature file, the model's features and its text, made once"""
    ctgs = swt.synth_ctgs()
    data = swt.synth_data(swt.synth_lines(ctgs))
    return ctgs, data, swt.features(ctgs, data), swt.model(ctgs, data)


@pytest.fixture(scope="module")
def rg(eng, synth):
    """an rg file over the same ctgs (no tab in a line: read_range cuts there, the loader does not): its bytes and the
    rg: records read_range makes of its lines"""
    ctgs = synth[0]
    lines = [ln for ln in swt.synth_lines(ctgs, seed=31, n=1500) if "\t" not in ln]
    return "\n".join(lines).encode(), host.read_range(eng, ctgs, lines)


def seq_arrays(ctgs):
    return [np.frombuffer(c["seq"], np.uint8) for c in ctgs]


class SwTables(LocTables):
    """LocTables and, per interval of the ctg index (the Locator's order), the seqset slot and the ctg's place"""

    def __init__(self, eng, ctgs, slots=None, rg_records=None):
        super().__init__(eng, ctgs, rg_records)
        self.order = locator_order(ctgs)
        slot_of = {c["id"]: (i if slots is None else slots[i]) for i, c in enumerate(ctgs)}
        self.slot = np.array([slot_of[c["id"]] for c in self.order], np.uint32)
        self.cs = np.array([c["chr_start"] for c in self.order], np.int32)
        self.ce = np.array([c["chr_end"] for c in self.order], np.int32)


def abi_sw(eng, T, ss, data, size=100, mx=20, resize=500, actions=GC):
    """(rc, text, text_off, n_features, n_rows) of gams_gpu_sw_feature_text"""
    text, nb, nf, rows = C.c_void_p(), C.c_uint64(), C.c_uint64(), C.c_uint64()
    off = np.full(len(T.order) + 1, 77, np.uint64)
    count = bool(actions & COUNT)
    rc = L.gams_gpu_sw_feature_text(eng.h, None if ss is None else ss.p, T.ix, T.chr, T.ids, T.slot.ctypes.data,
                                    T.cs.ctypes.data, T.ce.ctypes.data, data, len(data), size, mx, resize, actions,
                                    T.rg_ix if count else None, T.rg_group.ctypes.data if count else None, C.byref(text),
                                    C.byref(nb), off.ctypes.data, C.byref(nf), C.byref(rows))
    return rc, (C.string_at(text, nb.value) if rc == 0 and nb.value else b""), off, nf.value, rows.value


def in_id_order(T, text, off):
    """the slices of the entry's text, the ctgs in id byte order: what host.sw_text returns"""
    ids = sorted(range(len(T.order)), key=lambda i: T.order[i]["id"].encode())
    return b"".join(text[int(off[i]):int(off[i + 1])] for i in ids)


def multi(eng, ctgs, feats, **kw):
    """host.sw_multi over the model's features, the ctgs in id byte order"""
    ids = swt.id_order(ctgs)
    return host.sw_multi([eng], [ctgs[i] for i in ids], [feats[i] for i in ids], **kw).encode()


def test_golden_rg_file(eng, s288c):
    ctgs = all_ctgs(s288c)
    data = read_bytes("spo11_hot.rg")
    got = host.sw_text(eng, ctgs, data)
    assert host.last_operator_device() == 1
    assert got == swt.model(ctgs, data)
    feats = swt.features(ctgs, data)
    assert sum(len(f) for f in feats) == 69
    per_ctg = "".join(host.sw(eng, ctgs[i], feats[i]) for i in swt.id_order(ctgs) if feats[i])
    assert got.decode() == per_ctg
    rows = got.split(b"\n")[:-1]
    assert len(rows) > 2000 and any(r.startswith(b"sw:feature:ctg:I:2:32:1\t") for r in rows)


def test_entry_slices_counts_determinism_and_stages(eng, synth):
    ctgs, data, feats, want = synth
    ss = engine.SeqSet(eng, seq_arrays(ctgs))
    T = SwTables(eng, ctgs)
    try:
        rc, text, off, nf, rows = abi_sw(eng, T, ss, data)
        assert rc == 0, L.gams_gpu_last_error(eng.h)
        assert in_id_order(T, text, off) == want
        assert nf == sum(len(f) for f in feats) and rows == want.count(b"\n") == text.count(b"\n")
        assert off[0] == 0 and off[-1] == len(text) and np.all(np.diff(off.astype(np.int64)) >= 0)
        for i, c in enumerate(T.order):                        # every slice holds its ctg's rows, and only those
            part = text[int(off[i]):int(off[i + 1])]
            assert all(r.startswith(b"sw:feature:" + c["id"].encode() + b":") for r in part.split(b"\n")[:-1]), c["id"]
            assert bool(part) == bool(feats[[x["id"] for x in ctgs].index(c["id"])])
        rc2, text2, off2, nf2, rows2 = abi_sw(eng, T, ss, data)
        assert (rc2, text2, nf2, rows2) == (0, text, nf, rows) and np.array_equal(off, off2)
        ms = (C.c_float * 16)()
        n = C.c_uint32()
        assert L.gams_gpu_last_stage_ms(eng.h, ms, 16, C.byref(n)) == 0 and n.value == STAGES
        assert all(ms[k] >= 0 for k in range(STAGES))
    finally:
        T.close()
        ss.close()


def test_host_operator_equals_the_model(eng, synth):
    ctgs, data, _, want = synth
    assert host.sw_text(eng, ctgs, data) == want and host.last_operator_device() == 1


@pytest.mark.parametrize("size,mx,resize", [(100, 20, 500), (100, 0, 500), (50, 5, 333), (10, 40, 5000), (200, 3, 100)])
def test_parameters(eng, synth, size, mx, resize):
    """81 slots a feature are more than a wavefront, max = 0 is the M row alone.  A file of 600 lines with the same edge
    lines: the oracle's flank statistics at resize 5000 cost seconds on the full one"""
    ctgs = synth[0]
    data = swt.synth_data(swt.synth_lines(ctgs, seed=37, n=600))
    got = host.sw_text(eng, ctgs, data, size, mx, resize)
    assert host.last_operator_device() == 1
    assert got == swt.model(ctgs, data, size, mx, resize)


@pytest.mark.parametrize("actions", [("count",), ("gc", "count")])
def test_actions_from_both_rg_sources(eng, synth, rg, actions):
    ctgs, data, feats, _ = synth
    rg_data, rg_records = rg
    want = multi(eng, ctgs, feats, actions=actions, rg_records=rg_records)
    assert any(r.split(b"\t")[8] not in (b"", b"0") for r in want.split(b"\n")[:-1])
    assert host.sw_text(eng, ctgs, data, actions=actions, rg_records=rg_records) == want and host.last_operator_device() == 1
    assert multi(eng, ctgs, feats, actions=actions, rg_data=rg_data) == want
    assert host.sw_text(eng, ctgs, data, actions=actions, rg_data=rg_data) == want and host.last_operator_device() == 1


def test_count_alone_reads_no_sequence(eng, synth, rg):
    ctgs, data, feats, _ = synth
    rg_data, rg_records = rg
    want = multi(eng, ctgs, feats, actions=("count",), rg_records=rg_records)
    bare = [{k: v for k, v in c.items() if k != "seq"} for c in ctgs]
    assert host.sw_text(eng, bare, data, actions=("count",), rg_data=rg_data) == want and host.last_operator_device() == 1
    seqs = seq_arrays(ctgs)
    ss = engine.SeqSet(eng, seqs, upload=False)                # a plane-only seqset, and no slot named at all
    T = SwTables(eng, ctgs, rg_records=rg_records)
    try:
        off, img, plane = image_of(ss, seqs)
        ss.upload_ranges(None, plane, 0, int(off[-1]) + seqs[-1].size)
        assert host.sw_text(eng, ctgs, data, actions=("count",), rg_data=rg_data, seqset=ss) == want
        none = [dict(c, slot=None) for c in bare]
        assert host.sw_text(eng, none, data, actions=("count",), rg_records=rg_records, seqset=ss) == want
        assert host.last_operator_device() == 1
        rc, text, off, nf, rows = abi_sw(eng, T, None, data, actions=COUNT)        # s = NULL
        assert rc == 0 and in_id_order(T, text, off) == want
        # gc needs the bytes
        assert abi_sw(eng, T, ss, data, actions=GC | COUNT)[0] == _lib.ESTATE
        assert abi_sw(eng, T, None, data, actions=GC)[0] == _lib.EINVAL
        assert L.gams_gpu_sw_feature_text(eng.h, None, T.ix, T.chr, T.ids, None, T.cs.ctypes.data, T.ce.ctypes.data, data,
                                          len(data), 100, 20, 500, COUNT, None, None, C.byref(C.c_void_p()),
                                          C.byref(C.c_uint64()), off.ctypes.data, C.byref(C.c_uint64()),
                                          C.byref(C.c_uint64())) == _lib.EINVAL       # count without rg_ix
        with pytest.raises(host.HostError) as ei:
            host.sw_text(eng, ctgs, data, seqset=ss)
        assert ei.value.code == _lib.ESTATE
    finally:
        T.close()
        ss.close()


def test_resident_seqset_gives_the_same_text(eng, synth):
    ctgs, data, _, want = synth
    seqs = seq_arrays(ctgs)
    ss = engine.SeqSet(eng, seqs)
    try:
        assert host.sw_text(eng, ctgs, data, seqset=ss) == want and host.last_operator_device() == 1
        perm = [3, 0, 5, 1, 4, 2]                              # the seqset in another order than the ctgs
        ss2 = engine.SeqSet(eng, [seqs[perm.index(k)] for k in range(6)])
        try:
            assert host.sw_text(eng, [dict(c, slot=perm[i]) for i, c in enumerate(ctgs)], data, seqset=ss2) == want
        finally:
            ss2.close()
    finally:
        ss.close()


def test_refusals(eng, synth):
    ctgs, data, _, want = synth
    seqs = seq_arrays(ctgs)
    ss = engine.SeqSet(eng, seqs)
    T = SwTables(eng, ctgs)
    try:
        # located by overlap, the middle (30044) behind the end of ctg:I:1: refused when kept, never looked at when dropped
        first, bad = b"I:100-200\n", b"I:29990-30099\n"
        assert abi_sw(eng, T, ss, first + bad)[0] == _lib.EINVAL
        assert b"line 2" in L.gams_gpu_last_error(eng.h)
        rc, text, off, nf, rows = abi_sw(eng, T, ss, bad + first)
        assert (rc, nf) == (0, 1) and text == swt.interval_text(ctgs, bad + first)
        with pytest.raises(host.HostError) as ei:
            host.sw_text(eng, ctgs, first + bad)
        assert ei.value.code == _lib.EINVAL
        assert abi_sw(eng, T, ss, data, size=1)[0] == _lib.EINVAL
        assert abi_sw(eng, T, ss, data, mx=-1)[0] == _lib.EINVAL
        assert abi_sw(eng, T, ss, data, resize=1)[0] == _lib.EINVAL
        assert abi_sw(eng, T, ss, data, actions=4)[0] == _lib.EINVAL
        # empty input, a single located line
        for empty in (b"", b"# ranges\nI:5-9\n"):
            rc, text, off, nf, rows = abi_sw(eng, T, ss, empty)
            assert (rc, text, nf, rows) == (0, b"", 0, 0) and not off.any()
            assert host.sw_text(eng, ctgs, empty) == b""
        # a refused byte: the entry says so, the operator runs the host's passes and prints the same text
        hi = data + b"\nnonsense \xc3\xa9\n"
        assert abi_sw(eng, T, ss, hi)[0] == _lib.EUNSUPPORTED
        assert host.sw_text(eng, ctgs, hi) == want and host.last_operator_device() == 0
        assert host.sw_text(eng, ctgs, hi, seqset=ss) == want and host.last_operator_device() == 0
    finally:
        T.close()
        ss.close()
    # ctg:I:2 has kept features and no sequence: a seqset of the other five
    slots = [0, None, 1, 2, 3, 4]
    ss = engine.SeqSet(eng, [s for s, k in zip(seqs, slots) if k is not None])
    T = SwTables(eng, ctgs, [NONE if k is None else k for k in slots])
    try:
        assert abi_sw(eng, T, ss, data)[0] == _lib.EINVAL
        with pytest.raises(host.HostError) as ei:
            host.sw_text(eng, [dict(c, slot=k) for c, k in zip(ctgs, slots)], data, seqset=ss)
        assert ei.value.code == _lib.EINVAL
    finally:
        T.close()
        ss.close()
