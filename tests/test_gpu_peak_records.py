"""The records `gams peak` stores, written on the device: gams_gpu_peak_records_text through the C ABI and
host.peak_records_text above it, byte for byte against the pure-Python model (tests/peak_records.py, which renumbers and
reformats the oracle-backed rows of tests/peak_text.py).  tests/test_peak_records_cpu.py holds the model and the host
formatter to account on the CPU."""
import ctypes as C
import json

import numpy as np
import pytest

import peak_records as pr
import peak_text as pt
from gams_amd import _lib, engine, host
from test_gpu_peak_text import PeakTables, in_id_order, seq_arrays
from test_gpu_text_edges import first_difference
from test_gpu_wave_plane import image_of
from test_rg_text_cpu import parse_line

pytestmark = pytest.mark.gpu

L = _lib.load()
FORMATS = {"records": _lib.LOADER_RECORDS, "tsv": _lib.LOADER_TSV, "resp": _lib.LOADER_RESP}
STAGE, TSV_STAGE = 98304, 32768          # kPeakRecStage, kPeakStage (csrc/text.hip)


@pytest.fixture(scope="module")
def eng():
    e = engine.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def synth():
    """the synthetic ctgs and the bytes of their wave TSV, made once"""
    ctgs = pt.synth_ctgs()
    return ctgs, pt.synth_data(pt.synth_lines(ctgs, n=3000))


class Device:
    """a resident seqset of the ctgs' bases and the tables of the C ABI"""

    def __init__(self, eng, ctgs):
        self.ss = engine.SeqSet(eng, seq_arrays(ctgs))
        self.T = PeakTables(eng, ctgs)

    def close(self):
        self.T.close()
        self.ss.close()


def abi_records(eng, d, data, fmt, base=None, ss=None):
    """(rc, text, text_off, serial_next per interval, n_rows, text_bytes) of gams_gpu_peak_records_text; base: {ctg id: n}"""
    T = d.T
    text, nb, rows = C.c_void_p(), C.c_uint64(77), C.c_uint64(77)
    off = np.full(len(T.order) + 1, 77, np.uint64)
    sb = None if base is None else np.array([base.get(c["id"], 0) for c in T.order], np.int32)
    nxt = np.full(len(T.order), -7, np.int32)
    rc = L.gams_gpu_peak_records_text(eng.h, (ss or d.ss).p, T.ix, T.chr, T.ids, T.slot.ctypes.data, T.cs.ctypes.data,
                                      T.ce.ctypes.data, data, len(data), FORMATS.get(fmt, fmt),
                                      None if sb is None else sb.ctypes.data, C.byref(text), C.byref(nb), off.ctypes.data,
                                      nxt.ctypes.data, C.byref(rows))
    return rc, (C.string_at(text, nb.value) if rc == 0 and nb.value else b""), off, nxt, rows.value, nb.value


def one_ctg(n=20000, seed=3, cid="ctg:I:1"):
    rng = np.random.default_rng(seed)
    return dict(id=cid, chr_id="I", chr_start=1, chr_end=n, seq=rng.choice(np.frombuffer(b"ACGT", np.uint8), n).tobytes())


def lines_of(k, step=30, signal=lambda i: "1" if i % 2 else "-1"):
    """k + 1 located lines in one ctg: the first one, which is dropped, then k kept ones, every start distinct, shuffled"""
    order = np.random.default_rng(k).permutation(k)
    rows = ["I:%d-%d\t0.5\t%s\n" % (10 + step * i, 10 + step * i + 7 + i % 11, signal(i)) for i in order]
    return ("I:2-3\t0.5\tfirst\n" + "".join(rows)).encode()


# ---- 1. the three formats ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", list(FORMATS))
def test_formats_equal_the_model_from_host_sequences_and_a_resident_seqset(eng, synth, fmt):
    ctgs, data = synth
    want, nxt = pr.model(ctgs, data, fmt)
    assert want.count(b"\n") > 2500
    got, got_nxt = host.peak_records_text(eng, ctgs, data, fmt=fmt)
    assert host.last_operator_device() == 1
    assert got == want, first_difference(got, want)
    assert got_nxt == nxt
    ss = engine.SeqSet(eng, seq_arrays(ctgs))
    try:
        got, got_nxt = host.peak_records_text(eng, ctgs, data, fmt=fmt, seqset=ss)
        assert host.last_operator_device() == 1
        assert got == want and got_nxt == nxt
        if fmt == "tsv":
            assert got == host.peak_text(eng, ctgs, data, seqset=ss) and host.last_operator_device() == 1
    finally:
        ss.close()


def test_entry_slices_stages_and_two_calls(eng, synth):
    ctgs, data = synth
    want, _ = pr.model(ctgs, data, "resp")
    d = Device(eng, ctgs)
    try:
        rc, text, off, nxt, rows, nb = abi_records(eng, d, data, "resp")
        assert rc == 0 and rows == want.count(b"*3\r\n") and nb == len(want)
        assert off[0] == 0 and off[-1] == len(text) and np.all(np.diff(off.astype(np.int64)) >= 0)
        assert in_id_order(d.T, text, off) == want
        ms, n = (C.c_float * 16)(), C.c_uint32()
        assert L.gams_gpu_last_stage_ms(eng.h, ms, 16, C.byref(n)) == 0 and n.value == 10
        rc2, text2, off2, nxt2, rows2, _ = abi_records(eng, d, data, "resp")
        assert (rc2, text2, rows2) == (0, text, rows) and np.array_equal(off, off2) and np.array_equal(nxt, nxt2)
    finally:
        d.close()


# ---- 2. serials -------------------------------------------------------------------------------------------------------
def test_serials_continue_the_counters(eng, synth):
    ctgs, data = synth
    base = {"ctg:I:1": 8, "ctg:II:1": 99, "ctg:I:2": 0, pt.ONE_LINE: 41, pt.TWO_LINES: 5}
    for fmt in ("resp", "records", "tsv"):
        want, nxt = pr.model(ctgs, data, fmt, base)
        got, got_nxt = host.peak_records_text(eng, ctgs, data, fmt=fmt, serial_base=base)
        assert host.last_operator_device() == 1
        assert got == want, (fmt, first_difference(got, want))
        assert got_nxt == nxt
    want, nxt = pr.model(ctgs, data, "resp", base)
    # the ids cross 9 -> 10 and 99 -> 100, and the $len in front of them follows
    for rid, n in (("peak:ctg:I:1:9", 14), ("peak:ctg:I:1:10", 15), ("peak:ctg:II:1:100", 17), ("peak:ctg:I:1:100", 16),
                   ("peak:ctg:I:2:1", 14), ("peak:ctg:III:1:6", 16)):
        assert len(rid) == n and ("$%d\r\n%s\r\n$" % (n, rid)).encode() in want, rid
    assert nxt[pt.ONE_LINE] == 41 and nxt[pt.TWO_LINES] == 6 and nxt["ctg:I:1"] > 500 and nxt[pt.LONG_ID] > 100
    with pytest.raises(host.HostError) as ei:
        host.peak_records_text(eng, ctgs, data, serial_base={"ctg:II:1": -1})
    assert ei.value.code == _lib.EINVAL


def test_serials_end_at_int32_max(eng):
    c = one_ctg()
    d = Device(eng, [c])
    base = {c["id"]: 2147483640}
    try:
        seven, eight = lines_of(7), lines_of(8)
        want, nxt = pr.model([c], seven, "resp", base)
        rc, text, off, got_nxt, rows, _ = abi_records(eng, d, seven, "resp", base)
        assert (rc, rows) == (0, 7) and text == want and got_nxt[0] == 2147483647 == nxt[c["id"]]
        assert b"peak:ctg:I:1:2147483647" in text
        rc, text, off, got_nxt, rows, nb = abi_records(eng, d, eight, "resp", base)
        assert rc == _lib.EINVAL and (text, rows, nb) == (b"", 0, 0) and not off.any()
        assert b"INT32_MAX" in L.gams_gpu_last_error(eng.h)
        rc, text, off, got_nxt, rows, nb = abi_records(eng, d, eight, "resp", {c["id"]: -1})
        assert rc == _lib.EINVAL and nb == 0
        # the handle stays usable
        rc, text, _, got_nxt, rows, _ = abi_records(eng, d, eight, "resp", {c["id"]: 2147483639})
        assert (rc, rows) == (0, 8) and text == pr.model([c], eight, "resp", {c["id"]: 2147483639})[0]
        assert got_nxt[0] == 2147483647
        with pytest.raises(host.HostError) as ei:
            host.peak_records_text(eng, [c], eight, fmt="tsv", serial_base=base, seqset=d.ss)
        assert ei.value.code == _lib.EINVAL
    finally:
        d.close()


# ---- 3. block seams ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kept", [255, 256, 257, 513])
def test_one_ctg_across_the_row_block_seams(eng, kept):
    """one ctg whose kept peaks end on, fill and pass a block of 256 rows; with an empty ctg in front of it the bucket opens
    on a block's first lane"""
    ctgs = [dict(one_ctg(1000, 4, "ctg:I:0"), chr_start=50001, chr_end=51000), one_ctg()]
    data = lines_of(kept)
    want, nxt = pr.model(ctgs, data, "resp", {"ctg:I:1": 95})
    assert want.count(b"*3\r\n") == kept
    got, got_nxt = host.peak_records_text(eng, ctgs, data, fmt="resp", serial_base={"ctg:I:1": 95})
    assert host.last_operator_device() == 1
    assert got == want, first_difference(got, want)
    assert got_nxt == nxt == {"ctg:I:0": 0, "ctg:I:1": 95 + kept}


# ---- 4. blocks beyond the stage ---------------------------------------------------------------------------------------
def test_blocks_beyond_the_stage_beside_staged_ones(eng):
    """130-byte name prefixes on chromosomes I and III: RESP rows of ~570 bytes, 256 of them beyond the 96-KB stage, written
    straight to global memory; the lines of chromosome II keep short names and their blocks are staged"""
    ctgs = pt.synth_ctgs()
    chrom = lambda ln: (parse_line(ln.split("\t")[0].encode()) or ("",))[0]
    long_ = [ln for ln in pt.synth_lines(ctgs, seed=17, n=1500, long_names=True) if chrom(ln) != "II"]
    short = [ln for ln in pt.synth_lines(ctgs, seed=19, n=2500) if chrom(ln) == "II"]
    data = pt.synth_data(long_[:700] + short + long_[700:])
    d = Device(eng, ctgs)
    try:
        for fmt in ("resp", "records", "tsv"):
            want, nxt = pr.model(ctgs, data, fmt)
            rc, text, off, got_nxt, rows, _ = abi_records(eng, d, data, fmt)
            assert rc == 0
            got = in_id_order(d.T, text, off)
            assert got == want, (fmt, first_difference(got, want))
            assert [int(v) for v in got_nxt] == [nxt[c["id"]] for c in d.T.order]
            # the blocks the writer saw: 256 rows each, in the entry's order
            sizes = []
            recs = text.split(b"*3\r\n")[1:] if fmt == "resp" else text.split(b"\n")[:-1]
            assert len(recs) == rows
            for b in range(0, len(recs), 256):
                sizes.append(sum(len(r) + (4 if fmt == "resp" else 1) for r in recs[b:b + 256]))
            stage = TSV_STAGE if fmt == "tsv" else STAGE
            assert sum(sizes) == len(text) and min(sizes[:-1]) <= stage, (fmt, sizes)
            if fmt != "records":                               # (a block of long RECORDS rows is within a few KB of the stage)
                assert max(sizes) > stage, (fmt, sizes)
    finally:
        d.close()


# ---- 5. JSON edges ----------------------------------------------------------------------------------------------------
def flat_commands(stream):
    """every command of a RESP stream through host.resp_parse -> [[arg, ...], ...]"""
    out, at = [], 0
    while at < len(stream):
        flat, used = host.resp_parse(stream[at:])
        assert used > 0
        toks = flat.split("\n")
        assert toks[0] == "*3" and toks[-1] == ""
        out.append([t.split(" ", 1)[1] for t in toks[1:-1]])
        at += used
    return out


def test_json_edges(eng):
    """gc 0.0 and 1.0 (an A/T-only and a G/C-only stretch), an amplitude 0.0 between two peaks of equal gc, an empty
    signal, quotes and backslashes in a signal, a name prefix and the ctg id; every RESP command parses back to
    ["SET", id, json] and the JSON to the eleven fields of the TSV row"""
    rng = np.random.default_rng(8)
    seq = bytearray(rng.choice(np.frombuffer(b"ACGT", np.uint8), 4000).tobytes())
    seq[1000:1200] = b"AT" * 100
    seq[2000:2200] = b"GC" * 100
    ctgs = [dict(id='ctg:"I\\:1', chr_id="I", chr_start=101, chr_end=4100, seq=bytes(seq))]
    lines = ["I:150-160\t0.1\tdropped",
             "I:1101-1150\t0\ta\"b\\c",                   # gc 0
             "I:1151-1200\t0\t",                           # gc 0 again: amplitude 0; an empty signal
             "q\"\\.I(+):2101-2150\t1\t\\\\\"\"",           # gc 1; a name prefix to escape
             "I:2251-2400\t0.6\t1",                       # half inside the G/C stretch
             "I:500-520\t0.4\t-1"]
    data = ("\n".join(lines) + "\n").encode()
    tsv, _ = pr.model(ctgs, data, "tsv", {ctgs[0]["id"]: 9})
    rows = [r.split("\t") for r in tsv.decode().split("\n")[:-1]]
    assert [r[3] for r in rows] == [rows[0][3], "0", "0", "1", rows[4][3]] and rows[2][6] == "0" and rows[1][9] == "0"
    assert rows[3][9] != "0" and rows[3][6] == "1"
    for fmt in ("tsv", "records", "resp"):
        want, _ = pr.model(ctgs, data, fmt, {ctgs[0]["id"]: 9})
        got, _ = host.peak_records_text(eng, ctgs, data, fmt=fmt, serial_base={ctgs[0]["id"]: 9})
        assert host.last_operator_device() == 1
        assert got == want, (fmt, first_difference(got, want))
    assert b'"gc":0.0,' in got and b'"gc":1.0,' in got and b'"left_amplitude":0.0,' in got and b'"right_amplitude":1.0,' in got
    assert b'"signal":"",' in got and b'"range":"q\\"\\\\.I:2101-2150"' in got and b'"id":"peak:ctg:\\"I\\\\:1:10"' in got
    cmds = flat_commands(got)
    assert len(cmds) == len(rows) == 5
    for (verb, rid, js), f in zip(cmds, rows):
        assert verb == "SET" and rid == f[0]
        d = json.loads(js)
        assert list(d) == pr.KEYS
        for k, x in zip(pr.KEYS, f):
            if k in pr.FLOATS:
                assert isinstance(d[k], float) and np.float32(d[k]) == np.float32(float(x)), (k, x)
            elif k in pr.STRINGS:
                assert d[k] == x, k
            else:
                assert d[k] == int(x), k


# ---- 6. what the device refuses ---------------------------------------------------------------------------------------
def test_a_control_byte_in_a_kept_signal_goes_to_the_host(eng):
    c = one_ctg()
    data = lines_of(300, signal=lambda i: "s\x01g" if i == 200 else "1")
    d = Device(eng, [c])
    try:
        for fmt in ("records", "resp"):
            rc, text, off, nxt, rows, nb = abi_records(eng, d, data, fmt, {c["id"]: 3})
            assert rc == _lib.EUNSUPPORTED and (text, rows, nb) == (b"", 0, 0) and not off.any() and nxt[0] == 3
            want, want_nxt = pr.model([c], data, fmt, {c["id"]: 3})
            assert b"s\\u0001g" in want and b"\x01" not in want
            got, got_nxt = host.peak_records_text(eng, [c], data, fmt=fmt, serial_base={c["id"]: 3}, seqset=d.ss)
            assert host.last_operator_device() == 0
            assert got == want, first_difference(got, want)
            assert got_nxt == want_nxt == {c["id"]: 303}
        rc, text, off, nxt, rows, _ = abi_records(eng, d, data, "tsv", {c["id"]: 3})
        assert (rc, rows) == (0, 300) and text == pr.model([c], data, "tsv", {c["id"]: 3})[0] and b"s\x01g" in text
        # in a name prefix too; in the dropped first line of the ctg it is nobody's business
        pre = lines_of(5).replace(b"I:40-", b"n\x02m.I:40-")              # (a kept line: lines_of drops its own first)
        assert pre.count(b"\x02") == 1
        assert abi_records(eng, d, pre, "records")[0] == _lib.EUNSUPPORTED
        assert abi_records(eng, d, b"I:5-9\t0.5\t\x01\n" + lines_of(5), "records")[0] == 0
    finally:
        d.close()


# ---- 7. early ends ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("data", [b"", b"#range\tgc_content\tsignal\n",
                                  b"I:5-9\t0.1\t1\nII:2000-2004\t0.2\t1\nIII:7-9\t0.3\t-1\n"],
                         ids=["empty", "header", "one_line_per_ctg"])
def test_nothing_kept(eng, synth, data):
    ctgs, _ = synth
    base = {"ctg:I:1": 4, "ctg:II:2": 17}
    d = Device(eng, ctgs)
    try:
        for fmt in FORMATS:
            rc, text, off, nxt, rows, nb = abi_records(eng, d, data, fmt, base)
            assert (rc, text, rows, nb) == (0, b"", 0, 0) and not off.any()
            assert [int(v) for v in nxt] == [base.get(c["id"], 0) for c in d.T.order]
        rc, _, off, nxt, _, _ = abi_records(eng, d, data, "resp")                 # no bases: zeros
        assert rc == 0 and not off.any() and not nxt.any()
        got, got_nxt = host.peak_records_text(eng, ctgs, data, fmt="resp", serial_base=base, seqset=d.ss)
        assert got == b"" and got_nxt == {c["id"]: base.get(c["id"], 0) for c in ctgs} and host.last_operator_device() == 1
    finally:
        d.close()


# ---- 8. whose text it is ----------------------------------------------------------------------------------------------
def test_the_text_of_peak_text_outlives_a_records_call(eng, synth):
    ctgs, data = synth
    d = Device(eng, ctgs)
    try:
        T = d.T
        text, nb, rows = C.c_void_p(), C.c_uint64(), C.c_uint64()
        off = np.zeros(len(T.order) + 1, np.uint64)
        assert L.gams_gpu_peak_text(eng.h, d.ss.p, T.ix, T.chr, T.ids, T.slot.ctypes.data, T.cs.ctypes.data, T.ce.ctypes.data,
                                    data, len(data), C.byref(text), C.byref(nb), off.ctypes.data, C.byref(rows)) == 0
        before = C.string_at(text, nb.value)
        rc, rec, _, _, _, _ = abi_records(eng, d, data, "resp", {"ctg:I:1": 1000})
        assert rc == 0 and len(rec) > 2 * len(before)
        assert C.string_at(text, nb.value) == before
        rc, tsv, off2, _, _, _ = abi_records(eng, d, data, "tsv")
        assert rc == 0 and tsv == before and np.array_equal(off, off2)
        assert C.string_at(text, nb.value) == before
        assert abi_records(eng, d, data, "resp", {"ctg:I:1": 1000})[1] == rec
    finally:
        d.close()


# ---- 9. arguments -----------------------------------------------------------------------------------------------------
def test_a_bad_format_and_a_plane_only_seqset(eng, synth):
    ctgs, data = synth
    d = Device(eng, ctgs)
    seqs = seq_arrays(ctgs)
    plane_only = engine.SeqSet(eng, seqs, upload=False)
    try:
        for fmt in (3, -1, 99):
            assert abi_records(eng, d, data, fmt)[0] == _lib.EINVAL
        off, img, plane = image_of(plane_only, seqs)
        plane_only.upload_ranges(None, plane, 0, int(off[-1]) + seqs[-1].size)
        for fmt in FORMATS:
            assert abi_records(eng, d, data, fmt, ss=plane_only)[0] == _lib.ESTATE
        assert abi_records(eng, d, data, "resp")[0] == 0
    finally:
        plane_only.close()
        d.close()
