"""CPU checks of the records `gams peak` stores (gams_gpu_peak_records_text, host.peak_records_text): the JSON float rule
(host.fmt_f32_json) over its domain, the pure-Python model (tests/peak_records.py) against records written by hand, the
host formatter of the operator's host route against the model, and that the entry is declared, bound and exported.
tests/test_gpu_peak_records.py compares the device with the model."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import peak_records as pr
import peak_text as pt
from gams_amd import _lib, host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fmt_f32_json_round_trips_and_is_the_shortest_positional_text():
    rng = np.random.default_rng(5)
    lo, hi = np.float32(1e-5), np.float32(1.0)
    vals = [np.float32(0), np.float32(1), np.float32(0.5), np.float32(0.0268), np.float32(0.3) - np.float32(0.1), lo]
    vals += list(np.exp(rng.uniform(np.log(1e-5), 0.0, 5000)).astype(np.float32))       # every decade alike
    vals += list(rng.uniform(1e-5, 1.0, 5000).astype(np.float32))
    for v in vals:
        if not (v == 0 or lo <= v <= hi):
            continue                                            # (the f32 cast may round a draw below the f32 1e-5)
        s = host.fmt_f32_json(float(v))
        assert np.float32(float(s)) == v, (v, s)
        assert s == np.format_float_positional(v, unique=True, trim="0"), (v, s)
        assert "." in s and "e" not in s
    assert host.fmt_f32_json(0.0) == "0.0" and host.fmt_f32_json(1.0) == "1.0"
    assert host.fmt_f32_json(0.0268) == "0.0268" and host.fmt_f32_json(float(lo)) == "0.00001"


@pytest.mark.parametrize("v", [5e-6, 9.9e-6, float("nan"), -0.0, -0.5, 1.0000001, 2.0, float("inf"), 1e-40])
def test_fmt_f32_json_raises_outside_its_set(v):
    with pytest.raises(host.HostError):
        host.fmt_f32_json(v)


# three peaks in one ctg over A/T-only bases: gc 0 everywhere, so every amplitude is 0; the first line is dropped
HAND_CTG = dict(id="ctg:I:1", chr_id="I", chr_start=1, chr_end=1000, seq=b"AT" * 500)
HAND = b'I:5-9\t0.1\tx\nnm.I(+):101-200\t0.2\ta"b\\c\nI:301\t0.3\t\n'
HAND_JSON_1 = ('{"id":"peak:ctg:I:1:8","range":"nm.I:101-200","length":100,"gc":0.0,"signal":"a\\"b\\\\c",'
               '"left_wave_length":101,"left_amplitude":0.0,"left_signal":"a\\"b\\\\c",'
               '"right_wave_length":102,"right_amplitude":0.0,"right_signal":""}')
HAND_JSON_2 = ('{"id":"peak:ctg:I:1:9","range":"I:301","length":1,"gc":0.0,"signal":"",'
               '"left_wave_length":102,"left_amplitude":0.0,"left_signal":"a\\"b\\\\c",'
               '"right_wave_length":700,"right_amplitude":0.0,"right_signal":""}')


def test_the_model_against_records_written_by_hand():
    base = {"ctg:I:1": 7}
    tsv, nxt = pr.model([HAND_CTG], HAND, "tsv", base)
    assert tsv == (b'peak:ctg:I:1:8\tnm.I:101-200\t100\t0\ta"b\\c\t101\t0\ta"b\\c\t102\t0\t\n'
                   b'peak:ctg:I:1:9\tI:301\t1\t0\t\t102\t0\ta"b\\c\t700\t0\t\n')
    assert nxt == {"ctg:I:1": 9}
    rec, _ = pr.model([HAND_CTG], HAND, "records", base)
    assert rec.decode() == "peak:ctg:I:1:8\t" + HAND_JSON_1 + "\npeak:ctg:I:1:9\t" + HAND_JSON_2 + "\n"
    resp, _ = pr.model([HAND_CTG], HAND, "resp", base)
    assert resp.decode() == ("*3\r\n$3\r\nSET\r\n$14\r\npeak:ctg:I:1:8\r\n$%d\r\n%s\r\n" % (len(HAND_JSON_1), HAND_JSON_1) +
                             "*3\r\n$3\r\nSET\r\n$14\r\npeak:ctg:I:1:9\r\n$%d\r\n%s\r\n" % (len(HAND_JSON_2), HAND_JSON_2))
    for text in (HAND_JSON_1, HAND_JSON_2):
        d = json.loads(text)
        assert list(d) == pr.KEYS and d["gc"] == 0.0
    assert json.loads(HAND_JSON_1)["signal"] == 'a"b\\c'


def test_the_models_tsv_with_zero_bases_is_peak_texts():
    ctgs = pt.synth_ctgs()
    data = pt.synth_data(pt.synth_lines(ctgs, n=600))
    want = pt.model(ctgs, data)
    assert want.count(b"\n") > 400
    got, nxt = pr.model(ctgs, data, "tsv")
    assert got == want
    assert sum(nxt.values()) == want.count(b"\n") and nxt[pt.ONE_LINE] == 0 and nxt[pt.TWO_LINES] == 1
    # ... and the three formats carry the same fields
    rec, _ = pr.model(ctgs, data, "records", {"ctg:I:1": 99})
    rows = got.decode("latin-1").split("\n")[:-1]
    recs = rec.decode("latin-1").split("\n")[:-1]
    assert len(rows) == len(recs)
    for row, r in zip(rows, recs):
        rid, js = r.split("\t", 1)
        d, f = json.loads(js), row.split("\t")
        assert list(d) == pr.KEYS and d["id"] == rid
        assert rid.rsplit(":", 1)[0] == f[0].rsplit(":", 1)[0]
        assert int(rid.rsplit(":", 1)[1]) == int(f[0].rsplit(":", 1)[1]) + (99 if rid.startswith("peak:ctg:I:1:") else 0)
        assert [str(d[k]) if k not in pr.FLOATS else None for k in pr.KEYS[1:]] == \
               [x if k not in pr.FLOATS else None for k, x in zip(pr.KEYS[1:], f[1:])]
        assert all(np.float32(d[k]) == np.float32(float(x)) for k, x in zip(pr.KEYS, f) if k in pr.FLOATS)


def test_the_host_formatter_is_the_models():
    """host.peak_rows_records (gams::peak_records_rows, the formatter of the operator's host route) over rows with
    quotes, backslashes, every control byte a signal can hold, gc 0 and 1"""
    ctl = "".join(chr(c) for c in range(1, 0x20) if chr(c) not in "\t\n")
    rows = [["peak:ctg:I:1:10", 'n"m\\.I:5-9', "5", "0", "1", "5", "0", "1", "-3", "0.026800007", 'q"\\'],
            ['peak:c"\\:2147483647', "I:7", "1", "1", "", "1", "1", "s" + ctl, "2", "0.00011", ctl],
            ["peak:ctg:I:1:11", "I:7-9", "3", "0.5", "-1", "-2147483648", "0.0268", "", "2147483647", "0.1", "1"]]
    tsv = "".join("\t".join(f) + "\n" for f in rows).encode("latin-1")
    for fmt in ("tsv", "records", "resp"):
        want = "".join(pr.record(f, fmt) for f in rows).encode("latin-1")
        assert host.peak_rows_records(tsv, fmt) == want, fmt
    js = pr.json_of(rows[1])
    assert "\\u0001" in js and "\\b" in js and "\\f" in js and "\\r" in js and "\\u001f" in js and "\\u000b" in js
    assert json.loads(js)["right_signal"] == ctl
    with pytest.raises(host.HostError):                        # an amplitude serde_json prints with an exponent
        host.peak_rows_records(b"peak:c:1\tI:7\t1\t0.5\t1\t1\t0.000001\t1\t2\t0\t1\n", "records")
    with pytest.raises(host.HostError):
        host.peak_rows_records(b"peak:c:1\tI:7\t1\n", "records")


def test_the_entry_is_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "gams_gpu.h")).read()
    name = "gams_gpu_peak_records_text"
    assert re.search(r"\bint\s+" + name + r"\s*\(", hdr)
    assert name in _lib.PROTOTYPES and len(_lib.PROTOTYPES[name][1]) == 17
    assert hasattr(C.CDLL(_lib.SO_PATH), name)
    assert hasattr(_lib.load(), name)
    lib = host.load()
    for sym in ("gams_host_peak_records_text", "gams_host_peak_rows_records", "gams_host_fmt_f32_json"):
        assert hasattr(lib, sym), sym
    # null arguments and a bad format never reach the device
    text, nb, rows = C.c_void_p(), C.c_uint64(), C.c_uint64()
    assert _lib.load().gams_gpu_peak_records_text(None, None, None, None, None, None, None, None, None, 0, 0, None,
                                                  C.byref(text), C.byref(nb), None, None, C.byref(rows)) == _lib.EINVAL
    with pytest.raises(ValueError):
        host.peak_records_text(None, [], b"", fmt="json")
