"""CPU checks behind gams_spans_create_runlist_text / host.AnnoSet: the model of tests/runlist_text.py against json.load
on the golden intergenic.json, the host reader (gams::read_runlist_json through host.read_runlist_json) against the
model on the edge documents, each GAMS_EINVAL case by its own document, the new entries' declarations, and the reader's
translation unit alone behind the stand-alone driver tests/runlist_main.cpp (host compiler with the address and
undefined-behaviour sanitizers, no HIP, no device) on every edge document and each of them cut at every byte."""
import ctypes as C
import json
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import helpers
import runlist_text as rt
from gams_amd import _lib, host

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN_SPANS = [25, 85, 32, 176, 47, 79, 30, 122, 62, 69, 75, 110, 99, 88, 140, 108]


def golden_bytes():
    with open(os.path.join(helpers.S288C, "intergenic.json"), "rb") as fh:
        return fh.read()


# ---- the model and the host reader on the fixture ---------------------------------------------------------------------
def test_golden_fixture():
    data = golden_bytes()
    js = json.loads(data)
    want = rt.model(data)
    assert list(want) == list(js) and [v[0].size for v in want.values()] == GOLDEN_SPANS
    for k, text in js.items():                              # already normalised: the model gives the file's spans back
        assert rt.runlist_of(zip(want[k][0].tolist(), want[k][1].tolist())) == text
    ref = helpers.read_runlists("intergenic.json")
    assert rt.same_sets(want, ref)
    assert rt.device_takes(data)
    got = host.read_runlist_json(data)
    assert rt.same_sets(got, want)
    assert all(v[0].dtype == np.int32 and v[1].dtype == np.int32 for v in got.values())


# ---- edge documents ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(rt.EDGE_OK))
def test_edge_documents(name):
    data = rt.EDGE_OK[name]
    want = rt.model(data)
    assert rt.same_sets(host.read_runlist_json(data), want), name


def test_edge_documents_say_what_they_claim():
    m = {k: rt.model(v) for k, v in rt.EDGE_OK.items()}
    assert list(m["escapes in keys"]) == ['a"b\\c/\b\f\n\r\tAé\U0001f600', "x\0y"]
    assert list(m["duplicate key"]) == ["I", "II"] and m["duplicate key"]["I"][0].tolist() == [20, 40]
    assert [v[0].size for v in m["empty values"].values()] == [0, 0, 1]
    assert m["negative spans"]["I"][0].tolist() == [-20, -5, 3] and m["negative spans"]["I"][1].tolist() == [-9, -1, 4]
    assert m["joins into one"]["I"][0].tolist() == [1] and m["joins into one"]["I"][1].tolist() == [50]
    assert m["single number"]["I"][0].tolist() == [7] == m["single number"]["I"][1].tolist()
    assert m["int32 max"]["I"][1].tolist() == [rt.I32_MAX] and m["int32 max"]["II"][0].tolist() == [1, rt.I32_MAX - 1]
    assert m["int32 max"]["III"][0].tolist() == [rt.I32_MIN]
    assert m["no group"] == {} and m["no group, white space"] == {}
    assert rt.same_sets(m["compact"], m["pretty"]) and rt.same_sets(m["compact"], m["crlf"])
    assert b"\r\n" in rt.EDGE_OK["crlf"] and b"\n" in rt.EDGE_OK["pretty"] and b" " not in rt.EDGE_OK["compact"]
    assert m["empty tokens"]["I"][0].tolist() == [1, 5] and m["empty tokens"]["II"][0].size == 0
    # the device's grammar is the narrower one: what it takes, the host reads the same way
    takes = {k for k, v in rt.EDGE_OK.items() if rt.device_takes(v)}
    assert takes == {"empty values", "joins into one", "single number", "no group", "no group, white space", "compact",
                     "pretty", "crlf", "empty key"}
    assert not any(rt.device_takes(v) for v in rt.EDGE_EINVAL.values())


@pytest.mark.parametrize("name", sorted(rt.EDGE_EINVAL))
def test_einval_documents(name):
    data = rt.EDGE_EINVAL[name]
    with pytest.raises(rt.Invalid):
        rt.model(data)
    with pytest.raises(host.HostError) as ei:
        host.read_runlist_json(data)
    assert ei.value.code == _lib.EINVAL, name


def test_normalise_and_directory_model():
    lo, hi = rt.normalise([(5, 9), (1, 3), (4, 4), (20, 30), (25, 27), (31, 31), (40, 41)])
    assert lo.tolist() == [1, 20, 40] and hi.tolist() == [9, 31, 41]
    assert rt.normalise([])[0].size == 0
    assert rt.normalise([(rt.I32_MAX, rt.I32_MAX), (rt.I32_MAX - 1, rt.I32_MAX - 1)])[1].tolist() == [rt.I32_MAX]
    # build_dir: dir[b] = spans with biased lo below the bucket's edge, dir[nb] = n; nb <= n
    key0, shift, nb, d = rt.span_dir(np.array([1, 2, 3, 1000], np.int32))
    assert (key0, nb) == (2**31 + 1, 4) and shift == 8 and d.tolist() == [0, 3, 3, 3, 4]
    assert rt.span_dir(np.array([7], np.int32))[1:3] == (0, 1)
    spread = np.linspace(1, rt.I32_MAX - 1, 8193).astype(np.int64).astype(np.int32)
    assert rt.span_dir(spread)[1] >= 18 and rt.span_dir(np.arange(100, 164, 2, dtype=np.int32))[1] == 1
    assert rt.span_dir(np.zeros(0, np.int32))[2] == 0


# ---- the new entries ---------------------------------------------------------------------------------------------------
def test_new_entries_are_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "gams_gpu.h")).read()
    assert re.search(r"\bint\s+gams_spans_create_runlist_text\s*\(", hdr) and re.search(r"\bint\s+gams_spans_read\s*\(", hdr)
    lib = C.CDLL(_lib.SO_PATH)
    vp, u64p = C.c_void_p, C.POINTER(C.c_uint64)
    assert _lib.PROTOTYPES["gams_spans_create_runlist_text"] == (C.c_int, [vp, vp, C.c_uint64, C.POINTER(vp), C.POINTER(vp),
                                                                           C.POINTER(C.c_uint32), u64p])
    assert _lib.PROTOTYPES["gams_spans_read"] == (C.c_int, [vp, vp, vp, vp, vp, C.c_uint64, u64p])
    for name in ("gams_spans_create_runlist_text", "gams_spans_read", "gams_names_read"):
        assert hasattr(lib, name), name
    hl = C.CDLL(host.SO_PATH)
    for name in ("gams_host_anno_set_create", "gams_host_anno_set_destroy", "gams_host_anno_text_set", "gams_host_anno_set_device",
                 "gams_host_read_runlist_json", "gams_host_read_runlist_json_get", "gams_host_runlist_load"):
        assert hasattr(hl, name), name
    for fn in (host.AnnoSet, host.read_runlist_json, host.read_runlist_text, host.runlist_load):
        assert callable(fn)
    assert "runlist.hip" in open(os.path.join(ROOT, "gams_amd", "csrc", "Makefile")).read()
    assert "gams_spans_create_runlist_text" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_null_arguments_without_a_device():
    lib = _lib.load()
    sp, nm = C.c_void_p(1), C.c_void_p(1)
    ng, ns = C.c_uint32(), C.c_uint64()
    assert lib.gams_spans_create_runlist_text(None, b"{}", 2, C.byref(sp), C.byref(nm), C.byref(ng), C.byref(ns)) == _lib.EINVAL
    assert sp.value is None and nm.value is None            # nothing is created on any return but GAMS_OK
    assert lib.gams_spans_read(None, None, None, None, None, 0, C.byref(ns)) == _lib.EINVAL


# ---- the reader's translation unit alone, under the sanitizers ---------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("runlist") / "runlist_main"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(HERE, "runlist_main.cpp"),
                           os.path.join(ROOT, "gams_amd", "host", "gams_runlist.cpp"), "-o", str(exe)])
    return str(exe)


def show(sets):
    return ";".join(k.encode("utf-8").hex() + "=" + ",".join(f"{a}:{b}" for a, b in zip(v[0].tolist(), v[1].tolist()))
                    for k, v in sets.items())


def test_driver_on_every_document_and_every_cut(driver, tmp_path):
    docs = [rt.EDGE_OK[k] for k in sorted(rt.EDGE_OK)] + [rt.EDGE_EINVAL[k] for k in sorted(rt.EDGE_EINVAL)]
    docs.append(golden_bytes()[:1500] + b'"}')              # a longer value, cut inside numbers, dashes and commas
    path = tmp_path / "docs.bin"
    path.write_bytes(b"".join(struct.pack("<I", len(d)) + d for d in docs))
    res = subprocess.run([driver, str(path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert res.returncode == 0 and res.stderr == "", res.stderr[-2000:]
    lines = res.stdout.split("\n")[:-1]
    assert len(lines) == 2 * len(docs)
    accepted = 0
    for i, d in enumerate(docs):
        want = rt.verdict(d)
        assert lines[2 * i] == (f"D {i} E" if want is None else f"D {i} A {show(want)}"), d
        cuts = "".join("E" if rt.verdict(d[:k]) is None else "A" for k in range(len(d)))
        assert lines[2 * i + 1] == f"T {i} {cuts}", d
        accepted += cuts.count("A")
    assert accepted >= 2          # a document that ends in white space stays whole without it; every other cut is invalid
