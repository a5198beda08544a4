#!/usr/bin/env python3
"""The records `gams peak` stores, on an A. thaliana-shaped genome: the 65 k rows of host.wave in -> one record per kept
peak out, from a resident seqset (the workload of profiles/peak_text.txt, leg A).

    tools/bench_peak_records.py [--runs 7] [--out FILE] [--swapped LIB] [--lines N]

Every figure is measured in a process of its own (this tool starts one child per figure, one after the other), behind
two warming calls, and is the median of --runs calls:

  (a) records / tsv / resp   host.peak_records_text(eng, ctgs, data, fmt, seqset=ss): wall-clock around the Python call,
                             the C++ operator alone (host.last_operator_ms) and the ten stages of the entry
                             (gams_gpu_last_stage_ms);
  (b) replaced               what a host did before: host.peak_text(eng, ctgs, data, seqset=ss), then the operator's own
                             host formatter over those rows (host.peak_rows_records(rows, "resp")); the two timed apart;
  (c) stage                  gams_gpu_peak_records_text through the C ABI in the three formats: the write stage and the
                             sum of the ten.  With --swapped LIB the same on a second build of libgams_gpu.so, compiled
                             with -DGAMS_PEAK_REC_STAGE=32768 -DGAMS_PEAK_REC_TSV_STAGE=98304: RESP and RECORDS behind
                             the 32-KB stage of peak_text, TSV behind the 96-KB one.  With --lines N, (c) again on N
                             synthetic position-sorted rows over the same ctgs (bench_peak_e2e.synth_rows): many row
                             blocks a CU, where a stage that leaves room for one workgroup a CU has something to lose.

The child that makes the wave rows writes them to a file the others read; (b)'s text is compared with (a)'s."""
import argparse
import ctypes as C
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench_peak_e2e import synth_rows  # noqa: E402
from gams_amd import _lib, engine, host, synth  # noqa: E402

STAGES = ("lines", "parse", "locate", "first", "keep", "offsets", "order", "gc", "rows", "write")
FORMATS = {"records": _lib.LOADER_RECORDS, "tsv": _lib.LOADER_TSV, "resp": _lib.LOADER_RESP}
WARM = 2


def genome():
    return [dict(id=c["id"], chr_id=c["chr_id"], chr_start=c["chr_start"], chr_end=c["chr_end"], seq=c["seq"])
            for c in synth.genome_ctgs(synth.ATHA_LENGTHS, 500000)]


def stage_ms(eng):
    ms, n = (C.c_float * 16)(), C.c_uint32()
    eng.check(eng.lib.gams_gpu_last_stage_ms(eng.h, ms, 16, C.byref(n)))
    assert n.value == len(STAGES)
    return [float(ms[k]) for k in range(n.value)]


def med(xs):
    return statistics.median(xs)


def spread(xs):
    return f"{med(xs):8.3f} (min {min(xs):.3f}, max {max(xs):.3f})"


def stages_line(per_call):
    cols = list(zip(*per_call))
    return "  ".join(f"{k} {med(v) * 1e3:.0f}" for k, v in zip(STAGES, cols)) + f"  | sum {med([sum(c) for c in per_call]) * 1e3:.0f}"


def fig_wave(args):
    eng = engine.Engine(0)
    ctgs = genome()
    rows = host.wave(eng, ctgs)
    with open(args.rows, "w") as fh:
        fh.write(rows if rows.endswith("\n") else rows + "\n")
    print(f"device {eng.device_info()}; {len(ctgs)} ctgs, {sum(len(c['seq']) for c in ctgs)} bases; "
          f"{rows.count(chr(10))} wave rows, {os.path.getsize(args.rows)} bytes", flush=True)
    eng.close()


def fig_format(args, fmt):
    eng = engine.Engine(0)
    ctgs = genome()
    data = open(args.rows, "rb").read()
    ss = engine.SeqSet(eng, [c["seq"] for c in ctgs])
    wall, op, st = [], [], []
    for r in range(WARM + args.runs):
        t0 = time.perf_counter()
        text, nxt = host.peak_records_text(eng, ctgs, data, fmt=fmt, seqset=ss)
        t = (time.perf_counter() - t0) * 1e3
        assert host.last_operator_device() == 1
        if r >= WARM:
            wall.append(t)
            op.append(host.last_operator_ms())
            st.append(stage_ms(eng))
    print(f"(a) {fmt:8s} {sum(nxt.values())} records, {len(text)} bytes ({len(text) / max(sum(nxt.values()), 1):.0f} a record)")
    print(f"    wall ms {spread(wall)} | operator ms {spread(op)}")
    print(f"    stages, us: {stages_line(st)}", flush=True)
    if args.keep:
        open(args.keep, "wb").write(text)
    ss.close()
    eng.close()


def fig_replaced(args):
    eng = engine.Engine(0)
    ctgs = genome()
    data = open(args.rows, "rb").read()
    ss = engine.SeqSet(eng, [c["seq"] for c in ctgs])
    t_rows, op_rows, t_fmt = [], [], []
    for r in range(WARM + args.runs):
        t0 = time.perf_counter()
        rows = host.peak_text(eng, ctgs, data, seqset=ss)
        t1 = time.perf_counter()
        op = host.last_operator_ms()
        assert host.last_operator_device() == 1
        t2 = time.perf_counter()
        resp = host.peak_rows_records(rows, "resp")
        t3 = time.perf_counter()
        if r >= WARM:
            t_rows.append((t1 - t0) * 1e3)
            op_rows.append(op)
            t_fmt.append((t3 - t2) * 1e3)
    same = args.keep and resp == open(args.keep, "rb").read()
    print(f"(b) replaced: host.peak_text, then the host formatter to RESP; {len(rows)} bytes of rows -> {len(resp)} bytes"
          f"{' (the text of (a) resp, compared)' if same else ' (NOT compared)'}")
    print(f"    peak_text wall ms {spread(t_rows)} | operator ms {spread(op_rows)}")
    print(f"    host formatter wall ms {spread(t_fmt)}")
    print(f"    together, wall ms {spread([a + b for a, b in zip(t_rows, t_fmt)])}", flush=True)
    ss.close()
    eng.close()


def fig_stage(args):
    """the C ABI on one build of libgams_gpu.so (no host layer in the process): tables as gams::Locator lays them out"""
    lib = _lib.bind(os.path.abspath(args.lib)) if args.lib else _lib.load()
    eng = engine.Engine(0, lib=lib)
    ctgs = genome()
    data = ("\n".join(synth_rows(ctgs, args.lines)) + "\n").encode() if args.lines else open(args.rows, "rb").read()
    ss = engine.SeqSet(eng, [c["seq"] for c in ctgs])
    chrs = sorted({c["chr_id"] for c in ctgs}, key=lambda k: k.encode())
    order = [c for k in chrs for c in ctgs if c["chr_id"] == k]
    slot_of = {c["id"]: i for i, c in enumerate(ctgs)}
    goff = np.cumsum([0] + [sum(c["chr_id"] == k for c in ctgs) for k in chrs]).astype(np.uint64)
    ix = engine.Index(eng, goff, [c["chr_start"] for c in order], [c["chr_end"] + 1 for c in order])

    def names(xs):
        p = C.c_void_p()
        eng.check(lib.gams_names_create(eng.h, len(xs), (C.c_char_p * len(xs))(*[x.encode() for x in xs]), C.byref(p)))
        return p

    chr_nm, id_nm = names(chrs), names([c["id"] for c in order])
    slot = np.array([slot_of[c["id"]] for c in order], np.uint32)
    cs = np.array([c["chr_start"] for c in order], np.int32)
    ce = np.array([c["chr_end"] for c in order], np.int32)
    off = np.zeros(len(order) + 1, np.uint64)
    print(f"(c) {args.lib or 'this build'}" + (f", {args.lines} synthetic lines" if args.lines else ""))
    for fmt in ("resp", "records", "tsv"):
        st, nb, rows, text = [], C.c_uint64(), C.c_uint64(), C.c_void_p()
        for r in range(WARM + args.runs):
            eng.check(lib.gams_gpu_peak_records_text(eng.h, ss.p, ix.p, chr_nm, id_nm, slot.ctypes.data, cs.ctypes.data,
                                                     ce.ctypes.data, data, len(data), FORMATS[fmt], None, C.byref(text),
                                                     C.byref(nb), off.ctypes.data, None, C.byref(rows)))
            if r >= WARM:
                st.append(stage_ms(eng))
        w = [c[-1] * 1e3 for c in st]
        print(f"    {fmt:8s} {rows.value} rows, {nb.value} bytes: write us {med(w):6.1f} (min {min(w):.1f}, max {max(w):.1f}) "
              f"| rows us {med([c[-2] * 1e3 for c in st]):.1f} | ten stages us {med([sum(c) * 1e3 for c in st]):.0f}", flush=True)
    lib.gams_names_destroy(eng.h, chr_nm)
    lib.gams_names_destroy(eng.h, id_nm)
    ix.close()
    ss.close()
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--swapped", default=None, help="a build of libgams_gpu.so with the two stage sizes swapped")
    ap.add_argument("--lines", type=int, default=0, help="(c) once more on this many synthetic rows")
    ap.add_argument("--figure", default=None, help="(internal) the one figure this process measures")
    ap.add_argument("--rows", default=None, help="(internal) the file of wave rows")
    ap.add_argument("--keep", default=None, help="(internal) where (a) resp leaves its text for (b)")
    ap.add_argument("--lib", default=None, help="(internal) the build (c) runs on")
    args = ap.parse_args()
    if args.runs < 5:
        ap.error("--runs: at least 5")
    if args.figure:
        if args.figure == "wave":
            fig_wave(args)
        elif args.figure in FORMATS:
            fig_format(args, args.figure)
        elif args.figure == "replaced":
            fig_replaced(args)
        else:
            fig_stage(args)
        return
    out = open(args.out, "w") if args.out else None
    with tempfile.TemporaryDirectory() as tmp:
        rows, keep = os.path.join(tmp, "wave.tsv"), os.path.join(tmp, "resp.bin")
        figures = [["wave"], ["records"], ["tsv"], ["resp", "--keep", keep], ["replaced", "--keep", keep], ["stage"]]
        if args.swapped:
            figures.append(["stage", "--lib", args.swapped])
        if args.lines:
            figures.append(["stage", "--lines", str(args.lines)])
            if args.swapped:
                figures.append(["stage", "--lines", str(args.lines), "--lib", args.swapped])
        for f in figures:
            cmd = [sys.executable, os.path.abspath(__file__), "--runs", str(args.runs), "--rows", rows, "--figure"] + f
            p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
            print(p.stdout, end="", flush=True)
            if out:
                out.write(p.stdout)
                out.flush()
            if p.returncode != 0:                               # nothing more is started behind a failure
                sys.exit(f"figure {f[0]} ended with {p.returncode}")


if __name__ == "__main__":
    main()
