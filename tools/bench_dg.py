#!/usr/bin/env python3
"""The ΔG column on the workload of profiles/sw_text.txt: 1e5 point features on a 30-Mb chromosome in 1-Mb ctgs, the
rows of size 100 / max 20 (4.09e6 windows of 100 bases), the seqset resident.  In one process, after a warming call each:

  1. the ΔG kernel alone over the rows' ranges (gams_gpu_range_dg_batch, the library's event pair around the kernel),
     with its terms in LDS and in a register read with ds_bpermute, next to sw_kernel<true, false> on the same rows;
  2. gams_gpu_sw_dg_batch whole (wall time to the values in host memory) against gams_dg_polymer_host over the same rows
     on 16 host threads, values compared bit for bit;
  3. gams_gpu_sw_text_dg against gams_gpu_sw_text_actions on the same call, alternating: what the column costs.

usage: tools/bench_dg.py [--reps 5] [--features 100000] [--out FILE]"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--features", type=int, default=100000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from gams_amd import _lib, engine, host, synth

    sink = open(args.out, "w") if args.out else None

    def say(line=""):
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    def med(v):
        return f"median {statistics.median(v):9.3f} ms  (min {min(v):9.3f} .. max {max(v):9.3f})"

    eng = engine.Engine(0)
    G = _lib.load()
    rng = np.random.default_rng(5)
    chrom = synth.chromosome(30_000_000, 9)
    ctgs = synth.gen_ctgs("9", chrom, piece=1000000)
    per = args.features // len(ctgs)
    feats = [np.sort(rng.integers(c["chr_start"] + 1, c["chr_end"] + 1, per)) for c in ctgs]
    seqs = [np.ascontiguousarray(np.frombuffer(c["seq"], np.uint8) if not isinstance(c["seq"], np.ndarray) else c["seq"])
            for c in ctgs]
    ss = engine.SeqSet(eng, seqs)
    sel = np.arange(len(ctgs), dtype=np.uint32)
    cst = np.array([c["chr_start"] for c in ctgs], np.int32)
    foff = (np.arange(len(ctgs) + 1) * per).astype(np.uint64)
    fs = np.concatenate(feats).astype(np.int32)
    fe = fs.copy()
    names = [c["chr_id"] for c in ctgs]
    ids = [f"feature:{c['id']}:{j + 1}" for c in ctgs for j in range(per)]
    d = host.DeltaG()
    kms = C.c_float()

    def kernel_ms():
        assert G.gams_gpu_last_kernel_ms(eng.h, C.byref(kms)) == 0
        return kms.value

    # the rows (and sw_kernel<true, false>'s time on them)
    n = C.c_uint64()
    roff = np.zeros(sel.size + 1, np.uint64)
    a = (eng.h, ss.p, sel.size, sel.ctypes.data, cst.ctypes.data, foff.ctypes.data, fs.ctypes.data, fe.ctypes.data, 100, 20, 500)
    eng.check(G.gams_gpu_sw_batch(*a, None, 0, roff.ctypes.data, C.byref(n)))
    rows = np.zeros(n.value, _lib.SW_ROW_DTYPE)
    sw_ms = []
    for rep in range(args.reps + 1):
        eng.check(G.gams_gpu_sw_batch(*a, rows.ctypes.data, rows.size, roff.ctypes.data, C.byref(n)))
        if rep:
            sw_ms.append(kernel_ms())
    say(f"ΔG of the sw windows: {fs.size} point features on {len(ctgs)} ctgs of 1 Mb, size 100, max 20: {rows.size} rows, "
        f"{int((rows['end'] - rows['start'] + 1).sum()) / 1e6:.0f} Mb of window bases; {args.reps} repetitions after a warming call")
    say(f"device: {eng.device_info()}")
    say(f"1. sw_kernel<true, false> (gc statistics of the same rows)      {med(sw_ms)}")

    # 1. the kernel alone, both table placements
    which = np.repeat(np.arange(sel.size, dtype=np.uint32), np.diff(roff).astype(np.int64))
    r_off = roff.copy()
    rs, re_ = np.ascontiguousarray(rows["start"]), np.ascontiguousarray(rows["end"])
    ref = None
    res = {_lib.DG_TABLE_LDS: [], _lib.DG_TABLE_BPERMUTE: []}
    out = np.zeros(rows.size, np.float32)
    for rep in range(args.reps + 1):
        for mode in res:                                                 # alternating
            eng.check(G.gams_gpu_dg_set_table(eng.h, mode))
            eng.check(G.gams_gpu_range_dg_batch(eng.h, ss.p, sel.size, sel.ctypes.data, cst.ctypes.data, r_off.ctypes.data,
                                                rs.ctypes.data, re_.ctypes.data, C.byref(d.table), out.ctypes.data))
            if ref is None:
                ref = out.copy()
            assert out.tobytes() == ref.tobytes()
            if rep:
                res[mode].append(kernel_ms())
    eng.check(G.gams_gpu_dg_set_table(eng.h, _lib.DG_TABLE_LDS))
    say(f"1. dg_kernel, the sixteen terms in LDS                          {med(res[_lib.DG_TABLE_LDS])}")
    say(f"1. dg_kernel, the terms in a register read with ds_bpermute     {med(res[_lib.DG_TABLE_BPERMUTE])}")
    bases = int((rows["end"] - rows["start"] + 1).sum())
    say(f"   ({bases / statistics.median(res[_lib.DG_TABLE_LDS]) / 1e6:.1f} G bases/s with the terms in LDS; "
        f"{int(np.isnan(ref).sum())} of the rows are None)")

    # 2. the array entry whole against the host twin on 16 threads
    dev, cpu = [], []
    got = np.zeros(rows.size, np.float32)
    o64 = (rs.astype(np.int64) - cst[which].astype(np.int64)).astype(np.uint64)
    ln = (re_ - rs + 1).astype(np.uint32)
    b = (eng.h, ss.p, sel.size, sel.ctypes.data, cst.ctypes.data, foff.ctypes.data, fs.ctypes.data, fe.ctypes.data, 100, 20,
         C.byref(d.table))
    for rep in range(args.reps + 1):
        t0 = time.perf_counter()
        eng.check(G.gams_gpu_sw_dg_batch(*b, got.ctypes.data, got.size, None, C.byref(n)))
        t1 = time.perf_counter()
        twin = host.dg_ranges_host(d, seqs, which, o64, ln, 16)
        t2 = time.perf_counter()
        assert got.tobytes() == ref.tobytes() and twin.tobytes() == ref.tobytes()
        if rep:
            dev.append((t1 - t0) * 1e3)
            cpu.append((t2 - t1) * 1e3)
    say(f"2. gams_gpu_sw_dg_batch, features to the values in host memory  {med(dev)}")
    say(f"2. gams_dg_polymer_host over the same rows, 16 host threads     {med(cpu)}")
    say("   (bit-equal; the host figure has the rows' ranges in hand already, the device figure makes them)")

    # 3. the text with and without the column
    old, new = [], []
    for rep in range(args.reps + 1):
        for name in ("old", "new"):
            t0 = time.perf_counter()
            if name == "old":
                rc, text, _ = engine.sw_text_actions(eng, ss, sel, names, cst, foff, fs, fe, ids, 100, 20, 500, _lib.SW_GC)
            else:
                rc, text, _ = engine.sw_text_dg(eng, ss, sel, names, cst, foff, fs, fe, ids, 100, 20, 500, _lib.SW_GC, d.table)
            dt = (time.perf_counter() - t0) * 1e3
            assert rc == 0 and text.count(b"\n") == rows.size
            if rep:
                (old if name == "old" else new).append(dt)
            size = len(text)
    say(f"3. gams_gpu_sw_text_actions (-a gc), wall through the binding   {med(old)}")
    say(f"3. gams_gpu_sw_text_dg      (-a gc), wall through the binding   {med(new)}   ({size / 1e6:.0f} MB of text)")
    say(f"   the column costs {statistics.median(new) - statistics.median(old):.1f} ms a call "
        "(both figures include the binding's id strings and its copy of the text)")
    ss.close()
    eng.close()


if __name__ == "__main__":
    main()
