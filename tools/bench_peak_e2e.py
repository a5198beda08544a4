#!/usr/bin/env python3
"""`gams wave` then `gams peak` (peak.rs:24-177) on an A. thaliana-shaped genome through the host layer: the wave TSV rows
(65 k) in -> the Peak rows out, and the same on a synthetic wave TSV of 10^6 position-sorted lines over the same ctg
table.  Two arms, alternating: host.peak (the lines split, parsed and bucketed on the host, one range_gc call) and
host.peak_text (the bytes of the file to the finished rows on the device), the latter uploading the sequences for the
call and on a resident seqset.  Both inputs are position-sorted, so the arms print the same text (asserted).

    tools/bench_peak_e2e.py [--rounds N] [--lines N] [--out FILE]

ms are wall-clock around the Python call (the binding's own copies included: host.peak joins its lines into one buffer,
timed apart as `join`); for peak_text also the C++ operator's own time (host.last_operator_ms: Locator, name tables,
seqset if it uploads one, the entry, the concatenation in id order) and the entry's stages (gams_gpu_last_stage_ms)."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gams_amd import engine, host, synth  # noqa: E402

STAGES = ("lines", "parse", "locate", "first", "keep", "offsets", "order", "gc", "rows", "write")


def synth_rows(ctgs, n, seed=5):
    """n wave rows over the ctgs, position-sorted inside each: ranges of 100-300 bases inside their ctg"""
    rng = np.random.default_rng(seed)
    total = sum(c["chr_end"] - c["chr_start"] + 1 for c in ctgs)
    rows = []
    for c in ctgs:
        k = max(2, round(n * (c["chr_end"] - c["chr_start"] + 1) / total))
        s = np.sort(rng.integers(c["chr_start"], c["chr_end"] - 300, k))
        e = s + rng.integers(99, 300, k)
        g = rng.integers(0, 100, k)
        sg = rng.integers(0, 2, k) * 2 - 1
        rows += [f"{c['chr_id']}:{a}-{b}\t0.{x}\t{y}" for a, b, x, y in zip(s.tolist(), e.tolist(), g.tolist(), sg.tolist())]
    return rows


def stage_ms(eng):
    ms = (C.c_float * 16)()
    n = C.c_uint32()
    eng.check(eng.lib.gams_gpu_last_stage_ms(eng.h, ms, 16, C.byref(n)))
    return [float(ms[k]) for k in range(n.value)]


def leg(eng, ctgs, ss, rows, rounds, say):
    data = ("\n".join(rows) + "\n").encode()
    t0 = time.perf_counter()
    "\n".join(rows).encode()
    join_ms = (time.perf_counter() - t0) * 1e3
    say(f"  {len(rows)} lines, {len(data)} bytes; join of the lines (inside host.peak's wall time): {join_ms:.1f} ms")
    want = None
    for r in range(rounds + 1):                          # round 0 warms the pools and is not reported
        t0 = time.perf_counter()
        a = host.peak(eng, ctgs, rows).encode()
        t_host = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        b = host.peak_text(eng, ctgs, data)
        t_up, op_up, dev = (time.perf_counter() - t0) * 1e3, host.last_operator_ms(), host.last_operator_device()
        st_up = stage_ms(eng)
        t0 = time.perf_counter()
        c = host.peak_text(eng, ctgs, data, seqset=ss)
        t_res, op_res = (time.perf_counter() - t0) * 1e3, host.last_operator_ms()
        st_res = stage_ms(eng)
        assert a == b == c and dev == 1
        want = a
        if r == 0:
            continue
        say(f"  round {r}: host.peak {t_host:8.1f} ms | peak_text uploading {t_up:7.1f} ms (operator {op_up:7.1f}) | "
            f"resident seqset {t_res:7.1f} ms (operator {op_res:7.1f})")
        say("           stages, us (uploading): " + "  ".join(f"{k} {v * 1e3:.0f}" for k, v in zip(STAGES, st_up)))
        say("           stages, us (resident):  " + "  ".join(f"{k} {v * 1e3:.0f}" for k, v in zip(STAGES, st_res)))
    say(f"  {want.count(b'%c' % 10)} Peak rows, {len(want)} bytes, identical in the three arms")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--lines", type=int, default=1_000_000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out = open(args.out, "w") if args.out else None

    def say(s):
        print(s, flush=True)
        if out:
            out.write(s + "\n")
            out.flush()

    eng = engine.Engine(0)
    ctgs = [dict(id=c["id"], chr_id=c["chr_id"], chr_start=c["chr_start"], chr_end=c["chr_end"], seq=c["seq"])
            for c in synth.genome_ctgs(synth.ATHA_LENGTHS, 500000)]
    ss = engine.SeqSet(eng, [c["seq"] for c in ctgs])
    say(f"device {eng.device_info()}; {len(ctgs)} ctgs, {sum(len(c['seq']) for c in ctgs)} bases")
    say("leg A: the rows of host.wave over the genome")
    leg(eng, ctgs, ss, host.wave(eng, ctgs).splitlines(), args.rounds, say)
    say(f"leg B: {args.lines} synthetic position-sorted rows on the same ctg table")
    leg(eng, ctgs, ss, synth_rows(ctgs, args.lines), args.rounds, say)
    ss.close()
    eng.close()


if __name__ == "__main__":
    main()
