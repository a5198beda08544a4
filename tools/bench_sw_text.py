#!/usr/bin/env python3
"""`sw` from the bytes of a feature file: today's route (read_range on the lines, the ids made in Python, sw_multi)
against host.sw_text with host sequences and host.sw_text on a resident SeqSet, in one process, alternating.  The
input is that of bench_sw_e2e.py: a 30-Mb synthetic chromosome in 1-Mb ctgs and 1e5 point features, written as range
lines; leg A position-sorted (the shape of a real feature file), leg B the same lines shuffled.

usage: tools/bench_sw_text.py [--reps 5] [--features 100000] [--out FILE]
Per route: the wall time of the whole route from the bytes (or lines) to the text, and the time inside the C++
operators (today's route: the read_range call has no inner clock, so its wall time, plus sw_multi_timed's operator
ms; sw_text: gams_host_last_operator_ms), as median and min .. max over the repetitions after one warming call each;
then the stages of the entry from the library's stopwatch."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STAGES = ("lines (upload + line index)", "parse", "locate", "first line per ctg (atomicMin)", "keep + count (atomicAdd)",
          "offsets (scan)", "order (radix sort)", "gather + middle check", "geometry (rows per feature, scans)",
          "rows (sw_kernel)", "text lengths", "text write")


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

    eng = engine.Engine(0)
    G = _lib.load()
    rng = np.random.default_rng(5)
    chrom = synth.chromosome(30_000_000, 9)
    ctgs = synth.gen_ctgs("9", chrom, piece=1000000)
    by_id = sorted(ctgs, key=lambda c: c["id"].encode())                 # sw.rs:97: the ctgs in id order
    pos = np.sort(np.concatenate([rng.integers(c["chr_start"] + 1, c["chr_end"] + 1, args.features // len(ctgs))
                                  for c in ctgs]))
    sorted_lines = [f"9:{p}" for p in pos]
    legs = {"A sorted": sorted_lines, "B shuffled": [sorted_lines[i] for i in rng.permutation(len(sorted_lines))]}
    ss = engine.SeqSet(eng, [np.frombuffer(c["seq"], np.uint8) if not isinstance(c["seq"], np.ndarray) else c["seq"]
                             for c in ctgs])
    say(f"sw from the bytes of a feature file: {len(sorted_lines)} point features on {len(ctgs)} ctgs of 1 Mb "
        f"(size 100, max 20, resize 500, -a gc), {args.reps} repetitions a route after a warming call, routes alternating")
    say(f"device: {eng.device_info()}")

    def today(lines):
        t0 = time.perf_counter()
        recs = host.read_range(eng, ctgs, lines)
        t_rr = (time.perf_counter() - t0) * 1e3
        feats, serial = {c["id"]: [] for c in ctgs}, {}
        for cid, r in recs:
            serial[cid] = serial.get(cid, 0) + 1
            s, _, e = r.split(":")[1].partition("-")
            feats[cid].append((f"feature:{cid}:{serial[cid]}", int(s), int(e or s)))
        text, op = host.sw_multi_timed([eng], by_id, [feats[c["id"]] for c in by_id])
        return text.encode(), (time.perf_counter() - t0) * 1e3, t_rr + op

    def text_host(data):
        t0 = time.perf_counter()
        out = host.sw_text(eng, ctgs, data)
        return out, (time.perf_counter() - t0) * 1e3, host.last_operator_ms()

    def text_resident(data):
        t0 = time.perf_counter()
        out = host.sw_text(eng, ctgs, data, seqset=ss)
        return out, (time.perf_counter() - t0) * 1e3, host.last_operator_ms()

    for leg, lines in legs.items():
        data = ("\n".join(lines) + "\n").encode()
        routes = (("today: read_range + ids in Python + sw_multi", lambda: today(lines)),
                  ("sw_text, host sequences                     ", lambda: text_host(data)),
                  ("sw_text, resident SeqSet                    ", lambda: text_resident(data)))
        res = {name: [] for name, _ in routes}
        ref = None
        stage_ms = None
        for rep in range(args.reps + 1):                                  # rep 0 warms the handle's buffers
            for name, run in routes:
                out, wall, op = run()
                if ref is None:
                    ref = out
                assert out == ref, name
                if name.startswith("sw_text"):
                    assert host.last_operator_device() == 1
                if rep:
                    res[name].append((wall, op))
                if name.startswith("sw_text, resident"):
                    ms, n = (C.c_float * 16)(), C.c_uint32()
                    assert G.gams_gpu_last_stage_ms(eng.h, ms, 16, C.byref(n)) == 0 and n.value == len(STAGES)
                    stage_ms = [ms[k] for k in range(n.value)]
        say()
        say(f"leg {leg}: {ref.count(10)} rows, {len(ref) / 1e6:.0f} MB of text, identical from the three routes")
        for name, _ in routes:
            for what, col in (("wall    ", 0), ("operator", 1)):
                v = [r[col] for r in res[name]]
                say(f"leg {leg}: {name} {what} median {statistics.median(v):8.1f} ms  (min {min(v):8.1f} .. max {max(v):8.1f})")
        base = statistics.median(r[1] for r in res[routes[0][0]])
        for name, _ in routes[1:]:
            say(f"leg {leg}: {name.strip()}: today's route spends {base / statistics.median(r[1] for r in res[name]):.2f}x its time inside the operators")
        for k, v in enumerate(stage_ms):
            say(f"leg {leg}:     stage {STAGES[k]:38s} {v:9.3f} ms")
        say(f"leg {leg}:     stages together {sum(stage_ms):9.3f} ms (the rest of the operator: ctg index and name tables, the seqset"
            " upload where there is one, the two read-backs, the copy into id order by a few threads)")
    ss.close()
    eng.close()


if __name__ == "__main__":
    main()
