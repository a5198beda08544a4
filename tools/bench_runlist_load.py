#!/usr/bin/env python3
"""Loading the span set of `anno` from the bytes of a runlist JSON file: the device route (gams::AnnoSet ->
gams_spans_create_runlist_text) against the parent's route (the host reader gams::read_runlist_json + gams_spans_create),
and gams_spans_create alone on arrays that are ready, from the bytes in host memory to a usable set.

Shapes: 4e6 spans in 4 groups (the set of tools/bench_aux.py) and 1e6 spans in 16 groups, each once as a normalised
file (what every runlist() output is) and once with the same spans shuffled, a fifth of them cut into two pieces that
overlap.  All arms run in this one process, alternating, `--rounds` times; every figure is the best of its calls, with
the calls beside it.  The device route's split per stage comes from the library's stopwatch.

usage: tools/bench_runlist_load.py [--rounds 3] [--scale 1.0]"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STAGES = ("upload", "mark (quotes, refused bytes)", "count (structure, token starts)", "parse (tokens) + order test",
          "normalise (sort, running max, join)", "build (cum, directory, cells)")


def spans_of(n_groups, per_group, rng):
    sets = []
    for _ in range(n_groups):
        cuts = np.sort(rng.choice(np.arange(1, 2_000_000_000, 97), 2 * per_group, replace=False))
        sets.append((cuts[0::2].astype(np.int64), (cuts[1::2] - 1).astype(np.int64)))
    return sets


def runlist_text(lo, hi):
    return ",".join(map("%d-%d".__mod__, zip(lo.tolist(), hi.tolist())))


def documents(n_groups, per_group, seed):
    rng = np.random.default_rng(seed)
    sets = spans_of(n_groups, per_group, rng)
    plain, messy = [], []
    for g, (lo, hi) in enumerate(sets):
        plain.append(f'"{g + 1}": "{runlist_text(lo, hi)}"')
        cut = (rng.random(lo.size) < 0.2) & (hi - lo > 20)            # [lo, mid + 5] and [mid, hi] overlap
        mid = (lo + hi) // 2
        lo2 = np.concatenate([lo, mid[cut]])
        hi2 = np.concatenate([np.where(cut, mid + 5, hi), hi[cut]])
        order = rng.permutation(lo2.size)
        messy.append(f'"{g + 1}": "{runlist_text(lo2[order], hi2[order])}"')
    wrap = lambda rows: ("{\n  " + ",\n  ".join(rows) + "\n}\n").encode()
    return wrap(plain), wrap(messy), n_groups * per_group


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--scale", type=float, default=1.0)
    args = ap.parse_args()
    from gams_amd import _lib, engine, host

    G = _lib.load()
    eng = engine.Engine(0)
    print(f"span set from the bytes of a runlist JSON file; device {eng.device_info()}", flush=True)
    for n_groups, per_group in ((4, int(1_000_000 * args.scale)), (16, int(62_500 * args.scale))):
        plain, messy, n_spans = documents(n_groups, per_group, 7)
        for leg, data in (("normalised", plain), ("shuffled with overlaps", messy)):
            tag = f"[{n_spans} spans, {n_groups} groups, {leg}, {len(data) / 1e6:.1f} MB]"
            ready = host.read_runlist_json(data)
            off = np.cumsum([0] + [v[0].size for v in ready.values()]).astype(np.uint64)
            lo = np.concatenate([v[0] for v in ready.values()])
            hi = np.concatenate([v[1] for v in ready.values()])
            assert lo.size == n_spans
            ms = {"device": [], "host": [], "create": []}
            stages = []
            for _ in range(args.rounds + 1):                       # the first round warms the handle's buffers
                assert host.runlist_load(eng, data, device_route=True) == n_spans and host.last_operator_device() == 1
                ms["device"].append(host.last_operator_ms())
                stage, ns = (C.c_float * 16)(), C.c_uint32()
                assert G.gams_gpu_last_stage_ms(eng.h, stage, 16, C.byref(ns)) == 0
                stages.append([stage[k] for k in range(ns.value)])
                assert host.runlist_load(eng, data, device_route=False) == n_spans and host.last_operator_device() == 0
                ms["host"].append(host.last_operator_ms())
                sp = C.c_void_p()
                t0 = time.perf_counter()
                eng.check(G.gams_spans_create(eng.h, n_groups, off.ctypes.data, lo.ctypes.data, hi.ctypes.data, C.byref(sp)))
                ms["create"].append((time.perf_counter() - t0) * 1e3)
                G.gams_spans_destroy(eng.h, sp)
            names = (("device", "device route  AnnoSet -> gams_spans_create_runlist_text"),
                     ("host", "parent's route read_runlist_json + gams_spans_create  "),
                     ("create", "gams_spans_create alone, arrays ready               "))
            for key, name in names:
                calls = ", ".join(f"{m:.2f}" for m in ms[key])
                print(f"{tag} {name} {min(ms[key][1:]):9.2f} ms (calls: {calls})", flush=True)
            d, h, c = (min(ms[k][1:]) for k in ("device", "host", "create"))
            print(f"{tag} the device route takes {d / h:.3f} of the parent's route and {d / c:.3f} of gams_spans_create alone",
                  flush=True)
            for k, v in enumerate(stages[1 + int(np.argmin(ms["device"][1:]))]):       # of the best call
                print(f"{tag}     stage {STAGES[k]:38s} {v * 1e3:9.1f} us", flush=True)
            # the two routes build the same set
            a, b = host.AnnoSet(eng, data), host.read_runlist_json(data)
            got = a.spans()
            assert a.device and list(got) == list(b) and all(np.array_equal(got[k][0], b[k][0]) and
                                                              np.array_equal(got[k][1], b[k][1]) for k in b)
            a.close()
            print(f"{tag} the device's set equals the host reader's", flush=True)
    eng.close()


if __name__ == "__main__":
    main()
