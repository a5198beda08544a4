#!/usr/bin/env python3
"""`sw -a gc`, `sw -a count` and `sw -a gc -a count` (host buffers in -> TSV rows out) on an Atha-chr1-shaped
chromosome (30 Mb, piece 1e6 -> 30 ctgs) with 1e5 point features and 1e6 rg ranges, nearly all 1 bp (SNP-like) and
0.1 % of them 100 bp - 20 kb long.  Reports the operator ms of each action set (upload + kernels + row text, what
host.sw_multi_timed measures) and, for the sets with count, the rg index build inside it on its own.
  python3 tools/bench_sw_count.py [--reps 5]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gams_amd import engine, host, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
args = ap.parse_args()

eng = engine.Engine(0)
rng = np.random.default_rng(5)
chrom = synth.chromosome(30_000_000, 9)
ctgs = synth.gen_ctgs("9", chrom, piece=1000000)
flist = []
for c in ctgs:
    fs = np.sort(rng.integers(c["chr_start"], c["chr_end"] + 1, 100000 // len(ctgs)))
    flist.append([(f"feature:{c['id']}:{i + 1}", int(s), int(s)) for i, s in enumerate(fs)])
recs = []
per = 1_000_000 // len(ctgs) + 1
for c in ctgs:
    s = rng.integers(c["chr_start"], c["chr_end"] + 1, per)
    ln = np.where(rng.random(per) < 0.001, rng.integers(100, 20000, per), 0)
    e = np.minimum(s + ln, c["chr_end"])
    recs += [(c["id"], f"9:{a}-{b}") for a, b in zip(s.tolist(), e.tolist())]
print(f"{len(ctgs)} ctgs, {sum(len(f) for f in flist)} features, {len(recs)} rgs", flush=True)

result = {}
for name, actions, rg in (("gc", ("gc",), ()), ("count", ("count",), recs), ("gc+count", ("gc", "count"), recs)):
    host.sw_multi_timed([eng], ctgs, flist, actions=actions, rg_records=rg)       # warm-up
    ops, ixs = [], []
    for _ in range(args.reps):
        text, ms = host.sw_multi_timed([eng], ctgs, flist, actions=actions, rg_records=rg)
        ops.append(ms)
        ixs.append(host.last_sw_index_ms() if rg else 0.0)
    op, ix = statistics.median(ops), statistics.median(ixs)
    result[name] = dict(operator_ms=round(op, 2), index_ms=round(ix, 2), without_index_ms=round(op - ix, 2),
                        min_ms=round(min(ops), 2), max_ms=round(max(ops), 2), rows=text.count("\n"),
                        mb=round(len(text) / 1e6, 1))
    print(f"-a {' -a '.join(actions)}: operator {op:.1f} ms (min {min(ops):.1f}, max {max(ops):.1f}; {args.reps} runs), "
          f"of which rg index build {ix:.1f} ms -> {op - ix:.1f} ms without it; {text.count(chr(10))} rows, "
          f"{len(text) / 1e6:.0f} MB", flush=True)
gc = result["gc"]["without_index_ms"]
result["gc+count / gc (without index)"] = round(result["gc+count"]["without_index_ms"] / gc, 3)
result["count / gc (without index)"] = round(result["count"]["without_index_ms"] / gc, 3)
print(json.dumps(result))
eng.close()
