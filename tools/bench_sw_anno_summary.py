#!/usr/bin/env python3
"""The sw summary with Prop columns (host.sw_summary(..., anno=)) on the workload of bench_sw_summary.py
(a 30-Mb synthetic chromosome in 1-Mb ctgs, 1e5 point features, size 100, max 20, resize 500, -a gc):

  (a) host.sw_summary on a resident SeqSet with 0, 1, 2 and 4 resident span sets;
  (b) the route to the same table without the join: host.sw_text, host.anno_text over its output once per set, then the
      NumPy aggregation of bench_sw_summary.py extended by the Prop columns;

in one process, alternating, median of --reps after a warming call.  The sets are SURVEY 8(d)'s shape -- disjoint spans of
100-3000 bases -- at two densities (gaps of 100-3000 and of 3000-27000 bases), each twice with another seed for the run
with four.  The tables of (a) must be byte-equal to (b)'s, column for column, before any time is reported.  Then the rows
stage of the summary entry for 0 / 1 / 2 / 4 sets from the library's stopwatch, and beside it the kernel time of
gams_gpu_cover (span_cover_kernel) over the same rows' ranges, per set: the yardstick for the fused lookup.

usage: tools/bench_sw_anno_summary.py [--reps 5] [--features 100000] [--out FILE]
       tools/bench_sw_anno_summary.py --zero-only [--root TREE] [--reps 9]
--zero-only prints the rows stage of host.sw_summary without sets and nothing else; --root names another checkout of this
project to import gams_amd from (a build of the parent commit), so that the two builds can be run alternating on one box."""
import argparse
import ctypes as C
import json
import os
import re
import statistics
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from bench_sw_summary import CHUNK, avg4, field_units   # noqa: E402

ROWS_STAGE = 9                                           # of the summary entry's ten stages


def span_set(chr_id, length, gap_lo, gap_hi, seed):
    """disjoint spans of 100-3000 bases with gaps of gap_lo .. gap_hi over [1, length] -> the runlist JSON's bytes"""
    rng = np.random.default_rng(seed)
    n = int(length // (1550 + (gap_lo + gap_hi) // 2) * 1.2) + 16
    w = rng.integers(100, 3001, n)
    g = rng.integers(gap_lo, gap_hi + 1, n)
    lo = np.cumsum(w + g) - w
    keep = lo + w - 1 <= length
    lo, w = lo[keep], w[keep]
    return json.dumps({chr_id: ",".join("%d-%d" % (a, a + b - 1) for a, b in zip(lo.tolist(), w.tolist()))}).encode(), int(lo.size)


def aggregate(text, mx, n_sets):
    """the annotated rows' text -> (COUNT, S[.., 4], NaN[.., 4], P[.., n_sets]): the GROUP BY distance of the SQL, in NumPy"""
    a = np.frombuffer(text, np.uint8)
    tabs = np.flatnonzero(a == 9).reshape(-1, 8 + n_sets)
    ends = np.flatnonzero(a == 10)
    count = np.zeros(mx + 1, np.int64)
    s = np.zeros((mx + 1, 4), np.int64)
    nan = np.zeros((mx + 1, 4), np.int64)
    p = np.zeros((mx + 1, n_sets), np.int64)
    for lo in range(0, tabs.shape[0], CHUNK):
        t, e = tabs[lo:lo + CHUNK], ends[lo:lo + CHUNK]
        dist = field_units(a, t[:, 2] + 1, t[:, 3])[0] // 10000
        count += np.bincount(dist, minlength=mx + 1)
        for k in range(4):
            m, isnan = field_units(a, t[:, 3 + k] + 1, t[:, 4 + k])
            s[:, k] += np.bincount(dist, weights=m, minlength=mx + 1).astype(np.int64)   # < 2^53: exact in a double
            nan[:, k] += np.bincount(dist, weights=isnan, minlength=mx + 1).astype(np.int64)
        for k in range(n_sets):
            q = field_units(a, t[:, 8 + k] + 1, t[:, 9 + k] if k + 1 < n_sets else e)[0]
            p[:, k] += np.bincount(dist, weights=q, minlength=mx + 1).astype(np.int64)
    return count, s, nan, p


def table_text(count, s, nan, p, prefixes):
    out = ["\t".join(["distance", "AVG_gc_content", "AVG_gc_mean", "AVG_gc_stddev", "AVG_gc_cv"] +
                     ["AVG_%sProp" % x for x in prefixes] + ["COUNT"]) + "\n"]
    for d in range(count.size):
        if count[d]:
            out.append("\t".join([str(d)] + ["nan" if nan[d, k] else avg4(s[d, k], count[d]) for k in range(4)] +
                                 [avg4(p[d, k], count[d]) for k in range(len(prefixes))] + [str(count[d])]) + "\n")
    return "".join(out).encode()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--features", type=int, default=100000)
    ap.add_argument("--out", default=None)
    ap.add_argument("--zero-only", action="store_true")
    ap.add_argument("--root", default=os.path.dirname(HERE))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
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
    pos = np.sort(np.concatenate([rng.integers(c["chr_start"] + 1, c["chr_end"] + 1, args.features // len(ctgs))
                                  for c in ctgs]))
    data = ("\n".join(f"9:{p}" for p in pos) + "\n").encode()
    ss = engine.SeqSet(eng, [np.frombuffer(c["seq"], np.uint8) if not isinstance(c["seq"], np.ndarray) else c["seq"]
                             for c in ctgs])
    mx = 20

    def rows_stage():
        ms, n = (C.c_float * 16)(), C.c_uint32()
        assert G.gams_gpu_last_stage_ms(eng.h, ms, 16, C.byref(n)) == 0 and n.value == 10, n.value
        return ms[ROWS_STAGE]

    if args.zero_only:
        v = []
        for rep in range(args.reps + 1):
            host.sw_summary(eng, ctgs, data, mx=mx, seqset=ss)
            assert host.last_operator_device() == 1
            if rep:
                v.append(rows_stage())
        say(f"rows stage without sets, {os.path.abspath(args.root)}: median {statistics.median(v):.4f} ms "
            f"(min {min(v):.4f} .. max {max(v):.4f}) of {len(v)}: " + " ".join("%.4f" % x for x in v))
        ss.close()
        eng.close()
        return

    shapes = (("dense", 100, 3000, 101), ("sparse", 3000, 27000, 103), ("dense2", 100, 3000, 107), ("sparse2", 3000, 27000, 109))
    sets = []
    for name, g0, g1, seed in shapes:
        js, n = span_set("9", chrom.size, g0, g1, seed)
        t0 = time.perf_counter()
        aset = host.AnnoSet(eng, js)
        sets.append((name, aset))
        say(f"set {name}: {n} spans of 100-3000 bases, gaps {g0}-{g1}, {len(js) / 1e6:.1f} MB of JSON, resident after "
            f"{(time.perf_counter() - t0) * 1e3:.1f} ms (device route: {aset.device})")
    say(f"sw summary with Prop columns: {pos.size} point features on {len(ctgs)} ctgs of 1 Mb (size 100, max {mx}, resize 500, "
        f"-a gc), {args.reps} repetitions a route after a warming call, routes alternating")
    say(f"device: {eng.device_info()}")
    seen = {}

    def fused(k):
        def run():
            t0 = time.perf_counter()
            out = host.sw_summary(eng, ctgs, data, mx=mx, seqset=ss, anno=sets[:k] if k else None)
            wall, op = (time.perf_counter() - t0) * 1e3, host.last_operator_ms()
            assert host.last_operator_device() == 1
            seen["rows %d" % k] = rows_stage()
            return out, wall, op
        return run

    def unfused(k):
        def run():
            t0 = time.perf_counter()
            text = host.sw_text(eng, ctgs, data, seqset=ss)
            op = host.last_operator_ms()
            for _, aset in sets[:k]:
                text = host.anno_text(eng, ctgs, aset, text)
                assert host.last_operator_device() == 1
                op += host.last_operator_ms()
            seen["text"] = text
            t1 = time.perf_counter()
            out = table_text(*aggregate(text, mx, k), [p for p, _ in sets[:k]])
            seen["aggregate ms"] = (time.perf_counter() - t1) * 1e3
            return out, (time.perf_counter() - t0) * 1e3, op
        return run

    routes = [("(a) sw_summary, %d resident sets                      " % k, fused(k), k) for k in (0, 1, 2, 4)]
    routes += [("(b) sw_text + anno_text x %d + NumPy aggregation      " % k, unfused(k), k) for k in (2, 4)]
    res = {name: [] for name, _, _ in routes}
    rows = {k: [] for k in (0, 1, 2, 4)}
    agg = {2: [], 4: []}
    tables = {}
    for rep in range(args.reps + 1):                                      # rep 0 warms the handle's buffers
        for name, run, k in routes:
            out, wall, op = run()
            tables.setdefault((name[:3], k), out)
            assert out == tables[(name[:3], k)], name
            if rep:
                res[name].append((wall, op))
                if name.startswith("(a)"):
                    rows[k].append(seen["rows %d" % k])
                else:
                    agg[k].append(seen["aggregate ms"])

    def cut(table, keep):                                                 # the columns of (b)'s table that (a) with k sets prints
        return b"".join(b"\t".join(f for i, f in enumerate(ln.split(b"\t")) if i in keep) + b"\n" for ln in table.split(b"\n")[:-1])

    assert tables[("(a)", 4)] == tables[("(b)", 4)] and tables[("(a)", 2)] == tables[("(b)", 2)]
    assert tables[("(a)", 1)] == cut(tables[("(b)", 4)], (0, 1, 2, 3, 4, 5, 9))
    assert tables[("(a)", 0)] == cut(tables[("(b)", 4)], (0, 1, 2, 3, 4, 9))
    text = seen["text"]
    say()
    say(f"{text.count(10)} rows, {len(text) / 1e6:.0f} MB of text behind route (b) with four sets; the tables have "
        f"{tables[('(a)', 4)].count(10) - 1} lines and are byte-equal between (a) and (b) for 0, 1, 2 and 4 sets")
    for name, _, _ in routes:
        for what, col in (("wall    ", 0), ("operator", 1)):
            v = [r[col] for r in res[name]]
            say(f"{name} {what} median {statistics.median(v):9.2f} ms  (min {min(v):9.2f} .. max {max(v):9.2f})")
    for k in (2, 4):
        say(f"    of (b)'s wall with {k} sets, the NumPy aggregation: median {statistics.median(agg[k]):9.1f} ms")
    for k in (0, 1, 2, 4):
        say(f"rows stage (summarising kernel + merge), {k} sets: median {statistics.median(rows[k]):.4f} ms "
            f"(min {min(rows[k]):.4f} .. max {max(rows[k]):.4f})")
    base = statistics.median(rows[0])
    for k in (1, 2, 4):
        say(f"    marginal cost per set at {k} sets: {(statistics.median(rows[k]) - base) / k:.4f} ms")
    # the yardstick: span_cover_kernel over the same rows' ranges (the clip is the range itself: a window lies in its ctg)
    m = re.findall(rb"\t9:(\d+)-(\d+)\t", text)
    qs = np.array([int(a) for a, _ in m], np.int32)
    qe = np.array([int(b) for _, b in m], np.int32)
    assert qs.size == text.count(10)
    grp = np.zeros(qs.size, np.uint32)
    prop = np.zeros(qs.size, np.float32)
    for name, aset in sets[:2]:
        v = []
        for rep in range(args.reps + 1):
            assert G.gams_gpu_cover(eng.h, aset._sp, grp.ctypes.data, qs.ctypes.data, qe.ctypes.data, qs.ctypes.data,
                                    qe.ctypes.data, qs.size, prop.ctypes.data) == 0
            ms = C.c_float()
            assert G.gams_gpu_last_kernel_ms(eng.h, C.byref(ms)) == 0
            if rep:
                v.append(ms.value)
        say(f"gams_gpu_cover over the same {qs.size} ranges, set {name}: kernel median {statistics.median(v):.4f} ms "
            f"(min {min(v):.4f} .. max {max(v):.4f}); mean prop {float(prop.mean()):.4f}")
    for _, aset in sets:
        aset.close()
    ss.close()
    eng.close()


if __name__ == "__main__":
    main()
