#!/usr/bin/env python3
"""The per-distance summary of the sw rows: (a) today's way to the table -- host.sw_text, then a vectorised NumPy
aggregation of its text -- against (b) host.sw_summary with host sequences and (c) host.sw_summary on a resident SeqSet,
in one process, alternating.  The input is that of bench_sw_text.py: a 30-Mb synthetic chromosome in 1-Mb ctgs and 1e5
point features written as range lines; leg A position-sorted, leg B the same lines shuffled.

usage: tools/bench_sw_summary.py [--reps 5] [--features 100000] [--out FILE]
Per route: the wall time from the bytes to the table's text and the time inside the C++ operator
(gams_host_last_operator_ms; for (a) that of sw_text alone: the aggregation has no operator), as median and min .. max
over the repetitions after one warming call each; then the stages of the summary entry, and of sw_text's entry beside
them, from the library's stopwatch.  The three tables must be byte-equal."""
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
          "offsets (scan)", "order (radix sort)", "gather + middle check", "geometry (rows per feature, scan)",
          "rows (summarising sw_kernel + merge)")
TEXT_STAGES = STAGES[:8] + ("geometry (rows per feature, scans)", "rows (sw_kernel)", "text lengths", "text write")
CHUNK = 1 << 19                                                          # rows parsed at a time


def field_units(a, s, e):
    """the decimal fields a[s[i]:e[i]] as integers m of m / 10^4, and which of them are NaN ("-0" is 0)"""
    width = int((e - s).max())
    idx = s[:, None] + np.arange(width, dtype=np.int64)[None, :]
    ch = np.where(idx < e[:, None], a[np.minimum(idx, a.size - 1)], 0).astype(np.int64)
    nan = ch[:, 0] == ord("N")
    dig = (ch >= 48) & (ch <= 57)
    frac = dig & (np.cumsum(ch == 46, axis=1) > 0)
    whole = dig & ~frac
    n_whole = whole.sum(1)
    w_rank = np.cumsum(whole, axis=1) - 1
    f_rank = np.cumsum(frac, axis=1) - 1
    power = np.where(whole, n_whole[:, None] - 1 - w_rank + 4, np.where(frac, 3 - f_rank, 0))
    m = (np.where(dig, ch - 48, 0) * 10 ** np.clip(power, 0, 18)).sum(1)
    return np.where(nan, 0, m), nan


def aggregate(text, mx):
    """the rows' text -> (COUNT[mx + 1], S[mx + 1, 4], NaN[mx + 1, 4]): the GROUP BY distance of the SQL, in NumPy"""
    a = np.frombuffer(text, np.uint8)
    tabs = np.flatnonzero(a == 9).reshape(-1, 8)                         # a row has eight tabs
    count = np.zeros(mx + 1, np.int64)
    s = np.zeros((mx + 1, 4), np.int64)
    nan = np.zeros((mx + 1, 4), np.int64)
    for lo in range(0, tabs.shape[0], CHUNK):
        t = tabs[lo:lo + CHUNK]
        dist = field_units(a, t[:, 2] + 1, t[:, 3])[0] // 10000
        count += np.bincount(dist, minlength=mx + 1)
        for k in range(4):
            m, isnan = field_units(a, t[:, 3 + k] + 1, t[:, 4 + k])
            s[:, k] += np.bincount(dist, weights=m, minlength=mx + 1).astype(np.int64)   # < 2^53: exact in a double
            nan[:, k] += np.bincount(dist, weights=isnan, minlength=mx + 1).astype(np.int64)
    return count, s, nan


def avg4(num, den):
    q, r = divmod(int(num), int(den))
    if 2 * r > den or (2 * r == den and q % 2):
        q += 1
    ip, fr = divmod(q, 10000)
    return str(ip) + ("." + ("%04d" % fr).rstrip("0") if fr else "")


def table_text(count, s, nan):
    out = ["distance\tAVG_gc_content\tAVG_gc_mean\tAVG_gc_stddev\tAVG_gc_cv\tCOUNT\n"]
    for d in range(count.size):
        if count[d]:
            out.append("\t".join([str(d)] + ["nan" if nan[d, k] else avg4(s[d, k], count[d]) for k in range(4)] + [str(count[d])]) + "\n")
    return "".join(out).encode()


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
    pos = np.sort(np.concatenate([rng.integers(c["chr_start"] + 1, c["chr_end"] + 1, args.features // len(ctgs))
                                  for c in ctgs]))
    sorted_lines = [f"9:{p}" for p in pos]
    legs = {"A sorted": sorted_lines, "B shuffled": [sorted_lines[i] for i in rng.permutation(len(sorted_lines))]}
    ss = engine.SeqSet(eng, [np.frombuffer(c["seq"], np.uint8) if not isinstance(c["seq"], np.ndarray) else c["seq"]
                             for c in ctgs])
    mx = 20
    say(f"sw summary from the bytes of a feature file: {len(sorted_lines)} point features on {len(ctgs)} ctgs of 1 Mb "
        f"(size 100, max {mx}, resize 500, -a gc), {args.reps} repetitions a route after a warming call, routes alternating")
    say(f"device: {eng.device_info()}")

    def stages(n_want):
        ms, n = (C.c_float * 16)(), C.c_uint32()
        assert G.gams_gpu_last_stage_ms(eng.h, ms, 16, C.byref(n)) == 0 and n.value == n_want, n.value
        return [ms[k] for k in range(n.value)]

    seen = {}

    def text_then_numpy(data):
        t0 = time.perf_counter()
        text = host.sw_text(eng, ctgs, data, seqset=ss)
        op = host.last_operator_ms()
        seen["text stages"] = stages(len(TEXT_STAGES))
        seen["rows"], seen["bytes"] = text.count(b"\n") if "rows" not in seen else seen["rows"], len(text)
        t1 = time.perf_counter()
        out = table_text(*aggregate(text, mx))
        seen["aggregate ms"] = (time.perf_counter() - t1) * 1e3
        return out, (time.perf_counter() - t0) * 1e3, op

    def summary_host(data):
        t0 = time.perf_counter()
        out = host.sw_summary(eng, ctgs, data, mx=mx)
        return out, (time.perf_counter() - t0) * 1e3, host.last_operator_ms()

    def summary_resident(data):
        t0 = time.perf_counter()
        out = host.sw_summary(eng, ctgs, data, mx=mx, seqset=ss)
        wall, op = (time.perf_counter() - t0) * 1e3, host.last_operator_ms()
        seen["summary stages"] = stages(len(STAGES))
        return out, wall, op

    for leg, lines in legs.items():
        data = ("\n".join(lines) + "\n").encode()
        routes = (("(a) sw_text (resident SeqSet) + NumPy aggregation", lambda: text_then_numpy(data)),
                  ("(b) sw_summary, host sequences                   ", lambda: summary_host(data)),
                  ("(c) sw_summary, resident SeqSet                  ", lambda: summary_resident(data)))
        res = {name: [] for name, _ in routes}
        agg, rows_text, rows_sum = [], [], []
        ref = None
        seen.pop("rows", None)
        for rep in range(args.reps + 1):                                  # rep 0 warms the handle's buffers
            for name, run in routes:
                out, wall, op = run()
                if ref is None:
                    ref = out
                assert out == ref, name
                if name.startswith(("(b)", "(c)")):
                    assert host.last_operator_device() == 1
                if rep:
                    res[name].append((wall, op))
            if rep:
                agg.append(seen["aggregate ms"])
                rows_text.append(seen["text stages"][9])
                rows_sum.append(seen["summary stages"][9])
        say()
        say(f"leg {leg}: {seen['rows']} rows, {seen['bytes'] / 1e6:.0f} MB of text behind route (a); the table has "
            f"{ref.count(10) - 1} lines, byte-equal from the three routes")
        for name, _ in routes:
            for what, col in (("wall    ", 0), ("operator", 1)):
                v = [r[col] for r in res[name]]
                say(f"leg {leg}: {name} {what} median {statistics.median(v):8.1f} ms  (min {min(v):8.1f} .. max {max(v):8.1f})")
        say(f"leg {leg}:     of (a)'s wall, the NumPy aggregation: median {statistics.median(agg):8.1f} ms  "
            f"(min {min(agg):8.1f} .. max {max(agg):8.1f})")
        wall = {name[:3]: statistics.median(r[0] for r in res[name]) for name, _ in routes}
        op = {name[:3]: statistics.median(r[1] for r in res[name]) for name, _ in routes}
        say(f"leg {leg}: wall (b) / (a) = {wall['(b)'] / wall['(a)']:.4f}, (c) / (a) = {wall['(c)'] / wall['(a)']:.4f}; "
            f"operator (c) / sw_text's operator = {op['(c)'] / op['(a)']:.4f}")
        for k, v in enumerate(seen["summary stages"]):
            say(f"leg {leg}:     summary stage {STAGES[k]:38s} {v:9.3f} ms")
        say(f"leg {leg}:     summary stages together {sum(seen['summary stages']):9.3f} ms")
        for k, v in enumerate(seen["text stages"]):
            say(f"leg {leg}:     sw_text stage {TEXT_STAGES[k]:38s} {v:9.3f} ms")
        say(f"leg {leg}:     rows stage over the repetitions: summarising median {statistics.median(rows_sum):.3f} ms "
            f"(min {min(rows_sum):.3f} .. max {max(rows_sum):.3f}); sw_text's median {statistics.median(rows_text):.3f} ms "
            f"(min {min(rows_text):.3f} .. max {max(rows_text):.3f})")
    ss.close()
    eng.close()


if __name__ == "__main__":
    main()
