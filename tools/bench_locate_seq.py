#!/usr/bin/env python3
"""`gams locate --seq` (locate.rs:124-134) on an A. thaliana-shaped genome through the host layer, the genome resident as
a seqset: three range files in -> their FASTA records out.
    (a) 10^5 ranges of length uniform 1-2000, the query shape of SURVEY section 8 d C5
    (b) 10^6 point ranges
    (c) every ctg whole
Two routes, alternating, in one process: host.locate_seq (every ctg's whole sequence joined into one text per call, a
map of strings and a substr per range on the host: the route in front of this entry) and host.locate_seq_text on the
resident seqset (the bytes of the file to the finished text on the device).  Both print the same text (asserted).

    tools/bench_locate_seq.py [--rounds N] [--scale F] [--out FILE]

ms are wall-clock around the Python call, which ends in the read-back of the text; for locate_seq_text also the entry's
stages (gams_gpu_last_stage_ms).  The yardstick of the copy stage is one device-to-device copy of text_bytes bytes (a
torch.uint8 copy_ between two resident tensors, timed with events).  Medians over the rounds, after one warming round;
min - max is the spread.  --scale < 1 shrinks the genome and the files (a rehearsal, not a measurement)."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gams_amd import engine, host, synth  # noqa: E402

STAGES = ("lines", "parse", "locate", "lengths", "offsets", "copy")


def range_lines(ctgs, n, max_len, seed):
    """n ranges of length uniform 1..max_len, each inside one ctg (ctgs drawn by length), in genome order"""
    rng = np.random.default_rng(seed)
    lens = np.array([c["chr_end"] - c["chr_start"] + 1 for c in ctgs], np.int64)
    which = np.sort(rng.choice(len(ctgs), n, p=lens / lens.sum()))
    length = rng.integers(1, max_len + 1, n)
    length = np.minimum(length, lens[which] - 1)
    start = np.array([c["chr_start"] for c in ctgs], np.int64)[which] + 1 + (rng.random(n) * (lens[which] - length - 1)).astype(np.int64)
    chrs = [ctgs[i]["chr_id"] for i in which.tolist()]
    if max_len == 1:
        return [f"{c}:{s}" for c, s in zip(chrs, start.tolist())]
    return [f"{c}:{s}-{e}" for c, s, e in zip(chrs, start.tolist(), (start + length - 1).tolist())]


def stage_ms(eng):
    ms = (C.c_float * 16)()
    n = C.c_uint32()
    eng.check(eng.lib.gams_gpu_last_stage_ms(eng.h, ms, 16, C.byref(n)))
    return [float(ms[k]) for k in range(n.value)]


def d2d_ms(nbytes, rounds):
    """one device-to-device copy of nbytes, ms: the median of `rounds` behind a warming one"""
    import torch

    a = torch.empty(nbytes, dtype=torch.uint8, device="cuda:0")
    b = torch.empty(nbytes, dtype=torch.uint8, device="cuda:0")
    a.random_(0, 256)
    out = []
    for r in range(rounds + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        b.copy_(a)
        e1.record()
        e1.synchronize()
        if r:
            out.append(e0.elapsed_time(e1))
    del a, b
    torch.cuda.empty_cache()
    return statistics.median(out)


def med(v):
    return f"{statistics.median(v):9.2f} ({min(v):.2f} - {max(v):.2f})"


def leg(eng, ctgs, ss, name, rgs, rounds, say):
    data = ("\n".join(rgs) + "\n").encode()
    t_old, t_new, stages = [], [], []
    want = None
    for r in range(rounds + 1):                          # round 0 warms the pools and is not reported
        t0 = time.perf_counter()
        a = host.locate_seq(eng, ctgs, rgs).encode()
        t_a = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        b = host.locate_seq_text(eng, ctgs, data, seqset=ss)
        t_b = (time.perf_counter() - t0) * 1e3
        assert host.last_operator_device() == 1 and a == b
        want = b
        if r:
            t_old.append(t_a)
            t_new.append(t_b)
            stages.append(stage_ms(eng))
    copy_ms = statistics.median(s[-1] for s in stages)
    yard = d2d_ms(len(want), rounds)
    say(f"{name}: {len(rgs)} lines, {len(data)} input bytes -> {want.count(b'>')} '>' bytes, {len(want)} text bytes")
    say(f"  host.locate_seq        ms: {med(t_old)}")
    say(f"  host.locate_seq_text   ms: {med(t_new)}   ({statistics.median(t_old) / statistics.median(t_new):.1f}x)")
    say("  stages, us (medians):      " + "  ".join(f"{k} {statistics.median(s[i] for s in stages) * 1e3:.0f}"
                                                    for i, k in enumerate(STAGES)))
    say(f"  copy stage {copy_ms * 1e3:.0f} us = {len(want) / copy_ms / 1e6:.1f} GB/s of text; device-to-device copy of the same "
        f"bytes {yard * 1e3:.0f} us; ratio {copy_ms / yard:.2f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out = open(args.out, "w") if args.out else None

    def say(s):
        print(s, flush=True)
        if out:
            out.write(s + "\n")
            out.flush()

    import torch

    torch.zeros(1, device="cuda:0")                      # torch's runtime opens the device before the library's does
    eng = engine.Engine(0)
    lengths = [max(20000, int(n * args.scale)) for n in synth.ATHA_LENGTHS]
    ctgs = [dict(id=c["id"], chr_id=c["chr_id"], chr_start=c["chr_start"], chr_end=c["chr_end"], seq=c["seq"])
            for c in synth.genome_ctgs(lengths, 500000)]
    ss = engine.SeqSet(eng, [c["seq"] for c in ctgs])
    say(f"device {eng.device_info()}; {len(ctgs)} ctgs, {sum(len(c['seq']) for c in ctgs)} bases; chunk "
        f"{eng.lib.gams_gpu_locate_seq_chunk()} bytes; medians of {args.rounds} (min - max)")
    whole = [f"{c['chr_id']}:{c['chr_start']}-{c['chr_end']}" for c in ctgs]
    leg(eng, ctgs, ss, "(a) ranges of 1-2000 bases", range_lines(ctgs, max(10, int(100_000 * args.scale)), 2000, 5), args.rounds, say)
    leg(eng, ctgs, ss, "(b) point ranges", range_lines(ctgs, max(10, int(1_000_000 * args.scale)), 1, 7), args.rounds, say)
    leg(eng, ctgs, ss, "(c) every ctg whole", whole, args.rounds, say)
    ss.close()
    eng.close()


if __name__ == "__main__":
    main()
