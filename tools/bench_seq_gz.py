#!/usr/bin/env python3
"""The `seq:{ctg}` values of `gams gen` as gzip members, on an A. thaliana-shaped genome (7 chromosomes, 119.7 Mb),
resident as host.gen_text leaves it (piece 500,000).

Arms, in one process:
  device    gams_gpu_seq_gz over every slot, MEMBERS and RESP, at each block size tried (gams_gpu_seq_gz_set_block):
            wall-clock around the call and its five stages (gams_gpu_last_stage_ms, HIP events);
  host      the route every host took before: SeqSet.download + host.encode_gz (zlib level 1, what the reference's
            flate2 Compression::fast() is) for every ctg, on one thread (the reference's own shape) and on 16.
Compressed size: the members' total at each block size against the total of host.encode_gz over the same ctgs.

    tools/bench_seq_gz.py [--rounds N] [--out FILE]

Round 0 of every arm warms the pools and is not reported; medians of the rest are.  Before any clock runs, the first,
a middle and the last member are inflated with Python's gzip and compared with the downloaded bases."""
import argparse
import ctypes as C
import gzip
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gams_amd import _lib, engine, host, synth  # noqa: E402
from bench_gen_text import fasta_bytes  # noqa: E402

STAGES = ("hist", "codes", "sizes", "pack", "copy")
BLOCKS = (16384, 32768, 65536)


def device_call(eng, ss, fmt, nm):
    out, n = C.c_void_p(), C.c_uint64()
    off = np.zeros(ss.lengths.size + 1, np.uint64)
    t0 = time.perf_counter()
    eng.check(eng.lib.gams_gpu_seq_gz(eng.h, ss.p, 0, ss.lengths.size, nm, fmt, C.byref(out), C.byref(n), off.ctypes.data))
    ms = (time.perf_counter() - t0) * 1e3
    st, ns = (C.c_float * 16)(), C.c_uint32()
    eng.check(eng.lib.gams_gpu_last_stage_ms(eng.h, st, 16, C.byref(ns)))
    return ms, [float(st[k]) for k in range(ns.value)], out, n.value, off


def host_route(ss, threads):
    def one(i):
        return len(host.encode_gz(ss.download(i)))

    t0 = time.perf_counter()
    if threads == 1:
        total = sum(one(i) for i in range(ss.lengths.size))
    else:
        with ThreadPoolExecutor(threads) as ex:
            total = sum(ex.map(one, range(ss.lengths.size)))
    return (time.perf_counter() - t0) * 1e3, total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--host-rounds", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out = open(args.out, "w") if args.out else None

    def say(s):
        print(s, flush=True)
        if out:
            out.write(s + "\n")
            out.flush()

    med = statistics.median
    eng = engine.Engine(0)
    with ThreadPoolExecutor(7) as ex:
        chroms = list(ex.map(lambda k: (str(k + 1), synth.chromosome(synth.ATHA_LENGTHS[k], k + 1)), range(len(synth.ATHA_LENGTHS))))
    ctgs, _, ss = host.gen_text(eng, fasta_bytes(chroms).tobytes())
    bases = int(ss.lengths.astype(np.uint64).sum())
    say(f"device {eng.device_info()}; {len(chroms)} chromosomes -> {len(ctgs)} ctgs, {bases} bases resident (gen_text, piece 500000)")
    ids = [c["id"].encode() for c in ctgs]
    nm = C.c_void_p()
    eng.check(eng.lib.gams_names_create(eng.h, len(ids), (C.c_char_p * len(ids))(*ids), C.byref(nm)))

    _, _, ptr, n, off = device_call(eng, ss, _lib.SEQ_GZ_MEMBERS, None)
    data = C.string_at(ptr, n)
    for i in (0, len(ctgs) // 2, len(ctgs) - 1):
        assert gzip.decompress(data[int(off[i]):int(off[i + 1])]) == ss.download(i), f"member {i} does not inflate to its bases"
    del data

    sizes = {}
    for block in BLOCKS:
        eng.check(eng.lib.gams_gpu_seq_gz_set_block(eng.h, block))
        for label, fmt, names in (("MEMBERS", _lib.SEQ_GZ_MEMBERS, None), ("RESP", _lib.LOADER_RESP, nm)):
            wall, stages = [], []
            for r in range(args.rounds + 1):
                ms, st, _, n, _ = device_call(eng, ss, fmt, names)
                if r:
                    wall.append(ms)
                    stages.append(st)
            if label == "MEMBERS":
                sizes[block] = n
            say(f"block {block:6d} {label:7s}: median of {args.rounds}: call {med(wall):7.2f} ms (min {min(wall):.2f}, max {max(wall):.2f}); "
                f"stages " + ", ".join(f"{k} {med([s[i] for s in stages]):.3f}" for i, k in enumerate(STAGES))
                + f"; {n} bytes out = {n / bases:.4f} of the bases")
    eng.check(eng.lib.gams_gpu_seq_gz_set_block(eng.h, _lib.SEQ_GZ_BLOCK))

    ref_total = None
    for threads in (16, 1):
        ms = []
        for r in range(args.host_rounds + 1):
            t, ref_total = host_route(ss, threads)
            if r:
                ms.append(t)
        say(f"host route, {threads:2d} thread(s): download + encode_gz (zlib level 1) of every ctg: median of {args.host_rounds}: "
            f"{med(ms):.1f} ms (min {min(ms):.1f}, max {max(ms):.1f})")
    say(f"zlib level 1 total {ref_total} bytes = {ref_total / bases:.4f} of the bases; members / zlib level 1: "
        + ", ".join(f"block {b}: {sizes[b] / ref_total:.4f}" for b in BLOCKS))
    eng.lib.gams_names_destroy(eng.h, nm)
    ss.close()
    eng.close()


if __name__ == "__main__":
    main()
