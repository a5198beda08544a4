#!/usr/bin/env python3
"""The `seq:{ctg}` values back into a resident seqset, on the A. thaliana-shaped genome of tools/bench_seq_gz.py
(7 chromosomes, 119.7 Mb, piece 500,000): the host's inflate against the device inflater of the indexed members.

Routes, alternating in one process:
  (a) host    host.decode_gz_many on 16 threads over the plain members + a SeqSet of the bases (create + upload_all):
              the route every run that starts from the store took so far;
  (b) device  a SeqSet of the same lengths + gams_seqset_upload_gz over the indexed members, at each chunk tried
              (gams_gpu_seq_gz_set_chunk): wall-clock of the whole, of the call alone, and its four stages
              (gams_gpu_last_stage_ms, HIP events);
  (c) wave    host.wave_gz over the same values with inflate="host" against inflate="device", default parameters.
Size: the indexed members' total at each chunk, and the plain members', against host.encode_gz (zlib level 1).

    tools/bench_seq_gunzip.py [--rounds N] [--out FILE]

Round 0 of every route warms the pools and is not reported; medians, minima and maxima of the rest are.  Before any
clock runs, every slot the device filled is downloaded and compared with the bases."""
import argparse
import ctypes as C
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

STAGES = ("upload", "tables", "decode", "join")
CHUNKS = (1024, 2048, 4096)


def route_host(eng, members, lengths):
    t0 = time.perf_counter()
    seqs = host.decode_gz_many(members, lengths, 16)
    ss = engine.SeqSet(eng, seqs)
    eng.sync()
    ms = (time.perf_counter() - t0) * 1e3
    ss.close()
    return ms


def route_device(eng, members, lengths, keep=False):
    n = len(members)
    bufs = [np.frombuffer(m, np.uint8) for m in members]
    ptrs = (C.c_void_p * n)(*[b.ctypes.data for b in bufs])
    lens = np.array([b.size for b in bufs], np.uint64)
    st, nf = np.zeros(n, np.uint8), C.c_uint32()
    t0 = time.perf_counter()
    ss = engine.SeqSet(eng, [range(int(k)) for k in lengths], upload=False)      # (only the lengths are read)
    t1 = time.perf_counter()
    eng.check(eng.lib.gams_seqset_upload_gz(eng.h, ss.p, 0, n, ptrs, lens.ctypes.data, st.ctypes.data, C.byref(nf)))
    t2 = time.perf_counter()
    assert nf.value == 0 and not st.any(), "the device left members to the host"
    ms, k = (C.c_float * 16)(), C.c_uint32()
    eng.check(eng.lib.gams_gpu_last_stage_ms(eng.h, ms, 16, C.byref(k)))
    if keep:
        return ss
    ss.close()
    return (t2 - t0) * 1e3, (t2 - t1) * 1e3, [float(ms[i]) for i in range(k.value)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out = open(args.out, "w") if args.out else None

    def say(s):
        print(s, flush=True)
        if out:
            out.write(s + "\n")
            out.flush()

    def spread(v):
        return f"{statistics.median(v):7.2f} ms (min {min(v):.2f}, max {max(v):.2f})"

    med = statistics.median
    eng = engine.Engine(0)
    with ThreadPoolExecutor(7) as ex:
        chroms = list(ex.map(lambda k: (str(k + 1), synth.chromosome(synth.ATHA_LENGTHS[k], k + 1)), range(len(synth.ATHA_LENGTHS))))
    ctgs, _, ss = host.gen_text(eng, fasta_bytes(chroms).tobytes())
    lengths = ss.lengths.copy()
    bases = int(lengths.astype(np.uint64).sum())
    say(f"device {eng.device_info()}; {len(chroms)} chromosomes -> {len(ctgs)} ctgs, {bases} bases (gen_text, piece 500000)")
    truth = [ss.download(i) for i in range(len(ctgs))]
    plain = host.seq_gz(eng, ss)
    indexed = {}
    for chunk in CHUNKS:
        eng.check(eng.lib.gams_gpu_seq_gz_set_chunk(eng.h, chunk))
        indexed[chunk] = host.seq_gz(eng, ss, indexed=True)
    eng.check(eng.lib.gams_gpu_seq_gz_set_chunk(eng.h, _lib.SEQ_GZ_CHUNK))
    ss.close()
    with ThreadPoolExecutor(16) as ex:
        zlib1 = sum(ex.map(lambda s: len(host.encode_gz(s)), truth))
    say(f"zlib level 1: {zlib1} bytes; plain members {sum(map(len, plain))} = {sum(map(len, plain)) / zlib1:.4f} of it; indexed: "
        + ", ".join(f"chunk {c}: {sum(map(len, indexed[c]))} = {sum(map(len, indexed[c])) / zlib1:.4f}" for c in CHUNKS))
    for chunk in CHUNKS:
        back = route_device(eng, indexed[chunk], lengths, keep=True)
        for i, t in enumerate(truth):
            assert back.download(i) == t, f"chunk {chunk}: slot {i} differs from its bases"
        back.close()

    a, b = [], {c: [] for c in CHUNKS}
    for r in range(args.rounds + 1):
        t = route_host(eng, plain, lengths)
        if r:
            a.append(t)
        for chunk in CHUNKS:
            t = route_device(eng, indexed[chunk], lengths)
            if r:
                b[chunk].append(t)
    say(f"(a) host   decode_gz_many(16 threads) + SeqSet (create, upload_all), median of {args.rounds}: {spread(a)}")
    for chunk in CHUNKS:
        say(f"(b) device chunk {chunk:4d}: create + gams_seqset_upload_gz: {spread([x[0] for x in b[chunk]])}; the call alone: "
            f"{spread([x[1] for x in b[chunk]])}; stages "
            + ", ".join(f"{k} {med([x[2][i] for x in b[chunk]]):.3f} (min {min(x[2][i] for x in b[chunk]):.3f}, max {max(x[2][i] for x in b[chunk]):.3f})"
                        for i, k in enumerate(STAGES)))

    jobs = {"host": [dict(c, gz=m) for c, m in zip(ctgs, plain)],
            "device": [dict(c, gz=m) for c, m in zip(ctgs, indexed[_lib.SEQ_GZ_CHUNK])]}
    texts, c = {}, {"host": [], "device": []}
    for r in range(args.rounds + 1):
        for how in ("host", "device"):
            t0 = time.perf_counter()
            texts[how], _ = host.wave_gz(eng, jobs[how], inflate=how)
            if r:
                c[how].append((time.perf_counter() - t0) * 1e3)
    assert texts["host"] == texts["device"], "the two routes print different rows"
    windows = sum(max(0, (int(n) - 100) // 10 + 1) for n in lengths)
    for how in ("host", "device"):
        say(f"(c) wave_gz inflate={how:6s} (chunk {_lib.SEQ_GZ_CHUNK}), median of {args.rounds}: {spread(c[how])}; "
            f"{windows / med(c[how]) / 1e6:.3f} x 10^9 windows/s from the store's bytes")
    eng.close()


if __name__ == "__main__":
    main()
