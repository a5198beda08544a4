#!/usr/bin/env python3
"""`gams gen` from the bytes of a FASTA file to a resident seqset (bytes and G/C plane) plus the ctg table, on an
A. thaliana-shaped genome: 7 chromosomes, 119.7 Mb, lines of 60 bases, the file's bytes in page-locked memory.

Two arms, alternating in one process:
  gen_text  gams_gpu_gen_text and its accessors (counts, chrs, ctgs, seqset): one upload of the file;
  baseline  the route every host took before: the FASTA joined on the host (records split at '>', the '\\n' of every
            record dropped: one pass of bytes.replace per chromosome over a bytes copy of the file made outside the
            clock), host.gen per chromosome (upload, scan, table), the ctgs sliced, engine.SeqSet create + upload_all,
            and a sync, so that both arms end with the seqset resident.
Both arms must give the same table and the same device bytes (asserted on every ctg's first and last KiB).

    tools/bench_gen_text.py [--rounds N] [--out FILE]

ms are wall-clock around the calls; round 0 warms the pools and is not reported; the medians of the rest are.  The
stages of gen_text are gams_gpu_last_stage_ms (HIP events; `table` is the host's part between the scan and the place)."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gams_amd import _lib, engine, host, synth  # noqa: E402

STAGES = ("h2d", "mark/compact", "scan", "host table", "place")
WIDTH = 60


def fasta_bytes(chroms):
    """the FASTA text of [(name, uint8 bases)] at WIDTH bases a line, as one uint8 array"""
    parts = []
    for name, a in chroms:
        parts.append(np.frombuffer(b">" + name.encode() + b"\n", np.uint8))
        full, rem = divmod(a.size, WIDTH)
        body = np.empty(full * (WIDTH + 1) + (rem + 1 if rem else 0), np.uint8)
        rows = body[:full * (WIDTH + 1)].reshape(full, WIDTH + 1)
        rows[:, :WIDTH] = a[:full * WIDTH].reshape(full, WIDTH)
        rows[:, WIDTH] = 10
        if rem:
            body[-rem - 1:-1] = a[full * WIDTH:]
            body[-1] = 10
        parts.append(body)
    return np.concatenate(parts)


def arm_gen_text(eng, ptr, n, piece):
    L = eng.lib
    t0 = time.perf_counter()
    g, prm = C.c_void_p(), _lib.GenParams(piece, 50, 5000)
    eng.check(L.gams_gpu_gen_text(eng.h, ptr, n, C.byref(prm), C.byref(g)))
    n_chr, n_ctg, nb = C.c_uint32(), C.c_uint32(), C.c_uint64()
    eng.check(L.gams_gen_counts(eng.h, g, C.byref(n_chr), C.byref(n_ctg), C.byref(nb)))
    names, off = np.zeros(nb.value, np.uint8), np.zeros(n_chr.value + 1, np.uint64)
    clen, tab = np.zeros(n_chr.value, np.uint32), np.zeros(n_ctg.value, _lib.GEN_CTG_DTYPE)
    eng.check(L.gams_gen_chrs(eng.h, g, names.ctypes.data, off.ctypes.data, clen.ctypes.data))
    eng.check(L.gams_gen_ctgs(eng.h, g, tab.ctypes.data))
    p = C.c_void_p()
    eng.check(L.gams_gen_seqset(eng.h, g, C.byref(p)))
    ms = (time.perf_counter() - t0) * 1e3
    stage, ns = (C.c_float * 16)(), C.c_uint32()
    eng.check(L.gams_gpu_last_stage_ms(eng.h, stage, 16, C.byref(ns)))
    L.gams_gen_destroy(eng.h, g)
    raw = names.tobytes()
    chrs = [raw[int(off[i]):int(off[i + 1])].decode() for i in range(n_chr.value)]
    table = [(chrs[t["chr"]], int(t["serial"]), int(t["chr_start"]), int(t["chr_end"])) for t in tab]
    ss = engine.SeqSet.adopt(eng, p.value, (tab["chr_end"] - tab["chr_start"] + 1).astype(np.uint32))
    return ms, [float(stage[k]) for k in range(ns.value)], table, ss


def arm_baseline(eng, data, piece):
    t0 = time.perf_counter()
    chroms = []
    for rec in data.split(b">")[1:]:                       # the host FASTA join
        head, _, body = rec.partition(b"\n")
        chroms.append((head.split()[0].decode(), body.replace(b"\n", b"")))
    t1 = time.perf_counter()
    table, slices = [], []
    for name, seq in chroms:                               # upload + scan + table, per chromosome
        a = np.frombuffer(seq, np.uint8)
        for row in host.gen(eng, name, a, piece=piece).splitlines():
            f = row.split("\t")
            s, e = int(f[3]), int(f[4])
            table.append((name, int(f[0].rsplit(":", 1)[1]), s, e))
            slices.append(a[s - 1:e])
    t2 = time.perf_counter()
    ss = engine.SeqSet(eng, slices)                        # classify + stage + the second upload
    eng.sync()
    t3 = time.perf_counter()
    return [(t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3, (t3 - t0) * 1e3], table, ss, slices


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--piece", type=int, default=500000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out = open(args.out, "w") if args.out else None

    def say(s):
        print(s, flush=True)
        if out:
            out.write(s + "\n")
            out.flush()

    eng = engine.Engine(0)
    with ThreadPoolExecutor(7) as ex:                      # (chromosomes are seeded on their own)
        chroms = list(ex.map(lambda k: (str(k + 1), synth.chromosome(synth.ATHA_LENGTHS[k], k + 1)), range(len(synth.ATHA_LENGTHS))))
    text = fasta_bytes(chroms)
    pin = C.c_void_p()
    eng.check(eng.lib.gams_gpu_host_alloc(eng.h, text.size, C.byref(pin)))
    np.frombuffer((C.c_uint8 * text.size).from_address(pin.value), np.uint8)[:] = text
    data = text.tobytes()
    say(f"device {eng.device_info()}; {len(chroms)} chromosomes, {sum(a.size for _, a in chroms)} bases, FASTA of {text.size} "
        f"bytes at width {WIDTH} (page-locked); piece {args.piece}, fill 50, min 5000")
    new_ms, new_st, base_ms = [], [], []
    for r in range(args.rounds + 1):
        ms, st, tab_new, ss_new = arm_gen_text(eng, pin.value, text.size, args.piece)
        parts, tab_base, ss_base, slices = arm_baseline(eng, data, args.piece)
        assert tab_new == tab_base, "the arms' ctg tables differ"
        for i, a in enumerate(slices):
            got = ss_new.download(i)
            assert got[:1024] == a[:1024].tobytes() and got[-1024:] == a[-1024:].tobytes(), f"ctg {i}: device bytes differ"
        if r == 0:
            assert all(ss_new.download(i, plane=True) == ss_base.download(i, plane=True) for i in range(len(slices)))
        ss_new.close()
        ss_base.close()
        if r == 0:
            continue
        new_ms.append(ms)
        new_st.append(st)
        base_ms.append(parts)
        say(f"  round {r}: gen_text {ms:8.2f} ms (" + ", ".join(f"{k} {v:.2f}" for k, v in zip(STAGES, st)) + f") | baseline "
            f"{parts[3]:8.1f} ms (join {parts[0]:.1f}, host.gen per chromosome {parts[1]:.1f}, SeqSet + upload_all {parts[2]:.1f})")
    med = statistics.median
    say(f"{len(tab_new)} ctgs, identical tables and device bytes in both arms")
    say(f"median of {args.rounds}: gen_text {med(new_ms):.2f} ms; stages: "
        + ", ".join(f"{k} {med([s[i] for s in new_st]):.2f}" for i, k in enumerate(STAGES)))
    say(f"median of {args.rounds}: baseline {med([p[3] for p in base_ms]):.1f} ms; join {med([p[0] for p in base_ms]):.1f}, "
        f"host.gen per chromosome {med([p[1] for p in base_ms]):.1f}, SeqSet + upload_all {med([p[2] for p in base_ms]):.1f}")
    say(f"baseline / gen_text = {med([p[3] for p in base_ms]) / med(new_ms):.1f}")
    eng.lib.gams_gpu_host_free(eng.h, pin)
    eng.close()


if __name__ == "__main__":
    main()
