#!/usr/bin/env python3
"""Loading the rg index from a range file: the host's passes over strings (read_range + set_rg_index) against the
device loader (Locator::set_rg_index_text -> gams_index_create_range_text), on the Atha-shaped ctg table of
bench_text_e2e.py.  Leg A: 1e6 range lines sorted by position (the shape of a real .rg file: a wavefront's lines fall
on one ctg and the per-ctg atomics pile onto one counter); leg B: the same lines shuffled (they spread).

usage: tools/bench_rg_load.py [--parent DIR] [--rounds 2] [--lines 1000000]
Every arm is a fresh child process of its own.  With --parent DIR (a directory holding libgams_gpu.so and libgams_host.so
of the parent commit) the arms alternate parent, this build, parent, ...  The parent's host layer has no clock around its
loader, so the parent arm times the one loader call it exports (gams_host_read_range: the ctg index, the line split,
read_range and the rows' text; no set_rg_index); this build's arm times the same call, and inside the operator
(gams_host_rg_load -> gams_host_last_operator_ms) both paths from the same bytes to the finished index, best of three
after a warming call, with one line per stage of the device loader from the library's stopwatch."""
import argparse
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STAGES = ("lines (upload + line index)", "parse", "locate", "first line per ctg (atomicMin)", "keep + count (atomicAdd)",
          "offsets (scan)", "order (radix sort)", "gather", "index build")


def table_and_lines(n, seed=3):
    from gams_amd import synth

    rng = np.random.default_rng(seed)
    ctgs = []
    for k, ln in enumerate(synth.ATHA_LENGTHS):
        pos, i = 1, 0
        while pos <= ln:
            end = min(ln, pos + 499999)
            if ln - end < 5000:
                end = ln
            i += 1
            ctgs.append(dict(id=f"ctg:{k + 1}:{i}", chr_id=str(k + 1), chr_start=pos, chr_end=end, seq=b""))
            pos = end + 1
    pick = np.sort(rng.integers(0, len(ctgs), n))
    starts = np.array([c["chr_start"] for c in ctgs])[pick] + np.sort(rng.integers(0, 400000, n))
    order = np.lexsort((starts, pick))
    pick, starts = pick[order], starts[order]
    ends = starts + rng.integers(0, 2000, n)
    lines = [f"{ctgs[p]['chr_id']}:{s}-{e}" for p, s, e in zip(pick, starts, ends)]
    shuffled = [lines[i] for i in rng.permutation(n)]
    return ctgs, {"A sorted": lines, "B shuffled": shuffled}


def child(args):
    from gams_amd import _lib, host

    from gams_amd import engine

    if args.libdir:                       # an older build: bind what it has, and of its host layer the one call timed here
        _lib._lib = _lib.bind(os.path.join(args.libdir, "libgams_gpu.so"), strict=False)
        H = C.CDLL(os.path.join(args.libdir, "libgams_host.so"))
        sp = C.POINTER(C.c_char_p)
        H.gams_host_read_range.restype = C.c_void_p
        H.gams_host_read_range.argtypes = [C.c_void_p, C.c_uint32, sp, sp, C.c_void_p, C.c_void_p, C.c_char_p]
        H.gams_host_free.argtypes = [C.c_void_p]
        H.gams_host_last_error.restype = C.c_char_p
    else:
        H = host.load()
    G = _lib.load()
    eng = engine.Engine(0)
    ctgs, legs = table_and_lines(args.lines)
    n, ids, chrs, st, en = host._ctg_arrays(ctgs)
    tag = f"[{args.arm}]"
    for leg, lines in legs.items():
        data = ("\n".join(lines) + "\n").encode()
        wall = []
        for _ in range(3):
            t0 = time.perf_counter()
            p = H.gams_host_read_range(eng.h, n, ids, chrs, st.ctypes.data, en.ctypes.data, data)
            wall.append((time.perf_counter() - t0) * 1e3)
            assert p, H.gams_host_last_error()
            rows = C.string_at(p).count(b"\n")
            H.gams_host_free(p)
        print(f"{tag} leg {leg}: gams_host_read_range (ctg index + line split + read_range + row text) {min(wall):8.1f} ms "
              f"(calls: {', '.join(f'{w:.1f}' for w in wall)}), {rows} kept of {len(lines)} lines", flush=True)
        if args.arm == "parent":
            continue
        res = {}
        for text_path in (False, True, False, True):              # the two paths alternate
            ms = []
            for _ in range(4):                                    # the first call warms the handle's buffers
                groups = host.rg_load(eng, ctgs, data, text_path=text_path)
                ms.append(host.last_operator_ms())
            assert host.last_operator_device() == int(text_path)
            res.setdefault(text_path, []).append((min(ms[1:]), ms, groups))
        for text_path, name in ((False, "host path  read_range + set_rg_index"), (True, "device path set_rg_index_text      ")):
            best = min(r[0] for r in res[text_path])
            calls = "; ".join(", ".join(f"{m:.1f}" for m in r[1]) for r in res[text_path])
            print(f"{tag} leg {leg}: {name} operator {best:8.2f} ms (calls: {calls}), {res[text_path][0][2]} ctgs with a group",
                  flush=True)
        assert res[False][0][2] == res[True][0][2]
        print(f"{tag} leg {leg}: device path is {min(r[0] for r in res[False]) / min(r[0] for r in res[True]):.1f}x the host path",
              flush=True)
        stage, ns = (C.c_float * 16)(), C.c_uint32()
        assert G.gams_gpu_last_stage_ms(eng.h, stage, 16, C.byref(ns)) == 0
        for k in range(ns.value):
            print(f"{tag} leg {leg}:     stage {STAGES[k]:34s} {stage[k] * 1e3:9.1f} us", flush=True)
        # the two paths build the same index: the counts of 1e5 of the file's own ranges agree
        q = ("\n".join(lines[:100000]) + "\n").encode()
        recs = host.read_range(eng, ctgs, lines)
        assert host.locate_text(eng, ctgs, q, count=True, rg_data=data) == host.locate_text(eng, ctgs, q, count=True, rg_records=recs)
        print(f"{tag} leg {leg}: locate --count of 1e5 lines agrees between rg_data= and rg_records=", flush=True)
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--lines", type=int, default=1_000_000)
    ap.add_argument("--arm", default=None)
    ap.add_argument("--libdir", default=None)
    args = ap.parse_args()
    if args.arm:
        return child(args)
    arms = ([("parent", args.parent)] if args.parent else []) + [("this build", None)]
    print("rg index from the bytes of a range file: the host's passes over strings against the device loader\n"
          "The gams_host_read_range lines (both arms) time the one loader call the parent exports: it includes the ctg index\n"
          "and the rows' text, leaves out set_rg_index, and is NOT the figure the comparison is read from.  The comparison\n"
          "is the two 'operator' lines of this build: read_range + set_rg_index (the parent's code, unchanged) against\n"
          "set_rg_index_text, from the same bytes to the finished index.", flush=True)
    for r in range(args.rounds):
        for arm, libdir in arms:
            cmd = [sys.executable, os.path.abspath(__file__), "--arm", arm, "--lines", str(args.lines)]
            if libdir:
                cmd += ["--libdir", os.path.abspath(libdir)]
            print(f"--- round {r + 1}: {arm}", flush=True)
            rc = subprocess.run(cmd, timeout=600).returncode
            if rc != 0:
                sys.exit(f"arm {arm!r} ended with status {rc}")


if __name__ == "__main__":
    main()
