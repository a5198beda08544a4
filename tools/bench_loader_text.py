#!/usr/bin/env python3
"""The rg / feature loaders over several files and their records as text, on the Atha-shaped ctg table of
bench_rg_load.py: 1e6 range lines as ONE file and as FOUR files of 2.5e5, sorted by position (leg A) and shuffled (leg B).
From the bytes in host memory to (a) the rg index and (b) the records as RECORDS and RESP text.

usage: tools/bench_loader_text.py [--parent DIR] [--rounds 2] [--lines 1000000] [--one-file-only]
Every arm is a fresh child process of its own.  With --parent DIR (a directory holding libgams_gpu.so and libgams_host.so
of the parent commit) the arms alternate parent, this build, parent, ...  Both arms time, through the calls both builds
export, the parent's route -- the ONE-file index load on the device (gams_host_rg_load, operator ms: the figure that must
not get slower), and for four files gams_host_read_range per file (what rg_records= is made from) and
gams_host_loader_records per file.  This build's arm then times the new entries from the same bytes, best of three
after a warming call, with the library's stopwatch per stage: gams_index_create_range_files and gams_gpu_loader_text
(RECORDS, RESP) over one file and over four.  --one-file-only: the ONE-file index line alone in every arm, for more
rounds of the figure whose spread between rounds the arms are compared against."""
import argparse
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_rg_load import table_and_lines  # noqa: E402

STAGES = ("lines (upload + line index)", "parse", "locate", "first line per (file, ctg)", "keep + count", "offsets (scan)",
          "order (radix sort)")
INDEX_STAGES = STAGES + ("gather", "index build")
TEXT_STAGES = STAGES + ("serials", "row lengths", "write")


def best(call, n=3):
    call()                                    # warms the handle's buffers
    ms = []
    for _ in range(n):
        t0 = time.perf_counter()
        out = call()
        ms.append((time.perf_counter() - t0) * 1e3)
    return min(ms), ms, out


def child(args):
    from gams_amd import _lib, engine, host

    libdir = args.libdir or os.path.join(ROOT, "gams_amd")
    G = _lib._lib = _lib.bind(os.path.join(libdir, "libgams_gpu.so"), strict=False)
    H = C.CDLL(os.path.join(libdir, "libgams_host.so"))      # bound by hand: only what both builds export
    sp = C.POINTER(C.c_char_p)
    H.gams_host_read_range.restype = C.c_void_p
    H.gams_host_read_range.argtypes = [C.c_void_p, C.c_uint32, sp, sp, C.c_void_p, C.c_void_p, C.c_char_p]
    H.gams_host_loader_records.restype = C.c_void_p
    H.gams_host_loader_records.argtypes = [C.c_void_p, C.c_uint32, sp, sp, C.c_void_p, C.c_void_p, C.c_char_p, C.c_char_p]
    H.gams_host_rg_load.restype = C.c_int64
    H.gams_host_rg_load.argtypes = [C.c_void_p, C.c_uint32, sp, sp, C.c_void_p, C.c_void_p, C.c_char_p, C.c_uint64, C.c_int]
    H.gams_host_last_operator_ms.restype = C.c_double
    H.gams_host_free.argtypes = [C.c_void_p]
    eng = engine.Engine(0)
    ctgs, legs = table_and_lines(args.lines)
    n, ids, chrs, st, en = host._ctg_arrays(ctgs)
    tag = f"[{args.arm}]"

    def rows_of(fn, *a):
        p = fn(eng.h, n, ids, chrs, st.ctypes.data, en.ctypes.data, *a)
        assert p
        k = C.string_at(p).count(b"\n")
        H.gams_host_free(p)
        return k

    for leg, lines in legs.items():
        one = ("\n".join(lines) + "\n").encode()
        q = len(lines) // 4
        four = [("\n".join(lines[k * q:(k + 1) * q if k < 3 else len(lines)]) + "\n").encode() for k in range(4)]
        # the parent's route, timed in both arms
        ms = []
        for _ in range(5):
            assert H.gams_host_rg_load(eng.h, n, ids, chrs, st.ctypes.data, en.ctypes.data, one, len(one), 1) >= 0
            ms.append(H.gams_host_last_operator_ms())
        print(f"{tag} leg {leg}: ONE file -> index on the device (gams_host_rg_load, operator) {min(ms[1:]):8.2f} ms "
              f"(calls: {', '.join(f'{m:.2f}' for m in ms)})", flush=True)
        if args.one_file_only:
            continue
        w, calls, kept = best(lambda: sum(rows_of(H.gams_host_read_range, f) for f in four))
        print(f"{tag} leg {leg}: four files -> host.read_range per file (the source of rg_records=) {w:8.1f} ms "
              f"(calls: {', '.join(f'{m:.1f}' for m in calls)}), {kept} kept", flush=True)
        w, calls, recs = best(lambda: sum(rows_of(H.gams_host_loader_records, f, None) for f in four))
        print(f"{tag} leg {leg}: four files -> host.loader_records per file (RECORDS text)         {w:8.1f} ms "
              f"(calls: {', '.join(f'{m:.1f}' for m in calls)}), {recs} records", flush=True)
        assert kept == recs
        if args.arm == "parent":
            continue
        # this build: the new entries on the tables a Locator makes
        by_chr = {}
        for c in ctgs:
            by_chr.setdefault(c["chr_id"], []).append(c)
        names = sorted(by_chr, key=lambda k: k.encode())
        order = [c for k in names for c in by_chr[k]]
        off = np.cumsum([0] + [len(by_chr[k]) for k in names]).astype(np.uint64)
        cs = np.array([c["chr_start"] for c in order], np.uint32)
        ce = np.array([c["chr_end"] + 1 for c in order], np.uint32)
        ix, chr_nm, id_nm = C.c_void_p(), C.c_void_p(), C.c_void_p()
        assert G.gams_index_create(eng.h, len(names), off.ctypes.data, cs.ctypes.data, ce.ctypes.data, C.byref(ix)) == 0
        arr = (C.c_char_p * len(names))(*[k.encode() for k in names])
        assert G.gams_names_create(eng.h, len(names), arr, C.byref(chr_nm)) == 0
        arr = (C.c_char_p * len(order))(*[c["id"].encode() for c in order])
        assert G.gams_names_create(eng.h, len(order), arr, C.byref(id_nm)) == 0
        stage, ns = (C.c_float * 16)(), C.c_uint32()

        def stages(names_):
            assert G.gams_gpu_last_stage_ms(eng.h, stage, 16, C.byref(ns)) == 0
            for k in range(ns.value):
                print(f"{tag} leg {leg}:     stage {names_[k]:30s} {stage[k] * 1e3:9.1f} us", flush=True)

        for label, files in (("ONE file  ", [one]), ("four files", four)):
            bufs = [np.frombuffer(f, np.uint8) for f in files]
            ptrs = (C.c_void_p * len(bufs))(*[b.ctypes.data for b in bufs])
            lens = np.array([b.size for b in bufs], np.uint64)
            grp = np.zeros(len(order), np.uint32)

            def index():
                rg, k = C.c_void_p(), C.c_uint64()
                assert G.gams_index_create_range_files(eng.h, ix, chr_nm, len(bufs), ptrs, lens.ctypes.data, C.byref(rg),
                                                       grp.ctypes.data, C.byref(k)) == 0
                G.gams_index_destroy(eng.h, rg)
                return k.value

            w, calls, k = best(index)
            print(f"{tag} leg {leg}: {label} -> index  gams_index_create_range_files {w:8.2f} ms "
                  f"(calls: {', '.join(f'{m:.2f}' for m in calls)}), {k} kept", flush=True)
            assert label != "four files" or k == kept
            index()
            stages(INDEX_STAGES)
            for fmt, fname in ((_lib.LOADER_RECORDS, "RECORDS"), (_lib.LOADER_RESP, "RESP   ")):
                toff = np.zeros(len(bufs) * len(order) + 1, np.uint64)

                def text():
                    t, nb, rows = C.c_void_p(), C.c_uint64(), C.c_uint64()
                    assert G.gams_gpu_loader_text(eng.h, ix, chr_nm, id_nm, len(bufs), ptrs, lens.ctypes.data, _lib.LOADER_RG,
                                                  None, 0, fmt, None, C.byref(t), C.byref(nb), toff.ctypes.data, None, None,
                                                  C.byref(rows)) == 0
                    return rows.value, nb.value

                w, calls, (rows, nb) = best(text)
                print(f"{tag} leg {leg}: {label} -> {fname} gams_gpu_loader_text          {w:8.2f} ms "
                      f"(calls: {', '.join(f'{m:.2f}' for m in calls)}), {rows} rows, {nb / 1e6:.1f} MB of text", flush=True)
                assert label != "four files" or rows == recs
                text()
                stages(TEXT_STAGES)
        G.gams_names_destroy(eng.h, chr_nm)
        G.gams_names_destroy(eng.h, id_nm)
        G.gams_index_destroy(eng.h, ix)
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--lines", type=int, default=1_000_000)
    ap.add_argument("--one-file-only", action="store_true")
    ap.add_argument("--arm", default=None)
    ap.add_argument("--libdir", default=None)
    args = ap.parse_args()
    if args.arm:
        return child(args)
    arms = ([("parent", args.parent)] if args.parent else []) + [("this build", None)]
    print("the loaders over several files and their records as text: the parent's route against the device entries\n"
          "The ONE-file index line is the same call in both arms (the parent's device loader): its spread between the rounds\n"
          "of one arm is the run-to-run spread, and the two arms are compared against it.", flush=True)
    for r in range(args.rounds):
        for arm, libdir in arms:
            cmd = [sys.executable, os.path.abspath(__file__), "--arm", arm, "--lines", str(args.lines)]
            if libdir:
                cmd += ["--libdir", os.path.abspath(libdir)]
            if args.one_file_only:
                cmd += ["--one-file-only"]
            print(f"--- round {r + 1}: {arm}", flush=True)
            rc = subprocess.run(cmd, timeout=600).returncode
            if rc != 0:
                sys.exit(f"arm {arm!r} ended with status {rc}")


if __name__ == "__main__":
    main()
