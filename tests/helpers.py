"""Shared test helpers: fixture loading and a tiny restatement of the host-side
bookkeeping around the hot path (ctg split, range parsing, rg/feature bucketing).

Citations are file:line under the reference (wang-q/gams).  The arithmetic the
tests check lives in oracle/ (CPU) and gams_amd/csrc (HIP); what is here is only
the glue the reference's own CLI tests go through before they reach it.
"""
import gzip
import json
import os
import re

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
S288C = os.path.join(GOLDEN, "S288c")


def read_fasta_gz(path):
    seqs, name, chunks = {}, None, []
    with gzip.open(path, "rb") as fh:
        for line in fh:
            line = line.rstrip(b"\r\n")
            if line.startswith(b">"):
                if name is not None:
                    seqs[name] = b"".join(chunks)
                name = line[1:].split()[0].decode()
                chunks = []
            else:
                chunks.append(line)
    if name is not None:
        seqs[name] = b"".join(chunks)
    return seqs


def gen_ctgs(chr_id, seq, piece=500000, fill=50, min_len=5000):
    """cmd_gams/gen.rs:81-157: valid regions -> --piece chunks -> ctg records."""
    a = np.frombuffer(seq, np.uint8)
    ok = np.isin(a, np.frombuffer(b"ACGTacgt", np.uint8))            # gen.rs:86-93
    # valid spans (1-based inclusive)
    d = np.diff(np.concatenate(([0], ok.view(np.int8), [0])))
    starts = np.flatnonzero(d == 1) + 1
    ends = np.flatnonzero(d == -1)
    spans = [[int(s), int(e)] for s, e in zip(starts, ends)]
    # fill(fill-1): holes of size <= fill-1 are closed (gen.rs:103)
    filled = []
    for s, e in spans:
        if filled and s - filled[-1][1] - 1 <= fill - 1:
            filled[-1][1] = e
        else:
            filled.append([s, e])
    # excise(min): spans shorter than min are dropped (gen.rs:104)
    filled = [sp for sp in filled if sp[1] - sp[0] + 1 >= min_len]
    ctgs = []
    serial = 0
    for pos, mx in filled:                                            # gen.rs:108-126
        cur = []
        while mx - pos + 1 > piece:
            cur.append([pos, pos + piece - 1])
            pos += piece
        if not cur:
            cur.append([pos, mx])
        else:
            cur[-1][1] = mx
        for s, e in cur:
            serial += 1
            ctgs.append(dict(id=f"ctg:{chr_id}:{serial}", chr_id=chr_id, chr_start=s, chr_end=e,
                             range=f"{chr_id}:{s}-{e}", length=e - s + 1, seq=seq[s - 1:e]))
    return ctgs


_RG = re.compile(r"^(?:(?P<name>[\w_]+)\.)?(?P<chr>[\w-]+)(?:\((?P<strand>[+-])\))?"
                 r"(?::(?P<start>\d+)(?:[_\-]+(?P<end>\d+))?)?$")


def parse_range(s):
    """intspan::Range::from_str: chr(strand):start-end; returns None if invalid."""
    m = _RG.match(s.strip())
    if not m or m.group("start") is None:
        return None
    start = int(m.group("start"))
    end = int(m.group("end")) if m.group("end") else start
    return m.group("chr"), start, end


def ctg_index(ctgs):
    """redis.rs:236-258: per chr, intervals (chr_start, chr_end+1, ctg_id) sorted."""
    idx = {}
    for c in ctgs:
        idx.setdefault(c["chr_id"], []).append((c["chr_start"], c["chr_end"] + 1, c["id"]))
    for k in idx:
        idx[k].sort()
    return idx


def load_s288c():
    seqs = read_fasta_gz(os.path.join(S288C, "genome.fa.gz"))
    return seqs


def read_lines(name):
    with open(os.path.join(S288C, name)) as fh:
        return [ln.rstrip("\n") for ln in fh]


def read_runlists(name):
    with open(os.path.join(S288C, name)) as fh:
        js = json.load(fh)
    out = {}
    for chr_id, rl in js.items():
        lo, hi = [], []
        for part in rl.split(","):
            if part in ("", "-"):
                continue
            if "-" in part:
                a, b = part.split("-")
            else:
                a = b = part
            lo.append(int(a))
            hi.append(int(b))
        out[chr_id] = (np.array(lo, np.int32), np.array(hi, np.int32))
    return out


def synth(n, seed, gc=0.4, lower=0.2, nrate=1e-4):
    rng = np.random.default_rng(seed)
    x = np.arange(n)
    p = gc + 0.06 * np.sin(2 * np.pi * x / 2300) + 0.04 * np.sin(2 * np.pi * x / 97000)
    is_gc = rng.random(n) < p
    pick = rng.random(n) < 0.5
    s = np.where(is_gc, np.where(pick, ord("G"), ord("C")), np.where(pick, ord("A"), ord("T"))).astype(np.uint8)
    s = np.where(rng.random(n) < lower, s | 0x20, s).astype(np.uint8)
    s[rng.random(n) < nrate] = ord("N")
    return s


GC_LETTERS, AT_LETTERS = b"GCgc", b"ATatN"


def periodic(n, unit, letters=0):
    """n bases whose G/C pattern is the boolean `unit` tiled: G/C positions draw from G C g c, the others from A T a t N
    (`letters` seeds the draw).  Which letter stands where changes no count, so the window counts repeat with the unit."""
    unit = np.asarray(unit, bool)
    rng = np.random.default_rng(letters)
    is_gc = np.tile(unit, n // unit.size + 1)[:n]
    gc = np.frombuffer(GC_LETTERS, np.uint8)[rng.integers(0, len(GC_LETTERS), n)]
    at = np.frombuffer(AT_LETTERS, np.uint8)[rng.integers(0, len(AT_LETTERS), n)]
    return np.where(is_gc, gc, at).astype(np.uint8)


def gc_unit(period, gc, seed):
    """a boolean unit of `period` bases, round(period * gc) of them G/C, at seeded random places"""
    unit = np.zeros(period, bool)
    unit[np.random.default_rng(seed).permutation(period)[:int(round(period * gc))]] = True
    return unit


def lag_sums(cnt, lag):
    """The integers the reference's z-score is made of (stat.rs:36 with :51-52), over prefix sums of the counts:
    for every window i >= lag, S1 = sum k and S2 = sum k^2 over the counts of windows [i-1-lag, i-1) (window `lag`:
    [0, lag)), Dn = lag*k[i] - S1 (signed) and V = lag*S2 - S1^2.  -> (i, S1, S2, Dn, V), int64 (exact below 2^63)."""
    k = np.asarray(cnt).astype(np.int64)
    p1 = np.concatenate(([0], np.cumsum(k)))
    p2 = np.concatenate(([0], np.cumsum(k * k)))
    i = np.arange(lag, k.size)
    a = np.where(i == lag, 0, i - 1 - lag)
    s1, s2 = p1[a + lag] - p1[a], p2[a + lag] - p2[a]
    return i, s1, s2, lag * k[i] - s1, lag * s2 - s1 * s1


def tie_states(cnt, lag):
    """The plain float64 model: z = D / sqrt(lag*V/(lag-1)) with D = |lag*k - S1| for every window i >= lag.
    -> [(z, windows)] for the distinct finite positive z, the most populous first."""
    i, _, _, dn, v = lag_sums(cnt, lag)
    with np.errstate(divide="ignore", invalid="ignore"):
        z = np.abs(dn) / np.sqrt(lag * v.astype(np.float64) / (lag - 1))
    ok = np.isfinite(z) & (z > 0)
    vals, inv = np.unique(z[ok], return_inverse=True)
    out = [(float(zv), i[ok][inv == j]) for j, zv in enumerate(vals)]
    out.sort(key=lambda t: (-t[1].size, t[0]))
    return out


def real_signals(cnt, lag, thr):
    """The verdict of real arithmetic, which is what an integer decision computes: window i signals iff
    D > thr * sqrt(lag*V/(lag-1)), for the f32 threshold the kernels are given (float64 throughout)."""
    i, _, _, dn, v = lag_sums(cnt, lag)
    r = float(np.float32(thr)) * np.sqrt(lag * v.astype(np.float64) / (lag - 1))
    sig = np.zeros(np.asarray(cnt).size, np.int32)
    sig[i] = np.where(np.abs(dn) > r, np.sign(dn), 0)
    return sig


KNIFE_DELTAS = (0.0, 1e-7, -1e-7, 1e-6, -1e-6, 3e-6, -3e-6, 1e-5, -1e-5, 3e-5, -3e-5)


def knife_thresholds(z0):
    """eleven f32 thresholds on and around the z-score z0 of one state: z0 * (1 + d)"""
    return [float(np.float32(z0 * (1.0 + d))) for d in KNIFE_DELTAS]


def longest_run(sig):
    """length of the longest stretch of consecutive nonzero entries"""
    nz = np.concatenate(([0], (np.asarray(sig) != 0).astype(np.int8), [0]))
    d = np.diff(nz)
    starts, ends = np.flatnonzero(d == 1), np.flatnonzero(d == -1)
    return int((ends - starts).max()) if starts.size else 0


def sweep_model(cnt, size, lag, thr, infl, s1, max_sweeps=1000):
    """The guess-and-iterate sweeps for influence != 1 (gams_amd/csrc/wave_repair.hpp: jac_filter_kernel, then
    jac_eval_kernel, over every window) in strict float32 and in the kernels' order of operations: filtered[] from the
    signals (stat.rs:42 inside runs of signalled windows, the data elsewhere), then every window i >= lag against mean / sd
    of filtered[i-1-lag, i-1) (window `lag`: [0, lag)), both sums left to right; from the influence == 1 answer `s1` until a
    sweep flips nothing.  -> (flips per sweep, the last one 0; the longest run of signalled windows in any state the
    filter saw; the final signals).  The iteration of tools/experiments/jacobi_model.py, bit for bit instead of in f64."""
    f32 = np.float32
    x = np.asarray(cnt).astype(f32) / f32(size)
    n = x.size
    infl, thr, flen = f32(infl), f32(thr), f32(lag)
    t1 = infl * x                                             # influence * x[i]
    omi = f32(1.0) - infl
    i = np.arange(lag, n)
    a = np.where(i == lag, 0, i - 1 - lag)
    sig = np.asarray(s1).astype(np.int32).copy()
    flips, run = [], 0
    while len(flips) < max_sweeps:
        run = max(run, longest_run(sig))
        f = x.copy()
        for j in np.flatnonzero(sig):                         # left to right: f[j-1] is final when j is reached
            f[j] = t1[j] + omi * f[j - 1]
        total = np.zeros(i.size, f32)
        for c in range(lag):
            total = total + f[a + c]
        mean = total / flen
        sq = np.zeros(i.size, f32)
        for c in range(lag):
            d = f[a + c] - mean
            sq = sq + d * d
        with np.errstate(invalid="ignore", divide="ignore"):
            sd = np.sqrt(sq / (flen - f32(1.0)))
            hit = np.abs(x[i] - mean) > thr * sd
        new = np.zeros(n, np.int32)
        new[i] = np.where(hit, np.where(x[i] > mean, 1, -1), 0)
        flips.append(int(np.count_nonzero(new != sig)))
        sig = new
        if flips[-1] == 0:
            break
    return flips, run, sig
