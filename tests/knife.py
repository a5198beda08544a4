"""Inputs that put the wave decision on a knife edge, shared by test_wave_knife_cpu.py and test_gpu_wave_knife.py.

A periodic sequence has periodic window counts, so its windows fall into a handful of states (k, S1, S2).  With
the threshold set to the float64 z-score of one state times (1 + d), |d| <= 3e-5, every window of that state has
|D - R| within a few 1e-5 of R: the reference's f32 comparison and the comparison in real arithmetic -- which is what
an integer decision computes -- then disagree on thousands of windows, and each of those must reach the exact path.
The second family saturates the sums (S1 = lag * size, S2 next to 2^24, Q2 prefixes next to 2^32, chunk prefixes
next to 2^16) on both sides of every arithmetic-width limit of wave_build_geometry.

Everything here is computed once per configuration and kept: sequences, oracle counts, thresholds, and the oracle's
signals per threshold (lazily)."""
import functools

import numpy as np

import helpers
from oracle import oracle as ora

N_STATES = 6          # the most populous states of a configuration: 6 x 11 = 66 thresholds
WINDOWS = 3000        # windows that can signal, per ctg

# (size, step, lag) -> the units of its ctgs: (period in bases, G/C fraction, seed)
KNIFE = {
    (100, 10, 100): [(130, 0.5, 1), (70, 0.9, 2), (90, 0.3, 3)],         # baked headline
    (100, 1, 100): [(37, 0.6, 1), (53, 0.45, 2)],                        # baked step 1
    (100, 5, 200): [(130, 0.93, 1), (85, 0.5, 2)],                       # size and step baked, lag an argument
    (255, 10, 257): [(1290, 0.985, 1), (170, 0.9, 2)],                   # run-time fast kernel, lag * size = 65535
    (50, 7, 33): [(77, 0.8, 1), (91, 0.4, 2), (63, 0.6, 3)],             # run-time fast kernel
    (255, 10, 258): [(1290, 0.985, 1), (170, 0.9, 2)],                   # generic, 8-bit counts, wide
    (300, 10, 218): [(170, 0.95, 1), (130, 0.5, 2)],                     # generic, 16-bit counts, narrow
    (300, 10, 250): [(170, 0.95, 1), (130, 0.5, 2)],                     # generic, 16-bit counts, wide
    (1000, 50, 30): [(730, 0.9, 1), (350, 0.5, 2)],                      # generic, large size
    (1000, 500, 100): [(6500, 0.9, 1), (3500, 0.5, 2)],                  # untiled
}


class Case:
    """one (size, step, lag) over fixed ctgs: oracle counts once, oracle / real-arithmetic signals per threshold"""

    def __init__(self, size, step, lag, seqs):
        self.size, self.step, self.lag = size, step, lag
        self.prm = (size, step, lag)
        self.seqs = [np.ascontiguousarray(s, np.uint8) for s in seqs]
        self.cnt = [ora.wave_windows(s, size, step, lag, 3.0, 1.0, want_signals=False)[0].copy() for s in self.seqs]
        self._sig = {}

    def oracle(self, thr, infl=1.0):
        """the oracle's signals of every ctg at this threshold (kept)"""
        key = (float(np.float32(thr)), float(infl))
        if key not in self._sig:
            self._sig[key] = [ora.wave_windows(s, self.size, self.step, self.lag, key[0], key[1])[2].copy()
                              for s in self.seqs]
        return self._sig[key]

    def disagreements(self, thr):
        """windows (over all ctgs) on which the oracle's f32 verdict is not the verdict of real arithmetic"""
        return sum(int(np.count_nonzero(o != helpers.real_signals(k, self.lag, thr)))
                   for o, k in zip(self.oracle(thr), self.cnt))

    def must_be_exact(self, thr):
        """a lower bound on the windows of one pass that the exact path has to see: those on which the oracle is not
        real arithmetic cannot have been decided by the integer form (bar the constant runs, V == 0 and D == 0, which
        the fast kernels settle from a table made in the reference's order)"""
        n = 0
        for o, k in zip(self.oracle(thr), self.cnt):
            i, _, _, dn, v = helpers.lag_sums(k, self.lag)
            n += int(np.count_nonzero((o != helpers.real_signals(k, self.lag, thr))[i] & ((v != 0) | (dn != 0))))
        return n

    def states(self, n=N_STATES):
        """the n most populous z values over all ctgs"""
        pop = {}
        for k in self.cnt:
            for z, w in helpers.tie_states(k, self.lag):
                pop[z] = pop.get(z, 0) + w.size
        return [z for z, _ in sorted(pop.items(), key=lambda t: (-t[1], t[0]))[:n]]

    def thresholds(self, n=N_STATES):
        return [t for z in self.states(n) for t in helpers.knife_thresholds(z)]

    def sums(self, ctgs=None):
        """(max S1, max S2) over every window that can signal, of the given ctgs (default: all)"""
        m1 = m2 = 0
        for k in (self.cnt if ctgs is None else [self.cnt[c] for c in ctgs]):
            _, s1, s2, _, _ = helpers.lag_sums(k, self.lag)
            m1, m2 = max(m1, int(s1.max())), max(m2, int(s2.max()))
        return m1, m2


@functools.lru_cache(maxsize=None)
def knife_case(size, step, lag):
    n = size + (lag + WINDOWS) * step
    seqs = [helpers.periodic(n + 37 * j, helpers.gc_unit(period, gc, seed), letters=seed)
            for j, (period, gc, seed) in enumerate(KNIFE[(size, step, lag)])]
    return Case(size, step, lag, seqs)


# ---- saturated sums -----------------------------------------------------------------------------------------------
def random_gc(n, gc, seed):
    """random content: P(G/C) = gc, letters of both cases, no pattern"""
    rng = np.random.default_rng(seed)
    return helpers.periodic(n, rng.random(n) < gc, letters=seed)


def blocks(n, lo, hi, step, seed):
    """blocks of all-G/C alternating with all-A/T, lengths drawn from [lo, hi) and no multiple of the step: the counts
    swing between 0 and size, and the block edges fall at every phase of the windows"""
    rng = np.random.default_rng(seed)
    unit, on = [], True
    while sum(len(u) for u in unit) < n:
        m = int(rng.integers(lo, hi))
        unit.append(np.full(m + (m % step == 0), on))
        on = not on
    return helpers.periodic(n, np.concatenate(unit)[:n], letters=seed)


# (size, step, lag, tile or 0): both sides of lag * size <= 65535, of the 8-bit count, of the 32-bit Q2 prefix, and the
# 16-bit chunk prefix (tile bytes (lag + 1) * step + size + 32 + tile * step next to 65,520)
SATURATED = [
    (255, 10, 257, 0),         # fast kernel: S1 reaches 65535 = lag * size, S2 16,711,425 = 0.996 * 2^24
    (254, 8, 258, 0),          # fast kernel, lag * size = 65532
    (255, 10, 258, 0),         # lag * size = 65790: generic, wide
    (256, 10, 255, 0),         # a count of 256: 16-bit K, lag * size = 65280, narrow
    (2000, 40, 32, 1024),      # q2max = 1058 * 4e6 = 0.985 * 2^32: narrow
    (2000, 40, 32, 1280),      # q2max beyond 2^32: wide
    (300, 31, 218, 1792),      # 62,673 tile bytes
    (276, 34, 125, 1792),      # 65,520 tile bytes: the limit itself
]


@functools.lru_cache(maxsize=None)
def saturated_case(size, step, lag):
    """ctg 0: random at G/C 0.999 (V != 0); ctg 1: all-G/C and all-A/T blocks whose lengths are no multiple of the
    step; ctg 2: all G/C (the constant table)"""
    n = size + (lag + WINDOWS) * step
    lo = max(size + size // 2, 3 * step) | 1
    seqs = [random_gc(n, 0.999, 11), blocks(n + 41, lo, 3 * lo, step, 12), random_gc(n + 5, 2.0, 13)]
    return Case(size, step, lag, seqs)


def saturated_thresholds(case):
    return [1.0, 2.0, 3.0] + case.thresholds(2)


def tile_bytes(size, step, lag, tile):
    return (lag + 1) * step + size + 32 + tile * step


def q2_prefix_max(case, tile):
    """the largest prefix of k^2 a tile of `tile` windows (with its lag + 1 windows in front) holds, over ctg 0"""
    k = case.cnt[0].astype(np.int64)
    p2 = np.concatenate(([0], np.cumsum(k * k)))
    best = 0
    for w0 in range(0, k.size, tile):
        wh = w0 - case.lag - 1 if w0 > case.lag else 0
        best = max(best, int(p2[min(w0 + tile, k.size)] - p2[wh]))
    return best
