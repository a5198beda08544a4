"""The wave decision at knife-edge thresholds and with saturated sums, against the CPU oracle, bit for bit.

The wave kernels decide |x - mean| > thr * sd in integer / squared form and hand a window to the reference's f32
order only inside a derived guard band.  tests/knife.py builds the inputs on which that band and the
arithmetic widths are stressed, and test_wave_knife_cpu.py shows on the oracle alone that they are: thousands of
windows per configuration on which f32 and real arithmetic differ, sums at the limit of every width.  Here every
decision path (kernel_name() is asserted first) runs them: dense counts, dense signals and peaks of every ctg, with
the default guard, with the derived bound alone (safety 1.0) and with every window exact; the fast kernels from the
bytes and from the G/C plane; exact_count() at least the windows that no integer form can have decided.

A band that is too thin, or a sum that does not fit its width, fails here on signal mismatches."""
import numpy as np
import pytest

import knife
from gams_amd import _lib, engine

pytestmark = pytest.mark.gpu

BOTH = _lib.WAVE_PEAKS | _lib.WAVE_DENSE
PLANE, BYTES = _lib.WAVE_INPUT_PLANE, _lib.WAVE_INPUT_BYTES
FAST_RT = "wave_fast_kernel<4, 0, 0, 0, false, 256>"
DIRECT = "wave_direct_count_kernel + wave_direct_signal_kernel"


def tile_name(k16, wide):
    return "wave_tile_kernel<%s, %s>" % ("unsigned short" if k16 else "unsigned char", "true" if wide else "false")


@pytest.fixture(scope="module")
def eng():
    e = engine.Engine(0)
    yield e
    e.close()


class Tally:
    """what a test compared and what differed: one assertion at the end says how many windows were wrong"""

    def __init__(self):
        self.passes = self.windows = self.must = self.exact = 0
        self.bad, self.short = [], []

    def compare(self, plan, case, thr, infl, tag):
        osig = case.oracle(thr, infl)
        pk = plan.peaks()
        exp = []
        for c, (ocnt, os_) in enumerate(zip(case.cnt, osig)):
            cnt, sig = plan.dense(c)
            assert np.array_equal(cnt, ocnt), (tag, thr, c, np.flatnonzero(cnt != ocnt)[:5])
            n = int(np.count_nonzero(sig.astype(np.int32) != os_))
            if n:
                self.bad.append((tag, thr, c, n))
            idx = np.flatnonzero(os_)
            rec = np.zeros(idx.size, _lib.PEAK_DTYPE)
            rec["ctg"], rec["window"], rec["gc_count"], rec["signal"] = c, idx, ocnt[idx], os_[idx]
            exp.append(rec)
            self.windows += ocnt.size
        if not np.array_equal(pk, np.concatenate(exp)):
            self.bad.append((tag + " peaks", thr, -1, abs(int(pk.size) - sum(e.size for e in exp))))
        self.passes += 1

    def done(self, what):
        wrong = sum(b[3] for b in self.bad if b[2] >= 0)
        print(f"{what}: {self.passes} passes, {self.windows} window-decisions, exact path {self.exact} "
              f"(at least {self.must} needed), {wrong} signal mismatches")
        assert not self.bad, f"{what}: {wrong} signal mismatches in {len(self.bad)} comparisons, first {self.bad[:4]}"
        # windows on which the oracle is not real arithmetic cannot have been decided by the integer form
        assert not self.short, f"{what}: exact path below its floor in {len(self.short)} passes, first {self.short[:4]}"


def run_passes(eng, case, thresholds, name, tile=0, threads=0, infl=1.0, inputs=(None,), counts_exact=True,
               all_exact_at=1):
    """one seqset, one plan per threshold: default guard and safety 1.0 for each input form, and every window exact
    for the first `all_exact_at` thresholds"""
    tally = Tally()
    ss = engine.SeqSet(eng, case.seqs)
    try:
        for n, thr in enumerate(thresholds):
            plan = engine.WavePlan(eng, ss, case.size, case.step, case.lag, thr, infl, flags=BOTH, tile_windows=tile)
            if threads:
                plan.set_threads(threads)
            assert plan.kernel_name() == name, (case.prm, thr, plan.kernel_name())
            need = case.must_be_exact(thr) if counts_exact and infl == 1.0 else 0
            guards = [("default", 1.5, False), ("safety 1", 1.0, False)] + ([("all exact", 1.5, True)] if n < all_exact_at else [])
            for mode in inputs:
                if mode is not None:
                    plan.set_input(mode)
                for tag, safety, all_exact in guards:
                    plan.set_guard(safety, all_exact)
                    plan.run()
                    if mode is not None:
                        assert plan.last_input() == mode
                    tally.compare(plan, case, thr, infl, f"{tag}{'' if mode is None else ', plane' if mode == PLANE else ', bytes'}")
                    if counts_exact and infl == 1.0:
                        got = plan.exact_count()
                        if got < need:
                            tally.short.append((tag, thr, got, need))
                        tally.exact += got
                        tally.must += need
            plan.close()
    finally:
        ss.close()
    return tally


# (size, step, lag), tile, threads, the kernel, both input forms?
KNIFE_PATHS = [
    ((100, 10, 100), 0, 0, "wave_fast_kernel<4, 100, 10, 100, false, 256>", True),      # baked headline, W = 4
    ((100, 10, 100), 3072, 0, "wave_fast_kernel<12, 100, 10, 100, false, 256>", True),  # ... and the W = 12 of a genome
    ((100, 1, 100), 7168, 64, "wave_fast_kernel<28, 100, 1, 100, false, 64>", True),    # baked step 1, a tile per wave
    ((100, 1, 100), 5120, 0, "wave_fast_kernel<20, 100, 1, 100, false, 256>", True),
    ((100, 5, 200), 0, 0, "wave_fast_kernel<4, 100, 5, 0, false, 256>", True),          # size and step baked, lag an argument
    ((255, 10, 257), 0, 0, FAST_RT, True),                                              # run-time, lag * size = 65535
    ((50, 7, 33), 0, 0, FAST_RT, True),
    ((255, 10, 258), 1024, 0, tile_name(False, True), False),                           # generic, 8-bit counts, wide
    ((300, 10, 218), 1024, 0, tile_name(True, False), False),                           # generic, 16-bit counts, narrow
    ((300, 10, 250), 1024, 0, tile_name(True, True), False),                            # generic, 16-bit counts, wide
    ((1000, 50, 30), 0, 0, tile_name(True, False), False),                              # generic, large size
    ((1000, 500, 100), 0, 0, DIRECT, False),                                            # untiled
]


@pytest.mark.parametrize("prm,tile,threads,name,fast", KNIFE_PATHS, ids=[f"{p[0]}-{p[1]}" for p in KNIFE_PATHS])
def test_knife_thresholds_on_every_decision_path(eng, prm, tile, threads, name, fast):
    case = knife.knife_case(*prm)
    thr = case.thresholds()
    assert len(thr) == 66
    tally = run_passes(eng, case, thr, name, tile, threads, inputs=(BYTES, PLANE) if fast else (None,),
                       counts_exact=name != DIRECT)
    if name != DIRECT:
        assert tally.must >= 1000          # (the floor test_wave_knife_cpu.py holds the inputs to, seen from here)
    tally.done(f"{prm} {name}")


@pytest.mark.parametrize("prm", [(100, 10, 100), (50, 7, 33)])
@pytest.mark.parametrize("infl", [0.5, 0.0])
def test_knife_thresholds_through_the_repair_sweeps(eng, prm, infl):
    """influence != 1: the sweeps evaluate every window themselves (jac_eval_kernel), at the thresholds of three states"""
    case = knife.knife_case(*prm)
    tally = run_passes(eng, case, case.thresholds(3), "jac_eval_kernel", infl=infl, counts_exact=False, all_exact_at=0)
    tally.done(f"{prm} influence {infl}")


# (size, step, lag, tile) of knife.SATURATED -> the kernel that has to hold the sums
SATURATED_PATHS = {
    (255, 10, 257, 0): FAST_RT,
    (254, 8, 258, 0): FAST_RT,
    (255, 10, 258, 0): tile_name(False, True),
    (256, 10, 255, 0): tile_name(True, False),
    (2000, 40, 32, 1024): tile_name(True, False),
    (2000, 40, 32, 1280): tile_name(True, True),
    (300, 31, 218, 1792): tile_name(True, False),
    (276, 34, 125, 1792): tile_name(True, False),
}


@pytest.mark.parametrize("size,step,lag,tile", knife.SATURATED)
def test_saturated_sums_on_both_sides_of_every_width(eng, size, step, lag, tile):
    """ctgs of random G/C 0.999, of all-G/C and all-A/T blocks, and of G/C alone, at thresholds 1, 2, 3 and the knife
    thresholds of two states: S1 = lag * size, S2 next to 2^24 (fast kernel), a count of 256, the Q2 prefix next to
    2^32 and beyond it, chunk prefixes up to the 65,520 bytes of the largest tile"""
    case = knife.saturated_case(size, step, lag)
    name = SATURATED_PATHS[(size, step, lag, tile)]
    fast = name == FAST_RT
    # (a tile the 16-bit chunk prefix or the LDS could not hold would have been cut down or sent to the untiled kernels:
    # the kernel's name and, for the Q2 prefix, its narrow / wide form say the requested tile was taken)
    tally = run_passes(eng, case, knife.saturated_thresholds(case), name, tile if tile else (0 if fast else 1024),
                       inputs=(BYTES, PLANE) if fast else (None,), all_exact_at=1)
    tally.done(f"{(size, step, lag, tile)} {name}")
