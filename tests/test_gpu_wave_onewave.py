"""The one-wave cut of the narrow body: wave_fast_onewave_kernel cuts the tile of wave_fast_kernel<12, 100,
10, 100, NT, 256> -- 3,072 K slots, 2,971 windows -- as 64 threads x 48 windows, a workgroup of one wave, with K laid over
the tile's bit stream and the tiles at a ctg start counted from a zeroed pad.  Every case runs one seqset four ways -- the
wide body on the plane, the two-wave cut, the one-wave cut, the bytes -- asserts what each pass ran, and compares the peaks
and the exact-path count of all four with the CPU oracle's and with each other.

All plans ask for 3,072-window tiles, as in tests/test_gpu_wave_narrow.py (whose helpers these are).  A thread of the
one-wave cut owns 48 windows in two runs of 24: window `lag` = 100 of a ctg is thread 2's q = 4, and a ctg of 101 .. 196
windows puts the tile's last window on every q of threads 2 and 3 -- across the seam of the runs at 23 | 24, the halves of
the 64-bit masks at 31 | 32, the renewals of the bound on S1 at 12, 24 and 36, and q = 47."""
import numpy as np
import pytest

import knife
from gams_amd import _lib, engine
from test_gpu_wave_narrow import HEAD, NAME, TW, bases, headline_plan, mixed, oracle_of, oracle_peaks, records
from test_wave_cut_cpu import AUTO_CUT

pytestmark = pytest.mark.gpu

PLANE, BYTES, AUTO_IN = _lib.WAVE_INPUT_PLANE, _lib.WAVE_INPUT_BYTES, _lib.WAVE_INPUT_AUTO
WIDE, NARROW, AUTO_BODY = _lib.WAVE_BODY_WIDE, _lib.WAVE_BODY_NARROW, _lib.WAVE_BODY_AUTO
CUT_AUTO, TWO, ONE = _lib.WAVE_CUT_AUTO, _lib.WAVE_CUT_TWO_WAVES, _lib.WAVE_CUT_ONE_WAVE
# way -> body, cut and input asked for, and the (body, cut) the pass then reports
WAYS = (("wide", WIDE, CUT_AUTO, PLANE, (WIDE, 0)), ("two waves", NARROW, TWO, PLANE, (NARROW, TWO)),
        ("one wave", NARROW, ONE, PLANE, (NARROW, ONE)), ("bytes", AUTO_BODY, CUT_AUTO, BYTES, (WIDE, 0)))


@pytest.fixture(scope="module")
def eng():
    e = engine.Engine(0)
    yield e
    e.close()


def ran(plan):
    return plan.last_body(), plan.last_cut()


def four_ways(eng, seqs, prm=HEAD, all_exact=False, fresh=False):
    """-> the oracle's peaks, after all four ways have produced exactly them.  fresh: a new plan for every way, so that
    each meets the slots of a new plan (tw / 8 records a tile) and not the ones an earlier way's reader has regrown."""
    exp = oracle_peaks(seqs, prm)
    decidable = sum(max(len(oracle_of(s, prm)[0]) - prm[2], 0) for s in seqs)
    ss = engine.SeqSet(eng, seqs)

    def new_plan():
        plan = headline_plan(eng, ss, prm)
        if all_exact:
            plan.set_guard(1.5, True)
        return plan

    try:
        plan = new_plan()
        got, exact = {}, {}
        for way, body, cut, inp, want in WAYS:
            if fresh and got:
                plan.close()
                plan = new_plan()
            plan.set_body(body)
            plan.set_cut(cut)
            plan.set_input(inp)
            plan.run()
            assert plan.last_input() == inp and ran(plan) == want, (way, ran(plan))
            got[way] = plan.peaks().copy()
            # (a reader that met an overflowing tile has regrown the slots and run the pass again: the same body and cut)
            assert plan.last_input() == inp and ran(plan) == want, (way, ran(plan))
            exact[way] = plan.exact_count()
            assert plan.kernel_name() == NAME                  # the list entry, whichever body and cut ran
        assert records(got["wide"]) == exp
        for way in ("two waves", "one wave", "bytes"):
            assert np.array_equal(got[way], got["wide"]), way
        # the exact path: the same windows however the tile is cut (every cut renews its bound on S1 per twelve windows)
        assert exact["bytes"] == exact["wide"] == exact["two waves"] == exact["one wave"] <= decidable, exact
        if all_exact:
            assert exact["one wave"] == decidable, exact
        if fresh:
            plan.close()
            plan = new_plan()
        plan.set_body(AUTO_BODY)
        plan.set_cut(CUT_AUTO)
        plan.set_input(AUTO_IN)
        plan.run()
        assert plan.last_input() == PLANE and ran(plan) == (NARROW, AUTO_CUT)      # what wave_select_cut says
        assert np.array_equal(plan.peaks(), got["wide"])
        assert ran(plan) == (NARROW, AUTO_CUT)
        plan.close()
    finally:
        ss.close()
    return exp


def test_last_window_through_every_q_of_threads_2_and_3(eng):
    wins = list(range(101, 197))
    seqs = mixed([bases(n) + k % 10 for k, n in enumerate(wins)], 71)          # + ragged tails shorter than a step
    # threshold 0.5: most windows signal, and so does the LAST window of most ctgs -- the one a wrong mask or bound loses
    exp = four_ways(eng, seqs, prm=(100, 10, 100, 0.5, 1.0))
    last_q = {(wins[c] - 1) % 48 for c, w, *_ in exp if w == wins[c] - 1}
    assert len(last_q) >= 36 and {q for q in (23, 24, 31, 32, 36, 47, 0) if q in last_q} >= {24, 32, 36}, sorted(last_q)
    four_ways(eng, seqs)                                                        # and at the headline's threshold


def test_short_ctgs_of_1_to_100_windows(eng):
    # 1 .. 99 windows: fewer than `lag`, where the reference panics -- the plan is refused, so no cut ever sees such a tile
    for n in (1, 2, 24, 48, 50, 99):
        ss = engine.SeqSet(eng, mixed([bases(150), bases(n)], 72))
        with pytest.raises(_lib.GamsError) as ei:
            engine.WavePlan(eng, ss, *HEAD, tile_windows=3072)
        assert ei.value.code == _lib.ESHORT
        ss.close()
    # exactly `lag` windows: nothing in the ctg can signal; its tiles (nK = 201 slots) run between tiles that do
    wins = [100, 150, 100, 100, 197, 100]
    exp = four_ways(eng, mixed([bases(n) + k for k, n in enumerate(wins)], 72), prm=(100, 10, 100, 0.5, 1.0))
    assert exp and {c for c, *_ in exp} == {1, 4}


def test_second_tile_behind_a_full_one(eng):
    # the second tile runs with vb >= 0: 2,970 / 2,971 / 2,972 windows, and a second tile of 24 .. 102 windows
    wins = [TW - 1, TW, TW + 1] + [TW + n for n in (24, 25, 48, 49, 101, 102)]
    exp = four_ways(eng, mixed([bases(n) for n in wins], 73))
    assert {c for c, *_ in exp} == set(range(len(wins)))
    assert any(w >= TW for _, w, *_ in exp)


@pytest.mark.parametrize("seed", [74, 75])
def test_ctg_start_tiles_behind_full_tiles(eng, seed):
    rng = np.random.default_rng(seed)
    lens = [1090 + seed, bases(2 * TW + 7), 4097, bases(TW) + 3, 12345, bases(TW + 50), 1100, 61007]
    four_ways(eng, [rng.integers(0, 256, n, dtype=np.uint8) for n in lens])


def test_constant_runs_at_ctg_starts_and_tile_seams(eng):
    # homopolymer and N runs longer than (lag + 1) * step + size = 1,110 bases: at a ctg's start (the zeroed pad next to
    # real zeros), across the seam at window 2,971, and a ctg of G alone
    seq = np.frombuffer(b"ACGTacgtNn", np.uint8)[np.random.default_rng(76).integers(0, 10, 40000)].copy()
    seq[:1500] = ord("G")
    seq[28400:31600] = ord("c")
    seq[33000:34300] = ord("N")
    four_ways(eng, [seq, np.full(bases(300), ord("G"), np.uint8), mixed([bases(TW + 5)], 77)[0]])


def test_every_window_through_the_exact_path(eng):
    # exact_signal_wave for every decidable window, its owner and q found from the two halves of the lane's 64-bit mask
    four_ways(eng, mixed([20000, bases(150)], 78), all_exact=True)


def test_knife_thresholds_of_one_periodic_input(eng):
    case = knife.knife_case(*HEAD[:3])
    seq = case.seqs[0]
    ss = engine.SeqSet(eng, [seq])
    try:
        for thr in case.thresholds():
            osig, ocnt = case.oracle(thr)[0], case.cnt[0]
            idx = np.flatnonzero(osig)
            exp = [(0, int(i), int(ocnt[i]), int(osig[i])) for i in idx]
            plan = headline_plan(eng, ss, (100, 10, 100, thr, 1.0))
            exact = {}
            for way, body, cut, inp, want in WAYS:
                plan.set_body(body)
                plan.set_cut(cut)
                plan.set_input(inp)
                plan.run()
                assert ran(plan) == want, (thr, way)
                assert records(plan.peaks()) == exp, (thr, way)
                exact[way] = plan.exact_count()
            assert len(set(exact.values())) == 1, (thr, exact)
            plan.close()
    finally:
        ss.close()


def test_threshold_0_overflows_the_slots_and_reruns(eng):
    # nearly every window from `lag` on signals (all but those that sit exactly on the mean): up to 48 records a thread.
    # A new plan gives a tile a slot of tw / 8 = 371 records: both tiles overflow, the kernel stores what fits and counts
    # the rest, the first reader regrows the slots and runs the pass again -- through the same body and cut.
    prm = (100, 10, 100, 0.0, 1.0)
    seqs = mixed([40000], 79)
    exp = oracle_peaks(seqs, prm)
    cap = TW // 8
    assert sum(1 for _, w, *_ in exp if w < TW) > 2 * cap and sum(1 for _, w, *_ in exp if w >= TW) > 2 * cap
    wins = {w for _, w, *_ in exp}
    assert any(all(48 * t + q in wins for q in range(48)) for t in range(3, 61))   # a thread of tile 0 full of records
    assert four_ways(eng, seqs, prm=prm, fresh=True) == exp


def test_three_plans_on_three_lanes_and_peaks_at_the_thread_seam(eng):
    # the benchmark's timed region in small: a plan per seqset on lanes 0, 1, 2, the taper off, passes in flight; at
    # threshold 1 a third of the windows signal, so records sit at q = 47 of one thread and q = 0 of the next
    prm = (100, 10, 100, 1.0, 1.0)
    batches = [mixed([bases(2 * TW + 7), 15000 + 100 * j, bases(TW)], 80 + j) for j in range(3)]
    sets = [engine.SeqSet(eng, b) for b in batches]
    plans = []
    for j, ss in enumerate(sets):
        p = headline_plan(eng, ss, prm)
        p.set_lane(j)
        p.set_taper(0)
        plans.append(p)
    for b in batches:
        wins = {(c, w) for c, w, *_ in oracle_peaks(b, prm)}
        assert any((c, w + 1) in wins for c, w in wins if w % TW % 48 == 47)
    for cut in (ONE, TWO, CUT_AUTO):
        for p in plans:
            p.set_cut(cut)
        for i in range(12):
            plans[i % 3].run()
        eng.sync()
        for p, b in zip(plans, batches):
            assert p.last_input() == PLANE and ran(p) == (NARROW, cut if cut else AUTO_CUT)
            assert records(p.peaks()) == oracle_peaks(b, prm)
    for p in plans:
        p.close()
    for ss in sets:
        ss.close()


def test_forced_one_wave_where_the_narrow_body_cannot_run(eng):
    seqs = mixed([30000, 12000], 83)
    ss = engine.SeqSet(eng, seqs)
    for flags, tile, inp in ((_lib.WAVE_PEAKS | _lib.WAVE_DENSE, 3072, AUTO_IN), (_lib.WAVE_PEAKS, 2048, AUTO_IN),
                             (_lib.WAVE_PEAKS, 3072, BYTES)):
        plan = engine.WavePlan(eng, ss, *HEAD, flags=flags, tile_windows=tile)
        plan.set_input(inp)
        plan.set_cut(ONE)
        with pytest.raises(_lib.GamsError) as ei:
            plan.run()
        assert ei.value.code == _lib.ESTATE
        for cut in (TWO, CUT_AUTO):                            # these ask for nothing where no narrow body runs
            plan.set_cut(cut)
            plan.run()
            assert ran(plan) == (WIDE, 0) and records(plan.peaks()) == oracle_peaks(seqs, HEAD)
        plan.close()
    plan = headline_plan(eng, ss)
    with pytest.raises(_lib.GamsError) as ei:
        plan.set_cut(3)
    assert ei.value.code == _lib.EINVAL
    plan.set_body(WIDE)                                        # the wide kernel on a narrow-fit pass: no cut to report
    plan.set_cut(ONE)
    plan.run()
    assert ran(plan) == (WIDE, 0) and records(plan.peaks()) == oracle_peaks(seqs, HEAD)
    plan.close()
    ss.close()
