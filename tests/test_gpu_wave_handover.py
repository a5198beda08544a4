"""influence != 1 beyond the guess-and-iterate sweeps: the hand-over of a batch to wave_serial_wave_kernel inside
wave_jac_settle (wave.hip) -- after kJacMaxSweeps = 48 sweeps without a flip-free one, or at a run of more than
kJacRunCap = 8192 signalled windows -- on both sides of either limit, the plans that never sweep (lag > 16000: the
one-wavefront-per-ctg ring up to lag 16383, one lane per ctg beyond), and the readers of a pass that was handed over.

Which path ran is asserted, not assumed: gams_wave_plan_settled reports it, and helpers.sweep_model (the plain sweeps
in strict float32, on the CPU) says for every case how many sweeps the iteration takes and how long its runs get, so
that each test states its own precondition.  Every answer is compared with the oracle."""
import functools
import math

import numpy as np
import pytest

import helpers
from helpers import synth
from gams_amd import _lib, engine, host
from oracle import oracle as ora

pytestmark = pytest.mark.gpu

BOTH = _lib.WAVE_PEAKS | _lib.WAVE_DENSE
MAX_SWEEPS, RUN_CAP, FIRST_BATCH, BATCH = 48, 8192, 6, 8       # kJacMaxSweeps, kJacRunCap, kJacFirstBatch, later batches
TAIL = b"ACGT" * 3000 + b"N" * 500 + b"GGCC" * 2000


@pytest.fixture(scope="module")
def eng():
    e = engine.Engine(0)
    yield e
    e.close()


@functools.lru_cache(maxsize=None)
def seq_of(n, seed):
    return synth(n, seed).tobytes()


@functools.lru_cache(maxsize=None)
def oracle_of(seq, size, step, lag, thr, infl):
    cnt, _, sig = ora.wave_windows(seq, size, step, lag, thr, infl)
    cnt.setflags(write=False)
    sig.setflags(write=False)
    return cnt, sig


@functools.lru_cache(maxsize=None)
def model_of(seq, size, step, lag, thr, infl):
    """(sweeps up to and including the first flip-free one, longest run of signalled windows in any state) of the plain
    sweeps; the model's fixed point is the oracle's answer"""
    cnt, s1 = oracle_of(seq, size, step, lag, thr, 1.0)
    flips, run, sig = helpers.sweep_model(cnt, size, lag, thr, infl, s1)
    assert flips[-1] == 0 and np.array_equal(sig, oracle_of(seq, size, step, lag, thr, infl)[1])
    return len(flips), run


def expected_settled(m, run):
    """what wave_jac_settle implies for a plan on the plain sweeps: 6 sweeps are queued with the pass, batches of 8 while
    none was flip-free, never more than 48; the batch is handed over past 48 sweeps or at a run beyond the cap"""
    serial = m > MAX_SWEEPS or run > RUN_CAP
    sweeps = FIRST_BATCH if m <= FIRST_BATCH else min(MAX_SWEEPS, FIRST_BATCH + BATCH * math.ceil((m - FIRST_BATCH) / BATCH))
    return sweeps, serial


def check_against_oracle(plan, seqs, prm, pk=None, tag=None):
    """dense counts and signals of every ctg, and the peaks (window, signal, gc_count, in (ctg, window) order)"""
    pk = plan.peaks() if pk is None else pk
    dense = bool(plan.flags & _lib.WAVE_DENSE)
    exp_ctg, exp_win, exp_sig, exp_cnt = [], [], [], []
    for c, sq in enumerate(seqs):
        ocnt, osig = oracle_of(sq, *prm)
        if dense:
            cnt, sig = plan.dense(c)
            assert np.array_equal(cnt, ocnt), (prm, tag, c)
            bad = np.flatnonzero(sig.astype(np.int32) != osig)
            assert bad.size == 0, (prm, tag, c, bad.size, bad[:5], sig[bad[:5]], osig[bad[:5]])
        idx = np.flatnonzero(osig)
        exp_ctg.append(np.full(idx.size, c))
        exp_win.append(idx)
        exp_sig.append(osig[idx])
        exp_cnt.append(ocnt[idx])
    assert pk.size == sum(a.size for a in exp_win), (prm, tag, pk.size)
    assert np.array_equal(pk["ctg"], np.concatenate(exp_ctg)) and np.array_equal(pk["window"], np.concatenate(exp_win)), (prm, tag)
    assert np.array_equal(pk["signal"], np.concatenate(exp_sig)) and np.array_equal(pk["gc_count"], np.concatenate(exp_cnt)), (prm, tag)
    return pk


def run_twice_and_check(eng, seqs, prm, flags=BOTH):
    """two passes on one plan (the second starts from the first one's tables and flags), every ctg against the oracle
    -> (settled() before the peaks were read, settled() after, kernel name, peaks)"""
    ss = engine.SeqSet(eng, seqs)
    plan = engine.WavePlan(eng, ss, *prm, flags=flags)
    name = plan.kernel_name()
    plan.run()
    plan.run()
    before = plan.settled()
    pk = check_against_oracle(plan, seqs, prm)
    after = plan.settled()
    plan.close()
    ss.close()
    return before, after, name, pk


# ---- B1: the run cap ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,size,infl,run,differs,serial", [
    (83_010, 100, 0.5, 8192, 34, False),        # 8292 windows: the run is exactly the cap
    (83_020, 100, 0.5, 8193, 32, True),         # 8293 windows: one more
    (83_321, 401, 0.0, 8193, 2172, True),       # the same run in the guess; far from the answer: the guess cannot pass
])
def test_run_cap_both_sides(eng, n, size, infl, run, differs, serial):
    """Threshold -1 signals every tested window of the influence-1 guess: a single run of n_win - lag windows, which
    jac_filter_kernel walks up to 8192 and abandons (kJacAbandon) at 8193.  Every window is a peak, so the slots of
    tile_windows / 8 records overflow: peaks() regrows them and runs the pass again, and the hand-over happens a second
    time inside that call -- settled() says the same before and after."""
    prm = (size, 10, 100, -1.0, infl)
    seq = seq_of(n, 71)
    ocnt, osig = oracle_of(seq, *prm)
    s1 = oracle_of(seq, size, 10, 100, -1.0, 1.0)[1]
    assert np.count_nonzero(s1) == ocnt.size - 100 == run and int(np.count_nonzero(s1 != osig)) == differs
    m, longest = model_of(seq, *prm)
    assert (m, longest) == (2, run)
    before, after, name, pk = run_twice_and_check(eng, [seq], prm)
    assert name == "jac_eval_kernel"
    assert before[1] is serial and after[1] is serial, (before, after)
    if not serial:
        assert before[0] == after[0] == expected_settled(m, longest)[0] == 6
    if infl == 0.5:
        assert np.array_equal(pk["window"], np.arange(100, ocnt.size)) and pk.size == run    # every record, in window order


# ---- B2: the sweep limit --------------------------------------------------------------------------------------------
SWEEP_ROWS = [
    # size, lag, thr, model m, longest run, serial
    (401, 100, 2.0, 76, 495, True),
    (401, 30, 1.0, 72, 689, True),
    (450, 50, 2.0, 148, 1032, True),
    (500, 100, 1.0, 51, 664, True),             # just over 48
    (401, 30, 0.5, 47, 5911, False),            # just under: the 47th sweep flips nothing, 48 were queued
]


@pytest.mark.parametrize("size,lag,thr,m,run,serial", SWEEP_ROWS)
def test_sweep_limit_both_sides(eng, size, lag, thr, m, run, serial):
    """influence 0 with size > 400 takes the plain sweeps (the jac0_* kernels need a (size + 1)^2 table); no run comes
    near the cap, so only the limit of 48 sweeps can hand the ctg over."""
    prm = (size, 10, lag, thr, 0.0)
    seq = seq_of(60_000, 72)
    assert model_of(seq, *prm) == (m, run) and run < RUN_CAP
    assert expected_settled(m, run)[1] is serial
    before, after, name, _ = run_twice_and_check(eng, [seq], prm)
    assert name == "jac_eval_kernel"
    assert before == after and after[1] is serial, (before, after)
    if not serial:
        assert after[0] == expected_settled(m, run)[0] == 48


@pytest.fixture(scope="module")
def batch(s288c):
    """the ctg that runs into the sweep limit in the middle of a batch"""
    return [bytes(s288c["Mito"][:20_000]), seq_of(60_000, 72), TAIL]


@pytest.mark.parametrize("size,lag,thr,m,run,serial", [r for r in SWEEP_ROWS if r[5]])
def test_sweep_limit_hands_the_whole_batch_over(eng, batch, size, lag, thr, m, run, serial):
    """the flips are counted over the batch: ctg 1 exhausts the sweeps, all three ctgs go to the serial kernel and
    every one of them equals the oracle"""
    prm = (size, 10, lag, thr, 0.0)
    assert model_of(batch[1], *prm) == (m, run)
    before, after, _, _ = run_twice_and_check(eng, batch, prm)
    assert before[1] is True and after[1] is True, (before, after)


@pytest.mark.parametrize("lag,thr,infl,m", [(100, 3.0, 0.5, 2), (100, 0.3, 0.25, 5), (100, 0.3, 1.5, 3), (100, 1.0, 0.999, 1)])
def test_ordinary_plans_do_not_hand_over(eng, lag, thr, infl, m):
    """controls: the first batch of six sweeps settles these, nothing is handed over"""
    prm = (100, 10, lag, thr, infl)
    seq = seq_of(60_000, 72)
    got_m, run = model_of(seq, *prm)
    assert got_m == m and run < RUN_CAP
    before, after, name, _ = run_twice_and_check(eng, [seq], prm)
    assert name == "jac_eval_kernel"
    assert before == after == (6, False) == expected_settled(m, run), (before, after)


# ---- B3: plans that never sweep ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("infl", [3.0, -0.5])
@pytest.mark.parametrize("lag,extra,kernel", [
    (16_000, 300, "jac_eval_kernel"),            # the last lag that still sweeps
    (16_001, 300, "wave_serial_wave_kernel"),
    (16_383, 300, "wave_serial_wave_kernel"),    # lag + 1 = 16384 floats: the LDS ring is exactly full
    (16_384, 64, "wave_serial_kernel"),          # one lane per ctg beyond the ring
    (20_000, 64, "wave_serial_kernel"),
])
def test_lags_beyond_the_sweeps(eng, lag, extra, kernel, infl):
    """lag > 16000: the recurrence itself computes the pass.  With 16,000 values in the history an influence inside
    [0, 1] gives the influence-1 answer (a kernel that ignored the recurrence would pass), 3.0 and -0.5 do not: the
    oracle's answer differs from its own influence-1 answer in at least 10 windows, asserted here."""
    prm = (20, 1, lag, 1.0, infl)
    seq = seq_of(lag + extra + 19, 80)
    ocnt, osig = oracle_of(seq, *prm)
    assert ocnt.size == lag + extra
    assert np.count_nonzero(osig != oracle_of(seq, 20, 1, lag, 1.0, 1.0)[1]) >= 10
    before, after, name, _ = run_twice_and_check(eng, [seq], prm)
    assert name == kernel
    if lag > 16_000:
        assert before == after == (0, True)


def test_lag_one_is_serial_and_never_signals(eng):
    """lag 1: the sample sd of one value is NaN, nothing signals; influence != 1 makes the plan serial, and lag < 2
    keeps it off the sweeps"""
    prm = (100, 10, 1, 3.0, 0.5)
    seq = seq_of(20_000, 72)
    before, after, name, pk = run_twice_and_check(eng, [seq], prm)
    assert name == "wave_serial_wave_kernel" and before == after == (0, True)
    assert pk.size == 0 and not oracle_of(seq, *prm)[1].any()


# ---- B4: the readers on top of a hand-over ----------------------------------------------------------------------------
B4 = (401, 10, 100, 2.0, 0.0)
NAMES, STARTS = ["Mito", "a-long_name.7", "tail"], [1, 1_999_000_001, 5]


def test_peaks_only_plan_after_a_hand_over(eng, batch):
    ss = engine.SeqSet(eng, batch)
    both = engine.WavePlan(eng, ss, *B4, flags=BOTH)
    only = engine.WavePlan(eng, ss, *B4, flags=_lib.WAVE_PEAKS)
    for plan in (both, only):
        plan.run()
        plan.run()
    pk = check_against_oracle(both, batch, B4)
    assert np.array_equal(only.peaks(), pk)
    check_against_oracle(only, batch, B4)
    assert both.settled()[1] is True and only.settled()[1] is True
    both.close()
    only.close()
    ss.close()


def test_both_held_passes_of_depth_two_after_a_hand_over(eng, batch):
    ss = engine.SeqSet(eng, batch)
    plan = engine.WavePlan(eng, ss, *B4, flags=BOTH)
    plan.set_depth(2)
    plan.run()
    plan.run()
    for age in (1, 0):
        plan.select(age)
        check_against_oracle(plan, batch, B4, tag=age)
        assert plan.settled()[1] is True, age
    plan.close()
    ss.close()


def test_rows_and_signal_text_after_a_hand_over(eng, batch):
    """gams_wave_rows_*, gams_wave_signal_text and the host operator over a pass that the serial kernel computed:
    the oracle's text, per ctg"""
    kw = dict(size=B4[0], step=B4[1], lag=B4[2], threshold=B4[3], influence=B4[4])
    ctgs = [dict(id=f"ctg:{nm}:1", chr_id=nm, chr_start=st, chr_end=st + len(sq) - 1, seq=sq)
            for nm, st, sq in zip(NAMES, STARTS, batch)]
    exp_rows = [ora.wave_proc_ctg(c["chr_id"], c["chr_start"], c["chr_end"], c["seq"], coverage=0.2, **kw) for c in ctgs]
    exp_sig = [ora.wave_proc_ctg(c["chr_id"], c["chr_start"], c["chr_end"], c["seq"], is_signal=True, **kw) for c in ctgs]
    assert all(len(r) > 0 for r in exp_rows)
    ss = engine.SeqSet(eng, batch)
    plan = engine.WavePlan(eng, ss, *B4, flags=_lib.WAVE_PEAKS)
    plan.rows_setup(NAMES, STARTS, 0.2)
    for rep in range(2):
        plan.run()
        plan.rows_begin()
        text, off = plan.rows_end()
    assert plan.settled()[1] is True
    assert [text[int(off[c]):int(off[c + 1])].decode() for c in range(3)] == exp_rows
    assert int(off[-1]) == len(text)
    plan.close()
    plan = engine.WavePlan(eng, ss, *B4, flags=_lib.WAVE_DENSE)
    for rep in range(2):
        plan.run()
        text, off = plan.signal_text(NAMES, STARTS)
    assert plan.settled()[1] is True
    assert [text[int(off[c]):int(off[c + 1])].decode() for c in range(3)] == exp_sig
    plan.close()
    ss.close()
    assert host.wave(eng, ctgs, coverage=0.2, **kw) == "".join(exp_rows)
    assert host.wave(eng, ctgs, is_signal=True, **kw) == "".join(exp_sig)
