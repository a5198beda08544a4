"""The narrow body of the headline tile: wave_fast_narrow_kernel cuts the tile of wave_fast_kernel<12, 100,
10, 100, NT, 256> as 128 threads x 24 windows for plane-fed peaks-only passes.  Every case runs one seqset three ways --
the wide body on the plane, the narrow body on the plane, the bytes -- asserts what each pass ran, and compares the
peaks of all three with the CPU oracle's; a dense twin plan (which keeps the wide kernel) gives counts and signals.

All plans ask for 3,072-window tiles (gams_wave_plan_set_tile): that is the headline entry on inputs of kilobases, where
the library's own ladder would take W = 4.  A tile then holds 2,971 windows, 24 a thread.  Window `lag` = 100 of a ctg
always belongs to thread 4 of the ctg's first tile (q = 4: tiles start on window 0 and the lag is baked), so what slides
with the ctg's length is the tile's LAST window: through every q of threads 4 and 5 for 100 .. 125 windows."""
import ctypes as C

import numpy as np
import pytest

from gams_amd import _lib, engine
from oracle import oracle as ora

pytestmark = pytest.mark.gpu

PLANE, BYTES, AUTO_IN = _lib.WAVE_INPUT_PLANE, _lib.WAVE_INPUT_BYTES, _lib.WAVE_INPUT_AUTO
WIDE, NARROW, AUTO = _lib.WAVE_BODY_WIDE, _lib.WAVE_BODY_NARROW, _lib.WAVE_BODY_AUTO
AUTO_RUNS = NARROW                    # what GAMS_WAVE_BODY_AUTO launches for a plane-fed headline pass
BOTH = _lib.WAVE_PEAKS | _lib.WAVE_DENSE
HEAD = (100, 10, 100, 3.0, 1.0)
TILE = 3072                           # gams_wave_plan_set_tile: W = 12 of 256 threads = W = 24 of 128
TW = 2971                             # windows of that tile
NAME = "wave_fast_kernel<12, 100, 10, 100, false, 256>"


def bases(n_win):
    """length of a ctg of n_win windows of 100 / 10"""
    return (n_win - 1) * 10 + 100


@pytest.fixture(scope="module")
def eng():
    e = engine.Engine(0)
    yield e
    e.close()


def mixed(lengths, seed):
    """ctgs of the given lengths, alternately random bytes 0..255 (lower-case g / c among them) and ACGTN text in both cases"""
    rng = np.random.default_rng(seed)
    text = np.frombuffer(b"ACGTNacgtn", np.uint8)
    out = []
    for k, n in enumerate(lengths):
        if k & 1:
            out.append(np.ascontiguousarray(text[rng.integers(0, 10, n)]))
        else:
            out.append(rng.integers(0, 256, n, dtype=np.uint8))
    return out


_ORACLE = {}


def oracle_of(seq, prm):
    key = (seq.tobytes(), prm)
    if key not in _ORACLE:
        ocnt, _, osig = ora.wave_windows(seq, *prm)
        _ORACLE[key] = (ocnt, osig)
    return _ORACLE[key]


def oracle_peaks(seqs, prm):
    exp = []
    for c, s in enumerate(seqs):
        ocnt, osig = oracle_of(s, prm)
        exp += [(c, int(i), int(ocnt[i]), int(osig[i])) for i in np.flatnonzero(osig != 0)]
    return exp


def records(pk):
    return [(int(r["ctg"]), int(r["window"]), int(r["gc_count"]), int(r["signal"])) for r in pk]


def headline_plan(eng, ss, prm=HEAD, flags=_lib.WAVE_PEAKS):
    plan = engine.WavePlan(eng, ss, *prm, flags=flags, tile_windows=TILE)
    assert plan.kernel_name() == NAME, plan.kernel_name()
    return plan


def three_ways(eng, seqs, prm=HEAD, all_exact=False, twin=True, fresh=False):
    """-> the oracle's peaks, after the wide body, the narrow body and the byte form have all produced exactly them.
    fresh: a new plan for every way, so that each way starts from the slots of a new plan (tw / 8 records a tile) and
    not from the ones an earlier way's reader has regrown."""
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
        for way, body, inp in (("wide", WIDE, PLANE), ("narrow", NARROW, PLANE), ("bytes", AUTO, BYTES)):
            if fresh and got:
                plan.close()
                plan = new_plan()
            plan.set_body(body)
            plan.set_input(inp)
            plan.run()
            assert plan.last_input() == inp, way
            assert plan.last_body() == (NARROW if way == "narrow" else WIDE), way
            got[way] = plan.peaks().copy()
            # (a reader that met an overflowing tile has regrown the slots and run the pass again: the same body)
            assert plan.last_input() == inp and plan.last_body() == (NARROW if way == "narrow" else WIDE), way
            exact[way] = plan.exact_count()
            assert plan.kernel_name() == NAME                  # the list entry, whichever body ran
        assert records(got["wide"]) == exp
        assert np.array_equal(got["narrow"], got["wide"]) and np.array_equal(got["bytes"], got["wide"])
        # the exact path: the same windows whatever is read and however the tile is cut (the narrow body takes its
        # bound on S1 per twelve windows, like the wide one)
        assert exact["bytes"] == exact["wide"] == exact["narrow"] <= decidable, exact
        if all_exact:
            assert exact["wide"] == exact["narrow"] == decidable, exact
        if fresh:
            plan.close()
            plan = new_plan()
        plan.set_body(AUTO)
        plan.set_input(AUTO_IN)
        plan.run()
        assert plan.last_input() == PLANE and plan.last_body() == AUTO_RUNS
        assert np.array_equal(plan.peaks(), got["wide"])
        assert plan.last_body() == AUTO_RUNS
        plan.close()
        if twin:                                               # dense rows: a plan of the wide kernel only
            dense = headline_plan(eng, ss, prm, flags=BOTH)
            dense.run()
            assert dense.last_body() == WIDE and dense.last_input() == PLANE
            for c, s in enumerate(seqs):
                ocnt, osig = oracle_of(s, prm)
                cnt, sig = dense.dense(c)
                assert np.array_equal(cnt, ocnt) and np.array_equal(sig.astype(np.int32), osig), c
            assert records(dense.peaks()) == exp
            dense.close()
    finally:
        ss.close()
    return exp


def test_last_thread_partial_run_and_tile_seams(eng):
    # one tile less a window, exactly one, one more (a second tile of a single window); two tiles -1 / 0 / +1
    wins = [TW - 1, TW, TW + 1, 2 * TW - 1, 2 * TW, 2 * TW + 1]
    exp = three_ways(eng, mixed([bases(n) for n in wins], 31))
    assert {c for c, *_ in exp} == set(range(6))               # every ctg has peaks to order


@pytest.mark.parametrize("seed", [41, 42, 43])
def test_ctg_start_tile_of_every_short_length(eng, seed):
    # vb < 0: the run-time phase 2 in 128 threads.  100 windows (window `lag` absent: nothing can signal) to 125: the
    # tile's last window at every q of thread 4 (windows 96 .. 119) and q = 0 .. 5 of thread 5.  The seeds shift the
    # bytes under the same geometry, and with them the ctgs' offsets in the buffer.
    wins = list(range(100, 126))
    seqs = mixed([bases(n) + (seed + k) % 10 for k, n in enumerate(wins)], seed)     # + ragged tails shorter than a step
    three_ways(eng, seqs)


def test_ctg_shorter_than_size_is_refused_and_lag_windows_never_signal(eng):
    for n in (60, 99, 100):                                    # no window at all / one window
        seqs = mixed([n, bases(400)], 44)
        ss = engine.SeqSet(eng, seqs)
        with pytest.raises(_lib.GamsError) as ei:
            engine.WavePlan(eng, ss, *HEAD, tile_windows=TILE)
        assert ei.value.code == _lib.ESHORT
        with pytest.raises(ValueError):
            ora.wave_windows(seqs[0], *HEAD)
        ss.close()
    # a ctg of exactly `lag` windows next to a normal one: its tile runs and leaves no record
    seqs = mixed([bases(100), bases(700)], 45)
    exp = three_ways(eng, seqs, prm=(100, 10, 100, 2.0, 1.0))
    assert exp and all(c == 1 for c, *_ in exp)


def test_constant_runs_across_tile_seams(eng):
    # a homopolymer run and an N run, each longer than (lag + 1) * step + size = 1,110 bases, across the seams at
    # windows 2,971 (base 29,710) and 5,942 (base 59,420): V == 0 and D == 0 there, settled by the const_sig table
    seq = np.frombuffer(b"ACGTacgtNn", np.uint8)[np.random.default_rng(46).integers(0, 10, 70000)].copy()
    seq[28400:31600] = ord("G")
    seq[58500:61000] = ord("N")
    seq[64000:65300] = ord("c")
    three_ways(eng, [seq, mixed([bases(TW + 5)], 47)[0]])


def test_every_window_through_the_exact_path(eng):
    # all_exact: exact_signal_wave for every decidable window, its owner found from the lane with W = 24
    three_ways(eng, mixed([20000], 48), all_exact=True, twin=False)


def test_threshold_minus_one_overflows_the_slots_and_reruns(eng):
    # every window from `lag` on signals.  A new plan gives a tile a slot of tw / 8 = 371 records; tile 0 holds 2,871
    # peaks and tile 1 all of its 1,020: both overflow, the kernel stores what fits and counts the rest, the first reader
    # regrows the slots and runs the pass again -- through the same body.  A plan per way: a plan keeps its regrown
    # slots, so on a shared plan only the first way would meet the overflow.
    prm = (100, 10, 100, -1.0, 1.0)
    seqs = mixed([40000], 49)
    exp = oracle_peaks(seqs, prm)
    assert len(exp) == (40000 - 100) // 10 + 1 - 100
    assert [w for _, w, *_ in exp] == list(range(100, 100 + len(exp)))
    cap = TW // 8
    assert sum(1 for _, w, *_ in exp if w < TW) == TW - 100 > cap and sum(1 for _, w, *_ in exp if w >= TW) == 1020 > cap
    assert three_ways(eng, seqs, prm=prm, fresh=True) == exp


def test_empty_batch_next_to_a_normal_one(eng):
    # a seqset without a ctg: its headline plan has no tile and a pass launches nothing -- whatever body or input is
    # asked for -- while a normal seqset's plan on the same engine runs its three ways between the empty passes
    empty = engine.SeqSet(eng, [])
    seqs = mixed([bases(TW + 40), 9000], 57)
    ep = engine.WavePlan(eng, empty, *HEAD, tile_windows=TILE)
    assert ep.total_windows == 0
    for body in (AUTO, NARROW, WIDE, NARROW):
        ep.set_body(body)
        ep.run()
        assert ep.last_body() == WIDE                          # no kernel ran, so not the narrow one
        assert ep.peaks().size == 0 and ep.peaks_count() == 0
        three_ways(eng, seqs, twin=body == AUTO)
    ep.run()
    assert ep.peaks().size == 0 and ep.last_body() == WIDE
    ep.close()
    empty.close()


@pytest.mark.parametrize("seed", [51, 52, 53])
def test_random_bytes_six_ctgs_of_mixed_lengths(eng, seed):
    rng = np.random.default_rng(seed)
    lens = [1090 + seed, 30011, 4097, bases(TW) + 3, 12345, 61007]
    seqs = [rng.integers(0, 256, n, dtype=np.uint8) for n in lens]
    three_ways(eng, seqs, twin=seed == 51)


def test_dense_and_influence_plans_keep_the_wide_kernel(eng):
    seqs = mixed([30000, 12000], 54)
    ss = engine.SeqSet(eng, seqs)
    for prm, flags in ((HEAD, BOTH), (HEAD, _lib.WAVE_DENSE), ((100, 10, 100, 3.0, 0.5), _lib.WAVE_PEAKS)):
        plan = engine.WavePlan(eng, ss, *prm, flags=flags, tile_windows=TILE)
        plan.run()
        assert plan.last_body() == WIDE and plan.last_input() == PLANE
        if flags & _lib.WAVE_PEAKS:
            assert records(plan.peaks()) == oracle_peaks(seqs, prm)
        plan.set_body(NARROW)
        with pytest.raises(_lib.GamsError) as ei:
            plan.run()
        assert ei.value.code == _lib.ESTATE
        plan.set_body(WIDE)
        plan.run()
        assert plan.last_body() == WIDE
        plan.close()
    # other entries of the list, a thread-count request and the tapered table have no narrow body either
    for tile, threads in ((2048, 0), (1024, 0), (TILE, 128)):
        plan = engine.WavePlan(eng, ss, *HEAD, tile_windows=tile)
        if threads:
            plan.set_threads(threads)
        plan.set_body(NARROW)
        with pytest.raises(_lib.GamsError) as ei:
            plan.run()
        assert ei.value.code == _lib.ESTATE
        plan.set_body(AUTO)
        plan.run()
        assert plan.last_body() == WIDE and records(plan.peaks()) == oracle_peaks(seqs, HEAD)
        plan.close()
    ss.close()


def test_stale_plane_reads_bytes_through_the_wide_kernel(eng):
    seqs = mixed([20000, 30001, 11000], 55)
    ss = engine.SeqSet(eng, seqs)
    plan = headline_plan(eng, ss)
    plan.run()
    assert (plan.last_input(), plan.last_body()) == (PLANE, AUTO_RUNS)
    assert records(plan.peaks()) == oracle_peaks(seqs, HEAD)
    # a range of bytes without its plane: the plane is stale, the pass reads the bytes -- the wide kernel holds that body
    seqs[2] = mixed([11000], 56)[0]
    off, nb = ss.layout()
    img = np.zeros(nb, np.uint8)
    for o, s in zip(off, seqs):
        img[int(o):int(o) + s.size] = s
    ss.upload_image(img, int(off[2]), int(off[2]) + seqs[2].size)
    plan.run()
    assert (plan.last_input(), plan.last_body()) == (BYTES, WIDE)
    assert records(plan.peaks()) == oracle_peaks(seqs, HEAD)
    plan.set_body(NARROW)
    with pytest.raises(_lib.GamsError) as ei:
        plan.run()
    assert ei.value.code == _lib.ESTATE
    plan.set_body(AUTO)
    # everything again with its plane (gams_seqset_upload_all): plane-fed and narrow again
    arrs = [np.ascontiguousarray(s) for s in seqs]
    ptrs = (C.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
    eng.check(eng.lib.gams_seqset_upload_all(eng.h, ss.p, ptrs))
    plan.run()
    assert (plan.last_input(), plan.last_body()) == (PLANE, AUTO_RUNS)
    assert records(plan.peaks()) == oracle_peaks(seqs, HEAD)
    plan.set_body(NARROW)
    plan.run()
    assert plan.last_body() == NARROW and records(plan.peaks()) == oracle_peaks(seqs, HEAD)
    eng.sync()
    plan.close()
    ss.close()


def test_three_plans_on_three_lanes(eng):
    # the benchmark's timed region in small: a plan per seqset on lanes 0, 1, 2, the taper off, passes in flight
    batches = [mixed([bases(2 * TW + 7), 15000 + 100 * j, bases(TW)], 60 + j) for j in range(3)]
    sets = [engine.SeqSet(eng, b) for b in batches]
    plans = []
    for j, ss in enumerate(sets):
        p = headline_plan(eng, ss)
        p.set_lane(j)
        p.set_taper(0)
        assert p.kernel_name() == NAME
        plans.append(p)
    for i in range(12):
        plans[i % 3].run()
    eng.sync()
    for p, b in zip(plans, batches):
        assert (p.last_input(), p.last_body()) == (PLANE, AUTO_RUNS)
        assert records(p.peaks()) == oracle_peaks(b, HEAD)
        p.set_body(NARROW)
    for i in range(12):
        plans[i % 3].run()
    eng.sync()
    for p, b in zip(plans, batches):
        assert p.last_body() == NARROW and records(p.peaks()) == oracle_peaks(b, HEAD)
        p.close()
    for ss in sets:
        ss.close()
