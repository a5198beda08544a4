"""What a wave plan does with its pooled buffers over its life: every block a plan, its ways, its rows and its signal text
took is back in the handle's pools once the plan is closed -- once, and asked for with the sizes and in the order that let
the pools serve them from the same blocks.  gams_gpu_release_cached empties the pools and reports the bytes they held, so
a leaked block shows as fewer bytes than expected, a block returned twice as more (or as a crash), and a request of
another size or in another order as another count of 2-MiB pool granules.

Each scenario: empty the pools; the plan's calls, their results against the oracle (oracle/oracle.py, the row models of
tests/text_edges.py); close the plan; the held bytes, read before the seqset is closed (its two blocks stay out).  A pool
keeps at most 16 blocks, so a reading tells something only while a scenario's blocks number at most 15 per pool: the
count of each scenario, from the code, stands beside its literal.

One seqset for all: three ctgs of 40,000, 2,500 and 200 random bases; size 100, step 10, lag 10 give 3,991, 241 and 11
windows (the last ctg holds exactly lag + 1) in 4 + 1 + 1 tiles of 1,013 windows.

The HELD literals were recorded by running this file against the build of the commit BEFORE the plan's buffers moved to
one owning type and the readers' shared steps were folded (each buffer released by hand), never from the code under
test."""
import ctypes as C

import numpy as np
import pytest

import text_edges as te
from gams_amd import _lib, engine
from oracle import oracle as ora
from test_gpu_text_edges import assert_peaks, assert_text

pytestmark = pytest.mark.gpu

L = _lib.load()
MIB = 1 << 20
SIZE, STEP, LAG = 100, 10, 10
LENGTHS = (40_000, 2_500, 200)
NAMES, STARTS = ("I", "II", "III"), (1, 5_001, 99_990)
LONG_NAMES = (te.LONG_100, te.LONG_A, te.LONG_B)       # 194 bytes: beyond the name table the short names sized (128)

# held bytes after plan.close(), from the parent commit's build; (device blocks, page-locked blocks) a scenario takes
HELD = {
    "peaks": 12 * MIB,             # (5, 1): fixed, geom, slots, counters, dense; h_peaks
    "rows_rerun": 28 * MIB,        # (8, 3): + rows arena, rows tables, text; h_words, h_text, h_peaks
    "depth2_regrow": 16 * MIB,     # (7, 1): fixed, geom, dense, slots and counters per way; h_peaks
    "signal_text": 18 * MIB,       # (7, 2): fixed, geom, counters, dense_cnt, dense_sig, sig arena, text; h_words, h_text
    "repair_depth2": 34 * MIB,     # (14, 3): fixed, geom, jtiles, dense, slots / counters / dense_cnt / dense_sig / jac per
                                   #          way; h_ctl per way, h_peaks
    "depth3_tile": 20 * MIB,       # (9, 1): fixed, geom, dense, slots and counters per way; h_peaks
    "refused_create": 0,
}


@pytest.fixture(scope="module")
def eng():
    e = engine.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def seqs():
    rng = np.random.default_rng(20261019)
    return [np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].copy() for n in LENGTHS]


@pytest.fixture(scope="module")
def seqset(eng, seqs):
    ss = engine.SeqSet(eng, seqs)
    yield ss
    ss.close()


@pytest.fixture(scope="module")
def oracle_peaks(seqs):
    """(threshold, influence) -> the packed peak records of a pass, computed once"""
    cache = {}

    def get(thr, infl=1.0):
        if (thr, infl) not in cache:
            per = []
            for q in seqs:
                cnt, _, sig = ora.wave_windows(q, SIZE, STEP, LAG, thr, infl)
                per.append((cnt, sig))
            cache[(thr, infl)] = te.pack_peaks(per)
        return cache[(thr, infl)]

    return get


def held(eng):
    v = C.c_uint64()
    eng.check(L.gams_gpu_release_cached(eng.h, C.byref(v)))
    return v.value


def check_held(eng, name):
    got = held(eng)
    print(f"HELD {name}: {got} bytes = {got / MIB} MiB")
    assert got == HELD[name], (name, got)


def ctgs_of(seqs, names=NAMES):
    return [te.ctg(nm, st, q) for nm, st, q in zip(names, STARTS, seqs)]


def test_windows_of_the_fixture(eng, seqset):
    held(eng)
    plan = engine.WavePlan(eng, seqset, SIZE, STEP, LAG, 3.0, 1.0, flags=_lib.WAVE_PEAKS)
    assert [plan.ctg_windows(c) for c in range(3)] == [3991, 241, LAG + 1]
    plan.close()


def test_peaks_plan(eng, seqset, oracle_peaks):
    """(a) run, peaks(), close"""
    held(eng)
    plan = engine.WavePlan(eng, seqset, SIZE, STEP, LAG, 3.0, 1.0, flags=_lib.WAVE_PEAKS)
    plan.run()
    exp = oracle_peaks(3.0)
    assert exp.size > 0
    assert_peaks(plan, exp, "peaks")
    plan.close()
    check_held(eng, "peaks")


def test_rows_end_reruns_the_pass_into_larger_slots(eng, seqs, seqset, oracle_peaks):
    """(b) threshold -1: every tile overflows its slot of tw / 8 records, and gams_wave_rows_end is the first reader: it
    regrows the slots, runs the pass again and queues the rows once more.  peaks() afterwards does not regrow again."""
    held(eng)
    exp = oracle_peaks(-1.0)
    assert exp.size > sum(n - LAG for n in (3991, 241, 11)) - 50       # (nearly) every window from `lag` on
    rows = te.wave_rows_model(ctgs_of(seqs), exp, SIZE, STEP)[0]
    plan = engine.WavePlan(eng, seqset, SIZE, STEP, LAG, -1.0, 1.0, flags=_lib.WAVE_PEAKS)
    plan.rows_setup(NAMES, STARTS, 0.2)
    plan.run()
    plan.rows_begin()
    text, off = plan.rows_end()
    assert_text(text, off, rows, "rows after the rerun")
    assert_peaks(plan, exp, "peaks after the rerun")
    plan.select(0)
    assert_peaks(plan, exp, "peaks after select(0)")
    plan.run()
    plan.rows_begin()
    text2, off2 = plan.rows_end()
    assert text2 == text and off2.tolist() == off.tolist()
    plan.close()
    check_held(eng, "rows_rerun")


def test_depth2_peaks_reruns_both_held_passes(eng, seqset, oracle_peaks):
    """(c) depth 2, two runs, the older one selected: peaks() meets the overflow, both held passes run again into larger
    slots, the selection and the way rotation stay.  (test_gpu_wave.py's test_overflowing_tile_regrows_to_the_fullest_tile
    counts the records of such a plan; here every record is the oracle's and the held bytes are read.)"""
    held(eng)
    exp = oracle_peaks(-1.0)
    plan = engine.WavePlan(eng, seqset, SIZE, STEP, LAG, -1.0, 1.0, flags=_lib.WAVE_PEAKS)
    plan.set_depth(2)
    plan.run()
    plan.run()
    plan.select(1)
    assert_peaks(plan, exp, "age 1")
    plan.select(0)
    assert_peaks(plan, exp, "age 0")
    plan.select(1)
    assert_peaks(plan, exp, "age 1 again")
    plan.close()
    check_held(eng, "depth2_regrow")


def test_signal_text_twice_with_a_new_name_table(eng, seqs, seqset):
    """(d) DENSE plan: signal_text with short names, then with names beyond the name table the first call sized"""
    held(eng)
    kw = dict(size=SIZE, step=STEP, lag=LAG, threshold=3.0, influence=1.0)
    plan = engine.WavePlan(eng, seqset, SIZE, STEP, LAG, 3.0, 1.0, flags=_lib.WAVE_DENSE)
    plan.run()
    assert sum(len(x) for x in LONG_NAMES) > 2 * 64
    for names in (NAMES, LONG_NAMES):
        text, off = plan.signal_text(names, STARTS)
        exp = [ora.wave_proc_ctg(c["chr_id"], c["chr_start"], c["chr_end"], c["seq"], is_signal=True, **kw).encode()
               for c in ctgs_of(seqs, names)]
        assert_text(text, off, exp, ("signal", names[0]))
    plan.close()
    check_held(eng, "signal_text")


def test_repair_plan_at_depth2(eng, seqset, oracle_peaks):
    """(e) influence 0.5 (guess-and-iterate), PEAKS | DENSE, depth 2: 14 device blocks"""
    held(eng)
    exp = oracle_peaks(3.0, 0.5)
    assert exp.size > 0
    plan = engine.WavePlan(eng, seqset, SIZE, STEP, LAG, 3.0, 0.5, flags=_lib.WAVE_PEAKS | _lib.WAVE_DENSE)
    plan.set_depth(2)
    plan.run()
    plan.run()
    assert_peaks(plan, exp, "repair")
    plan.close()
    check_held(eng, "repair_depth2")


def test_depth_then_tile_replace_the_geometry_twice(eng, seqset, oracle_peaks):
    """(f) set_depth(3), then set_tile(2048): the geometry arena and the per-way slots are replaced twice on the way"""
    held(eng)
    exp = oracle_peaks(3.0)
    plan = engine.WavePlan(eng, seqset, SIZE, STEP, LAG, 3.0, 1.0, flags=_lib.WAVE_PEAKS)
    plan.set_depth(3)
    plan.set_tile(2048)
    plan.run()
    assert_peaks(plan, exp, "depth 3, tile 2048")
    plan.close()
    check_held(eng, "depth3_tile")


def test_refused_create_holds_nothing(eng, seqset, oracle_peaks):
    """(g) lag 12 over a ctg of 11 windows: GAMS_ESHORT before anything is allocated, and the handle keeps working"""
    held(eng)
    prm = _lib.WaveParams(SIZE, STEP, LAG + 2, 3.0, 1.0)
    p = C.c_void_p()
    rc = L.gams_wave_plan_create(eng.h, seqset.p, C.byref(prm), _lib.WAVE_PEAKS, C.byref(p))
    assert rc == _lib.ESHORT and not p.value, rc
    assert b"windows < lag" in L.gams_gpu_last_error(eng.h)
    check_held(eng, "refused_create")
    plan = engine.WavePlan(eng, seqset, SIZE, STEP, LAG, 3.0, 1.0, flags=_lib.WAVE_PEAKS)
    plan.run()
    assert_peaks(plan, oracle_peaks(3.0), "after the refusal")
    plan.close()
