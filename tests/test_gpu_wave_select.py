"""Every kernel pointer of wave.hip's instance table launched once, through the recipes of wave_instances.py: the NT =
false half on a small ragged seqset, the NT = true half on a seqset just over 64 MiB (that threshold itself).  The name
is asserted, one pass is run and compared with the CPU oracle.  (wave_fast_taper_kernel needs at least
12 * cus * 2,971 windows: test_gpu_wave_taper.py holds it, over the world of tests/taper.py.)"""
import numpy as np
import pytest

from helpers import synth
from gams_amd import _lib, engine
from oracle import oracle as ora
from wave_instances import INSTANCES

pytestmark = pytest.mark.gpu

THR = 3.0
_oracle = {}


def oracle(tag, seq, inst):
    """computed once per (ctg, parameters), shared by the recipes that have them in common"""
    key = (tag, inst.size, inst.step, inst.lag)
    if key not in _oracle:
        ocnt, _, osig = ora.wave_windows(seq, inst.size, inst.step, inst.lag, THR, 1.0)
        _oracle[key] = (ocnt, osig)
    return _oracle[key]


@pytest.fixture(scope="module")
def eng():
    e = engine.Engine(0)
    yield e
    e.close()


def make_plan(eng, ss, inst, flags):
    plan = engine.WavePlan(eng, ss, inst.size, inst.step, inst.lag, THR, 1.0, flags=flags, tile_windows=inst.tile_windows)
    plan.set_threads(inst.threads)
    return plan


def check_peaks(pk, c, osig, what):
    mine = pk[pk["ctg"] == c]
    idx = np.flatnonzero(osig)
    assert np.array_equal(mine["window"], idx) and np.array_equal(mine["signal"], osig[idx]), what


def test_every_instance_on_a_small_seqset(eng, s288c):
    # the pool of test_size_and_step_baked_lag_as_argument: four ragged ctgs of at most 120 kb
    pool = [bytes(s288c["I"][:120_000]), synth(41_234, 5).tobytes(), bytes(s288c["Mito"][:9_000]), synth(3_777, 6).tobytes()]
    sets = {}
    for inst in INSTANCES:
        # (a ctg with fewer windows than the lag is refused like the reference's panic, stat.rs:30)
        keep = tuple(i for i, sq in enumerate(pool) if (len(sq) - inst.size) // inst.step + 1 >= inst.lag)
        assert keep
        if keep not in sets:
            sets[keep] = engine.SeqSet(eng, [pool[i] for i in keep])
        plan = make_plan(eng, sets[keep], inst, _lib.WAVE_PEAKS | _lib.WAVE_DENSE)
        assert plan.kernel_name() == inst.kernel
        plan.run()
        pk = plan.peaks()
        for c, i in enumerate(keep):
            ocnt, osig = oracle(i, pool[i], inst)
            cnt, sig = plan.dense(c)
            assert np.array_equal(cnt, ocnt) and np.array_equal(sig.astype(np.int32), osig), (inst, c)
            check_peaks(pk, c, osig, (inst, c))
        plan.close()
    for ss in sets.values():
        ss.close()


def test_every_instance_with_streaming_loads(eng, s288c):
    checked = bytes(s288c["I"][:100_000])
    filler = np.tile(synth(1 << 20, 11), 64)                  # 64 MiB: with the checked ctg the seqset is just over
    ss = engine.SeqSet(eng, [checked, filler])
    assert ss.layout()[1] > 64 << 20
    for inst in INSTANCES:
        plan = make_plan(eng, ss, inst, _lib.WAVE_PEAKS)
        assert plan.kernel_name() == inst.kernel.replace("false", "true")
        plan.run()
        check_peaks(plan.peaks(), 0, oracle("checked", checked, inst)[1], inst)
        plan.close()
    ss.close()
