"""wave_fast_taper_kernel: the kernel every default wave pass runs on a batch of at least a round and a half of W = 12
tiles (12 * cus * 2,971 windows: 91 Mb at 256 CUs), held at its table, tail and slot edges.

The three tile bodies of that kernel are the device function of the plain kernels, inlined three times into one kernel
of its own launch bounds: a slip of that instantiation shows at no small shape.  So this module runs the smallest world
that reaches it (tests/taper.py: built for the device's own CU count, generated, one upload per module) -- tails whose
first ctgs sit exactly on the two boundaries of the table, ctgs of `lag` and `lag` + 1 windows, either side of every
tile size, last tiles of one window, ragged ends, random bytes and text, runs across tile seams -- and compares with the
CPU oracle over every ctg, record for record: the plane and the byte bodies, the dense phase, every tail shape of
gams_wave_plan_set_taper_shape, slots at their cap and their regrow, the device rows and the host operator, passes in
flight.  gams_wave_plan_tiles is held against the model of tests/taper.py throughout (the model against the library's
arithmetic on the CPU: test_wave_taper_cpu.py).

On 256 CUs the world is T = 9,131,912 windows (91.3 MB, 252 ctgs) in 3,797 tiles: 2,418 / 854 / 525 of W = 12 / 8 / 4."""
import types

import numpy as np
import pytest

import taper
from gams_amd import _lib, engine, host

pytestmark = pytest.mark.gpu

PLANE, BYTES = _lib.WAVE_INPUT_PLANE, _lib.WAVE_INPUT_BYTES
BOTH = _lib.WAVE_PEAKS | _lib.WAVE_DENSE
SLOT = 371                            # records of a new plan's slot: 2,971 / 8, sized from the W = 12 tile


@pytest.fixture(scope="module")
def eng():
    e = engine.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def world(eng):
    cus = eng.device_info()[1]
    lay = taper.layout(cus)
    seqs = taper.sequences(lay)
    ss = engine.SeqSet(eng, seqs)
    nt = "true" if ss.layout()[1] > (64 << 20) else "false"
    w = types.SimpleNamespace(cus=cus, lay=lay, seqs=seqs, ss=ss, table=taper.table(lay.counts, cus),
                              name=f"wave_fast_taper_kernel<100, 10, 100, {nt}>",
                              plain=f"wave_fast_kernel<12, 100, 10, 100, {nt}, 256>")
    yield w
    ss.close()


@pytest.fixture(scope="module")
def oracle3(world):
    dense = taper.oracle(world.seqs, 3.0)
    return dense, taper.peak_records(dense, _lib.PEAK_DTYPE)


@pytest.fixture(scope="module")
def oracle1(world):
    dense = taper.oracle(world.seqs, 1.0)
    return dense, taper.peak_records(dense, _lib.PEAK_DTYPE)


def new_plan(eng, world, thr=3.0, flags=_lib.WAVE_PEAKS):
    plan = engine.WavePlan(eng, world.ss, taper.SIZE, taper.STEP, taper.LAG, thr, 1.0, flags=flags)
    assert plan.kernel_name() == world.name, plan.kernel_name()
    return plan


def same(got, exp):
    """record arrays equal; the first difference named when they are not"""
    if got.size != exp.size:
        return f"{got.size} records, expected {exp.size}"
    bad = np.flatnonzero(got != exp)
    return f"{bad.size} records differ, the first: {got[bad[0]]} expected {exp[bad[0]]}" if bad.size else ""


def test_table_and_name(eng, world):
    """gams_wave_plan_tiles == the model for the default shape; the ctgs built on the two boundaries are W = 4 and
    W = 8, the 100-window ctg in front W = 12; the kernel's name, NT exactly when the seqset exceeds 64 MiB"""
    lay = world.lay
    plan = new_plan(eng, world)
    assert plan.total_windows == lay.T
    assert [plan.ctg_windows(i) for i in (0, lay.front, lay.w8[0], lay.big8, lay.w4[0], lay.big4, lay.counts.size - 1)] == \
        [int(lay.counts[i]) for i in (0, lay.front, lay.w8[0], lay.big8, lay.w4[0], lay.big4, lay.counts.size - 1)]
    tiles = plan.tiles()
    assert tiles.dtype == np.uint32 and tiles.shape == world.table.shape
    assert np.array_equal(tiles, world.table)
    w_of = dict(zip(tiles[:, 0].tolist(), tiles[:, 2].tolist()))
    assert w_of[lay.w4[0]] == 4 and w_of[lay.w4[0] - 1] == 8
    assert w_of[lay.w8[0]] == 8 and w_of[lay.front] == 12 and lay.front == lay.w8[0] - 1
    per_w = {w: int(np.count_nonzero(tiles[:, 2] == w)) for w in (12, 8, 4)}
    print(f"taper world: cus {world.cus}, T {lay.T}, x4 {lay.x4}, y8 {lay.y8}, {tiles.shape[0]} tiles, W = 12 / 8 / 4: {per_w}")
    assert all(per_w.values())
    assert ("true" in world.name) == (world.ss.layout()[1] > (64 << 20))
    plan.close()


def test_peaks_from_the_plane_and_from_the_bytes(eng, world, oracle3):
    """both inputs of the tapered kernel give the oracle's records, and so does the plain kernel on the same plan"""
    exp = oracle3[1]
    assert 0.001 * world.lay.T < exp.size < 0.05 * world.lay.T
    plan = new_plan(eng, world)
    exact = {}
    for inp in (PLANE, BYTES):
        plan.set_input(inp)
        plan.run()
        assert plan.last_input() == inp
        assert plan.kernel_name() == world.name
        assert not same(plan.peaks(), exp), inp
        exact[inp] = plan.exact_count()
    assert exact[PLANE] == exact[BYTES] > 0
    plan.set_taper(0)
    assert plan.kernel_name() == world.plain
    assert np.array_equal(plan.tiles(), taper.table(world.lay.counts, world.cus, taper=False))
    for inp in (PLANE, BYTES):
        plan.set_input(inp)
        plan.run()
        assert plan.last_input() == inp
        assert not same(plan.peaks(), exp), inp
    plan.close()


@pytest.mark.parametrize("shape", taper.SHAPES)
def test_every_tail_shape(eng, world, oracle3, shape):
    """gams_wave_plan_set_taper_shape: no tails at all, one tail only, both at the 8 % / 17 % caps, a handful of tiles"""
    plan = new_plan(eng, world)
    first = plan.tiles()
    plan.set_taper_shape(*shape)
    tiles = plan.tiles()
    assert np.array_equal(tiles, taper.table(world.lay.counts, world.cus, *shape))
    x4, y8 = taper.tails(world.lay.T, world.cus, *shape)
    assert (x4 == 0) == (shape[0] == 0) and (y8 == 0) == (shape[1] == 0)
    if shape == (100, 100):
        assert (x4, y8) == (world.lay.T * 8 // 100, world.lay.T * 17 // 100)
    # (the world ends in its shortest ctgs: even 1 % of a round holds some in either tail)
    assert set(np.unique(tiles[:, 2]).tolist()) == {12} | ({4} if shape[0] else set()) | ({8} if shape[1] else set())
    assert plan.kernel_name() == world.name
    plan.run()
    assert not same(plan.peaks(), oracle3[1])
    plan.set_taper_shape(taper.PCT4, taper.PCT8)
    assert np.array_equal(plan.tiles(), first) and np.array_equal(first, world.table)
    plan.close()


def test_tail_shape_refuses_what_is_no_percentage(eng, world):
    plan = new_plan(eng, world)
    for bad in ((-1, 50), (25, -1), (101, 50), (25, 101)):
        with pytest.raises(_lib.GamsError) as ei:
            plan.set_taper_shape(*bad)
        assert ei.value.code == _lib.EINVAL
    assert np.array_equal(plan.tiles(), world.table)
    plan.close()


@pytest.mark.parametrize("inp", [PLANE, BYTES])
def test_dense_rows(eng, world, oracle3, inp):
    """the dense phase of the three bodies: WAVE_DENSE does not switch the taper off.  Counts and signals of every ctg
    of the two tails, of the 100-window ctg in front of them, of the last three ctgs of the body and of every 20th one"""
    dense, exp = oracle3
    lay = world.lay
    plan = new_plan(eng, world, flags=BOTH)
    assert np.array_equal(plan.tiles(), world.table)
    plan.set_input(inp)
    plan.run()
    assert plan.last_input() == inp and plan.kernel_name() == world.name
    picked = list(lay.w8) + list(lay.w4) + [lay.front] + list(lay.body)[-3:] + list(lay.body)[::20]
    for i in picked:
        cnt, sig = plan.dense(i)
        assert np.array_equal(cnt, dense[i][0]), i
        assert np.array_equal(sig, dense[i][1]), i
    assert not same(plan.peaks(), exp)
    plan.close()


def test_slots_at_their_cap(eng, world, oracle1):
    """Threshold 1.0: about a third of the windows signal.  Every tile of a new plan has a slot of 371 records, sized
    from the W = 12 tile: most W = 4 tiles (923 windows) fit, every whole W = 8 and W = 12 tile of uniform ACGT
    overflows, and the first reader regrows the slots and runs the pass again.  The oracle says which tiles sit where
    (printed; on 256 CUs, whole tiles of ordinary ctgs: 255..391 of a W = 4 tile's windows signal, 389 such tiles stay
    below 371 records, 2 hold exactly 371, 2 hold 372; W = 8 tiles 608..798, W = 12 tiles 966..1,195)."""
    dense, exp = oracle1
    lay = world.lay
    per_tile = taper.tile_signal_counts(dense, world.table)
    w = world.table[:, 2]
    ordinary = np.ones(lay.counts.size, bool)              # uniform ACGT: the body and what lies behind a tail's big ctg
    ordinary[[lay.front] + taper.mixed(lay, lay.w8) + taper.mixed(lay, lay.w4)] = False
    full = world.table[:, 1] + np.where(w == 4, 923, np.where(w == 8, 1947, 2971)) <= lay.counts[world.table[:, 0]]
    full &= ordinary[world.table[:, 0]]
    for wk in (4, 8, 12):
        c = per_tile[(w == wk) & full]
        print(f"threshold 1.0, whole W = {wk} tiles: {c.size}, windows that signal {c.min()}..{c.max()}, "
              f"below / at / above the slot of {SLOT}: {np.count_nonzero(c < SLOT)} / {np.count_nonzero(c == SLOT)} / "
              f"{np.count_nonzero(c > SLOT)}; exactly 372: {np.count_nonzero(c == SLOT + 1)}")
    assert np.any(per_tile[w == 4] < SLOT) and np.any(per_tile[w == 8] > SLOT) and np.any(per_tile[w == 12] > SLOT)
    assert np.all(per_tile[(w == 8) & full] > SLOT) and np.all(per_tile[(w == 12) & full] > SLOT)
    assert exp.size == int(per_tile.sum()) > world.lay.T // 4
    plan = new_plan(eng, world, thr=1.0)
    plan.run()
    assert not same(plan.peaks(), exp)                 # after the regrow
    assert np.array_equal(plan.tiles(), world.table)
    plan.run()                                          # the regrown plan
    assert not same(plan.peaks(), exp)
    assert plan.peaks_count() == exp.size
    assert np.array_equal(plan.tiles(), world.table)
    plan.close()


def rows_text(ctgs, peaks, size, step, coverage):
    """the TSV rows of peak records, per ctg: the host layer's merge and formatting, as the device-rows tests of
    test_gpu_host.py form them"""
    gc = [host.fmt_f32(np.float32(k) / np.float32(size)) for k in range(size + 1)]
    first = np.searchsorted(peaks["ctg"], np.arange(len(ctgs) + 1))
    out = []
    for c, ctg in enumerate(ctgs):
        mine = peaks[first[c]:first[c + 1]]
        cmin, cmax = np.zeros(mine.size, np.int64), np.zeros(mine.size, np.int64)
        merged = np.zeros(mine.size, bool)
        for sgn in (1, -1):
            sel = np.flatnonzero(mine["signal"] == sgn)
            if sel.size:
                cmin[sel], cmax[sel], merged[sel] = host.merge_windows(mine["window"][sel], ctg["chr_start"], size, step, coverage)
        rows = []
        for i in range(mine.size):
            s = ctg["chr_start"] + int(mine["window"][i]) * step
            if merged[i]:
                if s == cmin[i]:
                    rows.append(f"{ctg['chr_id']}(+):{cmin[i]}-{cmax[i]}\t{gc[mine['gc_count'][i]]}\t{int(mine['signal'][i])}\n")
            else:
                rows.append(f"{ctg['chr_id']}:{s}-{s + size - 1}\t{gc[mine['gc_count'][i]]}\t{int(mine['signal'][i])}\n")
        out.append("".join(rows))
    return out


def test_device_rows_and_the_operator(eng, world, oracle3):
    """gams_wave_rows_* on a tapered table: the text and the ctg offsets of the tapered and of the plain launch, the
    text formed from the oracle's peaks, and host.wave over the same ctgs (its plan is tapered by default)"""
    ctgs = taper.ctg_dicts(world.seqs)
    per_ctg = rows_text(ctgs, oracle3[1], taper.SIZE, taper.STEP, 0.2)
    exp = "".join(per_ctg).encode()
    exp_off = np.concatenate([[0], np.cumsum([len(t) for t in per_ctg])]).astype(np.uint64)
    assert sum(1 for t in per_ctg if not t) >= 2           # the ctgs of `lag` windows have no row
    plan = new_plan(eng, world)
    plan.rows_setup([c["chr_id"] for c in ctgs], [c["chr_start"] for c in ctgs], 0.2)
    got = {}
    for mode in (1, 0):
        plan.set_taper(mode)
        assert plan.kernel_name() == (world.name if mode else world.plain)
        for rep in range(2):                                # (the second pass copies the text speculatively)
            plan.run()
            plan.rows_begin()
            text, off = plan.rows_end()
            got[mode, rep] = (bytes(text), off.copy())
    plan.close()
    for key, (text, off) in got.items():
        assert np.array_equal(off, exp_off), key
        assert text == exp, key
    assert host.wave(eng, ctgs).encode() == exp


def test_passes_in_flight(eng, world, oracle3):
    """a tapered table with three passes in flight: every held pass; back at depth 1 the table is the model's again"""
    plan = new_plan(eng, world)
    plan.set_taper(1)
    plan.set_depth(3)
    assert plan.kernel_name() == world.name and np.array_equal(plan.tiles(), world.table)
    plan.run_n(7)
    for age in range(3):
        plan.select(age)
        assert not same(plan.peaks(), oracle3[1]), age
    plan.set_taper(-1)
    assert plan.kernel_name() == world.plain               # depth 3: the library's own choice is no taper
    plan.set_depth(1)
    assert plan.kernel_name() == world.name and np.array_equal(plan.tiles(), world.table)
    plan.run()
    assert not same(plan.peaks(), oracle3[1])
    plan.close()
