"""The knife-edge and saturated inputs of tests/knife.py prove themselves on the CPU oracle alone: the GPU tests that
use them (test_gpu_wave_knife.py) mean something only if these hold.

- On every knife configuration the oracle's f32 verdict differs from the verdict of real arithmetic (float64
  D > thr * sqrt(n V / (n - 1)), which is what the integer decision of the wave kernels computes) on at least 1,000
  window-decisions over the 66 passes.  Each of those is a window the guard band must hand to the exact path.
  With the committed seeds (window-decisions that differ, in 66 passes; largest S1 / (lag * size)):
      100, 10, 100   14,501  0.90      100, 1, 100     4,761  0.60      100, 5, 200    11,049  0.93
      255, 10, 257   16,427  0.985     50, 7, 33      10,319  0.81      255, 10, 258   17,586  0.985
      300, 10, 218   11,615  0.95      300, 10, 250    8,627  0.95      1000, 50, 30   13,717  0.90
      1000, 500, 100 12,859  0.90
- The saturated inputs reach the sums they are there for.
- Every threshold lies in [1e-6, 1e6]: outside it the plan sends every window down the exact path and a pass would
  prove nothing about the band."""
import numpy as np
import pytest

import helpers
import knife

FLOOR = 1000


def test_helpers_model_the_oracle_away_from_the_edge():
    """lag_sums / real_signals are the oracle's decision wherever the threshold is not within 1e-3 of a window's z"""
    seq = helpers.synth(20000, 3)
    c = knife.Case(100, 10, 100, [seq])
    i, s1, s2, dn, v = helpers.lag_sums(c.cnt[0], 100)
    k = c.cnt[0].astype(np.int64)
    assert s1[0] == k[:100].sum() and s1[1] == k[:100].sum() and s1[2] == k[1:101].sum()       # windows 100, 101, 102
    assert s2[5] == (k[4:104] ** 2).sum() and dn[5] == 100 * k[105] - s1[5] and v[5] == 100 * s2[5] - s1[5] ** 2
    z = np.full(k.size, np.inf)
    z[i] = np.abs(dn) / np.sqrt(100 * v / 99.0)
    for thr in (1.0, 2.0, 3.0):
        far = np.abs(z / thr - 1.0) > 1e-3
        assert far.sum() > 0.99 * k.size
        assert np.array_equal(c.oracle(thr)[0][far], helpers.real_signals(k, 100, thr)[far])
    states = helpers.tie_states(k, 100)
    assert sum(w.size for _, w in states) == np.count_nonzero(np.isfinite(z) & (z > 0))
    assert all(np.allclose(z[w], zv, rtol=0, atol=0) for zv, w in states[:20])


def test_periodic_keeps_the_counts_periodic():
    unit = helpers.gc_unit(130, 0.5, 1)
    assert unit.sum() == 65
    s = helpers.periodic(5000, unit, letters=4)
    assert set(s.tobytes()) <= set(b"GCgcATatN") and len(set(s.tobytes())) == 9
    assert np.array_equal(np.isin(s, np.frombuffer(b"GCgc", np.uint8)), np.tile(unit, 39)[:5000])
    cnt = knife.Case(100, 10, 20, [s]).cnt[0]
    assert np.array_equal(cnt[13:], cnt[:-13])                       # 130 bases = 13 windows of step 10
    assert [len(t) for t in ([helpers.knife_thresholds(1.25)])] == [11]
    assert helpers.knife_thresholds(1.25)[0] == 1.25 and len(set(helpers.knife_thresholds(1.25))) == 11


@pytest.mark.parametrize("prm", list(knife.KNIFE))
def test_oracle_and_real_arithmetic_disagree_on_the_knife_inputs(prm):
    c = knife.knife_case(*prm)
    thr = c.thresholds()
    assert len(thr) == 66 and len(set(thr)) >= 60           # (1 + 1e-7 is one or two f32 steps: a pair may coincide)
    assert all(1e-6 <= t <= 1e6 for t in thr), (min(thr), max(thr))
    assert all(k.size - c.lag >= knife.WINDOWS for k in c.cnt) and 2 <= len(c.seqs) <= 3
    per = [c.disagreements(t) for t in thr]
    print(prm, "window-decisions where the oracle is not real arithmetic:", sum(per), "largest pass:", max(per),
          "S1 / (lag * size): %.3f" % (c.sums()[0] / (c.lag * c.size)))
    assert sum(per) >= FLOOR, (prm, sum(per))


def test_phase_decides_within_one_state():
    """windows of one state (k, S1, S2) differ in the order of their lag terms, and for some states the oracle signals
    on some of them and not on others at one threshold: the exact path's summation order is pinned, too"""
    split = []
    for prm in ((50, 7, 33), (100, 1, 100)):
        c = knife.knife_case(*prm)
        for ci, k in enumerate(c.cnt):
            i, s1, s2, _, _ = helpers.lag_sums(k, c.lag)
            _, state = np.unique(np.stack([k[i].astype(np.int64), s1, s2], 1), axis=0, return_inverse=True)
            state = state.ravel()
            for t in c.thresholds():
                hit = c.oracle(t)[ci][i] != 0
                on, size = np.bincount(state, hit), np.bincount(state)
                split += [(prm, ci, t, int(a), int(b)) for a, b in zip(on, size) if 0 < a < b]
    print("states split by phase:", len(split), split[:4])
    assert len(split) >= 10 and {s[0] for s in split} == {(50, 7, 33), (100, 1, 100)}


@pytest.mark.parametrize("size,step,lag,tile", knife.SATURATED)
def test_saturated_inputs_reach_their_sums(size, step, lag, tile):
    c = knife.saturated_case(size, step, lag)
    thr = knife.saturated_thresholds(c)
    assert len(thr) == 25 and all(1e-6 <= t <= 1e6 for t in thr)
    s1, s2 = c.sums([0])                                             # the random 0.999 content alone
    k_rand, k_blk, k_gc = c.cnt
    assert k_rand.max() == size and k_rand.min() < size              # V != 0 somewhere, and counts at the top
    assert k_blk.max() == size and k_blk.min() == 0                  # the blocks swing over the whole range
    assert np.all(k_gc == size)
    _, _, _, _, v = helpers.lag_sums(k_rand, lag)
    assert np.count_nonzero(v) > 0.5 * v.size
    print((size, step, lag, tile), "S1", s1, "of", lag * size, "S2 / 2^24 %.4f" % (s2 / 2.0 ** 24))
    if (size, step, lag) == (255, 10, 257):
        assert s1 == 65535 == lag * size and s2 >= 0.99 * 2 ** 24 and s2 < 2 ** 24
    if (size, step, lag) == (254, 8, 258):
        assert s1 == 65532 == lag * size and s2 >= 0.99 * 2 ** 24 and s2 < 2 ** 24
    if (size, step, lag) == (255, 10, 258):
        assert s1 == 65790 == lag * size                             # beyond 16 bits: the wide path must hold it
    if size == 256:
        assert k_rand.max() == 256                                   # needs the 16-bit K
    if size == 2000:
        q2 = knife.q2_prefix_max(c, tile)
        print("   Q2 prefix / 2^32: %.4f" % (q2 / 2.0 ** 32))
        assert (tile + lag + 2) * size * size < 2 ** 32 if tile == 1024 else (tile + lag + 2) * size * size >= 2 ** 32
        assert q2 > 0.98 * 2 ** 32 and (q2 < 2 ** 32) == (tile == 1024)
    if tile in (1792,):
        nbytes = knife.tile_bytes(size, step, lag, tile)
        assert 62000 < nbytes <= 65520 and knife.tile_bytes(size, step, lag, tile + 256) > 65520
