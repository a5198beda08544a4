"""CPU checks of the tapered tile table: wave_taper_tails / wave_taper_width of gams_amd/csrc/wave_select.hpp -- the
arithmetic wave_fill_tiles_tapered (wave.hip) runs -- through the stand-alone driver tests/wave_select_main.cpp
(`taper` mode; host compiler, no HIP, no device), against the Python model of tests/taper.py, which is written from the
documented rule.  Which ctg gets which tile width changes speed only, so no result test sees a slip here.

Then the layout of the world test_gpu_wave_taper.py runs, with the model alone."""
import os
import subprocess

import numpy as np
import pytest

import taper

HERE = os.path.dirname(os.path.abspath(__file__))
PCTS = (0, 1, 25, 50, 99, 100)
CUS = (32, 64, 256)


def split(total, piece):
    """ctgs of `piece` windows summing to `total`, the remainder in the last one"""
    if total <= 0:
        return []
    k = max(total // piece, 1)
    return [piece] * (k - 1) + [total - piece * (k - 1)]


def boundary_batch(total, cus, pct4, pct8, d4, d8):
    """a batch of `total` windows with a ctg whose `after` is x4 + d4 and one whose `after` is x4 + y8 + d8 (where a ctg
    of at least `lag` windows can start there), or None"""
    x4, y8 = taper.tails(total, cus, pct4, pct8)
    t4, t8 = x4 + d4, x4 + y8 + d8 - (x4 + d4)
    if t4 < taper.LAG or t8 < taper.LAG or total - t4 - t8 < taper.LAG:
        return None
    piece = max(total // 150, 3000)
    return split(total - t4 - t8, piece) + split(t8, 2 * taper.tile_windows(8) + 1) + split(t4, taper.tile_windows(4) + 1)


def batches():
    """-> [(cus, pct4, pct8, window counts)]"""
    out = []
    for cus in CUS:
        s = taper.slots(cus)
        floor = (s + s // 2) * taper.tile_windows(12)
        # just tapered: the 8 % / 17 % caps bind from 50 % on; far beyond: the slots terms bind even at 100 %.  Neither
        # total is a multiple of 100, so T * 8 / 100 and T * 17 / 100 are not whole
        for total in (floor + 1, 12_000 * s + 37):
            for pct4 in PCTS:
                for pct8 in PCTS:
                    for d4, d8 in ((0, 0), (1, 0), (0, 1), (1, 1)):
                        b = boundary_batch(total, cus, pct4, pct8, d4, d8)
                        if b is not None:
                            out.append((cus, pct4, pct8, b))
        for pct4 in PCTS:
            for pct8 in PCTS:
                out.append((cus, pct4, pct8, [floor + 1]))                       # a batch of one ctg
                out.append((cus, pct4, pct8, [taper.LAG] * 3000))                # 3,000 ctgs of `lag` windows
                out.append((cus, pct4, pct8, [taper.LAG] * 3000 + [floor]))      # ... in front of the tails' ctg
                out.append((cus, pct4, pct8, [floor] + [taper.LAG] * 3000))      # ... inside the tails
    return out


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("wave_taper") / "wave_select_main"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", os.path.join(HERE, "wave_select_main.cpp"),
                           "-o", str(exe)])
    return str(exe)


@pytest.fixture(scope="module")
def answers(driver):
    cases = batches()
    text = "".join(f"{cus} {p4} {p8} {taper.LAG} {len(b)} " + " ".join(map(str, b)) + "\n" for cus, p4, p8, b in cases)
    out = subprocess.run([driver, "taper"], input=text, stdout=subprocess.PIPE, text=True, check=True).stdout.split("\n")[:-1]
    assert len(out) == len(cases)
    got = []
    for line in out:
        v = np.array(line.split(), np.int64)
        got.append((int(v[0]), int(v[1]), v[2::2], v[3::2]))      # x4, y8, W per ctg, tiles per ctg
    return cases, got


def test_the_grid_reaches_what_it_is_for():
    """both terms of either minimum bind somewhere, fractions are cut before the multiply, every boundary is met"""
    bind = {k: 0 for k in ("slots4", "cap4", "slots8", "cap8", "frac_slots", "frac_cap", "at_x4", "past_x4", "at_xy", "past_xy")}
    for cus, p4, p8, b in batches():
        n = np.asarray(b, np.int64)
        total, s = int(n.sum()), taper.slots(cus)
        a4, c4 = s * p4 // 100 * 923, total * 8 // 100
        a8, c8 = s * p8 // 100 * 1947, total * 17 // 100
        bind["slots4"] += 0 < a4 < c4
        bind["cap4"] += c4 < a4
        bind["slots8"] += 0 < a8 < c8
        bind["cap8"] += c8 < a8
        bind["frac_slots"] += (s * p4) % 100 != 0 and (s * p8) % 100 != 0
        bind["frac_cap"] += (total * 8) % 100 != 0 and (total * 17) % 100 != 0 and c4 < a4 and c8 < a8
        x4, y8 = taper.tails(total, cus, p4, p8)
        after = total - (np.cumsum(n) - n)
        bind["at_x4"] += bool(np.any(after == x4))
        bind["past_x4"] += bool(np.any(after == x4 + 1))
        bind["at_xy"] += bool(np.any(after == x4 + y8))
        bind["past_xy"] += bool(np.any(after == x4 + y8 + 1))
    assert all(v >= 10 for v in bind.values()), bind


def test_driver_equals_the_model(answers):
    cases, got = answers
    bad = []
    for (cus, p4, p8, b), (x4, y8, w, tiles) in zip(cases, got):
        n = np.asarray(b, np.int64)
        mw = taper.widths(n, cus, p4, p8)
        mt = np.bincount(taper.table(n, cus, p4, p8)[:, 0], minlength=n.size)
        if (x4, y8) != taper.tails(int(n.sum()), cus, p4, p8) or not np.array_equal(w, mw) or not np.array_equal(tiles, mt):
            bad.append((cus, p4, p8, int(n.sum()), len(b), (x4, y8), taper.tails(int(n.sum()), cus, p4, p8)))
    assert not bad, f"{len(bad)} of {len(cases)} differ; the first: {bad[:3]}"


def test_invariants_of_the_table(answers):
    """without the model: widths never grow along the table; the W = 4 ctgs hold at most x4 windows and x4 at most 8 %
    of the batch; the W = 4 and W = 8 ctgs together at most x4 + y8; every ctg's tiles cover its windows exactly"""
    cases, got = answers
    for (cus, p4, p8, b), (x4, y8, w, tiles) in zip(cases, got):
        n = np.asarray(b, np.int64)
        total = int(n.sum())
        key = (cus, p4, p8, total, len(b))
        assert set(w.tolist()) <= {4, 8, 12}, key
        assert np.all(np.diff(w) <= 0), key
        assert int(n[w == 4].sum()) <= x4 and 100 * x4 <= 8 * total, key
        assert int(n[w <= 8].sum()) <= x4 + y8 and 100 * y8 <= 17 * total, key
        assert x4 <= taper.slots(cus) * taper.tile_windows(4) and y8 <= taper.slots(cus) * taper.tile_windows(8), key
        tw = 256 * w - taper.LAG - 1
        assert np.all((tiles - 1) * tw < n) and np.all(tiles * tw >= n), key


def test_defaults_of_the_model_are_the_documented_ones():
    assert (taper.PCT4, taper.PCT8) == (25, 50)
    assert [taper.tile_windows(w) for w in (4, 8, 12)] == [923, 1947, 2971]
    assert taper.tapered(12 * 256 * 2971, 256) and not taper.tapered(12 * 256 * 2971 - 1, 256)


@pytest.mark.parametrize("cus", [32, 256])
def test_world_layout(cus):
    """the world's builder alone: T, the two exact boundaries, every listed window count in either tail"""
    lay = taper.layout(cus)
    n = lay.counts
    assert lay.T == int(n.sum()) == 12 * cus * 2971 + taper.MARGIN and taper.tapered(lay.T, cus)
    assert (lay.x4, lay.y8) == taper.tails(lay.T, cus)
    after = lay.T - (np.cumsum(n) - n)
    assert after[lay.w4[0]] == lay.x4 and after[lay.w8[0]] == lay.x4 + lay.y8
    assert n[lay.front] == taper.LAG and lay.front == lay.w8[0] - 1 and after[lay.front] == lay.x4 + lay.y8 + taper.LAG
    w = taper.widths(n, cus)
    assert np.all(w[list(lay.w4)] == 4) and np.all(w[list(lay.w8)] == 8) and np.all(w[:lay.front + 1] == 12)
    assert lay.w4[-1] == n.size - 1 and lay.w8[-1] == lay.w4[0] - 1 and list(lay.body) == list(range(lay.front))
    assert np.all(n >= taper.LAG)
    for tail, big, wk in ((lay.w4, lay.big4, 4), (lay.w8, lay.big8, 8)):
        tw = taper.tile_windows(wk)
        have = set(n[list(tail)].tolist())
        assert {100, 101, tw - 1, tw, tw + 1, 2 * tw + 1, 2970, 2971, 2972} <= have
        assert big in tail
        # x4 is 2 * cus tiles of 923 windows: room for a ctg of 64 tiles beside the others from 80 CUs on
        room = (lay.x4 if wk == 4 else lay.y8) - sum(taper.edge_counts(wk))
        assert n[big] >= min(64 * tw + 1, room) and (n[big] >= 64 * tw + 1 or cus < 80)
        assert {taper.ragged(k) for k in tail} == set(range(10))
        # the smallest shape of test_gpu_wave_taper.py, 1 % / 1 % of a round, still has ctgs in either tail
        assert set(taper.widths(n, cus, 1, 1).tolist()) == {4, 8, 12}
    tiles = taper.table(n, cus)
    assert tiles.shape[0] == int(((n + (256 * w - 101) - 1) // (256 * w - 101)).sum())
    for wk in (4, 8, 12):                                  # a last tile of one window at every width but the body's
        last = np.flatnonzero((tiles[:, 2] == wk) & (n[tiles[:, 0]] - tiles[:, 1] == 1))
        assert last.size >= (wk != 12), wk


def test_world_sequences_small():
    """the bases of the 32-CU world: lengths with their ragged tails, both kinds of content, the runs across the seams"""
    lay = taper.layout(32)
    seqs = taper.sequences(lay)
    assert [s.size for s in seqs] == [taper.bases(int(c), taper.ragged(k)) for k, c in enumerate(lay.counts)]
    assert all(s.dtype == np.uint8 for s in seqs)
    for tail, big, wk in ((lay.w4, lay.big4, 4), (lay.w8, lay.big8, 8)):
        kinds = [bool(np.any(seqs[k] > 127)) for k in taper.mixed(lay, tail)]
        assert len(kinds) == 10 and taper.mixed(lay, tail)[0] == big
        assert all(set(np.unique(seqs[k]).tolist()) == set(b"ACGT") for k in tail if k not in taper.mixed(lay, tail))
        assert kinds[0::2] == [False] * len(kinds[0::2]) and kinds[1::2] == [True] * len(kinds[1::2])
        for seam, base in ((1, ord("G")), (2, ord("N"))):
            mid = seam * taper.tile_windows(wk) * 10
            assert np.all(seqs[big][mid - 600:mid + 600] == base) and taper.RUN > 1110
    assert set(np.unique(seqs[0]).tolist()) == set(b"ACGT")
    again = taper.sequence(lay, lay.big4)
    assert np.array_equal(again, seqs[lay.big4])
