"""CPU checks of wave_select_cut() (gams_amd/csrc/wave_select.hpp) through the stand-alone driver tests/wave_cut_main.cpp
(host compiler, no HIP, no device): the narrow body of the headline tile runs in one of two cuts -- two waves x 24 windows
or one wave x 48 -- exactly for the plans wave_select_body() calls narrow; and what the one-wave cut takes of the LDS, where
K lies over the tile's bit stream.  (That wave_select() and wave_select_body() answer what they did is checked by
tests/test_wave_select_cpu.py and tests/test_wave_body_cpu.py.)"""
import os
import subprocess

import pytest

import test_wave_select_cpu as sel
from test_wave_body_cpu import case

HERE = os.path.dirname(os.path.abspath(__file__))
AUTO, TWO_WAVES, ONE_WAVE = 0, 1, 2
AUTO_CUT = ONE_WAVE                   # what GAMS_WAVE_CUT_AUTO answers (profiles/one_wave_cut.txt)
LDS_PER_CU = 160 * 1024


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("wave_cut") / "wave_cut_main"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", os.path.join(HERE, "wave_cut_main.cpp"),
                           "-o", str(exe)])
    return str(exe)


def run(driver, req, cases):
    text = "".join(" ".join(map(str, (req,) + tuple(c))) + "\n" for c in cases)
    out = subprocess.run([driver], input=text, stdout=subprocess.PIPE, text=True, check=True).stdout.split("\n")[:-1]
    assert len(out) == len(cases)
    return [[ln.split("\t")[0]] + [int(v) for v in ln.split("\t")[1:]] for ln in out]


def check_cut(req, c, row):
    _, narrow, b_nth, b_w, b_lds, cut, nth, w, lds = row[:9]
    if not narrow:
        assert (cut, nth, w, lds) == (0, 0, 0, 0), (req, c, row)          # nothing to cut
        return
    want = AUTO_CUT if req == AUTO else req
    assert cut == want, (req, c, row)
    if cut == TWO_WAVES:
        assert (nth, w, lds) == (b_nth, b_w, b_lds) == (128, 24, b_lds), (req, c, row)
    else:
        assert (nth, w) == (64, 48) and 0 < lds < b_lds, (req, c, row)    # a smaller carve than the two-wave one
    assert nth * w == 3072                                                # every cut is of the same 3,072 K slots


def test_a_cut_exactly_for_the_narrow_plans(driver):
    cases = sel.grid() + [case(), case(depth=3), case(tw=3072), case(taper=1), case(nth=128), case(flags=sel.DENSE)]
    n_yes = 0
    for req in (AUTO, TWO_WAVES, ONE_WAVE):
        rows = run(driver, req, cases)
        for c, row in zip(cases, rows):
            check_cut(req, c, row)
        n_yes = sum(r[1] for r in rows)
        assert 0 < n_yes < len(cases)


def test_one_wave_carve_and_overlay(driver):
    (row,) = run(driver, ONE_WAVE, [case()])
    lds_two, lds = row[4], row[8]
    bm, k, pad = row[9:12]
    assert row[5:8] == [ONE_WAVE, 64, 48]
    assert lds < lds_two
    assert 28 * lds <= LDS_PER_CU                                         # the issue's floor: 28 one-wave workgroups a CU
    assert 32 * ((lds + 511) // 512 * 512) <= LDS_PER_CU                  # and all 32 waves of a CU even in 512-byte granules
    # K lies over pad | BM: the slots a thread reads (masked threads included) end inside it
    assert k >= 64 * 48 + 100 + 1 and k <= bm
    assert pad * 8 >= (100 + 1) * 10                                      # every bit in front of a ctg start is pad
    assert pad % 16 == 0 and (bm - pad) % 16 == 0                         # 16-byte pieces of plane behind a 16-byte aligned pad
    assert (bm - pad) * 8 >= 127 + 64 * 48 * 10 + 100                     # the tile's bits from a 128-base boundary
    assert lds == bm + (64 + 16) * 8                                      # ... and PS behind them: no scratch, no RK
