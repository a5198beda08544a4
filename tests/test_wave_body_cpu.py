"""CPU checks of wave_select_body() (gams_amd/csrc/wave_select.hpp) through the stand-alone driver tests/wave_body_main.cpp
(host compiler, no HIP, no device): which plans run their plane-fed passes in the narrow body (128 threads x 24 windows
over the tile of the (12, 100, 10, 100, 256) entry), what that body takes of the LDS, and that wave_select() itself still
answers what tests/wave_select_expected.json recorded."""
import json
import os
import subprocess

import pytest

import test_wave_select_cpu as sel

HERE = os.path.dirname(os.path.abspath(__file__))
PEAKS, DENSE = sel.PEAKS, sel.DENSE
HEADLINE = (100, 10, 100)
WIDE_NAMES = ("wave_fast_kernel<12, 100, 10, 100, false, 256>", "wave_fast_kernel<12, 100, 10, 100, true, 256>")
LDS_PER_CU = 160 * 1024


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("wave_body") / "wave_body_main"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", os.path.join(HERE, "wave_body_main.cpp"),
                           "-o", str(exe)])
    return str(exe)


def run(driver, cases):
    text = "".join(" ".join(map(str, c)) + "\n" for c in cases)
    out = subprocess.run([driver], input=text, stdout=subprocess.PIPE, text=True, check=True).stdout.split("\n")[:-1]
    assert len(out) == len(cases)
    return [ln.split("\t") for ln in out]


def case(prm=HEADLINE, flags=PEAKS, serial=0, repair=0, depth=1, total=sel.BIG, tw=0, nth=0, taper=0, cus=256,
         nbytes=1 << 20):
    return (prm[0], prm[1], prm[2], flags, serial, repair, depth, total, tw, nth, taper, cus, nbytes)


def check_body(c, row):
    """the body columns of one answer against the rule, stated over the inputs and the selected kernel's name"""
    name, lds_wide, taper = row[0], int(row[5]), int(row[6])
    narrow, nth, w, lds = (int(v) for v in row[8:12])
    dense, serial, nth_req = bool(c[3] & DENSE), bool(c[4]), c[9]
    want = name in WIDE_NAMES and not taper and not dense and not serial and nth_req == 0
    assert bool(narrow) == want, (c, row)
    if narrow:
        assert (c[0], c[1], c[2]) == HEADLINE and c[8] in (0, 3072), (c, row)
        assert (nth, w) == (128, 24), (c, row)
        assert 0 < lds <= lds_wide, (c, row)                  # the smaller PS / RK carve
        assert 16 * lds <= LDS_PER_CU, (c, row)               # sixteen two-wave workgroups per CU
    else:
        assert (nth, w, lds) == (0, 0, 0), (c, row)


def test_yes_for_the_headline_entry_only(driver):
    yes = [case(), case(depth=3), case(tw=3072), case(tw=3072, total=30_000), case(taper=-1, depth=2),
           case(nbytes=sel.MIB64 + 1), case(cus=64), case(total=768 * 3072, depth=2)]
    for c, row in zip(yes, run(driver, yes)):
        assert row[0] in WIDE_NAMES and row[8:11] == ["1", "128", "24"], (c, row)
        check_body(c, row)
    no = [case(flags=DENSE), case(flags=PEAKS | DENSE), case(serial=1, repair=1), case(serial=1, repair=1, flags=PEAKS | DENSE),
          case(serial=1, repair=0),
          case(nth=64), case(nth=128), case(nth=256),
          case(taper=1), case(taper=-1, depth=1),                                   # the tapered table
          case(tw=1024), case(tw=2048), case(tw=5120), case(tw=7168), case(tw=512), case(tw=4096),
          case(total=30_000),                                                       # a small batch: W = 4
          case(total=600 * 3072),                                                   # W = 8
          case(prm=(100, 10, 50)), case(prm=(100, 10, 200), tw=3072),               # the lag an argument
          case(prm=(100, 5, 100)), case(prm=(100, 20, 100)), case(prm=(100, 1, 100)), case(prm=(100, 1, 100), tw=3072),
          case(prm=(50, 7, 33), tw=3072), case(prm=(300, 10, 50)), case(prm=(100, 1000, 100))]
    for c, row in zip(no, run(driver, no)):
        assert row[8:12] == ["0", "0", "0", "0"], (c, row)
        check_body(c, row)


def test_body_over_the_selection_grid_and_selection_unchanged(driver):
    cases = sel.grid()
    with open(os.path.join(HERE, "wave_select_expected.json")) as fh:
        table = json.load(fh)
    assert len(table["rows"]) == len(cases)
    rows = run(driver, cases)
    n_yes = 0
    for c, row, want in zip(cases, rows, table["rows"]):
        assert row[:8] == [table["kernels"][want[0]]] + [str(v) for v in want[1:]], (c, row)   # wave_select, bit for bit
        check_body(c, row)
        n_yes += int(row[8])
    assert 0 < n_yes < len(cases)


def test_narrow_carve_is_the_wide_one_less_128_threads_of_ps_and_rk(driver):
    (row,) = run(driver, [case()])
    lds_wide, lds = int(row[5]), int(row[11])
    assert lds_wide - lds == 128 * 8 + 128 * 2                # 8 bytes of PS and 2 of RK a thread
    assert 16 * lds <= LDS_PER_CU
