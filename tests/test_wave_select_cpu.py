"""CPU checks of gams_amd/csrc/wave_select.hpp through the stand-alone driver tests/wave_select_main.cpp (host compiler,
no HIP, no device): the instance list against tests/wave_instances.py, and wave_select() over a grid of inputs against
tests/wave_select_expected.json.

That table was recorded from the code this refactor replaced (its wave_baked_kind, wave_*lds_bytes, wave_build_geometry,
the per-pass dispatch and the name code, copied unchanged into a scratch harness with stub structs), never from
wave_select() itself.  Tile size and thread count change speed only, so no result test sees a slip in them: this table
is what pins them.  `kernel` is the tile kernel the pass launches (for influence != 1 too, where
gams_wave_plan_kernel_name prints the repair or recurrence kernel that runs behind it)."""
import json
import os
import subprocess

import pytest

import wave_instances

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PEAKS, DENSE = 1, 2
MIB64 = 64 << 20                      # kStreamBytes: the NT half from the first byte above it
BIG = 40_000_000                      # windows of a 400-Mb batch at step 10
WS = (4, 8, 12, 20, 28)


def tile_thresholds():
    """total_windows one below and at every tile-count threshold of the ladder"""
    ts = []
    for w in WS:
        for tiles in (512, 768, 1024, 1536, 2048, 4096):
            ts += [tiles * 256 * w - 1, tiles * 256 * w]
    for per_tile in (64 * 28, 128 * 20):                      # 4096 one-wave W = 28 tiles, two-wave W = 20 tiles
        ts += [4096 * per_tile - 1, 4096 * per_tile]
    return ts + taper_thresholds()


def taper_thresholds():
    ts = []
    for cus in (256, 64):                                     # a round and a half of slots, tiles of 256 * 12 - 101 windows
        slots = 8 * cus
        ts += [(slots + slots // 2) * 2971 - 1, (slots + slots // 2) * 2971]
    return ts


BASE = [(100, 10, 100), (100, 1, 100), (100, 5, 200), (100, 20, 50), (50, 7, 33), (300, 10, 50), (100, 1000, 100)]
LADDER = BASE + [(100, 1, 200), (100, 5, 100), (100, 10, 50)]              # + the lag-as-argument forms of steps 1, 5, 10
NARROW = [(100, 1, 100), (100, 5, 200), (100, 1, 200), (100, 5, 100)]      # where DENSE changes the thread count
FAR = [(1000, 50, 30), (100, 10, 16001), (20, 1, 20000)]                   # size above 255, lags above 16000
BITS16 = [(255, 10, 257), (256, 10, 256), (100, 10, 655), (100, 10, 656), (1, 1, 65535), (128, 4, 512)]   # lag * size = 65535 | 65536
TW_REQS = (0, 1024, 2048, 3072, 5120, 7168, 512, 4096)       # every accepted request, then two the fast kernels refuse
NTH_REQS = (0, 64, 128, 256)


def lag_edges():
    """(params, W): lags just inside and outside lag + 1 <= 128 * W and lag + 1 <= (nth / 2) * W"""
    out = []
    for step in (1, 5, 10, 20):
        for w in WS:
            out += [((100, step, 128 * w - 1), w), ((100, step, 128 * w), w)]
    for step, w in ((1, 28), (5, 20)):
        for nth in (64, 128):
            out += [((100, step, nth // 2 * w - 1), w), ((100, step, nth // 2 * w), w)]
    return out


def grid():
    """-> the cases, each (size, step, lag, flags, serial, repair, depth, total_windows, tw_req, nth_req, taper_req, cus,
    set_bytes).  Influence enters the choice as serial / repair only (gams_wave_plan_create), so 0.5 and 0 are one case."""
    seen, cases = set(), []

    def add(prm, flags=PEAKS, infl=1.0, depth=1, total=BIG, tw=0, nth=0, taper=-1, cus=256, nbytes=1 << 20):
        serial = infl != 1.0
        repair = serial and 2 <= prm[2] <= 16000
        c = (prm[0], prm[1], prm[2], flags, int(serial), int(repair), depth, total, tw, nth, taper, cus, nbytes)
        if c not in seen:
            seen.add(c)
            cases.append(c)

    # the default ladder at every threshold, one pass at a time and in flight
    for prm in LADDER:
        for total in tile_thresholds():
            for depth in (1, 2):
                add(prm, depth=depth, total=total)
    for prm in NARROW:
        for total in tile_thresholds():
            for flags in (DENSE, PEAKS | DENSE):
                add(prm, flags=flags, total=total)
    # requests
    for prm in BASE + FAR + BITS16 + [(100, 1, 200), (100, 5, 100), (100, 10, 50)]:
        for tw in TW_REQS:
            for nth in NTH_REQS:
                add(prm, tw=tw, nth=nth)
    for prm, w in lag_edges():
        for tw in (0, 256 * w):
            for nth in NTH_REQS:
                for flags in (PEAKS, PEAKS | DENSE):
                    add(prm, flags=flags, tw=tw, nth=nth)
    for prm in NARROW:
        for tw in (0, 5120, 7168):
            for nth in NTH_REQS:
                for flags in (DENSE, PEAKS | DENSE):
                    add(prm, flags=flags, tw=tw, nth=nth)
    # influence, flags, depth
    for prm in LADDER + FAR[1:]:
        for infl in (1.0, 0.5, 0.0):
            for flags in (PEAKS, DENSE, PEAKS | DENSE):
                for depth in (1, 2, 3, 4):
                    for total in (30_000, BIG):
                        add(prm, flags=flags, infl=infl, depth=depth, total=total)
    # the taper
    for prm in ((100, 10, 100), (100, 10, 50)):
        for taper in (-1, 0, 1):
            for cus in (256, 64):
                for depth in (1, 2):
                    for total in taper_thresholds() + [BIG]:
                        for infl in (1.0, 0.5):
                            for nbytes in (MIB64, MIB64 + 1):
                                add(prm, infl=infl, depth=depth, total=total, taper=taper, cus=cus, nbytes=nbytes)
    # either side of 64 MiB
    for prm in LADDER:
        for nbytes in (MIB64, MIB64 + 1):
            for tw in (0, 3072, 512):
                add(prm, tw=tw, nbytes=nbytes)
    return cases


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("wave_select") / "wave_select_main"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", os.path.join(HERE, "wave_select_main.cpp"),
                           "-o", str(exe)])
    return str(exe)


def test_wave_select_header_is_plain_cxx():
    """no HIP in the selection: nothing but the C ABI header and the standard library is included"""
    src = open(os.path.join(ROOT, "gams_amd", "csrc", "wave_select.hpp")).read()
    incs = [ln.split()[1] for ln in src.splitlines() if ln.startswith("#include")]
    assert '"../../include/gams_gpu.h"' in incs
    assert all(i.startswith("<") and "hip" not in i for i in incs if i != '"../../include/gams_gpu.h"'), incs


def test_instance_list_and_recipes_agree(driver):
    listed = subprocess.check_output([driver, "list"], text=True).split("\n")[:-1]
    mine = [i.kernel for i in wave_instances.INSTANCES]
    assert len(set(listed)) == len(listed) and len(set(mine)) == len(mine)
    assert set(listed) - set(mine) == set(), "entries of the instance list without a recipe"
    assert set(mine) - set(listed) == set(), "recipes for entries the instance list does not hold"


def test_selection_matches_the_recorded_table(driver):
    cases = grid()
    with open(os.path.join(HERE, "wave_select_expected.json")) as fh:
        table = json.load(fh)
    assert table["columns"] == ["kernel", "nth", "tw", "max_win", "max_chunks", "lds_bytes", "taper", "direct"]
    assert len(table["rows"]) == len(cases), "the table was recorded over another grid"
    text = "".join(" ".join(map(str, c)) + "\n" for c in cases)
    out = subprocess.run([driver], input=text, stdout=subprocess.PIPE, text=True, check=True).stdout.split("\n")[:-1]
    assert len(out) == len(cases)
    bad = []
    for c, line, row in zip(cases, out, table["rows"]):
        want = [table["kernels"][row[0]]] + [str(v) for v in row[1:]]
        if line.split("\t") != want:
            bad.append((c, line.split("\t"), want))
    assert not bad, f"{len(bad)} of {len(cases)} differ; the first: {bad[:3]}"
    # the table reaches every family, both NT halves, and every entry of the list but the ones only a small batch's
    # requests reach (they are launched by test_gpu_wave_select.py)
    names = set(table["kernels"])
    assert any(k.startswith("wave_fast_taper_kernel<100, 10, 100, true") for k in names)
    assert any(k.startswith("wave_tile_kernel<unsigned short") for k in names) and any(k.startswith("wave_direct") for k in names)
    assert {i.kernel for i in wave_instances.INSTANCES} <= names
