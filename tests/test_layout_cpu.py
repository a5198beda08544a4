"""CPU checks of gams_amd/csrc/layout.hpp (the Carver and the layouts the query entries carve their pooled blocks with)
through the stand-alone driver tests/layout_main.cpp: host compiler, no HIP, no device.

For every layout: the sizing pass (null base) and the pointer pass take the same bytes; every field begins on a 256-B
boundary; fields follow each other without overlap and end inside the block; a field the old code gave max(n, 1)
elements keeps a slot of its own when n = 0.  The totals are compared with the closed forms the entries spelled out
by hand before the layouts existed (sw.hip, interval.hip and text.hip of that commit: `al(b) = (b + 255) & ~255`),
copied here with the record sizes of that source -- not derived from layout.hpp."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SW_CTG, INDEX_GROUP, COUNT_GROUP, IV_REC, BK_REC = 32, 80, 32, 16, 32     # sizeof of the device records


def al(b):
    return (b + 255) & ~255


# ---- the old closed forms ------------------------------------------------------------------------------------------
def sw_bytes(n_sel, nf):
    return al(n_sel * SW_CTG) + 3 * al(nf * 4) + al((nf + 1) * 8)


def range_gc_bytes(n_sel, n):
    return al(n_sel * SW_CTG) + 3 * al(n * 4)


def sw_tabs_bytes(n_sel, nf, names, ids):
    return al((n_sel + 1) * 8) + al((n_sel + 1) * 4) + al(names + 1) + al((nf + 1) * 4) + al(ids + 1)


def arena_bytes(ng, m):
    ng1, m1 = max(ng, 1), max(m, 1)
    bk_slots = (m >> 1) + 2 * ng + 2
    return (al(ng1 * INDEX_GROUP) + al(ng1 * COUNT_GROUP) + 2 * al(m1 * 4) + al(m1 * IV_REC) + al((m + ng + 1) * 4)
            + 2 * al(bk_slots * BK_REC))


def scratch_bytes(ng, m):
    m1 = max(m, 1)
    return 2 * al(m1 * 4) + 2 * al(m1 * 8) + 2 * al(m1 * 4) + al((ng + 1) * 4)


def text_bytes(nl, L, nbr, n_rgg, n_cpos, pre):
    return (al((nl + 2) * 8) + 5 * al(L * 4) + 2 * al(L * 8) + al(L) + 2 * al((nbr + 1) * 8) + al(n_rgg * 4)
            + 2 * al(n_cpos * 4) + al(pre + 1))


SW = [(1, 1), (1, 63), (1, 64), (3, 1000), (32000, 1)]
GROUPS = [(0, 0), (1, 0), (1, 1), (1, 63), (1, 64), (2, 65), (7, 1000), (3, 100001), (4000, 5)]
TEXT = [(1, 1, 1, 0, 0, 0), (0, 1, 1, 1, 0, 0), (63, 64, 1, 0, 1, 0), (255, 256, 1, 0, 3, 10), (256, 257, 2, 5, 0, 0),
        (1000, 1000, 4, 1, 0, 0), (70000, 70001, 274, 0, 12, 255)]
CASES = ([("sw",) + c for c in SW] + [("range_gc",) + c for c in SW]
         + [("sw_tabs", 1, 1, 0, 0), ("sw_tabs", 1, 1, 255, 256), ("sw_tabs", 3, 1000, 7, 30000), ("sw_tabs", 32000, 1, 64000, 1)]
         + [("arena",) + c for c in GROUPS] + [("scratch",) + c for c in GROUPS] + [("text",) + c for c in TEXT])
CLOSED = dict(sw=sw_bytes, range_gc=range_gc_bytes, sw_tabs=sw_tabs_bytes, arena=arena_bytes, scratch=scratch_bytes,
              text=text_bytes)
# fields the old code sized max(n, 1): a slot of their own even when empty (by position in the layout)
OWN_SLOT = dict(arena=range(7), scratch=range(7))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("layout") / "layout_main"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", os.path.join(HERE, "layout_main.cpp"), "-o",
                           str(exe)])
    return str(exe)


def run(driver, cases):
    text = "".join(" ".join(map(str, c)) + "\n" for c in cases)
    out = subprocess.run([driver], input=text, stdout=subprocess.PIPE, text=True, check=True).stdout.split("\n")[:-1]
    assert len(out) == len(cases)
    rows = []
    for c, line in zip(cases, out):
        cols = line.split("\t")
        assert cols[0] == c[0] and len(cols) > 3, line
        rows.append((int(cols[1]), int(cols[2]), [tuple(map(int, f.split(","))) for f in cols[3:]]))
    return rows


def test_layout_header_is_plain_cxx():
    """no HIP in the layouts: nothing but the standard library is included"""
    src = open(os.path.join(ROOT, "gams_amd", "csrc", "layout.hpp")).read()
    incs = [ln.split()[1] for ln in src.splitlines() if ln.startswith("#include")]
    assert incs and all(i.startswith("<") and "hip" not in i for i in incs), incs


def test_passes_agree_fields_aligned_and_disjoint(driver):
    for c, (sizing, pointers, fields) in zip(CASES, run(driver, CASES)):
        assert sizing == pointers, c
        end = 0
        for k, (off, extent) in enumerate(fields):
            assert off % 256 == 0, (c, k, off)
            assert off >= end, (c, k, "overlaps the field in front")
            if k in OWN_SLOT.get(c[0], ()) and k > 0:
                assert off > fields[k - 1][0], (c, k, "shares its slot with the field in front")
            end = off + extent
        assert end <= sizing, c


def test_totals_equal_the_old_closed_forms(driver):
    for c, (sizing, _, _) in zip(CASES, run(driver, CASES)):
        assert sizing == CLOSED[c[0]](*c[1:]), c


def test_tight_field_leaves_no_padding(driver):
    """the rows of sw.hip's device block: the counts begin where the rows end, and only they are padded"""
    cases = [("tight", 1, 1), ("tight", 10, 3), ("tight", 32, 64), ("tight", 0, 0)]
    for c, (sizing, pointers, fields) in zip(cases, run(driver, cases)):
        assert sizing == pointers == c[1] * 24 + al(c[2] * 4), c
        assert fields[0] == (0, c[1] * 24) and fields[1] == (c[1] * 24, c[2] * 4), c
