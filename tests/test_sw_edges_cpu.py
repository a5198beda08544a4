"""CPU proof that the cases of tests/sw_edges.py carry what they are built for, so that test_gpu_sw_edges.py cannot pass
vacuously: text block totals and their offsets inside a 16-byte unit around the writer's stage limit, ctgs on the seams
of the 512-row text blocks and empty intervals around them, ctg boundaries on the seams of the 256-feature workgroups,
more workgroups and blocks than the scan has threads, more intervals than features, which lines offend the middle check
and the smallest of them, line and interval counts on powers of two, the `chr:pos`, NaN and -0 rows, three-digit
serials and five-digit feature numbers.  Every figure is read off the model's text (sw_text.slices, held to
sw_text.interval_text and sw_text.model here)."""
import os
import re

import numpy as np
import pytest

import sw_edges as se
import sw_text as swt
from test_rg_text_cpu import locator_order
from test_rg_text_cpu import model as rg_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_constants_are_the_kernels():
    """512 rows a text block, 49,152 staged bytes, 256 features a workgroup, 1,024 scan threads: read from the sources"""
    sw = open(os.path.join(ROOT, "gams_amd", "csrc", "sw.hip")).read()
    text = open(os.path.join(ROOT, "gams_amd", "csrc", "text.hip")).read()
    assert "kSwTextBlock = %d;" % se.BLOCK in sw and "kSwTextStage = %d;" % se.STAGE in sw
    assert "char stage[kSwTextStage + 16]" in sw and "tot <= kSwTextStage" in sw
    w = se.FEAT_BLOCK
    assert re.search(r"sw_gather_kernel, dim3\(\(std::max\(K, nc\) \+ %du\) / %du\), dim3\(%d\)" % (w - 1, w, w), text)
    assert "nbf = (nf + %du) / %du;" % (w - 1, w) in sw
    for k in ("sw_geom_kernel", "sw_row_off_kernel"):
        assert re.search(r"%s, dim3\(nbf\), dim3\(%d\)" % (k, w), sw), k
        assert re.search(r"__launch_bounds__\(%d\) void %s\(" % (w, k), sw), k
    assert "sw_ctg_row_off_kernel, dim3(n_ctg / %du + 1u), dim3(%d)" % (w, w) in sw
    assert sw.count("dim3(1), dim3(%d), 0, st, " % se.SCAN_THREADS) >= 2          # both blk_offsets_scan_kernel launches


@pytest.mark.parametrize("name", se.SMALL_CASES)
def test_the_expected_text_is_the_models(name):
    """Expected lays sw_text.slices out by interval and by id: that is interval_text and model"""
    c, ex = se.case(name), se.expected(name)
    assert ex.text == swt.interval_text(c["ctgs"], c["data"], *se.params(c))
    assert ex.by_id == swt.model(c["ctgs"], c["data"], *se.params(c))
    assert ex.n_rows == ex.text.count(b"\n") == int(ex.row_off[-1]) and len(ex.text) == int(ex.text_off[-1])
    assert ex.n_features == int(ex.bucket_off[-1]) == len(ex.rows_per_feature()) > 0
    assert se.offenders(c["ctgs"], c["data"]) == []
    for i, (cg, rows) in enumerate(zip(ex.order, ex.rows)):       # every slice holds its ctg's rows, and only those
        assert all(r.startswith(b"sw:feature:" + cg["id"].encode() + b":") for r in rows)
        assert bool(rows) == bool(ex.kept[i])


# ---- 1. the stage limit and its alignment --------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(se.STAGE_CASES))
def test_stage_cases_hit_their_totals(name):
    targets, tail = se.STAGE_CASES[name]
    c, ex = se.case(name), se.expected(name)
    tot = ex.block_totals()
    assert [len(r) for r in ex.rows] == c["want_rows"] and ex.n_rows == se.BLOCK * len(targets) + tail
    assert tot[:len(targets)].tolist() == targets and len(tot) == len(targets) + (tail > 0)
    assert [x["id"] for x in locator_order(c["ctgs"])] == [x["id"] for x in c["ctgs"]]
    lens = {len(x["id"]) for x in c["ctgs"]}
    assert len(lens) >= 2 and max(lens) <= 80                        # a block is split between ctgs of different id lengths
    f = ex.fields()
    assert {r[2] for r in f} == {"M", "L", "R"} and len({len(r[1]) for r in f}) >= 2      # coordinate digit counts vary


def test_stage_cases_sit_on_the_limit_at_every_residue():
    tot = {k: se.expected(k).block_totals() for k in se.STAGE_CASES}
    blk0 = {k: se.expected(k).block_starts() for k in se.STAGE_CASES}
    assert [int(tot[k][0]) for k in ("under", "exact", "over")] == [se.STAGE - 1, se.STAGE, se.STAGE + 1]
    assert tot["exact_alone"].tolist() == [se.STAGE]
    # the exact block as the second one, 15 bytes into a 16-byte unit: stage[] filled to its last byte but one
    assert tot["second_exact_r15"][1] == se.STAGE and blk0["second_exact_r15"][1] % 16 == 15
    # a block that is not staged sets the offset of staged ones
    t, b = tot["over_then_staged"], blk0["over_then_staged"]
    assert t[0] > se.STAGE and (t[1:] <= se.STAGE).all() and b[1] % 16 != 0 and b[2] % 16 != 0
    staged = set()
    for k in se.STAGE_CASES:
        staged |= {int(x) % 16 for x, n in zip(blk0[k], tot[k]) if n <= se.STAGE}
    assert staged == set(range(16))
    assert (blk0["ladder"][:16] % 16).tolist() == list(range(16))


# ---- 2. text block seams and empty intervals ------------------------------------------------------------------------
def test_seam_cases_put_ctgs_on_the_block_seams():
    first = set()
    totals = set()
    for name, (spec, mx) in se.SEAM_CASES.items():
        c, ex = se.case(name), se.expected(name)
        assert [len(r) for r in ex.rows] == c["want_rows"] == [max(w, 0) for _, w in spec]
        assert ex.n_located == [0 if w == 0 else 1 if w < 0 else 1 + len(k) for (_, w), k in zip(spec, ex.kept)]
        totals.add(ex.n_rows)
        first |= {int(ex.row_off[i]) % se.BLOCK for i, r in enumerate(ex.rows) if r and ex.row_off[i] > 0}
    assert first >= {0, 1, 511}
    assert any(t % se.BLOCK == 0 for t in totals) and any(t % se.BLOCK == 1 and t > se.BLOCK for t in totals) and 1 in totals
    ex = se.expected("seam_2048")
    empty = [not r for r in ex.rows]
    assert empty[:2] == [True, True] and empty[-2:] == [True, True]            # first and last, of both kinds
    assert ex.n_located[:2] == [0, 1] and ex.n_located[-2:] == [1, 0]
    assert empty[3:6] == [True] * 3 and not empty[2] and not empty[6]            # a run between non-empty ones
    assert int(ex.row_off[-1]) == 4 * se.BLOCK                                  # the trailing empties sit on blk_off[nb]
    assert se.expected("single_row").n_rows == 1 and se.SEAM_CASES["single_row"][1] == 0
    ex = se.expected("seam_1025")
    assert int(ex.row_off[3]) == se.BLOCK and not ex.rows[3] and not ex.rows[4]  # an empty run begins on the seam


# ---- 3. feature prefix seams ----------------------------------------------------------------------------------------
def test_prefix_cases_put_ctg_boundaries_on_the_workgroup_seams():
    bounds = set()
    for name, nf in se.PREFIX_NF.items():
        c, ex = se.case(name), se.expected(name)
        assert ex.n_features == nf and se.params(c) == (10, 3, 40)
        bounds |= {int(b) for b in ex.bucket_off[1:-1]}
        per = ex.rows_per_feature()
        assert min(per) == (1 if name != "nf256" else 4) and max(per) == 7 and len(set(per)) >= 4, (name, set(per))
        # the prefix is not one a constant stride would give: a shifted prefix moves rows
        assert len(set(np.diff(np.cumsum(per)[::5]).tolist())) > 3
    assert {255, 256} <= bounds and set(se.PREFIX_NF.values()) == {255, 256, 257, 513}
    ex = se.expected("nf513")
    assert ex.bucket_off.tolist() == [0, 255, 256, 256, 256, 513] and ex.n_located[2:4] == [0, 1]


def test_big_case_has_more_workgroups_and_blocks_than_the_scan_has_threads():
    c = se.case("big")
    text = se.big_text()
    _, kept = swt.buckets(c["ctgs"], c["data"])
    nf = sum(len(b) for b in kept)
    rows = text.count(b"\n")
    assert nf == se.BIG_KEPT >= 262_145 + 3 and len(c["ctgs"]) == 3 and all(kept)
    assert -(-nf // se.FEAT_BLOCK) > se.SCAN_THREADS and rows >= 524_289 and -(-rows // se.BLOCK) > se.SCAN_THREADS
    assert se.params(c) == (10, 1, 20)
    heads = [r.split(b"\t", 1)[0] for r in text.split(b"\n")[:-1]]
    serial = np.array([int(h.rsplit(b":", 1)[1]) for h in heads])
    per = np.diff(np.append(np.flatnonzero(serial == 1), rows))
    assert per.size == nf and set(per.tolist()) == {2, 3} and (per == 2).sum() > 1000     # the counts vary
    for cg, b in zip(c["ctgs"], kept):                                # features near both ends of every ctg
        assert any(s <= cg["chr_start"] + 5 for s, _, _ in b) and any(e >= cg["chr_end"] - 5 for _, e, _ in b)


# ---- 4. intervals beyond the features -------------------------------------------------------------------------------
@pytest.mark.parametrize("n", se.MANY_COUNTS)
def test_many_cases_have_more_intervals_than_features(n):
    c, ex = se.case("many_%d" % n), se.expected("many_%d" % n)
    assert len(ex.order) == n and [x["id"] for x in ex.order] == [x["id"] for x in c["ctgs"]]
    assert [i for i, r in enumerate(ex.rows) if r] == se.many_kept(n)
    assert 0 < ex.n_features < se.FEAT_BLOCK <= n + 1                  # one workgroup of features, more of intervals
    assert all(300 <= len(x["seq"]) <= 600 for x in ex.order)
    lens = [len(x["id"]) for x in ex.order]
    assert min(lens) == 1 and max(lens) == 80 == lens[-1]
    assert sum(m == 1 and not k for m, k in zip(ex.n_located, ex.kept)) >= 5      # empty buckets among the empty intervals
    if n == 600:
        chrs = [x["chr_id"] for x in ex.order]
        assert len(set(chrs)) >= 5 and {len(k) for k in chrs} >= {1, 40}
        assert se.many_kept(n) == [0, 255, 256, 599] and chrs[255] != chrs[256] and len(ex.order[256]["id"]) == 1
    else:
        assert se.many_kept(n)[-1] == n - 1 and se.many_kept(n)[0] == 0
    assert ex.text != ex.by_id                                         # the ids sort otherwise than the Locator orders


# ---- 5. the middle check --------------------------------------------------------------------------------------------
def test_middle_probes_agree_with_the_table_and_the_model():
    ctgs = se.middle_ctgs()
    c = ctgs[0]
    assert (c["chr_start"], c["chr_end"]) == (1001, 4000)
    probes = dict(se.middle_probes(c))
    assert all(probes[k] == v for k, v in se.MIDDLE_TABLE.items() if k in probes)
    assert {"I:901-1102", "I:3899-4101", "I:1001-4000"} <= set(probes)       # the general lines meet the table's
    probes.update(se.MIDDLE_TABLE)
    assert sum(probes.values()) >= 10 and sum(not v for v in probes.values()) >= 10
    for line, ok in probes.items():
        data = se.probe_data(c, line)
        assert se.offenders(ctgs, data) == ([] if ok else [2]), line
        _, kept = swt.buckets(ctgs, data)
        assert len(kept[0]) == 1 and not kept[1] and not kept[2], line           # located to ctg:I:1, kept
        if ok:
            assert swt.model(ctgs, data, **_kw()).count(b"\n") >= 1
        else:
            with pytest.raises(swt.ModelError, match=r"line 2\b"):
                swt.features(ctgs, data)
        first = se.probe_data(c, line, first=True)                               # as the dropped first line: accepted
        assert se.offenders(ctgs, first) == [] and sum(len(f) for f in swt.features(ctgs, first)) == 1, line
    s_e = [tuple(int(x) for x in re.split(r"[:-]", k)[1:]) for k, v in probes.items()]
    assert any((e - s + 1) % 2 for s, e in s_e if e > s) and any((e - s + 1) % 2 == 0 for s, e in s_e)
    assert "I:4000" in probes and probes["I:4000"] and any(e < s for s, e in (t for t in s_e if len(t) == 2))
    assert probes["I:501-4500"] is True


def _kw():
    return dict(size=se.PARAMS["size"], mx=se.PARAMS["mx"], resize=se.PARAMS["resize"])


def test_several_offenders_and_their_minimum():
    ctgs = se.middle_ctgs()
    mins = []
    for reverse in (False, True):
        data = se.offenders_data(reverse)
        bad = se.offenders(ctgs, data)
        assert len(bad) == 4
        _, kept = swt.buckets(ctgs, data)
        of = {line + 1: i for i, b in enumerate(kept) for _, _, line in b}
        assert [of[n] for n in bad].count(0) == 1 and of[bad[0]] == 1           # the smallest is ctg:I:2's, not the first ctg's
        assert len(kept[0]) > se.FEAT_BLOCK                                      # and not in the first feature workgroup
        first_ctg = next(n for n in bad if of[n] == 0)
        assert first_ctg > bad[0]
        with pytest.raises(swt.ModelError, match=r"line %d\b" % first_ctg):     # the model stops at the first in ctg order
            swt.features(ctgs, data)
        mins.append(bad[0])
    assert mins[0] != mins[1]
    prefix = b"# c\n\n\r\n"
    assert se.offenders(ctgs, se.offenders_data(False, prefix)) == [n + 3 for n in se.offenders(ctgs, se.offenders_data())]


# ---- 6. key decode --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lines,n_ctg", se.KEY_CASES)
def test_key_cases_have_their_line_and_interval_counts(lines, n_ctg):
    c, ex = se.case("key_%d_%d" % (lines, n_ctg)), se.expected("key_%d_%d" % (lines, n_ctg))
    assert se.n_lines(c["data"]) == lines and len(ex.order) == n_ctg
    assert ex.kept[-1] and max(k[2] for k in ex.kept[-1]) == lines - 1            # the last line: kept, in the last interval
    assert ex.order[-1]["id"] == c["ctgs"][-1]["id"]
    if lines > 16:
        assert sum(bool(k) for k in ex.kept) == n_ctg


def test_key_cases_cover_the_powers_of_two():
    assert {k[0] for k in se.KEY_CASES} == {2, 3, 256, 257, 65_536, 65_537}
    assert {k[1] for k in se.KEY_CASES} == {1, 2, 3, 4, 7, 8}


# ---- 7. smallest geometries and widths ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(se.POINT_CASES))
def test_point_cases_print_single_bases(name):
    c, ex = se.case(name), se.expected(name)
    mx, resize = se.POINT_CASES[name]
    assert se.params(c) == (2, mx, resize) and mx in (0, 3) and resize in (2, 4)
    cg = c["ctgs"][0]
    assert all(s == e for s, e, _ in ex.kept[0])
    assert {cg["chr_start"] + 1, cg["chr_end"]} <= {s for s, _, _ in ex.kept[0]}
    m_rows = [r for r in ex.fields() if r[2] == "M"]
    assert len(m_rows) == ex.n_features and all(re.fullmatch(r"I:\d+", r[1]) for r in m_rows)     # chr:pos, no dash
    assert "I:%d" % (cg["chr_start"] + 1) in {r[1] for r in m_rows} and "I:%d" % cg["chr_end"] in {r[1] for r in m_rows}
    assert ex.n_rows == ex.n_features if mx == 0 else ex.n_rows > 5 * ex.n_features


def test_tiny_cases_print_nan_and_minus_zero():
    seen = set()
    for name in se.TINY_CASES:
        c, ex = se.case(name), se.expected(name)
        assert sorted(len(x["seq"]) for x in c["ctgs"])[:5] == [2, 15, 16, 17, 50] and len(c["ctgs"]) == 6
        assert all(ex.kept) and c["size"] == int(name[5:])
        for r in ex.fields():
            seen |= {(name, v) for v in r[4:8] if v in ("NaN", "-0")}
    assert seen == {(n, v) for n in se.TINY_CASES for v in ("NaN", "-0")}


def test_width_cases_reach_three_digit_serials_and_five_digit_ids():
    c, ex = se.case("serial"), se.expected("serial")
    assert c["mx"] == 50 and len(c["ctgs"][0]["seq"]) >= 1100
    assert max(s for _, _, s in ex.heads()) == 101 and ex.rows_per_feature()[0] == 101 > ex.rows_per_feature()[1]
    c, ex = se.case("ids"), se.expected("ids")
    assert c["mx"] == 0 and ex.n_features == ex.n_rows == 10_001 and len(c["ctgs"]) == 1
    nums = {n for _, n, _ in ex.heads()}
    assert {9_999, 10_000, 10_001} <= nums
    assert b"sw:feature:ctg:I:1:9999:1\t" in ex.text and b"sw:feature:ctg:I:1:10000:1\t" in ex.text


# ---- 8. -a count ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(se.COUNT_CASES))
def test_rg_sources_cover_some_chromosomes_only(name):
    c, ex = se.case(name), se.expected(name)
    data, records = se.rg_source(c["ctgs"], se.COUNT_CASES[name])
    assert b"\t" not in data
    buckets = rg_model(c["ctgs"], data)["buckets"]
    with_rows = [x for x, r in zip(ex.order, ex.rows) if r]
    has = {x["id"] for x, b in zip(c["ctgs"], buckets) if b}
    assert any(x["id"] in has for x in with_rows) and (any(x["id"] not in has for x in with_rows) or len(with_rows) == 1)
    assert set(se.COUNT_CASES) == set(se.SEAM_CASES) | set(se.MANY_CASES)
    assert {x["chr_id"] for x in c["ctgs"] if x["id"] in has} == set(se.COUNT_CASES[name])
    assert len(records) == sum(len(b) for b in buckets) and {cid for cid, _ in records} == has
