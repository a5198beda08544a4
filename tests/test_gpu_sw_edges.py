"""`gams sw` from the bytes of a feature file on the device at its edges: gams_gpu_sw_feature_text through the C ABI and
host.sw_text above it on the cases of tests/sw_edges.py, byte for byte against the pure-Python model
(tests/sw_text.py: the oracle's rows over the model's features).  test_sw_edges_cpu.py proves that the cases reach what
they are for: text blocks at, one under and one over the writer's 48-KB stage at every offset inside a 16-byte unit,
staged blocks behind unstaged ones; ctgs that begin on, one behind and one before the seams of the 512-row text
blocks, totals on a seam, empty intervals first, last and in runs; ctg boundaries on the seams of the 256-feature
workgroups, and more workgroups and text blocks than the offsets scan has threads; 255 to 600 intervals over a dozen
features; the middle check on its knife edge, the smallest of several offending lines; line and interval counts on
powers of two; windows of two bases, ctgs of 2 to 50 bases, serials of three and feature numbers of five digits;
the count action over the same inputs; two runs of one input."""
import re
import time

import numpy as np
import pytest

import sw_edges as se
import sw_text as swt
from gams_amd import _lib, engine, host
from test_gpu_sw_count import expected as oracle_rows
from test_gpu_sw_text import COUNT, GC, SwTables, abi_sw, in_id_order
from test_gpu_text_edges import first_difference

pytestmark = pytest.mark.gpu

L = _lib.load()


@pytest.fixture(scope="module")
def eng():
    e = engine.Engine(0)
    yield e
    e.close()


class Device:
    """the seqset (slot i holds ctgs[i]) and the tables of one case"""

    def __init__(self, eng, ctgs, rg_records=None):
        self.ss = engine.SeqSet(eng, [np.frombuffer(c["seq"], np.uint8) for c in ctgs])
        self.T = SwTables(eng, ctgs, rg_records=rg_records)

    def close(self):
        self.T.close()
        self.ss.close()


def check_entry(eng, name, with_host=False):
    """the entry's text is the model's, in the Locator's order; text_off slices it into the ctgs' rows, an interval
    without rows beginning where the next one does and the last entry being the text's length; in id order it is
    sw_text.model's text, which is what host.sw_text returns.  -> (text, text_off)"""
    c, ex = se.case(name), se.expected(name)
    d = Device(eng, c["ctgs"])
    try:
        rc, text, off, nf, rows = abi_sw(eng, d.T, d.ss, c["data"], *se.params(c))
        assert rc == 0, (name, rc, L.gams_gpu_last_error(eng.h).decode())
        assert [x["id"] for x in d.T.order] == [x["id"] for x in ex.order]
        assert text == ex.text, (name, first_difference(text, ex.text))
        assert (nf, rows) == (ex.n_features, ex.n_rows), name
        assert np.array_equal(off.astype(np.int64), ex.text_off), name
        assert int(off[-1]) == len(text)
        for i, part in enumerate(ex.parts):
            assert text[int(off[i]):int(off[i + 1])] == part, (name, ex.order[i]["id"])
        assert in_id_order(d.T, text, off) == ex.by_id
    finally:
        d.close()
    if with_host:
        got = host.sw_text(eng, c["ctgs"], c["data"], *se.params(c))
        assert host.last_operator_device() == 1, name
        assert got == ex.by_id, (name, first_difference(got, ex.by_id))
    return text, off


# ---- 1. the stage limit and its alignment --------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(se.STAGE_CASES))
def test_writer_blocks_at_the_stage_limit(eng, name):
    """sw_text_write_kernel with composed ids: a first block of kSwTextStage - 1, kSwTextStage (the last one staged) and
    kSwTextStage + 1 bytes (the first one written straight to global memory); the exact block 15 bytes into a 16-byte
    unit, which fills stage[] to its last byte but one; staged blocks behind an unstaged one; sixteen staged blocks at
    the sixteen offsets inside a 16-byte unit"""
    check_entry(eng, name)


# ---- 2. text block seams and empty intervals ------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(se.SEAM_CASES))
def test_ctgs_on_the_text_block_seams(eng, name):
    """sw_text_ctg_kernel: ctgs whose first row is row 0, 1 and 511 of a text block, totals of 4 blocks and of 2 blocks
    and a row, empty intervals (no line; one dropped line) first, last and in runs, one row in all: every text_off"""
    check_entry(eng, name, with_host=True)


# ---- 3. feature prefix seams ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(se.PREFIX_CASES))
def test_ctg_boundaries_on_the_feature_workgroup_seams(eng, name):
    """sw_geom_kernel / sw_row_off_kernel / sw_ctg_row_off_kernel: 255, 256, 257 and 513 kept features of 1 to 7 rows
    each, a ctg boundary between features 255 | 256 and 256 | 257"""
    check_entry(eng, name, with_host=True)


def test_more_feature_workgroups_and_text_blocks_than_the_scan_has_threads(eng):
    """262,148 kept features of 2 or 3 rows in 1,025 feature workgroups and more than 1,024 text blocks: a thread of
    blk_offsets_scan_kernel takes two, in the row prefix and in the text prefix.  The expected text is sw_text.model
    itself (some seconds on the CPU)."""
    c = se.case("big")
    want = se.big_text()
    t0 = time.perf_counter()
    got = host.sw_text(eng, c["ctgs"], c["data"], *se.params(c))
    print("host.sw_text of the big case: %.2f s, %d bytes" % (time.perf_counter() - t0, len(got)))
    assert host.last_operator_device() == 1
    assert got == want, first_difference(got, want)


# ---- 4. intervals beyond the features -------------------------------------------------------------------------------
@pytest.mark.parametrize("n", se.MANY_COUNTS)
def test_more_intervals_than_features(eng, n):
    """sw_gather_kernel's second index space: 255, 256, 257 and 600 intervals on up to six chromosomes over at most 14
    kept features in the first interval, intervals 255 and 256 and the last: igrp[] of an interval beyond the features'
    workgroup names the chromosome of its rows"""
    check_entry(eng, "many_%d" % n, with_host=True)


# ---- 5. the middle check --------------------------------------------------------------------------------------------
def refused_line(eng, d, data):
    """the line of the entry's GAMS_EINVAL message, which says `line N`"""
    rc, text, off, nf, rows = abi_sw(eng, d.T, d.ss, data, **se.PARAMS)
    assert rc == _lib.EINVAL and (text, rows) == (b"", 0)
    return L.gams_gpu_last_error(eng.h).decode()


def says_line(msg, n):
    return re.search(r"\bline %d\b" % n, msg) is not None


def test_middle_check_on_the_knife_edge(eng):
    """window.rs:98-110 in the gather: mid_l == chr_start and mid_r == chr_end are accepted, one base further refused,
    for odd and even lengths; a point on the last base, a feature over both ends, end < start; every refused line is
    accepted as the dropped first line of its ctg"""
    ctgs = se.middle_ctgs()
    c = ctgs[0]
    probes = dict(se.middle_probes(c))
    probes.update(se.MIDDLE_TABLE)
    d = Device(eng, ctgs)
    try:
        for line, ok in probes.items():
            data = se.probe_data(c, line)
            if ok:
                rc, text, off, nf, rows = abi_sw(eng, d.T, d.ss, data, **se.PARAMS)
                want = swt.interval_text(ctgs, data, **se.PARAMS)
                assert (rc, nf) == (0, 1) and text == want and rows == want.count(b"\n") > 0, line
            else:
                assert se.offenders(ctgs, data) == [2]
                assert says_line(refused_line(eng, d, data), 2), line
                with pytest.raises(host.HostError) as ei:
                    host.sw_text(eng, ctgs, data, **se.PARAMS)
                assert ei.value.code == _lib.EINVAL, line
                first = se.probe_data(c, line, first=True)
                rc, text, off, nf, rows = abi_sw(eng, d.T, d.ss, first, **se.PARAMS)
                assert (rc, nf) == (0, 1) and text == swt.interval_text(ctgs, first, **se.PARAMS), line
    finally:
        d.close()


def test_the_smallest_offending_line_is_reported(eng):
    """four offenders in three ctgs, the smallest line in the second ctg behind 300 kept features of the first: the
    atomicMin over lines, in two line orders, and behind comment, blank and \\r\\n lines"""
    ctgs = se.middle_ctgs()
    d = Device(eng, ctgs)
    try:
        for data in (se.offenders_data(), se.offenders_data(reverse=True), se.offenders_data(prefix=b"# c\n\n\r\n"),
                     se.offenders_data(reverse=True, prefix=b"\r\n" * 5)):
            bad = se.offenders(ctgs, data)
            assert len(bad) == 4
            msg = refused_line(eng, d, data)
            assert says_line(msg, bad[0]) and not any(says_line(msg, n) for n in bad[1:]), (msg, bad)
            with pytest.raises(host.HostError) as ei:
                host.sw_text(eng, ctgs, data, **se.PARAMS)
            assert ei.value.code == _lib.EINVAL
    finally:
        d.close()


def test_refusals_before_any_sw_launch(eng):
    """max beyond 2^24, and 16,385 features of 1 + 2^25 slots each: refused, never launched"""
    c = se.case("ids")
    cg = c["ctgs"][0]
    lines = [se.sacrificial(cg)] + [se.rng_line(cg, cg["chr_start"] + 1 + k % 10_000, cg["chr_start"] + 1 + k % 10_000)
                                    for k in range(16_385)]
    data = se.join_lines(lines)
    assert len(swt.buckets(c["ctgs"], data)[1][0]) == 16_385
    d = Device(eng, c["ctgs"])
    try:
        assert abi_sw(eng, d.T, d.ss, c["data"], 10, (1 << 24) + 1, 40)[0] == _lib.EUNSUPPORTED
        assert abi_sw(eng, d.T, d.ss, data, 10, 1 << 24, 40)[0] == _lib.EUNSUPPORTED
    finally:
        d.close()


# ---- 6. key decode --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lines,n_ctg", se.KEY_CASES)
def test_key_decode_at_powers_of_two(eng, lines, n_ctg):
    """key & line_mask and key >> popcount(line_mask) with 2, 3, 256, 257, 65,536 and 65,537 lines over 1 to 8
    intervals, the last line a kept feature of the last interval"""
    check_entry(eng, "key_%d_%d" % (lines, n_ctg))


# ---- 7. smallest geometries and widths ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", se.WIDTH_CASES)
def test_smallest_geometries_and_widest_fields(eng, name):
    """size 2 over point features (the M row a single base), ctgs of 2, 15, 16, 17 and 50 bases at size 2 and 100 (the
    NaN and -0 fields of a flank of no or one tile), serials up to 101, feature numbers up to 10,001"""
    check_entry(eng, name, with_host=True)


# ---- 8. -a count on the feature path --------------------------------------------------------------------------------
@pytest.mark.parametrize("actions", [("count",), ("gc", "count")])
@pytest.mark.parametrize("name", list(se.COUNT_CASES))
def test_count_over_the_seam_and_interval_cases(eng, name, actions):
    """the inputs of groups 2 and 4 with rg_count from an rg source over some chromosomes only, as records and as the
    bytes of the rg file; a ctg without rgs prints 0.  Expected: the oracle's rows with lapper_count in field 9"""
    c, ex = se.case(name), se.expected(name)
    rg_data, records = se.rg_source(c["ctgs"], se.COUNT_CASES[name])
    rgs = {}
    for cid, r in records:
        s, _, e = r.split(":")[1].partition("-")
        rgs.setdefault(cid, []).append((int(s), int(e or s)))
    feats = swt.features(c["ctgs"], c["data"])
    parts = {x["id"]: oracle_rows(x, f, rgs.get(x["id"]), actions, *se.params(c)).encode()
             for x, f in zip(c["ctgs"], feats)}
    by_id = b"".join(parts[k] for k in sorted(parts, key=lambda k: k.encode()))
    counts = [r.split(b"\t")[8] for r in by_id.split(b"\n")[:-1]]
    assert name == "single_row" or (b"0" in counts and any(v not in (b"", b"0") for v in counts))
    if "gc" in actions:                                                # all but field 9 are the gc rows
        assert [r.rsplit(b"\t", 1)[0] for r in by_id.split(b"\n")[:-1]] == [r.rsplit(b"\t", 1)[0] for r in ex.by_id.split(b"\n")[:-1]]
    got = host.sw_text(eng, c["ctgs"], c["data"], *se.params(c), actions=actions, rg_records=records)
    assert host.last_operator_device() == 1 and got == by_id, first_difference(got, by_id)
    got = host.sw_text(eng, c["ctgs"], c["data"], *se.params(c), actions=actions, rg_data=rg_data)
    assert host.last_operator_device() == 1 and got == by_id, first_difference(got, by_id)
    mask = (GC if "gc" in actions else 0) | COUNT
    d = Device(eng, c["ctgs"], rg_records=records)
    try:
        rc, text, off, nf, rows = abi_sw(eng, d.T, d.ss, c["data"], *se.params(c), actions=mask)
        assert rc == 0 and (nf, rows) == (ex.n_features, ex.n_rows)
        want = b"".join(parts[x["id"]] for x in ex.order)
        assert text == want, first_difference(text, want)
        lens = np.concatenate(([0], np.cumsum([len(parts[x["id"]]) for x in ex.order])))
        assert np.array_equal(off.astype(np.int64), lens)
    finally:
        d.close()


# ---- 9. determinism -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["exact", "second_exact_r15", "over_then_staged", "ladder", "many_600", "many_256"])
def test_two_runs_give_the_same_text_and_offsets(eng, name):
    text, off = check_entry(eng, name)
    text2, off2 = check_entry(eng, name)
    assert text == text2 and np.array_equal(off, off2)
