"""`gams peak` on the device at its edges: gams_gpu_peak_text through the C ABI on the cases of tests/peak_edges.py, byte
for byte against the pure-Python model (tests/peak_text.py).  test_peak_edges_cpu.py proves that the cases reach what
they are for: the row writer's blocks at, one over and just under its 32-KB stage at several offsets inside a 16-byte
unit, staged and unstaged blocks side by side; buckets that begin and end on the seams of the 256-row blocks; runs of
equal starts across a seam; starts with bits 30 and 29 set; keys of 64 and of 65 bits over more ctgs than the count scan
has threads; every round4 gc and the amplitudes' digits, zeros and powers of two through the formatters as compiled for
the device; more row blocks than the offsets scan has threads; the parser's own line edges."""
import numpy as np
import pytest

import peak_edges as pe
from gams_amd import _lib, engine, host
from test_gpu_peak_text import PeakTables, abi_peak, in_id_order
from test_gpu_text_edges import first_difference

pytestmark = pytest.mark.gpu

N64, N65 = pe.width_ctg_counts()


@pytest.fixture(scope="module")
def eng():
    e = engine.Engine(0)
    yield e
    e.close()


class Device:
    """the seqset and the tables of one case: the ctgs that have their bases at hand get the slots, in order"""

    def __init__(self, eng, ctgs):
        have = [c for c in ctgs if c["seq"]]
        slot_of = {c["id"]: k for k, c in enumerate(have)}
        self.ss = engine.SeqSet(eng, [np.frombuffer(c["seq"], np.uint8) for c in have])
        self.T = PeakTables(eng, ctgs, [slot_of.get(c["id"], pe.NONE) for c in ctgs])

    def close(self):
        self.T.close()
        self.ss.close()


def check_entry(eng, name, dev=None):
    """the entry's text is the model's, in the Locator's order; text_off slices it into the ctgs' rows, a ctg without
    rows beginning where the next one does; in id order it is peak_text.model's text"""
    c, ex = pe.case(name), pe.expected(name)
    d = dev or Device(eng, c["ctgs"])
    try:
        rc, text, off, rows = abi_peak(eng, d.T, d.ss, c["data"])
        assert rc == 0, (name, rc, eng.lib.gams_gpu_last_error(eng.h).decode())
        assert [x["id"] for x in d.T.order] == [x["id"] for x in ex.order]
        assert text == ex.text, (name, first_difference(text, ex.text))
        assert rows == ex.n_kept
        assert np.array_equal(off.astype(np.int64), ex.text_off), name
        for i, part in enumerate(ex.parts):
            assert text[int(off[i]):int(off[i + 1])] == part, (name, ex.order[i]["id"])
        assert in_id_order(d.T, text, off) == ex.by_id
    finally:
        if dev is None:
            d.close()


# ---- 1. the stage limit and its alignment --------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(pe.STAGE_CASES))
def test_writer_blocks_at_the_stage_limit(eng, name):
    """peak_row_write_kernel: a block of exactly kPeakStage bytes (the last one staged), of one byte more (the first one
    written straight to global memory) and of up to 63 bytes less, each beginning 0, 15 and some other number of bytes
    into a 16-byte unit; staged and unstaged blocks next to each other and a partial block at the end"""
    check_entry(eng, name)


# ---- 2. bucket and block seams ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(pe.SEAM_CASES))
def test_buckets_on_the_row_block_seams(eng, name):
    """peak_row's neighbour reads: a bucket's first row on slot 0 and its last on slot 255 of a block, buckets of one row
    on either, empty buckets and ctgs without lines between; 1, 255, 256, 257, 512 and 513 kept rows; peaks on chr_start
    and chr_end, overlapping neighbours; the same lines sorted by position and shuffled"""
    check_entry(eng, name)


# ---- 3. the sort key ----------------------------------------------------------------------------------------------
def test_runs_of_equal_starts_keep_the_order_of_the_file(eng):
    """300 lines with one start scattered through the file and 300 next to each other, each run across a block seam"""
    check_entry(eng, "ties")


def test_starts_at_the_top_of_the_range(eng):
    """a ctg that ends on 2,147,483,647 beside one at 1: bits 30 and 29 of the key's start, ten-digit coordinates"""
    check_entry(eng, "high")


def test_key_of_64_bits_answers_and_of_65_is_refused(eng):
    """65,537 lines over 65,535 ctgs: a key of 16 + 31 + 17 = 64 bits, kept peaks in the first ctg, a middle one and the
    last (the key's top bit), the count scan over more ctgs than it has threads, text_off for every ctg.  One ctg more
    and the key has 65 bits: GAMS_EUNSUPPORTED from the entry, the model's text from the operator's host passes.
    (The pure-Python model takes a few seconds for the two inputs; they are shared with the CPU test.)"""
    c = pe.case("width_%d" % N64)
    line_bits, ctg_bits = pe.key_bits(pe.n_lines(c["data"]), N64)
    assert ctg_bits + 31 + line_bits == 64 and sum(pe.key_bits(pe.n_lines(c["data"]), N65)) + 31 == 65
    check_entry(eng, "width_%d" % N64)
    c, ex = pe.case("width_%d" % N65), pe.expected("width_%d" % N65)
    d = Device(eng, c["ctgs"])
    try:
        rc, text, off, rows = abi_peak(eng, d.T, d.ss, c["data"])
        assert rc == _lib.EUNSUPPORTED and (text, rows) == (b"", 0) and not off.any()
        got = host.peak_text(eng, c["ctgs"], c["data"], seqset=d.ss)
        assert host.last_operator_device() == 0
        assert got == ex.by_id, first_difference(got, ex.by_id)
    finally:
        d.close()


# ---- 4. the device formatters over their domain ---------------------------------------------------------------------
def test_formatters_over_the_gc_and_amplitude_domain(eng):
    """sw_put_f4 on every m / 10^4 and gams_fmt_f32_short, as the amdgcn backend compiles it, on 6,800 distinct
    amplitudes: 0, 1, below 0.0001, above 0.5, around 2^-1 .. 2^-10, 3,500 of 8 and 432 of the domain's 443 of 9 digits"""
    check_entry(eng, "fmt")


# ---- 5. more row blocks than the scan has threads -------------------------------------------------------------------
def test_more_row_blocks_than_the_offsets_scan_has_threads(eng):
    """262,147 kept rows in 1,025 row blocks: a thread of blk_offsets_scan_kernel<unsigned long long> takes two.  The
    expected text is peak_text.model itself (about 5 s on the CPU), not a vectorised restatement."""
    c = pe.case("big")
    want = pe.big_text()
    got = host.peak_text(eng, c["ctgs"], c["data"])
    assert host.last_operator_device() == 1
    assert got == want, first_difference(got, want)


# ---- 6. line edges of peak_parse_kernel ---------------------------------------------------------------------------
def test_line_edges_of_the_parser(eng):
    """a last line that ends in \\r alone, an empty signal inside the input and at its end, a padded first field, an empty
    name, a strand and reprinted numbers, lines of two tabs; then a valid range with two fields behind 256 valid lines:
    W_EFIELD from a lane of the second workgroup"""
    d = Device(eng, pe.line_ctgs())
    try:
        for name in pe.LINE_CASES:
            check_entry(eng, name, d)
            got = host.peak_text(eng, pe.line_ctgs(), pe.LINE_CASES[name])
            assert got == pe.expected(name).by_id and host.last_operator_device() == 1, name
        rc, text, off, rows = abi_peak(eng, d.T, d.ss, pe.efield_data())
        assert rc == _lib.EINVAL and (text, rows) == (b"", 0)
        data = pe.efield_data()
        rc, text, off, rows = abi_peak(eng, d.T, d.ss, data[:data.rindex(b"I:5-9")])           # without it: 255 rows
        assert rc == 0 and rows == 255
    finally:
        d.close()
