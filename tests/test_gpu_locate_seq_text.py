"""`locate --seq` from the bytes of a range file on the device: gams_gpu_locate_seq_text through the C ABI and
host.locate_seq_text above it, against the pure-Python model of tests/locate_seq_text.py, byte for byte.  The sequences
are random bytes over 0..255 (the copy must not interpret them); rows are steered onto the seams between the copy's chunks
with filler rows sized from gams_gpu_locate_seq_chunk()."""
import ctypes as C

import numpy as np
import pytest

import locate_seq_text as lst
from gams_amd import _lib, engine, host
from test_gpu_text_ops import LocTables, abi_locate, all_ctgs
from test_gpu_wave_plane import image_of
from test_rg_text_cpu import locator_order

pytestmark = pytest.mark.gpu

L = _lib.load()
NONE = 0xffffffff
STAGES = 6                 # lines parse locate lengths offsets copy
CHUNK = L.gams_gpu_locate_seq_chunk()


@pytest.fixture(scope="module")
def eng():
    e = engine.Engine(0)
    yield e
    e.close()


def seq_arrays(ctgs):
    return [np.frombuffer(c["seq"], np.uint8) for c in ctgs]


class SeqTables(LocTables):
    """LocTables and, per interval of the ctg index (the Locator's order), the seqset slot and the ctg's place"""

    def __init__(self, eng, ctgs, slots=None):
        super().__init__(eng, ctgs)
        self.order = locator_order(ctgs)
        slot_of = {c["id"]: (i if slots is None else slots[i]) for i, c in enumerate(ctgs)}
        self.slot = np.array([slot_of[c["id"]] for c in self.order], np.uint32)
        self.cs = np.array([c["chr_start"] for c in self.order], np.int32)
        self.ce = np.array([c["chr_end"] for c in self.order], np.int32)


@pytest.fixture(scope="module")
def world(eng):
    """the synthetic ctgs, resident once: (ctgs, seqset, tables)"""
    ctgs = lst.synth_ctgs()
    ss = engine.SeqSet(eng, seq_arrays(ctgs))
    T = SeqTables(eng, ctgs)
    yield ctgs, ss, T
    T.close()
    ss.close()


def abi_raw(eng, T, ss, data):
    """(rc, pointer, text_bytes, n_rows) of gams_gpu_locate_seq_text"""
    text, nb, rows = C.c_void_p(), C.c_uint64(77), C.c_uint64(77)
    rc = L.gams_gpu_locate_seq_text(eng.h, ss.p, T.ix, T.chr, T.slot.ctypes.data, T.cs.ctypes.data, T.ce.ctypes.data, data,
                                    len(data), C.byref(text), C.byref(nb), C.byref(rows))
    return rc, text, nb.value, rows.value


def abi_seq(eng, T, ss, data):
    """(rc, text, n_rows)"""
    rc, text, nb, rows = abi_raw(eng, T, ss, data)
    return rc, (C.string_at(text, nb) if rc == 0 and nb else b""), rows


def last_error(eng):
    return L.gams_gpu_last_error(eng.h)


def check(eng, world, data):
    """the entry against the model on `data`; -> the text"""
    ctgs, ss, T = world
    want = lst.model(ctgs, data)
    rc, text, rows = abi_seq(eng, T, ss, data)
    assert rc == 0, last_error(eng)
    assert len(text) == len(want)
    assert text == want
    assert rows == len(lst.records(ctgs, data))
    return text


def join(lines, end=b"\n"):
    return b"".join(ln + end for ln in lines)


# ---- goldens --------------------------------------------------------------------------------------------------------
def test_golden_lines(eng, s288c):
    ctgs = all_ctgs(s288c)
    rgs = ["I:1000-1002", "I:1000-1010", "II:1000-1100", "I(+):100001-100010", "garbage", "I:100001"]
    data = join(r.encode() for r in rgs[:2]) + b"I:1000-1002\tspo11\t0.5\n" + join(r.encode() for r in rgs[2:])
    got = host.locate_seq_text(eng, ctgs, data)
    assert host.last_operator_device() == 1
    assert got == lst.model(ctgs, data)
    rows = got.split(b"\n")[:-1]
    assert rows == [b">I:1000-1002", b"ATA", b">I:1000-1010", b"ATACAATTATA", b">I:1000-1002", b"ATA",
                    b">I(+):100001-100010", s288c["I"][100000:100010]]
    assert host.locate_seq_text(eng, ctgs, join(r.encode() for r in rgs)) == host.locate_seq(eng, ctgs, rgs).encode()
    assert host.last_operator_device() == 1
    with pytest.raises(host.HostError) as ei:                  # located to ctg:I:1, which ends at 100000
        host.locate_seq_text(eng, ctgs, b"I:5-9\nI:100000-100001\n")
    assert ei.value.code == _lib.EINVAL and "0-based line 1 " in str(ei.value)


# ---- the synthetic file ---------------------------------------------------------------------------------------------
def test_file_counts_determinism_stages_and_own_buffer(eng, world):
    ctgs, ss, T = world
    data = lst.synth_data(lst.synth_lines(ctgs))
    want = check(eng, world, data)
    assert len(want) > 20 * CHUNK
    rc, ptr, nb, rows = abi_raw(eng, T, ss, data)
    assert (rc, nb, rows) == (0, len(want), len(lst.records(ctgs, data))) and C.string_at(ptr, nb) == want
    ms = (C.c_float * 16)()
    n = C.c_uint32()
    assert L.gams_gpu_last_stage_ms(eng.h, ms, 16, C.byref(n)) == 0 and n.value == STAGES
    assert all(ms[k] >= 0 for k in range(STAGES))
    # another text entry in between leaves this entry's text alone
    rc2, text2, rows2 = abi_locate(eng, T, data)
    assert rc2 == 0 and rows2 == rows and text2
    assert C.string_at(ptr, nb) == want
    # the operator above it, on the resident seqset and with the sequences uploaded for the call
    assert host.locate_seq_text(eng, ctgs, data, seqset=ss) == want and host.last_operator_device() == 1
    assert host.locate_seq_text(eng, ctgs, data) == want and host.last_operator_device() == 1
    assert host.locate_seq_text(eng, ctgs, lst.synth_data(lst.synth_lines(ctgs), crlf=1.0, final_newline=True), seqset=ss) == want


def test_alignment_grid(eng, world):
    """all 16 x 16 of (source offset mod 16, destination offset mod 16): rows of 40 bases from chr_start + 0..15 of a slot
    that is not the seqset's first, each moved by a filler row in front"""
    ctgs, ss, T = world
    c = ctgs[1]
    off, _ = ss.layout()
    assert off[1] > 0 and off[1] % 16 == 0
    lines, pos, seen = [], 0, set()
    for a in range(16):
        for d in range(16):
            row = b"I:%d-%d" % (c["chr_start"] + a, c["chr_start"] + a + 39)
            bases_at = 1 + len(row) + 1                        # of the row's first base, from the row's start
            fill = 9 + (d - (pos + 9 + bases_at)) % 16
            lines += lst.filler(fill) + [row]
            pos += fill
            seen.add((a, (pos + bases_at) % 16))
            pos += lst.row_len(row)
    assert len(seen) == 256
    text = check(eng, world, join(lines))
    assert len(text) == pos > CHUNK


def test_long_rows(eng, world):
    ctgs, ss, T = world
    c = ctgs[1]
    whole = b"I:%d-%d" % (c["chr_start"], c["chr_end"])
    assert len(c["seq"]) > 2 * CHUNK
    text = check(eng, world, whole)                            # the row is the text: its first and its last byte
    assert len(text) > 2 * CHUNK + 16 and text[:1] == b">" and text[-1:] == b"\n" and text[-2] == c["seq"][-1]
    first, last = b"I:%d-%d" % (c["chr_start"], c["chr_start"] + 1), b"I:%d" % c["chr_end"]
    for lead in (13, CHUNK - 5, 3 * CHUNK - len(whole) - 3 - 17):
        text = check(eng, world, join(lst.filler(lead) + [whole, first, last, whole]))
        assert len(text) // CHUNK >= 4
    # every ctg whole, in one file
    check(eng, world, join(b"%s:%d-%d" % (x["chr_id"].encode(), x["chr_start"], x["chr_end"]) for x in ctgs))


def test_short_rows(eng, world):
    ctgs, ss, T = world
    points = [b"I:%d" % (2 + k % 7) for k in range(3000)]      # 7 bytes a row: more than 2,000 rows in a chunk
    assert CHUNK // 7 > 1024
    text = check(eng, world, join(points))
    assert len(text) == 7 * 3000
    mid = [b"III:%d-%d" % (100 + k, 130 + k) for k in range(300)]   # more than 256 rows in one chunk
    assert sum(map(lst.row_len, mid)) < CHUNK
    check(eng, world, join(mid))
    # the first row of a chunk begins on the chunk's first byte, on the last byte of the chunk in front, one byte before
    for lead in (CHUNK, CHUNK - 1, CHUNK - 2):
        text = check(eng, world, join(lst.filler(lead) + points[:40] + mid[:3]))
        assert text[lead:lead + 1] == b">"


def test_every_piece_seam_on_a_chunks_last_byte(eng, world):
    ctgs, ss, T = world
    row = b"II:1010-1049"
    rg, nb = len(row), 40
    # the byte of the row that is the last of '>', of rg, the '\n' behind rg, the last base, the final '\n'
    for last in (0, rg, rg + 1, rg + 1 + nb, rg + 2 + nb):
        lead = CHUNK - 1 - last
        data = join(lst.filler(lead) + [row, b"I:7-9"])
        text = check(eng, world, data)
        assert text[lead:lead + 1] == b">" and text[lead + 1:lead + 1 + rg] == row
        # ... and on the last byte of the second chunk, behind a row that covers the whole first one
        check(eng, world, join(lst.filler(CHUNK + 11) + lst.filler(lead - 11) + [row, b"I:7-9"]))


def test_runs_of_dropped_lines(eng, world):
    ctgs, ss, T = world
    dropped = [lst.DROPPED[k % len(lst.DROPPED)] for k in range(300)]
    rows = [b"I:5-9", b"nm.II(-):1002-1100", b"III:25003"]
    lines = dropped + rows[:1] + dropped + rows[1:2] + dropped + lst.filler(CHUNK - 300)
    lines += [b"I:100-140"] + dropped + [b"I:200-290"] + dropped + rows[2:] + dropped     # a run of them at the chunk seam
    text = check(eng, world, join(lines))
    assert CHUNK < len(text) < 2 * CHUNK and text.startswith(b">I:5-9\n")
    assert abi_seq(eng, T, ss, join(dropped + dropped)) == (0, b"", 0)
    # more lines in one chunk than the copy keeps offsets of in LDS: it searches them in global memory
    many = dropped * 9
    assert len(check(eng, world, join(rows[:1] + many + [b"I:100-140"] + many + rows[2:] + many))) < 100


def test_small_and_exact_sizes(eng, world):
    assert len(check(eng, world, b"I:5\n")) == 7               # texts shorter than 16 bytes
    assert len(check(eng, world, b"I:2-3")) == 10
    assert len(check(eng, world, b"I:5\nI:6\n")) == 14
    for total in (16, 160, CHUNK, 2 * CHUNK, CHUNK + 16, CHUNK - 16):
        assert len(check(eng, world, join(lst.filler(total)))) == total
    assert len(check(eng, world, join(lst.filler(CHUNK - 7) + [b"I:5"]))) == CHUNK


def test_input_line_edges(eng, world):
    data = b"nm.I(-):5-9\r\nI:7\tx\ty\r\n\r\nyy.II(+):1002\r\nIII:10_12 \r\nI:00300-400"      # CRLF, no final newline
    text = check(eng, world, data)
    assert text.startswith(b">nm.I(-):5-9\n") and b"\n>yy.II(+):1002\n" in text and b">III:10_12 \n" in text
    check(eng, world, data + b"\r")                            # a last line keeps its '\r'
    check(eng, world, data + b"\r\n")
    check(eng, world, b"\n\n" + data + b"\n\n")


def test_reversed_and_point_ranges(eng, world):
    ctgs, ss, T = world
    check(eng, world, b"I:500-500\nI:500\nI:30090-30050\n")    # the reversed one lies between the ctgs: not located
    assert len(lst.records(ctgs, b"I:30090-30050\n")) == 0
    with pytest.raises(lst.ModelError):                        # located, hence refused
        lst.model(ctgs, b"I:500\nI:2000-1000\n")
    assert abi_seq(eng, T, ss, b"I:500\nI:2000-1000\n")[0] == _lib.EINVAL
    assert b"0-based line 1 " in last_error(eng)


def test_slots_permuted(eng, world):
    ctgs, ss, T = world
    data = lst.synth_data(lst.synth_lines(ctgs, seed=29, n=300))
    want = lst.model(ctgs, data)
    perm = [3, 0, 4, 1, 2]                                     # ctgs[i] lies in slot perm[i]
    seqs = seq_arrays(ctgs)
    ss2 = engine.SeqSet(eng, [seqs[perm.index(k)] for k in range(5)])
    T2 = SeqTables(eng, ctgs, perm)
    try:
        assert abi_seq(eng, T2, ss2, data)[:2] == (0, want)
        assert host.locate_seq_text(eng, [dict(c, slot=perm[i]) for i, c in enumerate(ctgs)], data, seqset=ss2) == want
    finally:
        T2.close()
        ss2.close()


# ---- refusals -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [b"I:29990-30001",             # one base past chr_end
                                 b"I:30100-30110",             # from one base before chr_start, still overlapping
                                 b"II:13000-13001"])           # over a ctg boundary: located to the ctg in front
def test_ranges_that_leave_their_ctg(eng, world, bad):
    ctgs, ss, T = world
    ok = [b"I:5-9", b"garbage", b"II:2000-2100"]
    for data, line in ((join(ok + [bad]), 3), (join([bad] + ok), 0),
                       (join(ok + [bad, b"I:70100-70101"]), 3), (join(ok + [b"I:70100-70101", bad]), 3)):
        with pytest.raises(lst.ModelError) as ei:
            lst.model(ctgs, data)
        assert (ei.value.line, ei.value.outside) == (line, True)
        rc, ptr, nb, rows = abi_raw(eng, T, ss, data)
        assert (rc, nb, rows) == (_lib.EINVAL, 0, 0)
        assert b"0-based line %d " % line in last_error(eng)
    with pytest.raises(host.HostError) as ei:
        host.locate_seq_text(eng, ctgs, join(ok + [bad]), seqset=ss)
    assert ei.value.code == _lib.EINVAL


def test_slots_that_do_not_hold_their_ctg(eng, world):
    ctgs, ss, T = world
    only_i = b"I:5-9\nI:40000-40010\nIV:5\n"                    # nothing is located to chromosomes II and III
    want = lst.model(ctgs, only_i)
    for slots in ([0, 1, NONE, 2, NONE],                       # no slot; a slot of another length (ctg:II:2 in ctg:II:1's)
                  [0, 1, 3, 2, 77]):                           # ... and a slot the seqset does not have
        T2 = SeqTables(eng, ctgs, slots)
        try:
            assert abi_seq(eng, T2, ss, only_i)[:2] == (0, want)                  # a ctg no line is located to
            assert abi_seq(eng, T2, ss, only_i + b"II:14000\n")[0] == _lib.EINVAL
            assert b"slot" in last_error(eng)
            assert abi_seq(eng, T2, ss, b"III:100-200\n" + only_i)[0] == _lib.EINVAL
        finally:
            T2.close()
    with pytest.raises(host.HostError) as ei:
        host.locate_seq_text(eng, [dict(c, slot=None if c["chr_id"] == "III" else i) for i, c in enumerate(ctgs)],
                             b"III:100-200\n", seqset=ss)
    assert ei.value.code == _lib.EINVAL


def test_plane_only_seqset_is_estate(eng, world):
    ctgs, _, T = world
    seqs = seq_arrays(ctgs)
    ss = engine.SeqSet(eng, seqs, upload=False)
    try:
        off, img, plane = image_of(ss, seqs)
        ss.upload_ranges(None, plane, 0, int(off[-1]) + seqs[-1].size)
        assert abi_seq(eng, T, ss, b"I:5-9\n")[0] == _lib.ESTATE
        with pytest.raises(host.HostError) as ei:
            host.locate_seq_text(eng, ctgs, b"I:5-9\n", seqset=ss)
        assert ei.value.code == _lib.ESTATE
    finally:
        ss.close()


def test_refused_bytes_run_the_host_path(eng, world):
    _, ss, T = world
    ctgs = lst.synth_ctgs(ascii_only=True)                     # the host path goes through strings
    data = lst.synth_data(lst.synth_lines(ctgs, seed=41, n=200)) + b"\nI:5-9\tcaf\xc3\xa9\nna\xc3\xafve.I:5-9\n"
    rc, ptr, nb, rows = abi_raw(eng, T, ss, data)
    assert (rc, nb, rows) == (_lib.EUNSUPPORTED, 0, 0)          # nothing is printed
    want = lst.model(ctgs, data)
    assert want.endswith(b">I:5-9\n" + ctgs[0]["seq"][4:9] + b"\n>na\xc3\xafve.I:5-9\n" + ctgs[0]["seq"][4:9] + b"\n")
    assert host.locate_seq_text(eng, ctgs, data) == want and host.last_operator_device() == 0
    ss2 = engine.SeqSet(eng, seq_arrays(ctgs))
    try:
        assert host.locate_seq_text(eng, ctgs, data, seqset=ss2) == want and host.last_operator_device() == 0
        assert host.locate_seq_text(eng, ctgs, data.replace(b"\xc3", b"c").replace(b"\xa9", b"e").replace(b"\xaf", b"i"),
                                    seqset=ss2).startswith(want[:1000]) and host.last_operator_device() == 1
    finally:
        ss2.close()


def test_nothing_in_nothing_out(eng, world):
    ctgs, ss, T = world
    for data in (b"", b"\n", b"# ranges\nIV:5-9\nI:1\n"):
        assert abi_seq(eng, T, ss, data) == (0, b"", 0)
        assert host.locate_seq_text(eng, ctgs, data, seqset=ss) == b"" and host.last_operator_device() == 1
