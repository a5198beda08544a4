"""The device TSV writers beyond their LDS stage and at block seams: the `wave` peak rows (rows_*_kernel), the
`wave --signal` rows (sig_*_kernel), the `sw` rows (sw_text_*_kernel) and the `locate` rows (text_row_*_kernel), byte for
byte against the models of tests/text_edges.py and the oracle.  test_text_edges_cpu.py proves the models and shows that
the inputs used here reach what they are for: blocks beyond the stage (the branch that writes to global memory directly),
blocks within 64 bytes of `tot <= stage` on either side, staged blocks at every offset inside a 16-byte unit, more blocks
than the one-workgroup scans have threads, chains across block seams, every decimal width, a plan's rows set up again,
`--signal` rows of a single position, gc_content texts beyond 10 bytes."""
import numpy as np
import pytest

import text_edges as te
from gams_amd import _lib, engine
from oracle import oracle as ora

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = engine.Engine(0)
    yield e
    e.close()


def first_difference(got, exp):
    n = min(len(got), len(exp))
    a, b = np.frombuffer(got[:n], np.uint8), np.frombuffer(exp[:n], np.uint8)
    bad = np.flatnonzero(a != b)
    at = int(bad[0]) if bad.size else n
    lo = max(0, at - 60)
    return f"lengths {len(got)} / {len(exp)}, first difference at byte {at}: got {got[lo:at + 60]!r}, expected {exp[lo:at + 60]!r}"


def assert_text(text, off, parts, what):
    """the text per ctg slice and the offsets: off[0] == 0, off[-1] == len(text), an empty ctg begins where the next does"""
    off = [int(x) for x in off]
    assert len(off) == len(parts) + 1 and off[0] == 0 and off[-1] == len(text), (what, off[0], off[-1], len(text))
    for c, exp in enumerate(parts):
        got = text[off[c]:off[c + 1]]
        assert got == exp, (what, f"ctg {c}", first_difference(got, exp))
        if not exp:
            assert off[c] == off[c + 1]
    assert off == np.concatenate(([0], np.cumsum([len(p) for p in parts]))).tolist(), what


def assert_peaks(plan, peaks, what, windows=None):
    """the packed records against the oracle's (`windows`: per ctg, the window ranges to compare)"""
    got = plan.peaks()
    if windows is None:
        assert got.size == peaks.size, what
        for f in ("ctg", "window", "gc_count", "signal"):
            assert np.array_equal(got[f], peaks[f]), (what, f)
        return
    for c, spans in enumerate(windows):
        for lo, hi in spans:
            a = got[(got["ctg"] == c) & (got["window"] >= lo) & (got["window"] < hi)]
            b = peaks[(peaks["ctg"] == c) & (peaks["window"] >= lo) & (peaks["window"] < hi)]
            assert a.size == b.size and a.tobytes() == b.astype(_lib.PEAK_DTYPE).tobytes(), (what, c, lo, hi)


def rows_twice(plan, exp, what):
    """run, begin, end -- twice: the second pass takes the speculative copy, sized by the first"""
    for rep in range(2):
        plan.run()
        plan.rows_begin()
        text, off = plan.rows_end()
        assert_text(text, off, exp, (what, f"pass {rep}"))


# ---- the peak rows --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size,step", te.ROWS_CONFIGS)
def test_peak_rows_beyond_the_stage_and_at_its_limit(eng, size, step):
    """rows_write_kernel's branch without the stage (blocks of a ctg with a long name: beyond twice the stage where every
    record is a head, on both sides of it where chains merge), one block in (stage - 64, stage] and one in
    (stage, stage + 64], staged blocks at every offset inside a 16-byte unit; coordinates of 1 to 10 digits with ends a
    digit longer than their starts; an empty ctg between two others and at the end."""
    case = te.rows_case(size, step)
    ctgs = case["ctgs"]
    exp, _, _, _ = te.wave_rows_model(ctgs, case["peaks"], size, step)
    ss = engine.SeqSet(eng, [c["seq"] for c in ctgs])
    plan = engine.WavePlan(eng, ss, size, step, case["lag"], case["threshold"], 1.0, flags=_lib.WAVE_PEAKS)
    plan.rows_setup([c["chr_id"] for c in ctgs], [c["chr_start"] for c in ctgs], 0.2)
    rows_twice(plan, exp, (size, step))
    assert_peaks(plan, case["peaks"], (size, step))
    plan.close()
    ss.close()


def test_peak_rows_over_more_blocks_than_the_heads_scan_has_threads(eng):
    """556,061 records in 1,087 blocks: every thread of rows_heads_kernel carries its running maximum over two blocks, and
    tails in blocks without a head of their sign take their head from the blocks in front (rows_tail_kernel's `pre`)."""
    case = te.rows_big_case()
    ctgs, peaks = case["ctgs"], case["peaks"]
    assert peaks.size > te.SCAN_THREADS * te.ROWS_BLOCK
    exp, _, _, _ = te.wave_rows_model(ctgs, peaks, case["size"], case["step"])
    ss = engine.SeqSet(eng, [c["seq"] for c in ctgs])
    plan = engine.WavePlan(eng, ss, case["size"], case["step"], case["lag"], case["threshold"], 1.0, flags=_lib.WAVE_PEAKS)
    plan.rows_setup([c["chr_id"] for c in ctgs], [c["chr_start"] for c in ctgs], 0.2)
    rows_twice(plan, exp, "big")
    got = plan.peaks()
    assert got.size == peaks.size
    spans = []
    for c in range(len(ctgs)):
        n = case["per_ctg"][c][0].size
        spans.append([(0, 20_000), (n // 2 - 10_000, n // 2 + 10_000), (n - 20_000, n)])
    assert_peaks(plan, peaks, "big", spans)
    plan.close()
    ss.close()


def test_rows_set_up_again_on_one_plan(eng):
    """gams_wave_rows_setup with the plan's rows already set: short names, then names of 100 and 90 bytes and starts of ten
    digits (the text outgrows the speculative copy sized by the pass before AND the page-locked buffer: the buffer is
    replaced, the part already copied moves over, the rest follows), short names again, other coverages; a refused setup
    leaves the last one in force.  Size 4, step 1 (coverage 1.5 links only some of the overlapping windows there) over the
    590 kb of the big case: 2.5 MB of text with the short names, 12.7 MB with the long ones."""
    size, step = 4, 1
    seqs = [c["seq"] for c in te.rows_big_case()["ctgs"]]
    per = [te.oracle_windows(q, size, step, te.ROWS_LAG, te.ROWS_THR) for q in seqs]
    peaks = te.pack_peaks(per)
    base = [te.ctg(te.LONG_100, 1_999_000_001, seqs[0]), te.ctg(te.LONG_100[:90], 10 ** 9 - 150_000, seqs[1])]
    short = [te.ctg("0", 1, seqs[0]), te.ctg("1", 14, seqs[1])]
    exp_short = te.wave_rows_model(short, peaks, size, step)[0]
    exp_long = te.wave_rows_model(base, peaks, size, step)[0]
    n_short, n_long = sum(map(len, exp_short)), sum(map(len, exp_long))
    # The first text's page-locked buffer is asked for with 5/4 of the text + 4 KiB; the pool rounds up to 2 MiB and may
    # hand out a kept block of up to twice the request (4 MiB for small ones).  The long text must not fit any of that.
    first = n_short + n_short // 4 + 4096
    assert n_long > max(2 * first, 4 << 20) + (1 << 20), (n_short, n_long)
    ss = engine.SeqSet(eng, [c["seq"] for c in base])
    plan = engine.WavePlan(eng, ss, size, step, te.ROWS_LAG, te.ROWS_THR, 1.0, flags=_lib.WAVE_PEAKS)

    def setup(ctgs, coverage=0.2):
        plan.rows_setup([c["chr_id"] for c in ctgs], [c["chr_start"] for c in ctgs], coverage)

    setup(short)
    rows_twice(plan, exp_short, "short names")
    setup(base)
    rows_twice(plan, exp_long, "long names")
    setup(short)
    rows_twice(plan, exp_short, "short names again")
    setup(base, 1.0)
    rows_twice(plan, exp_long, "coverage 1.0")
    setup(short, 1.1)
    with pytest.raises(_lib.GamsError) as ei:
        setup(base, 1.5)
    assert ei.value.code == _lib.EUNSUPPORTED
    rows_twice(plan, exp_short, "after a refused setup")
    assert_peaks(plan, peaks, "set up again")
    plan.close()
    ss.close()


# ---- `wave --signal` -------------------------------------------------------------------------------------------------
def test_signal_rows_beyond_the_stage_and_other_names_on_one_plan(eng):
    """sig_write_kernel without the stage (a 100-byte name: tiles beyond twice the stage), tiles within 64 bytes of the limit
    on either side, ctgs of 256 and 257 windows and of no multiple of 256; three calls on one plan: short names, longer ones
    that fit the name table the first call sized, and the case's own, which need a new one."""
    case = te.signal_case()
    ctgs = case["ctgs"]
    kw = dict(size=case["size"], step=case["step"], lag=case["lag"], threshold=case["threshold"], influence=1.0)
    ss = engine.SeqSet(eng, [c["seq"] for c in ctgs])
    plan = engine.WavePlan(eng, ss, kw["size"], kw["step"], kw["lag"], kw["threshold"], 1.0, flags=_lib.WAVE_DENSE)
    plan.run()
    starts = [c["chr_start"] for c in ctgs]
    for names in te.signal_name_sets(case) + (te.signal_name_sets(case)[0],):
        text, off = plan.signal_text(names, starts)
        exp = [ora.wave_proc_ctg(nm, c["chr_start"], c["chr_end"], c["seq"], is_signal=True, **kw).encode()
               for nm, c in zip(names, ctgs)]
        assert_text(text, off, exp, ("signal", names[0]))
    plan.close()
    ss.close()


def signal_model_text(eng, case):
    """-> (text, offsets) of gams_wave_signal_text for the case, the rows of te.signal_rows_model per ctg"""
    ctgs, size, step = case["ctgs"], case["size"], case["step"]
    ss = engine.SeqSet(eng, [c["seq"] for c in ctgs])
    plan = engine.WavePlan(eng, ss, size, step, case["lag"], case["threshold"], 1.0, flags=_lib.WAVE_DENSE)
    plan.run()
    text, off = plan.signal_text([c["chr_id"] for c in ctgs], [c["chr_start"] for c in ctgs])
    exp = [te.signal_rows_model(c, *te.oracle_windows(c["seq"], size, step, case["lag"], case["threshold"]), size, step)[0]
           for c in ctgs]
    plan.close()
    ss.close()
    return text, off, exp


def test_signal_rows_of_a_single_position(eng):
    """size 1, step 1: every row's range is one position and prints without an end (sig_row's `e != s`), from coordinate 1
    and across 10^4 inside a tile"""
    text, off, exp = signal_model_text(eng, te.point_signal_case())
    assert_text(text, off, exp, "single positions")


def test_rows_with_gc_texts_beyond_ten_bytes(eng):
    """size 82: gc_content texts of 11 and 12 bytes from the table, in single and merged peak rows and in `--signal` rows"""
    case = te.gc_long_case()
    ctgs, size, step = case["ctgs"], case["size"], case["step"]
    exp, _, _, _ = te.wave_rows_model(ctgs, case["peaks"], size, step)
    ss = engine.SeqSet(eng, [c["seq"] for c in ctgs])
    plan = engine.WavePlan(eng, ss, size, step, case["lag"], case["threshold"], 1.0, flags=_lib.WAVE_PEAKS)
    plan.rows_setup([c["chr_id"] for c in ctgs], [c["chr_start"] for c in ctgs], 0.2)
    rows_twice(plan, exp, "long gc texts")
    plan.close()
    ss.close()
    text, off, exp = signal_model_text(eng, case)
    assert_text(text, off, exp, "long gc texts, --signal")


# ---- `sw` -----------------------------------------------------------------------------------------------------------
def build_index(eng, rgs_per_group):
    off = np.concatenate([[0], np.cumsum([len(g) for g in rgs_per_group])]).astype(np.uint64)
    st = np.array([s for g in rgs_per_group for s, _ in g], np.int64).astype(np.uint32)
    sp = np.array([e + 1 for g in rgs_per_group for _, e in g], np.int64).astype(np.uint32)
    return engine.Index(eng, off, st, sp)


@pytest.mark.parametrize("actions", te.SW_ACTIONS)
def test_sw_rows_beyond_the_stage_and_at_its_limit(eng, actions):
    """sw_text_write_kernel without the stage under every action set (with count alone only the names carry a block over
    it), one block in (stage - 64, stage] and one in (stage, stage + 64], a ctg without features in the middle and one
    at the end, serials and distances of two digits, coordinates that gain a digit."""
    case = te.sw_case(actions)
    ctgs = case["ctgs"]
    a = te.sw_arrays(case)
    ss = engine.SeqSet(eng, [c["seq"] for c in ctgs])
    ix = build_index(eng, case["rgs"]) if "count" in actions else None
    bits = (_lib.SW_GC if "gc" in actions else 0) | (_lib.SW_COUNT if "count" in actions else 0)
    rc, text, off = engine.sw_text_actions(eng, ss, a["sel"], a["names"], a["cst"], a["foff"], a["fs"], a["fe"], a["ids"],
                                           te.SW_SIZE, te.SW_MAX, te.SW_RESIZE, bits, ix, a["sel"] if ix else None)
    assert rc == _lib.OK, eng.lib.gams_gpu_last_error(eng.h).decode()
    assert_text(text, off, [b"".join(mine) for mine in case["rows"]], actions)
    if ix:
        ix.close()
    ss.close()


def test_sw_rows_over_more_blocks_than_the_offsets_scan_has_threads(eng):
    """524,800 rows in 1,025 blocks: a thread of blk_offsets_scan_kernel<uint32_t> sums two blocks"""
    case = te.sw_big_case()
    c = case["ctgs"][0]
    a = te.sw_arrays(case)
    ss = engine.SeqSet(eng, [c["seq"]])
    rc, text, off = engine.sw_text_actions(eng, ss, a["sel"], a["names"], a["cst"], a["foff"], a["fs"], a["fe"], a["ids"],
                                           te.SW_SIZE, te.SW_MAX, te.SW_RESIZE, _lib.SW_GC)
    assert rc == _lib.OK, eng.lib.gams_gpu_last_error(eng.h).decode()
    exp = ora.sw_proc_ctg(c["chr_id"], c["chr_start"], c["chr_end"], c["seq"], case["feats"][0], te.SW_SIZE, te.SW_MAX,
                          te.SW_RESIZE).encode()
    assert exp.count(b"\n") == 524_800 > te.SCAN_THREADS * te.SW_BLOCK
    assert_text(text, off, [exp], "sw big")
    ss.close()


# ---- `locate`, `locate --count` -----------------------------------------------------------------------------------------
def test_locate_text_with_long_fields(eng):
    """text_row_write_kernel (no stage) with range fields of up to 200 bytes and ctg ids of 40: every range lies inside one
    ctg, so the expected rows are known by construction; the counts come from the oracle."""
    from test_gpu_text_ops import LocTables, abi_locate

    rng = np.random.default_rng(13)
    chrs = ["7", te.LONG_B.replace(".", "_")]
    ctgs = []
    for chrom in chrs:
        pos = 1 if chrom == "7" else 999_990_000
        for k in range(6):
            ln = int(rng.integers(3000, 9000))
            cid = f"ctg:{chrom[:30]}:{k + 1}".ljust(40 if k % 2 else 9, "z")
            ctgs.append(dict(id=cid, chr_id=chrom, chr_start=pos, chr_end=pos + ln - 1, seq=b""))
            pos += ln + int(rng.integers(0, 500))
    recs, rg_of = [], {}
    for c in ctgs:
        a = rng.integers(c["chr_start"], c["chr_end"] + 1, 200)
        b = np.minimum(a + rng.choice([0, 0, 5, 300], 200), c["chr_end"])
        rg_of[c["id"]] = (np.sort(a.astype(np.uint32)), np.sort((b + 1).astype(np.uint32)))
        recs += [(c["id"], f"{c['chr_id']}:{x}-{y}") for x, y in zip(a, b)]
    lines, exp, exp_count = [], [], []
    for i in range(3000):
        c = ctgs[int(rng.integers(0, len(ctgs)))]
        s = int(rng.integers(c["chr_start"] + 1, c["chr_end"] - 40))
        e = s + int(rng.choice([0, 1, 30]))
        name = "n" * int(rng.choice([0, 1, 60, 130])) + "."
        rg = f"{name if len(name) > 1 else ''}{c['chr_id']}{'(+)' if i % 3 == 0 else ''}:{s}" + (f"-{e}" if e != s else "")
        lines.append(rg + ("\tx" * (i % 3)))
        exp.append(f"{rg}\t{c['id']}\n")
        exp_count.append(f"{rg}\t{ora.lapper_count(*rg_of[c['id']], s, e)}\n")
    assert max(len(x.split("\t")[0]) for x in lines) >= 180 and max(len(c["id"]) for c in ctgs) == 40
    data = ("\n".join(lines) + "\n").encode()
    T = LocTables(eng, ctgs, recs)
    try:
        rc, text, rows = abi_locate(eng, T, data)
        assert rc == 0 and rows == len(lines)
        assert text == "".join(exp).encode(), first_difference(text, "".join(exp).encode())
        rc, text, rows = abi_locate(eng, T, data, count=True)
        assert rc == 0 and rows == len(lines)
        assert text == "".join(exp_count).encode(), first_difference(text, "".join(exp_count).encode())
    finally:
        T.close()
