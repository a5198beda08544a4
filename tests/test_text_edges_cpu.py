"""The models and inputs of test_gpu_text_edges.py, proven on the CPU (tests/text_edges.py).

1. The linear model of the `wave` rows equals the oracle's text (merge_ints compares every pair of peaks, so the oracle
   only handles a few thousand peaks a sign), the model of the `--signal` rows likewise.
2. The inputs of the earlier GPU tests (test_gpu_host.py) keep every writer block inside its LDS stage, more than 64
   bytes below its limit: computed from the models.
3. The inputs of every new GPU case meet the conditions the case was made for: blocks beyond twice the stage, blocks on
   both sides of `tot <= stage` within 64 bytes, staged blocks at every offset inside a 16-byte unit, more blocks than
   the one-workgroup scans have threads, chains across block seams, every decimal width.
4. The `--signal` rows of single positions print no end, and the size-82 case carries gc texts of 11 and 12 bytes.
These are conditions on the inputs: when one fails, the input is changed, never the assertion."""
import numpy as np
import pytest

import helpers
import text_edges as te
from oracle import oracle as ora

# (size, step): dmax = ceil(size / step) - 1 of 0, 1, 2 and 9
GEOMETRIES = [(1, 1), (3, 3), (3, 2), (3, 1), (7, 7), (7, 4), (7, 3), (100, 100), (100, 50), (100, 34), (100, 10)]


def test_geometries_cover_the_distances():
    assert {-(-s // p) - 1 for s, p in GEOMETRIES} == {0, 1, 2, 9}
    assert {s for s, _ in GEOMETRIES} == {1, 3, 7, 100}


@pytest.mark.parametrize("coverage", [0.2, 1.0])
@pytest.mark.parametrize("thr", [2.0, -1.0])
@pytest.mark.parametrize("size,step", GEOMETRIES)
def test_rows_model_equals_the_oracle(size, step, thr, coverage):
    """text for text, per ctg: names of several lengths, starts that make the coordinates gain digits, a quiet ctg"""
    n_win = 2500 if thr < 0 else 30_000                      # at most about 3,000 peaks a sign and ctg
    lag = 4 if thr < 0 else 20
    ln = (n_win - 1) * step + size
    ctgs = [te.ctg(te.LONG_B, 10 ** 9 - 40 * step, helpers.synth(ln, 3)),
            te.ctg("quiet", 5, np.frombuffer(b"ACGT" * (ln // 8 + 30), np.uint8)),
            te.ctg("I", 1, helpers.synth(ln // 2 + 13, 4)),
            te.ctg("at", 9, np.frombuffer(b"AT" * (50 * step + size), np.uint8))]
    per = [te.oracle_windows(c["seq"], size, step, lag, thr) for c in ctgs]
    peaks = te.pack_peaks(per)
    for sgn in (1, -1):
        assert max(int(((peaks["ctg"] == c) & (peaks["signal"] == sgn)).sum()) for c in range(len(ctgs))) <= 3200
    assert peaks.size > 200
    text, is_head, row_bytes, _ = te.wave_rows_model(ctgs, peaks, size, step)
    for c, t in zip(ctgs, text):
        exp = ora.wave_proc_ctg(c["chr_id"], c["chr_start"], c["chr_end"], c["seq"], size, step, lag, thr, 1.0, coverage)
        assert t.decode() == exp, (c["chr_id"], size, step, thr, coverage)
    assert text[3] == b"" and int(row_bytes.sum()) == sum(len(t) for t in text)
    assert np.all((row_bytes > 0) == is_head)


@pytest.mark.parametrize("size,step", [(1, 1), (7, 3), (100, 10), (100, 150)])
def test_signal_model_equals_the_oracle(size, step):
    c = te.ctg(te.LONG_B, 10 ** 6 - 50 * step, helpers.synth(400 * step + size, 8))
    cnt, sig = te.oracle_windows(c["seq"], size, step, 4, -1.0)
    text, row_bytes = te.signal_rows_model(c, cnt, sig, size, step)
    exp = ora.wave_proc_ctg(c["chr_id"], c["chr_start"], c["chr_end"], c["seq"], size, step, 4, -1.0, 1.0, 0.2, True)
    assert text.decode() == exp and row_bytes.size == cnt.size


def test_block_totals():
    rb = np.arange(1, 1301)
    tot = te.block_totals(rb, 512)
    assert tot.tolist() == [rb[:512].sum(), rb[512:1024].sum(), rb[1024:].sum()]
    assert te.block_starts(tot).tolist() == [0, tot[0], tot[0] + tot[1]]
    assert te.block_totals(np.zeros(0), 512).size == 0
    assert (te.ROWS_BLOCK, te.SIG_BLOCK, te.ROWS_STAGE, te.SW_BLOCK, te.SW_STAGE) == (512, 256, 16384, 512, 49152)


# ---- 2. the existing tests stay inside the stage -------------------------------------------------------------------
def _all_ctgs(s288c, piece):
    ctgs = []
    for chr_id in ("I", "Mito"):
        ctgs += helpers.gen_ctgs(chr_id, s288c[chr_id], piece=piece)
    return ctgs


def test_the_existing_row_tests_never_leave_the_stage(s288c):
    """test_gpu_host.test_device_rows_golden_and_against_the_host_merge (its ragged ctgs, the geometries of its nine
    configurations) and test_signal_text_from_the_device_equals_the_oracle (its ctgs, its geometries at influence 1):
    no block of either writer is beyond the stage, none within 64 bytes of it"""
    quiet = dict(id="ctg:quiet:1", chr_id="quiet", chr_start=5, chr_end=5 + 4000 - 1, seq=b"ACGT" * 1000)
    named = dict(id="ctg:a-long_name.7:1", chr_id="a-long_name.7", chr_start=1_999_000_001, chr_end=1_999_000_001 + 25000 - 1,
                 seq=bytes(s288c["Mito"][:25000]))
    pieces = _all_ctgs(s288c, 30000)
    ragged = pieces[:5] + [quiet] + pieces[5:] + [named, quiet]
    worst = 0
    for size, step, lag, thr in [(100, 10, 100, 3.0), (100, 1, 100, 3.0), (100, 100, 20, 2.0), (100, 150, 20, 2.0), (50, 7, 33, 2.0),
                                 (1, 1, 50, 2.0), (100, 10, 100, -1.0), (100, 3, 40, 1.0)]:
        per = [te.oracle_windows(c["seq"], size, step, lag, thr) for c in ragged]
        _, _, rb, _ = te.wave_rows_model(ragged, te.pack_peaks(per), size, step, want_text=False)
        worst = max(worst, int(te.block_totals(rb, te.ROWS_BLOCK).max()))
    assert worst <= te.ROWS_STAGE - 64, worst
    ctgs = pieces[:4] + [quiet] + pieces[4:7] + [named]
    worst = 0
    for size, step, lag, thr in [(100, 10, 100, 3.0), (100, 1, 100, 3.0), (1, 1, 50, 2.0), (50, 7, 33, 2.5), (300, 10, 250, 3.0),
                                 (100, 150, 20, 3.0)]:
        for c in ctgs:
            cnt, sig = te.oracle_windows(c["seq"], size, step, lag, thr)
            _, rb = te.signal_rows_model(c, cnt, sig, size, step, want_text=False)
            worst = max(worst, int(te.block_totals(rb, te.SIG_BLOCK).max()))
    assert worst <= te.ROWS_STAGE - 64, worst


def test_the_existing_sw_text_test_never_leaves_the_stage(s288c):
    """test_gpu_host.test_sw_text_from_the_device_equals_the_host_formatter, input for input"""
    rng = np.random.default_rng(21)
    ctgs = _all_ctgs(s288c, 40000)[:6]
    ctgs[2] = dict(ctgs[2], chr_id="chr_with-a.long_name")
    worst = 0
    for size, mx, resize in ((100, 20, 500), (100, 3, 100), (50, 40, 1000), (7, 2, 7)):
        lens = []
        for i, c in enumerate(ctgs):
            n = 0 if i == 3 else int(rng.integers(1, 40))
            a = np.sort(rng.integers(c["chr_start"], c["chr_end"] + 1, n))
            a[:2] = [c["chr_start"], c["chr_end"]][:n]
            b = np.minimum(a + rng.choice([0, 1, 30, 600], n), c["chr_end"])
            feats = [(f"feature:{c['id']}:{j + 1}", int(x), int(y)) for j, (x, y) in enumerate(zip(a, b))]
            lens += [len(r) for r in te.sw_rows(c, feats, ("gc",), None, size, mx, resize)]
        worst = max(worst, int(te.block_totals(lens, te.SW_BLOCK).max()))
    assert worst <= te.SW_STAGE - 64, worst


# ---- 3. the inputs of the new GPU cases ------------------------------------------------------------------------------
def _assert_stage_conditions(reports, what):
    """per writer, over its cases: a block beyond twice the stage, one just below and one just above the limit, staged
    blocks at every offset inside a 16-byte unit"""
    assert sum(r["over_twice"] for r in reports) >= 1, what
    assert sum(r["just_below"] for r in reports) >= 1, what
    assert sum(r["just_above"] for r in reports) >= 1, what
    assert set().union(*(r["staged_mis"] for r in reports)) == set(range(16)), what


def _rows_reports():
    out = []
    for size, step in te.ROWS_CONFIGS:
        case = te.rows_case(size, step)
        text, _, rb, _ = te.wave_rows_model(case["ctgs"], case["peaks"], size, step)
        out.append((case, text, te.stage_report(te.block_totals(rb, te.ROWS_BLOCK), te.ROWS_STAGE)))
    return out


def test_peak_rows_inputs():
    got = _rows_reports()
    _assert_stage_conditions([r for _, _, r in got], "peak rows")
    for case, text, rep in got:
        # every configuration has blocks beyond the stage and one block within 64 bytes on either side of the limit
        assert rep["unstaged"] >= 1 and rep["just_below"] >= 1 and rep["just_above"] >= 1, (case["size"], case["step"], rep)
        assert case["landed"] == (True, True), (case["size"], case["step"])      # both seam blocks by construction
        assert text[-1] == b"" and len(case["ctgs"][-1]["seq"]) >= case["size"]        # an empty ctg at the end
        assert len(case["ctgs"][0]["chr_id"]) >= 40 and case["ctgs"][0]["chr_start"] == 1_999_000_001
        assert case["ctgs"][2]["chr_id"] == "I" and case["ctgs"][2]["chr_start"] == 1
    assert {-(-s // p) - 1 for s, p in te.ROWS_CONFIGS} >= {0, 2}
    # with dmax 0 every record is a head, and a ctg between two others is empty (size 10 over ACGT repeated)
    assert got[0][1][1] == b""
    assert any(b"(+):" in b"".join(t) for _, t, _ in got)


def test_peak_rows_big_input():
    case = te.rows_big_case()
    peaks = case["peaks"]
    assert peaks.size > te.SCAN_THREADS * te.ROWS_BLOCK == 524_288
    text, is_head, rb, chain_id = te.wave_rows_model(case["ctgs"], peaks, case["size"], case["step"])
    crossed, headless = te.chain_seams(is_head, chain_id, peaks)
    assert crossed >= 100 and headless >= 1, (crossed, headless)
    # the widths change inside both ctgs
    for t in text:
        ws, we, _ = te.range_widths(t)
        assert len(ws) >= 2 and len(we) >= 2
    assert 9 in te.range_widths(text[0])[2]                   # 999,999,99x-1,000,000,00x


def test_chain_seams_on_a_hand_made_case():
    """records 0..1535 of one ctg, three blocks: crests at every even window, troughs at every odd one.  At dmax 2 each
    sign is one chain over all three blocks, so both seams are crossed and the middle and the last block hold no head;
    at dmax 1 every record is a chain of its own"""
    n = 3 * te.ROWS_BLOCK
    peaks = np.zeros(n, te.PEAK)
    peaks["window"] = np.arange(n)
    peaks["signal"] = np.where(np.arange(n) % 2 == 0, 1, -1)
    c = [te.ctg("x", 1, helpers.synth(n + 20, 1))]
    _, is_head, _, chain_id = te.wave_rows_model(c, peaks, 3, 1, want_text=False)        # dmax 2: two chains in all
    assert int(is_head.sum()) == 2
    assert te.chain_seams(is_head, chain_id, peaks) == (2, 2)                            # block 1, for either sign
    _, is_head, _, chain_id = te.wave_rows_model(c, peaks, 2, 1, want_text=False)        # dmax 1: every record alone
    assert int(is_head.sum()) == n and te.chain_seams(is_head, chain_id, peaks) == (0, 0)


def test_signal_inputs():
    case = te.signal_case()
    per, tot = te.signal_blocks(case)
    _assert_stage_conditions([te.stage_report(tot, te.ROWS_STAGE)], "--signal")
    n_win = [rb.size for rb in per]
    assert n_win[0] % te.SIG_BLOCK and n_win[1] % te.SIG_BLOCK and n_win[2] == 256 and n_win[3] == 257
    assert len(case["ctgs"][0]["chr_id"]) in range(36, 49) and len(case["ctgs"][1]["chr_id"]) == 100
    te.signal_name_sets(case)                                 # (asserts the three blobs' sizes)


def _sw_reports():
    out = []
    for actions in te.SW_ACTIONS:
        case = te.sw_case(actions)
        flat = [r for mine in case["rows"] for r in mine]
        out.append((case, flat, te.stage_report(te.block_totals([len(r) for r in flat], te.SW_BLOCK), te.SW_STAGE)))
    return out


def test_sw_inputs():
    got = _sw_reports()
    _assert_stage_conditions([r for _, _, r in got], "sw")
    for case, flat, rep in got:
        # under every action set -- count alone included, where only the names carry a block over the stage
        assert rep["over_twice"] >= 1 and rep["just_below"] >= 1 and rep["just_above"] >= 1, (case["actions"], rep)
        assert case["landed"] == (True, True), case["actions"]                    # both tuned blocks by construction
        assert case["rows"][2] == [] and case["rows"][-1] == [] and case["rows"][-2] != []
        serial = max(int(r.split(b"\t", 1)[0].rsplit(b":", 1)[1]) for r in flat)
        dist = max(int(r.split(b"\t")[3]) for r in flat)
        assert serial >= 10 and dist >= 10
        if "count" in case["actions"]:
            assert max(int(r.rstrip(b"\n").rsplit(b"\t", 1)[1]) for r in flat) >= 10      # counts of two digits
    big = te.sw_big_case()
    c, feats = big["ctgs"][0], big["feats"][0]
    # 41 rows a feature: all of them are further than max * size from either end
    assert min(f[1] for f in feats) - c["chr_start"] > te.SW_MAX * te.SW_SIZE + te.SW_SIZE
    assert c["chr_end"] - max(f[2] for f in feats) > te.SW_MAX * te.SW_SIZE + te.SW_SIZE
    assert len(feats) * (1 + 2 * te.SW_MAX) >= 524_800 > te.SCAN_THREADS * te.SW_BLOCK


def test_digit_inputs():
    """per writer: starts and ends of 1 .. 10 digits, rows whose end has a digit more than their start at 10^k for several
    k, k = 9 among them; gc texts of 9 characters and more in the rows and the --signal rows"""
    texts = {"peak rows": b"".join(b"".join(t) for _, t, _ in _rows_reports())
             + b"".join(te.wave_rows_model(te.rows_big_case()["ctgs"], te.rows_big_case()["peaks"], te.BIG_SIZE, te.BIG_STEP)[0])}
    sc = te.signal_case()
    sig_text = []
    for c in sc["ctgs"]:
        cnt, sig = te.oracle_windows(c["seq"], sc["size"], sc["step"], sc["lag"], sc["threshold"])
        sig_text.append(te.signal_rows_model(c, cnt, sig, sc["size"], sc["step"])[0])
    texts["--signal"] = b"".join(sig_text)
    texts["sw"] = b"".join(r for mine in te.sw_case(("gc", "count"))["rows"] for r in mine)
    for what, text in texts.items():
        ws, we, longer = te.range_widths(text)
        assert ws == set(range(1, 11)) and we == set(range(1, 11)), (what, ws, we)
        assert 9 in longer and len(longer) >= 4, (what, longer)
    assert {"0.33333334", "0.14285715"} <= set(te.gc_texts(3)) | set(te.gc_texts(7))
    for what in ("peak rows", "--signal"):
        gcs = {len(r.split(b"\t")[1]) for r in texts[what].split(b"\n") if r}
        assert max(gcs) >= 9 and min(gcs) == 1, (what, gcs)


# ---- 4. single positions and long gc texts --------------------------------------------------------------------------
def test_point_signal_inputs():
    """size 1: no expected `--signal` row has a `-` in its range field; the coordinates gain a digit inside a tile"""
    case = te.point_signal_case()
    assert (case["size"], case["step"]) == (1, 1) and [c["chr_start"] for c in case["ctgs"]] == [1, 10 ** 4 - 1500]
    for c in case["ctgs"]:
        cnt, sig = te.oracle_windows(c["seq"], 1, 1, case["lag"], case["threshold"])
        text, rb = te.signal_rows_model(c, cnt, sig, 1, 1)
        kw = dict(size=1, step=1, lag=case["lag"], threshold=case["threshold"], influence=1.0)
        assert text.decode() == ora.wave_proc_ctg(c["chr_id"], c["chr_start"], c["chr_end"], c["seq"], is_signal=True, **kw)
        rows = text.split(b"\n")[:-1]
        assert len(rows) == cnt.size == c["seq"].size > 10 * te.SIG_BLOCK and cnt.size % te.SIG_BLOCK
        assert all(b"-" not in r.split(b"\t")[0] for r in rows)
        assert {r.split(b"\t")[2] for r in rows} == {b"-1", b"0", b"1"} and {r.split(b"\t")[1] for r in rows} == {b"0", b"1"}
    w = 10 ** 4 - case["ctgs"][1]["chr_start"]                     # the window at 10^4
    assert 0 < w % te.SIG_BLOCK < te.SIG_BLOCK - 1 and w < case["ctgs"][1]["seq"].size


def test_gc_long_inputs():
    """size 82: peak rows, single and merged, and `--signal` rows carry gc texts of 11 and 12 bytes"""
    case = te.gc_long_case()
    c, size, step = case["ctgs"][0], case["size"], case["step"]
    assert size <= 255 and max(len(t) for t in te.gc_texts(size)) == te.GC_LONG_BYTES > 10
    rows = te.wave_rows_model(case["ctgs"], case["peaks"], size, step)[0][0]
    exp = ora.wave_proc_ctg(c["chr_id"], c["chr_start"], c["chr_end"], c["seq"], size, step, case["lag"], case["threshold"], 1.0, 0.2)
    assert rows.decode() == exp
    sig = te.signal_rows_model(c, *case["per_ctg"][0], size, step)[0]
    for what, text in (("peak rows", rows), ("--signal", sig)):
        f = [r.split(b"\t") for r in text.split(b"\n")[:-1]]
        assert {len(r[1]) for r in f} >= {11, te.GC_LONG_BYTES}, what
        assert sum(len(r[1]) > 10 for r in f) >= 20, what
    long_rows = [r.split(b"\t") for r in rows.split(b"\n")[:-1] if len(r.split(b"\t")[1]) > 10]
    assert any(b"(+)" in r[0] for r in long_rows) and any(b"(+)" not in r[0] for r in long_rows)
