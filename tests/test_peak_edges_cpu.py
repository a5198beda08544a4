"""CPU proof that the cases of tests/peak_edges.py carry what they are built for, so that test_gpu_peak_edges.py cannot
pass vacuously: block totals and their offsets inside a 16-byte unit around the writer's stage limit, buckets on the
seams of the 256-row blocks, runs of equal starts across a seam, starts with bits 30 and 29 set, keys of 64 and 65 bits,
the gc and amplitude domain of the device formatters, more row blocks than the scan has threads, the parser's line
edges.  Every figure is read off the model's text (peak_text.buckets / peak_text.ctg_rows, held to peak_text.model here)."""
import numpy as np
import pytest

import peak_edges as pe
import peak_text as pt
from gams_amd import host

N64, N65 = pe.width_ctg_counts()
WIDTH = ["width_%d" % N64, "width_%d" % N65]


@pytest.mark.parametrize("name", pe.SMALL_CASES + WIDTH)
def test_the_expected_text_is_the_models(name):
    """Expected puts peak_text.model's two halves together per ctg; in id order that is the model's text"""
    c, ex = pe.case(name), pe.expected(name)
    assert ex.by_id == pt.model(c["ctgs"], c["data"])
    assert ex.n_kept == ex.text.count(b"\n") == int(ex.bucket_off[-1]) and len(ex.text) == int(ex.text_off[-1])
    assert sorted(ex.text.split(b"\n")) == sorted(ex.by_id.split(b"\n"))


# ---- 1. the stage limit and its alignment --------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(pe.STAGE_CASES))
def test_stage_cases_hit_their_totals_and_residues(name):
    targets, tail, _ = pe.STAGE_CASES[name]
    ex = pe.expected(name)
    tot, blk0 = ex.block_totals(), ex.block_starts()
    assert ex.n_kept == pe.ROW_BLOCK * len(targets) + tail
    assert tot[:len(targets)].tolist() == targets and len(tot) == len(targets) + (tail > 0)
    assert len(ex.rows[0]) > 0 and len(ex.rows[1]) > 0                   # both ctgs have rows
    staged = tot <= pe.STAGE
    if name in pe.STAGE_SINGLE:
        assert len(tot) == 1 and blk0[0] == 0
        assert tot[0] == (pe.STAGE if name == "single_exact" else pe.STAGE + 1)
        return
    assert staged.any() and not staged.all()
    if name == "alternate":
        assert staged.tolist() == [True, False, True, False, True] and 0 < tail < pe.ROW_BLOCK
        assert tot[2] == pe.STAGE and tot[3] == pe.STAGE + 1 and blk0[2] % 16 != 0
        return
    kind, res = name.split("_r")
    assert blk0[1] % 16 == int(res) == tot[0] % 16                       # set with the bytes of the block in front
    if kind == "exact":
        assert tot[1] == pe.STAGE
    elif kind == "over":
        assert tot[1] == pe.STAGE + 1
    else:
        assert pe.STAGE - 64 < tot[1] < pe.STAGE


def test_stage_cases_cover_the_residues():
    seen = {}
    for name in pe.STAGE_CASES:
        if "_r" in name:
            kind, res = name.split("_r")
            seen.setdefault(kind, set()).add(int(res))
    assert all({0, 15} <= seen[k] for k in ("exact", "over", "under"))
    assert any(0 < r < 15 for s in seen.values() for r in s)
    # a row with a prefix and rows without in one block, and the prefix is the line's own: printed once
    ex = pe.expected("exact_r0")
    f = ex.fields()
    assert any(r[1].startswith("n") for r in f) and any(not r[1].startswith("n") for r in f[-100:])


# ---- 2. bucket and block seams ------------------------------------------------------------------------------------
def test_seam_cases_put_buckets_on_the_block_seams():
    first0 = last255 = single255 = single0 = between = 0
    totals = set()
    for name, (k, shuffled) in pe.SEAM_CASES.items():
        c, ex = pe.case(name), pe.expected(name)
        located, kept = pt.buckets(c["ctgs"], c["data"])                 # the ctgs are in the Locator's order here
        assert [x["id"] for x in ex.order] == [x["id"] for x in c["ctgs"]]
        assert located == pe.SEAM_LOCATED[k] and [len(b) for b in kept] == [max(m - 1, 0) for m in located]
        assert ex.n_kept == pe.SEAM_TOTALS[k]
        assert all(b"\n%s:%d\t" % (x["chr_id"].encode(), x["chr_start"]) in c["data"] for x in c["ctgs"])   # not located
        totals.add(ex.n_kept)
        off = np.concatenate(([0], np.cumsum([len(b) for b in kept])))
        full = [i for i, b in enumerate(kept) if b]
        for i in full:
            o0, o1 = int(off[i]), int(off[i + 1])
            first0 += o0 > 0 and o0 % pe.ROW_BLOCK == 0
            last255 += (o1 - 1) % pe.ROW_BLOCK == 255
            single255 += o1 - o0 == 1 and located[i] == 2 and o0 % pe.ROW_BLOCK == 255
            single0 += o1 - o0 == 1 and located[i] == 2 and o0 > 0 and o0 % pe.ROW_BLOCK == 0
        for a, b in zip(full, full[1:]):                                 # an empty bucket and a ctg without lines between
            gap = located[a + 1:b]
            between += 1 in gap and 0 in gap
        if ex.n_kept > 2:                                                # the file's order: by position, or not
            by_line = [sorted(b, key=lambda p: p[4]) for b in kept]
            assert all(p[0] <= q[0] for b in by_line for p, q in zip(b, b[1:])) != shuffled, name
    assert min(first0, last255, single255, single0, between) >= 1, (first0, last255, single255, single0, between)
    assert totals >= {1, 255, 256, 257, 513}


@pytest.mark.parametrize("name", ["n513_sorted", "n513_shuffled"])
def test_seam_cases_touch_the_ctg_ends_and_overlap(name):
    ex = pe.expected(name)
    on_start = on_end = 0
    for c, pk in zip(ex.order, ex.kept):
        on_start += any(p[0] == c["chr_start"] and p[1] > p[0] for p in pk)
        on_end += any(p[1] == c["chr_end"] for p in pk)
    assert on_start >= 2 and on_end >= 2
    f = ex.fields()
    assert any(int(r[5]) < 0 for r in f) and any(int(r[8]) < 0 for r in f)          # overlapping neighbours
    assert any(r[5] == "1" and r[6] == "0" for r in f)                               # the peak on chr_start: wave length 1
    assert {r[4] for r in f} >= {"1", "-1", ""}


# ---- 3. the sort key ----------------------------------------------------------------------------------------------
def test_tie_runs_cross_a_block_seam_in_line_order():
    ex = pe.expected("ties")
    pk = ex.kept[0]
    for start, tag in ((pe.TIE_A, "a"), (pe.TIE_B, "b")):
        idx = [k for k, p in enumerate(pk) if p[0] == start]
        assert len(idx) == pe.TIE_RUN >= 300 and idx == list(range(idx[0], idx[0] + pe.TIE_RUN))
        assert idx[0] // pe.ROW_BLOCK != idx[-1] // pe.ROW_BLOCK                     # the run crosses a row-block seam
        run = [pk[k] for k in idx]
        assert all(p[4] < q[4] for p, q in zip(run, run[1:]))                        # the model: by line number
        assert len({p[1] for p in run}) == pe.TIE_RUN and len({p[2] for p in run}) == pe.TIE_RUN
        assert all(p[2].startswith(tag) for p in run)
        gaps = [q[4] - p[4] for p, q in zip(run, run[1:])]
        if tag == "a":                                                               # scattered through the file ...
            assert max(gaps) > 1 and sum(g > 1 for g in gaps) > 100
            assert [int(p[2][1:]) for p in run] != sorted(int(p[2][1:]) for p in run)
        else:                                                                        # ... or next to each other
            assert set(gaps) == {1}


def test_high_starts_set_bits_30_and_29():
    ex = pe.expected("high")
    hi = ex.order.index(next(c for c in ex.order if c["chr_id"] == "H"))
    c, pk = ex.order[hi], ex.kept[hi]
    assert c["chr_end"] == 2_147_483_647 == pe.INT32_MAX and 20_000 <= len(c["seq"]) <= 99_000
    assert len(pk) >= 300 and all(p[0] >> 29 == 3 for p in pk)
    assert any(p[0] == c["chr_start"] for p in pk) and sum(p[1] == c["chr_end"] for p in pk) >= 2
    assert any(p[0] == p[1] == c["chr_end"] for p in pk)
    assert any(o["chr_start"] == 1 and k for o, k in zip(ex.order, ex.kept))         # beside a ctg at coordinate 1
    rows = [r for r in ex.fields() if r[0].startswith("peak:ctg:H:")]
    assert all(len(r[1].split(":")[1].split("-")[0]) == 10 for r in rows)            # ten digits in the range field
    assert rows[0][5] == "1" and rows[-1][8] == "1"                                  # both wave lengths at the ends


def test_key_width_cases_are_64_and_65_bits():
    for n_ctg, want in ((N64, 64), (N65, 65)):
        c, ex = pe.case("width_%d" % n_ctg), pe.expected("width_%d" % n_ctg)
        assert len(c["ctgs"]) == n_ctg > pe.SCAN_THREADS and pe.n_lines(c["data"]) == pe.WIDTH_LINES == 65_537
        line_bits, ctg_bits = pe.key_bits(pe.n_lines(c["data"]), n_ctg)
        assert ctg_bits + 31 + line_bits == want
        assert 200 <= c["n_peaks"] < 1000 and c["data"].count(b"#c\n") == pe.WIDTH_LINES - c["n_peaks"]
        with_rows = [i for i, r in enumerate(ex.rows) if r]
        assert with_rows == [0, n_ctg // 2, n_ctg - 1]                               # a low ctg, and the highest index
        assert (n_ctg - 1) >> (ctg_bits - 1) == 1 or want == 65                      # the key's top bit is set
        assert [c["slot"] for c in ex.order if c["slot"] is not None] == [0, 1, 2]
        assert all((c["slot"] is not None) == bool(r) for c, r in zip(ex.order, ex.rows))
        assert max(p[4] for pk in ex.kept for p in pk) == pe.WIDTH_LINES - 1         # the highest line number is kept
        assert ex.n_located[n_ctg // 2 + 1] == 1                                     # an empty bucket
        assert ex.text != ex.by_id                                                   # the ids sort otherwise


# ---- 4. the device formatters over their domain ---------------------------------------------------------------------
FMT_POW2_REACHED = 24        # of the 30 (k, below / at / above): no multiple of 10^-4 is 2^-5 .. 2^-10, so "at" ends at 2^-4


def test_fmt_case_covers_the_gc_and_amplitude_domain():
    ex = pe.expected("fmt")
    f = ex.fields()
    assert {r[3] for r in f} >= {host.fmt_f32(float(np.float32(m) / np.float32(1e4))) for m in range(10_001)}
    assert len({r[3] for r in f}) == 10_001
    # the model's amplitudes are fmt_f32 of the f32 differences of the printed gc values
    g, gp, gn = pe.amplitude_pairs(f)
    left, right = np.abs(g - gp), np.abs(g - gn)
    assert left.dtype == np.float32
    text = {}
    for v in np.unique(np.concatenate((left, right))):
        text[float(v)] = host.fmt_f32(float(v))
    assert [r[6] for r in f] == [text[float(v)] for v in left]
    assert [r[9] for r in f] == [text[float(v)] for v in right]
    amps = set(text.values())
    digits = [pt.sig_digits(a) for a in amps]
    print("amplitudes", len(amps), "with 9 digits", digits.count(9), "with 8", digits.count(8))
    assert len(amps) >= 2000 and digits.count(8) >= 500
    # Nine digits: the whole domain |fl(i / 10^4) - fl(j / 10^4)| holds only 443 distinct values that need them (399 in
    # [0.1, 0.125), 40 in [0.01, 0.015625), 4 just above 0.0001), so 500 distinct strings cannot be had from any input.
    # The case must hold 19 in 20 of those that exist, and 500 rows with one.
    fl = np.arange(10_001, dtype=np.float32) / np.float32(1e4)
    domain = np.unique(np.concatenate([np.unique(fl[d:] - fl[:-d]) for d in range(1, 10_001)]))
    nine = sum(pt.sig_digits(np.format_float_positional(x, unique=True, trim="-")) == 9 for x in domain)
    print("nine digits in the whole domain", nine)
    assert nine == 443 and digits.count(9) >= 0.95 * nine
    assert sum(pt.sig_digits(r[6]) == 9 for r in f) + sum(pt.sig_digits(r[9]) == 9 for r in f) >= 500
    vals = np.array(sorted(text), np.float64)
    assert "0" in amps and "1" in amps and ((vals > 0) & (vals < 1e-4)).any() and (vals > 0.5).any() and vals.max() == 1
    # Around the powers of two.  The values are differences of multiples of 10^-4, so "just" is one such step.
    reached = set()
    for k in range(1, 11):
        p = 2.0 ** -k
        if (vals == p).any():
            reached.add((k, "at"))
        if ((vals < p) & (vals >= p - 1.0001e-4)).any():
            reached.add((k, "below"))
        if ((vals > p) & (vals <= p + 1.0001e-4)).any():
            reached.add((k, "above"))
    print("powers of two reached", sorted(reached))
    assert len(reached) > 0
    assert {k for k, _ in reached} == set(range(1, 11))                  # every 2^-1 .. 2^-10 from one side at least
    assert len(reached) == FMT_POW2_REACHED


# ---- 5. more row blocks than the scan has threads -------------------------------------------------------------------
def test_big_case_has_more_row_blocks_than_the_scan_has_threads():
    text = pe.big_text()
    n = text.count(b"\n")
    assert n >= 262_145 and -(-n // pe.ROW_BLOCK) > pe.SCAN_THREADS
    assert len({r.split(b"\t")[0].rsplit(b":", 1)[0] for r in text.split(b"\n")[:-1:997]}) == 3     # three ctgs
    assert b"." not in text.split(b"\n")[5].split(b"\t")[1]                          # no prefixes


# ---- 6. line edges of peak_parse_kernel ---------------------------------------------------------------------------
def test_line_cases_say_what_they_mean():
    want = {k: pe.expected(k).text for k in pe.LINE_CASES}
    rows = {k: [r.split(b"\t") for r in t.split(b"\n")[:-1]] for k, t in want.items()}
    assert pe.LINE_CASES["cr_at_the_end"].endswith(b"\t1\r") and want["cr_at_the_end"].count(b"\t1\r") == 3
    assert len(rows["cr_at_the_end"]) == 3
    for k in ("empty_signal_in_a_line", "empty_signal_at_the_end"):
        assert [r[4] for r in rows[k]] == [b"-1", b"", b"x"] and rows[k][0][10] == b"" and rows[k][2][7] == b""
    assert pe.LINE_CASES["empty_signal_at_the_end"].endswith(b"0.1\t")
    assert want["empty_signal_in_a_line"] == want["empty_signal_at_the_end"]
    assert b"I:5-9 \t" in pe.LINE_CASES["padded_first_field"] and rows["padded_first_field"][1][1] == b"I:5-9"
    assert b"\n.I:5-9" in pe.LINE_CASES["empty_name"]
    assert [r[1] for r in rows["empty_name"]] == [b"m.I:1-3", b"I:5-9", b"I:50-60"]
    assert want["strand_and_reprinted_numbers"].decode().splitlines()[1:] == [
        "peak:ctg:I:1:2\tI:11\t1\t1\t\t3\t0.6\t1\t11\t0.5\t-1", "peak:ctg:I:1:3\ta.I:21-24\t4\t0.5\t-1\t11\t0.5\t\t977\t0\t-1"]
    assert pe.LINE_CASES["two_tabs"].count(b"\t\t\n") == 1 and pe.LINE_CASES["two_tabs"].endswith(b"\n\t\t")
    assert len(rows["two_tabs"]) == 2
    data = pe.efield_data()
    lines = data.split(b"\n")[:-1]
    assert len(lines) == 257 and all(len(ln.split(b"\t")) == 3 for ln in lines[:256]) and lines[256] == b"I:5-9\t0.1"
    with pytest.raises(pt.ModelError):
        pt.model(pe.line_ctgs(), data)
    assert pt.model(pe.line_ctgs(), data[:data.rindex(b"I:5-9")]).count(b"\n") == 255
