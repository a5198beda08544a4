"""Models and input builders for the tests of the device TSV writers beyond their LDS stage and at block seams
(test_text_edges_cpu.py proves them on the CPU, test_gpu_text_edges.py runs the kernels on them).

The writers: the `wave` peak rows (rows_*_kernel), the `wave --signal` rows (sig_*_kernel), the `sw` rows
(sw_text_*_kernel).  Each puts a block's text together in an LDS stage and takes another branch when the block
does not fit.  Nothing here imports the GPU package, and the oracle is imported inside the functions that need it.
"""
import functools

import numpy as np

import helpers

ROWS_BLOCK = 512        # kRowsBlock: records per workgroup of rows_write_kernel (gams_amd/csrc/wave_rows.hpp)
SIG_BLOCK = 256         # kSigRows: windows of one ctg per workgroup of sig_write_kernel (wave_rows.hpp)
ROWS_STAGE = 16_384     # kRowsStage: the LDS stage of rows_write_kernel and sig_write_kernel (wave_rows.hpp)
SW_BLOCK = 512          # kSwTextBlock: rows per workgroup of sw_text_write_kernel (gams_amd/csrc/sw.hip)
SW_STAGE = 49_152       # kSwTextStage: the LDS stage of sw_text_write_kernel (sw.hip)
SCAN_THREADS = 1024     # threads of rows_heads_kernel (wave_rows.hpp) and blk_offsets_scan_kernel (text_emit.hpp):
                        # beyond SCAN_THREADS blocks a thread takes several

PEAK = np.dtype([("ctg", np.uint32), ("window", np.uint32), ("gc_count", np.uint32), ("signal", np.int32)])

LONG_A = "chrUn_scaffold-0042.a_long_name_".ljust(50, "a")            # 50 bytes
LONG_B = "chr_with-a.long_name.7_".ljust(44, "b")                     # 44 bytes
LONG_100 = "scaffold_".ljust(100, "c")                                # 100 bytes
assert (len(LONG_A), len(LONG_B), len(LONG_100)) == (50, 44, 100)

_P10 = 10 ** np.arange(1, 19, dtype=np.int64)


def ndigits(v):
    """decimal digits of every non-negative integer of v"""
    return np.searchsorted(_P10, np.asarray(v, np.int64), side="right") + 1


@functools.lru_cache(maxsize=None)
def gc_texts(size):
    """the text of k / size for k = 0 .. size, as the reference prints an f32"""
    from oracle import oracle as ora

    return tuple(ora.fmt_f32(float(np.float32(k) / np.float32(size))) for k in range(size + 1))


def ctg(chr_id, chr_start, seq, serial=1):
    seq = np.ascontiguousarray(seq, np.uint8) if isinstance(seq, np.ndarray) else np.frombuffer(seq, np.uint8)
    return dict(id=f"ctg:{chr_id}:{serial}", chr_id=chr_id, chr_start=int(chr_start), chr_end=int(chr_start) + seq.size - 1,
                seq=seq)


def n_windows(length, size, step):
    return (length - size) // step + 1 if length >= size else 0


# ---- the rows of `wave` ------------------------------------------------------------------------------------------
def oracle_windows(seq, size, step, lag, thr):
    """(gc_count, signal) of every window of one ctg, from the oracle (influence 1)"""
    from oracle import oracle as ora

    cnt, _, sig = ora.wave_windows(seq, size, step, lag, thr, 1.0)
    return cnt, sig


def pack_peaks(per_ctg):
    """[(gc_count, signal) per ctg] -> the packed peak records of a pass, ordered by (ctg, window)"""
    parts = []
    for c, (cnt, sig) in enumerate(per_ctg):
        idx = np.flatnonzero(sig)
        rec = np.zeros(idx.size, PEAK)
        rec["ctg"], rec["window"], rec["gc_count"], rec["signal"] = c, idx, cnt[idx], sig[idx]
        parts.append(rec)
    return np.concatenate(parts) if parts else np.zeros(0, PEAK)


def wave_rows_model(ctgs, peaks, size, step, want_text=True):
    """The TSV rows of packed peak records (ordered by ctg, window), in linear time.

    Windows of one size on a grid of `step` overlap iff they are at most dmax = ceil(size / step) - 1 windows apart, and
    for every coverage the device path accepts each overlap links; the reference merges crests and troughs separately.
    So, per sign, the records of a ctg in window order fall into chains that break where two neighbours are more than
    dmax apart.  A chain of one record prints "{chr}:{s}-{e}", a longer one prints once, at its first record, as
    "{chr}(+):{first s}-{last e}"; both carry the first record's gc_content and the sign ("s" alone when e == s).
    -> (row text per ctg [bytes] or None, is_head[n], row_bytes[n], chain_id[n]): a row's bytes stand at its head, and
    chain_id numbers the chains (per sign) so that a caller can tell which records one chain holds."""
    n = peaks.size
    dmax = -(-size // step) - 1
    pc, pw = peaks["ctg"].astype(np.int64), peaks["window"].astype(np.int64)
    ps, pk = peaks["signal"].astype(np.int64), peaks["gc_count"].astype(np.int64)
    is_head = np.zeros(n, bool)
    merged = np.zeros(n, bool)
    last_w = pw.copy()
    chain_id = np.zeros(n, np.int64)
    n_chains = 0
    for sgn in (1, -1):
        idx = np.flatnonzero(ps == sgn)
        if idx.size == 0:
            continue
        c, w = pc[idx], pw[idx]
        opens = np.ones(idx.size, bool)
        opens[1:] = (c[1:] != c[:-1]) | (w[1:] - w[:-1] > dmax)
        first = np.flatnonzero(opens)
        last = np.append(first[1:], idx.size) - 1
        is_head[idx[first]] = True
        merged[idx[first]] = last > first
        last_w[idx[first]] = w[last]
        chain_id[idx] = n_chains + np.cumsum(opens) - 1
        n_chains += first.size
    heads = np.flatnonzero(is_head)
    starts = np.array([c["chr_start"] for c in ctgs], np.int64)
    names = [c["chr_id"] for c in ctgs]
    name_len = np.array([len(x.encode()) for x in names], np.int64)
    gct = gc_texts(size)
    gc_len = np.array([len(t) for t in gct], np.int64)
    hc = pc[heads]
    s = starts[hc] + pw[heads] * step
    e = starts[hc] + last_w[heads] * step + size - 1
    row_bytes = np.zeros(n, np.int64)
    row_bytes[heads] = (name_len[hc] + 3 * merged[heads] + 1 + ndigits(s) + np.where(e != s, 1 + ndigits(e), 0) + 1
                        + gc_len[pk[heads]] + 1 + np.where(ps[heads] > 0, 1, 2) + 1)
    text = None
    if want_text:
        rows = [[] for _ in ctgs]
        for c, m, a, b, k, g in zip(hc.tolist(), merged[heads].tolist(), s.tolist(), e.tolist(), pk[heads].tolist(),
                                    ps[heads].tolist()):
            rng = f"{a}-{b}" if b != a else f"{a}"
            rows[c].append(f"{names[c]}{'(+)' if m else ''}:{rng}\t{gct[k]}\t{g}\n")
        text = [("".join(r)).encode() for r in rows]
        per_ctg = np.bincount(pc, weights=row_bytes, minlength=len(ctgs)).astype(np.int64)
        assert [len(t) for t in text] == per_ctg.tolist()          # the lengths and the text are one model
    return text, is_head, row_bytes, chain_id


def signal_rows_model(c, cnt, sig, size, step, want_text=True):
    """`wave --signal`: a row "{chr}:{s}-{e}\\t{gc_content}\\t{signal}\\n" for every window of ctg `c` (a dict)
    -> (text [bytes] or None, row_bytes per window)"""
    w = np.arange(cnt.size, dtype=np.int64)
    s = c["chr_start"] + w * step
    e = s + size - 1
    gct = gc_texts(size)
    gc_len = np.array([len(t) for t in gct], np.int64)
    sig = np.asarray(sig).astype(np.int64)
    row_bytes = (len(c["chr_id"].encode()) + 1 + ndigits(s) + np.where(e != s, 1 + ndigits(e), 0) + 1 + gc_len[cnt] + 1
                 + np.where(sig < 0, 2, 1) + 1)
    text = None
    if want_text:
        name = c["chr_id"]
        text = "".join(f"{name}:{a}-{b}\t{gct[k]}\t{g}\n" if b != a else f"{name}:{a}\t{gct[k]}\t{g}\n"
                       for a, b, k, g in zip(s.tolist(), e.tolist(), cnt.tolist(), sig.tolist())).encode()
        assert len(text) == int(row_bytes.sum())
    return text, row_bytes


def sw_rows(c, feats, actions, rgs=None, size=100, mx=20, resize=500):
    """The `sw` rows of one ctg as a list of byte strings (each with its newline): the oracle's text, field 9 filled with
    the oracle's count over the ctg's rgs [(start, end)] when "count" is among the actions (None: no rg group, 0), fields
    5-8 blanked when "gc" is not (data.rs:58-83) -- the model of test_gpu_sw_count.expected, row by row."""
    from oracle import oracle as ora

    if not feats:
        return []
    text = ora.sw_proc_ctg(c["chr_id"], c["chr_start"], c["chr_end"], c["seq"], feats, size, mx, resize)
    if "gc" in actions and "count" not in actions:
        return [r.encode() for r in text.splitlines(True)]
    st = np.sort(np.array([s for s, _ in rgs or []], np.int64)).astype(np.uint32)
    sp = np.sort(np.array([e + 1 for _, e in rgs or []], np.int64)).astype(np.uint32)
    rows = []
    for row in text.splitlines():
        f = row.split("\t")
        assert len(f) == 9 and f[8] == ""
        if "count" in actions:
            a, _, b = f[1].rsplit(":", 1)[1].partition("-")         # "{chr}:{start}[-{end}]"
            ws, we = int(a), int(b or a)
            f[8] = str(ora.lapper_count(st, sp, ws, we)) if rgs is not None else "0"
        if "gc" not in actions:
            f[4:8] = ["", "", "", ""]
        rows.append(("\t".join(f) + "\n").encode())
    return rows


def block_totals(row_bytes, block):
    """bytes of every writer block: `block` consecutive entries of row_bytes (the peak rows: records, a row counted at its
    head; `sw`: the rows of the batch; `--signal`: the windows of ONE ctg -- call it per ctg and concatenate)"""
    row_bytes = np.asarray(row_bytes, np.int64)
    if row_bytes.size == 0:
        return np.zeros(0, np.int64)
    return np.add.reduceat(row_bytes, np.arange(0, row_bytes.size, block))


def block_starts(totals):
    """where every block's text begins (blk0): the exclusive prefix of the totals"""
    return np.concatenate(([0], np.cumsum(totals)[:-1])).astype(np.int64) if len(totals) else np.zeros(0, np.int64)


def stage_report(totals, stage):
    """what the input conditions ask of one writer's blocks"""
    totals = np.asarray(totals, np.int64)
    blk0 = block_starts(totals)
    staged = (totals <= stage) & (totals > 0)
    return dict(over_twice=int((totals > 2 * stage).sum()), unstaged=int((totals > stage).sum()),
                just_below=int(((totals > stage - 64) & (totals <= stage)).sum()),
                just_above=int(((totals > stage) & (totals <= stage + 64)).sum()),
                exact=int((totals == stage).sum()), staged_mis=sorted(set((blk0[staged] & 15).tolist())))


def range_widths(text):
    """-> (digit counts of the starts, digit counts of the ends, digit counts k of the starts of rows whose end has k + 1
    digits: the range crosses 10^k) over the rows of a TSV text; the range "{chr}[(+)]:{s}[-{e}]" is field 1, field 2 of
    an `sw` row"""
    ws, we, longer = set(), set(), set()
    for row in text.split(b"\n"):
        if not row:
            continue
        f = row.split(b"\t")
        rng = f[1] if row.startswith(b"sw:") else f[0]
        span = rng.rsplit(b":", 1)[1]
        a, _, b = span.partition(b"-")
        ws.add(len(a))
        we.add(len(b or a))
        if b and len(b) == len(a) + 1:
            longer.add(len(a))
    return ws, we, longer


def crossing_ctgs(ks, length, seed, margin=100, prefix="d"):
    """short ctgs that start `margin` bases below 10^k: their coordinates gain a digit inside the ctg"""
    return [ctg(f"{prefix}{k}", 10 ** k - margin, helpers.synth(length, seed + k)) for k in ks]


# ---- peak rows: unstaged blocks and blocks near the limit ----------------------------------------------------------
ROWS_LAG, ROWS_THR = 4, -1.0          # every window from `lag` on whose z-score exists is a record
ROWS_CONFIGS = ((10, 10), (1, 1), (7, 3), (3, 1))        # (size, step): dmax 0, 0, 2, 2


def _seam_total(row_bytes, n_front, block=ROWS_BLOCK):
    """bytes of the block that holds record n_front (the first record behind a seam)"""
    b = n_front // block
    return int(row_bytes[b * block:(b + 1) * block].sum())


@functools.lru_cache(maxsize=None)
def rows_case(size, step):
    """One seqset for the peak rows at (size, step), lag 4, threshold -1:

      0  a long name at 1,999,000,001          its blocks are beyond the stage (beyond twice the stage when every record
                                                is a head); trimmed until the block it shares with ctg 2 ends up in
                                                (stage - 64, stage]
      1  quiet   ACGT repeated
      2  I at 1                                 short rows: staged blocks at many offsets inside a 16-B unit
      3  a long name below 10^9                 trimmed until the block it shares with ctg 4 is in (stage, stage + 64]
      4  II below 10^5
      5.. d6 d7 d8                              coordinates gaining a digit at 10^6, 10^7, 10^8
      -1 at      AT repeated: no G/C at all, no record for any size -- an empty ctg at the end

    -> dict(ctgs, per_ctg = [(gc_count, signal)] from the oracle, peaks = the packed records)"""
    rng_len = 40_000 if step >= 10 else 24_000
    # with dmax >= 1 about a quarter of the records are heads: the long names have 100 and 130 bytes there, so that the
    # blocks of their ctgs lie on both sides of the stage (no name of a sensible length takes them beyond twice the stage)
    dmax = -(-size // step) - 1
    long_a, long_b = (LONG_A, LONG_B) if dmax == 0 else (LONG_100, LONG_100.ljust(130, "d"))
    full = [ctg(long_a, 1_999_000_001, helpers.synth(rng_len, 11)),
            ctg("quiet", 5, np.frombuffer(b"ACGT" * 1000, np.uint8)),
            ctg("I", 1, helpers.synth(rng_len + 1777, 12)),
            ctg(long_b, 10 ** 9 - 30 * step - 7, helpers.synth(rng_len, 13)),
            ctg("II", 10 ** 5 - 100 * step - 3, helpers.synth(rng_len // 2 + 501, 14))]
    full += crossing_ctgs((6, 7, 8), 150 * step + size, 20, margin=20 * step + 1)
    full.append(ctg("at", 77, np.frombuffer(b"AT" * 700, np.uint8)))
    wins = [oracle_windows(c["seq"], size, step, ROWS_LAG, ROWS_THR) for c in full]

    def trimmed(cut):
        """the case with ctg k shortened to cut[k] windows (a window's verdict depends on the windows before it only)"""
        ctgs, per = [], []
        for k, (c, (cnt, sig)) in enumerate(zip(full, wins)):
            nw = cut.get(k, cnt.size)
            ln = (nw - 1) * step + size
            ctgs.append(ctg(c["chr_id"], c["chr_start"], c["seq"][:ln]) if nw < cnt.size else c)
            per.append((cnt[:nw], sig[:nw]))
        return ctgs, per

    def land(cut, k, lo, hi):
        """shorten ctg k, a window at a time, until the block that holds its seam with the next ctg totals in (lo, hi].
        Candidates come from the row bytes of the untrimmed ctg (prefix sums); each is then checked with the model,
        since cutting a chain changes the row of its head."""
        ctgs, per = trimmed(cut)
        peaks = pack_peaks(per)
        _, _, rb, _ = wave_rows_model(ctgs, peaks, size, step, want_text=False)
        csum = np.concatenate(([0], np.cumsum(rb)))
        win_k = peaks["window"][peaks["ctg"] == k].astype(np.int64)
        n_before = int((peaks["ctg"] < k).sum())
        behind = n_before + win_k.size                  # the first record behind ctg k
        full = wins[k][0].size
        for nw in range(full, max(full - 8 * ROWS_BLOCK, ROWS_LAG + 1), -1):
            n_front = n_before + int(np.searchsorted(win_k, nw))
            b0 = n_front // ROWS_BLOCK * ROWS_BLOCK
            if n_front == b0:
                continue
            room = ROWS_BLOCK - (n_front - b0)
            guess = csum[n_front] - csum[b0] + csum[min(behind + room, peaks.size)] - csum[behind]
            if not lo < guess <= hi:
                continue
            cut[k] = nw
            ctgs2, per2 = trimmed(cut)
            peaks2 = pack_peaks(per2)
            _, _, rb2, _ = wave_rows_model(ctgs2, peaks2, size, step, want_text=False)
            if lo < _seam_total(rb2, n_front) <= hi:
                return True
        cut.pop(k, None)
        return False

    cut = {}
    landed = (land(cut, 0, ROWS_STAGE - 64, ROWS_STAGE), land(cut, 3, ROWS_STAGE, ROWS_STAGE + 64))
    ctgs, per = trimmed(cut)
    return dict(ctgs=ctgs, per_ctg=per, peaks=pack_peaks(per), landed=landed, size=size, step=step, lag=ROWS_LAG,
                threshold=ROWS_THR)


# ---- peak rows: more than SCAN_THREADS blocks ---------------------------------------------------------------------
BIG_SIZE, BIG_STEP = 3, 1              # dmax 2


@functools.lru_cache(maxsize=None)
def rows_big_case():
    """Two ctgs at size 3, step 1 with more than SCAN_THREADS * ROWS_BLOCK records, so that a thread of rows_heads_kernel
    carries its running maximum over several blocks.  Chains of random sequence hold a few dozen records and cross many
    block seams; stretches of GA repeated give windows that alternate between two counts, hence crests and troughs that
    alternate, hence one chain of each sign over the whole stretch: blocks without a head of either sign.  The first ctg
    crosses 10^9 and has a 44-byte name, the second begins at 1."""
    ga = np.frombuffer(b"GA" * 2500, np.uint8)
    a = helpers.synth(300_000, 31).copy()
    b = helpers.synth(290_000, 32).copy()
    a[100_000:105_000] = ga
    a[299_000:300_000] = ga[:1000]                       # a chain that ends with its ctg
    b[0:5000] = ga                                       # ... and one that begins with it
    b[200_000:203_000] = ga[:3000]
    ctgs = [ctg(LONG_B, 10 ** 9 - 150_000, a), ctg("II", 1, b)]
    per = [oracle_windows(c["seq"], BIG_SIZE, BIG_STEP, ROWS_LAG, ROWS_THR) for c in ctgs]
    return dict(ctgs=ctgs, per_ctg=per, peaks=pack_peaks(per), size=BIG_SIZE, step=BIG_STEP, lag=ROWS_LAG, threshold=ROWS_THR)


def chain_seams(is_head, chain_id, peaks, block=ROWS_BLOCK):
    """-> (block seams that a chain crosses, blocks that lie inside one chain and hold no head of that chain's sign)"""
    n = peaks.size
    sig = peaks["signal"]
    crossed, headless = 0, 0
    seams = np.arange(block, n, block)
    for sgn in (1, -1):
        idx = np.flatnonzero(sig == sgn)
        # the last record of this sign in front of every seam and the first one behind it
        pos = np.searchsorted(idx, seams)
        ok = (pos > 0) & (pos < idx.size)
        same = np.zeros(seams.size, bool)
        same[ok] = chain_id[idx[pos[ok] - 1]] == chain_id[idx[pos[ok]]]
        crossed_s = same
        if sgn == 1:
            any_cross = crossed_s.copy()
        else:
            any_cross |= crossed_s
        # a block [s, s + block) with a chain across both its seams and no head of the sign inside
        heads_in = np.add.reduceat((is_head & (sig == sgn)).astype(np.int64), np.arange(0, n, block))
        for j in range(seams.size - 1):
            if same[j] and same[j + 1] and heads_in[j + 1] == 0:
                headless += 1
    crossed = int(any_cross.sum()) if seams.size else 0
    return crossed, headless


# ---- `wave --signal` -------------------------------------------------------------------------------------------------
SIG_SIZE, SIG_STEP = 7, 3


def _len_for(n_win, size, step):
    return (n_win - 1) * step + size


@functools.lru_cache(maxsize=None)
def signal_case():
    """One seqset for `wave --signal` at size 7, step 3, lag 4, threshold -1 (gc texts of up to 10 characters):

      0  a name of about 40 bytes near 10^5     rows of about 64 bytes: tiles on both sides of the stage.  The name's length
                                                and the ctg's start (where the coordinates gain a digit inside a tile: two
                                                bytes a row) are searched until one tile is in (stage - 64, stage] and one
                                                in (stage, stage + 64]
      1  LONG_100 at 1,999,000,001              tiles beyond twice the stage; 1,000 windows (no multiple of 256)
      2  quiet, exactly 256 windows
      3  I at 1, exactly 257 windows
      4.. d4 .. d9                              coordinates gaining a digit at 10^4 .. 10^9
    (a plan takes no ctg with fewer than `lag` windows, so `--signal` has no ctg without rows)"""
    size, step = SIG_SIZE, SIG_STEP
    seq0 = helpers.synth(_len_for(40 * SIG_BLOCK + 77, size, step), 41)
    cnt0, sig0 = oracle_windows(seq0, size, step, ROWS_LAG, ROWS_THR)
    found = None
    for name_len in range(36, 49):
        for start in range(10 ** 5 - 3 * 256 * 38, 10 ** 5, 3 * 5):
            c0 = ctg(LONG_100[:name_len], start, seq0)
            _, rb = signal_rows_model(c0, cnt0, sig0, size, step, want_text=False)
            rep = stage_report(block_totals(rb, SIG_BLOCK), ROWS_STAGE)
            if rep["just_below"] and rep["just_above"] and len(rep["staged_mis"]) == 16:
                found = c0
                break
        if found:
            break
    assert found is not None, "no name length / start puts --signal tiles on both sides of the stage"
    ctgs = [found,
            ctg(LONG_100, 1_999_000_001, helpers.synth(_len_for(1000, size, step), 42)),
            ctg("quiet", 5, np.frombuffer(b"ACGT" * 1000, np.uint8)[:_len_for(256, size, step)]),
            ctg("I", 1, helpers.synth(_len_for(257, size, step) + 2, 43))]
    ctgs += crossing_ctgs((4, 5, 6, 7, 8, 9), _len_for(150, size, step), 50, margin=61)
    return dict(ctgs=ctgs, size=size, step=step, lag=ROWS_LAG, threshold=ROWS_THR)


def signal_blocks(case):
    """-> (row_bytes per ctg, the totals of all tiles in the writer's order)"""
    per, tot = [], []
    for c in case["ctgs"]:
        if c["seq"].size < case["size"]:
            per.append(np.zeros(0, np.int64))
            continue
        cnt, sig = oracle_windows(c["seq"], case["size"], case["step"], case["lag"], case["threshold"])
        _, rb = signal_rows_model(c, cnt, sig, case["size"], case["step"], want_text=False)
        per.append(rb)
        tot.append(block_totals(rb, SIG_BLOCK))
    return per, np.concatenate(tot)


def signal_name_sets(case):
    """three name lists for three gams_wave_signal_text calls on one plan: short names (a blob of a few bytes, so the call
    sizes its name table at 128 bytes), longer ones whose blob still fits 128 bytes, and the case's own, which do not"""
    n = len(case["ctgs"])
    short = [f"{k}" for k in range(n)]
    medium = [f"chr{k:02d}_{'m' * 5}" for k in range(n)]
    full = [c["chr_id"] for c in case["ctgs"]]
    assert len("".join(short)) <= 64 < len("".join(medium)) <= 128 < len("".join(sorted(set(full))))
    return short, medium, full


# ---- single positions, and gc texts beyond 10 bytes -------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def point_signal_case():
    """`wave --signal` at size 1, step 1, lag 4, threshold -1: every window is one position, so every row prints "{chr}:{s}"
    without an end (IntSpan's runlist of a single position).  I at 1, and d4 across 10^4 inside a tile of 256 windows.  (A
    plan takes no ctg with fewer than `lag` windows: there is no ctg without rows to put between them.)"""
    ctgs = [ctg("I", 1, helpers.synth(3001, 91)), ctg("d4", 10 ** 4 - 1500, helpers.synth(2777, 92))]
    return dict(ctgs=ctgs, size=1, step=1, lag=ROWS_LAG, threshold=ROWS_THR)


# The first size up to 255 whose gc text table holds the longest text found among those sizes, and that text's bytes
# ("0.0121951215" = 1 / 82; test_peak_text_cpu.py finds both with the formatter's driver).  The counts 1, 2, 3, 4 and 7 of
# that table have texts of 11 and 12 bytes.
GC_LONG_SIZE, GC_LONG_BYTES = 82, 12
GC_LONG_STEP = 41                      # dmax 1: single rows and merged ones


@functools.lru_cache(maxsize=None)
def gc_long_case():
    """One ctg of 20 kb for the peak rows and the `--signal` rows at size 82: the second half is A / T with a G or a C
    every 12 to 80 bases, so that its windows hold the few G/C whose gc_content text is longer than 10 bytes."""
    rng = np.random.default_rng(93)
    seq = helpers.synth(20_000, 94).copy()
    poor = np.where(rng.random(10_000) < 0.5, ord("A"), ord("T")).astype(np.uint8)
    at = np.cumsum(rng.integers(12, 81, 400))
    at = at[at < poor.size]
    poor[at] = np.where(rng.random(at.size) < 0.5, ord("G"), ord("c"))
    seq[10_000:] = poor
    c = ctg(LONG_B, 10 ** 6 - 9000, seq)
    per = [oracle_windows(seq, GC_LONG_SIZE, GC_LONG_STEP, ROWS_LAG, ROWS_THR)]
    return dict(ctgs=[c], per_ctg=per, peaks=pack_peaks(per), size=GC_LONG_SIZE, step=GC_LONG_STEP, lag=ROWS_LAG,
                threshold=ROWS_THR)


# ---- `sw` ---------------------------------------------------------------------------------------------------------
SW_SIZE, SW_MAX, SW_RESIZE = 10, 20, 50
SW_ACTIONS = (("gc",), ("count",), ("gc", "count"))


def _sw_feats(rng, c, n, id_of, edge=True):
    s = np.sort(rng.integers(c["chr_start"] + 30, c["chr_end"] - 30, n))
    ln = rng.choice([0, 0, 1, 7, 40], n)
    if edge and n >= 2:
        s[0], s[-1] = c["chr_start"], c["chr_end"]
        ln[0] = ln[-1] = 0
    return [(id_of(j), int(a), int(min(a + b, c["chr_end"]))) for j, (a, b) in enumerate(zip(s, ln))]


def _sw_batch_rows(ctgs, feats, rgs, actions):
    """-> (rows per ctg, per row of the batch: its ctg, per row: its feature's index inside the ctg)"""
    rows, row_ctg, row_feat = [], [], []
    for k, c in enumerate(ctgs):
        mine = sw_rows(c, feats[k], actions, rgs[k], SW_SIZE, SW_MAX, SW_RESIZE)
        rows.append(mine)
        # the serial restarts with every feature
        first = np.array([r.split(b"\t", 1)[0].endswith(b":1") for r in mine], bool)
        row_ctg.append(np.full(len(mine), k))
        row_feat.append(np.cumsum(first) - 1)
    return rows, np.concatenate(row_ctg), np.concatenate(row_feat)


@functools.lru_cache(maxsize=None)
def sw_case(actions):
    """One batch for gams_gpu_sw_text_actions at size 10, max 20, resize 50 under the action set `actions`:

      0  LONG_100 at 1,999,000,001, ids of 100 bytes      blocks beyond twice the stage under every action set
      1  medium names below 10^9                          rows near 96 bytes (the ids' length is derived from the rows'
                                                           measured mean); the ids of the features of ONE block are then
                                                           lengthened a byte at a time -- a feature's 41 rows move the
                                                           block by 41 bytes, less than the 64-byte window -- until the
                                                           block is in (stage - 64, stage]
      2  a ctg without features
      3  I at 1, ids of 1 to 3 bytes
      4  medium names below 10^5                          as ctg 1, into (stage, stage + 64]
      5  names and ids of about 40 bytes
      6.. d6 d7 d8                                        coordinates gaining a digit
      -1 a ctg without features, at the end

    -> dict(ctgs, feats [per ctg: (id, start, end)], rgs [per ctg: (start, end)], rows [per ctg: list of bytes])"""
    rng = np.random.default_rng(5)
    ctgs = [ctg(LONG_100, 1_999_000_001, helpers.synth(6000, 61)),
            ctg("chrM1", 10 ** 9 - 2500, helpers.synth(9000, 62)),
            ctg("none", 400, helpers.synth(2000, 63)),
            ctg("I", 1, helpers.synth(12000, 64)),
            ctg("chrM2", 10 ** 5 - 2500, helpers.synth(9000, 65)),
            ctg(LONG_B, 10 ** 4 - 700, helpers.synth(5000, 66))]
    ctgs += crossing_ctgs((6, 7, 8), 3000, 70, margin=1000)
    ctgs.append(ctg("last", 1, helpers.synth(1500, 67)))
    n_feat = [40, 100, 0, 250, 100, 40, 12, 12, 12, 0]
    id_of = [lambda j: f"feature:{LONG_100[:80]}:{j + 1:011d}", None, None, lambda j: f"f{j % 100}", None,
             lambda j: f"feature:ctg:{LONG_B[:24]}:{j + 1}"] + [lambda j: f"d:{j}"] * 3 + [None]
    rgs = []
    for c in ctgs:
        p = rng.integers(c["chr_start"], c["chr_end"] + 1, c["seq"].size // 2)
        ln = rng.choice([0, 0, 0, 3, 60], p.size)
        dense = c["chr_start"] + 500 + rng.integers(0, 40, 150)          # counts of two digits
        rgs.append([(int(a), int(a + b)) for a, b in zip(p, ln)] + [(int(a), int(a)) for a in dense])
    base = {}
    for k in (1, 4):                                    # the medium ctgs: ids of 20 bytes first, to measure the rows
        base[k] = _sw_feats(np.random.default_rng(100 + k), ctgs[k], n_feat[k], lambda j: "x" * 20, edge=False)

    def build(id_len):
        feats = []
        for k, c in enumerate(ctgs):
            if n_feat[k] == 0:
                feats.append([])
            elif k in base:
                feats.append([(f"{j:03d}".ljust(id_len[k][j], "y"), a, b) for j, (_, a, b) in enumerate(base[k])])
            else:
                feats.append(_sw_feats(np.random.default_rng(100 + k), c, n_feat[k], id_of[k]))
        return feats

    # the rows once with 20-byte ids on the medium ctgs; from there a byte of id is a byte of each row of its feature, so
    # the search runs on the lengths and the text is made once more at the end
    id_len = {k: np.full(n_feat[k], 20) for k in base}
    rows, row_ctg, row_feat = _sw_batch_rows(ctgs, build(id_len), rgs, actions)
    len20 = np.array([len(r) for mine in rows for r in mine], np.int64)

    def lengths():
        out = len20.copy()
        for k in base:
            sel = row_ctg == k
            out[sel] += id_len[k][row_feat[sel]] - 20
        return out

    for k in base:                                      # ids so long that the ctg's rows average stage / block bytes
        mean = len20[row_ctg == k].mean()
        id_len[k][:] = max(3, 20 + int(round(SW_STAGE / SW_BLOCK - mean)))
    landed = []
    for k, (lo, hi) in ((1, (SW_STAGE - 64, SW_STAGE)), (4, (SW_STAGE, SW_STAGE + 64))):
        first = int((row_ctg < k).sum())
        b = first // SW_BLOCK + 2                       # a block of ctg k's rows alone
        assert (b + 1) * SW_BLOCK <= first + int((row_ctg == k).sum())
        per_feat = np.bincount(row_feat[row_ctg == k], minlength=n_feat[k])
        in_blk = np.bincount(row_feat[b * SW_BLOCK:(b + 1) * SW_BLOCK], minlength=n_feat[k])
        whole = np.flatnonzero((in_blk == per_feat) & (per_feat > 0))       # features with all their rows in block b
        assert whole.size, "no feature with all its rows inside the block"
        ok = False
        for it in range(2000):
            tot = int(lengths()[b * SW_BLOCK:(b + 1) * SW_BLOCK].sum())
            if lo < tot <= hi:
                ok = True
                break
            j = int(whole[it % whole.size])
            id_len[k][j] += 1 if tot <= lo else -1
            assert id_len[k][j] >= 3
        landed.append(ok)
    feats = build(id_len)
    rows = _sw_batch_rows(ctgs, feats, rgs, actions)[0]
    return dict(ctgs=ctgs, feats=feats, rgs=rgs, rows=rows, landed=tuple(landed), actions=actions)


def sw_arrays(case):
    """the arguments of gams_gpu_sw_text_actions for every ctg of the case, in order"""
    ctgs, feats = case["ctgs"], case["feats"]
    sel = list(range(len(ctgs)))
    foff = np.concatenate([[0], np.cumsum([len(f) for f in feats])])
    return dict(sel=sel, names=[c["chr_id"] for c in ctgs], cst=[c["chr_start"] for c in ctgs], foff=foff,
                fs=[f[1] for fl in feats for f in fl], fe=[f[2] for fl in feats for f in fl],
                ids=[f[0] for fl in feats for f in fl])


SW_BIG_FEATURES = 12_800


@functools.lru_cache(maxsize=None)
def sw_big_case():
    """12,800 point features away from the ends of one ctg at max 20: 524,800 rows in one call, more than SCAN_THREADS
    blocks, so that a thread of blk_offsets_scan_kernel takes two of them"""
    c = ctg("7", 99_000, helpers.synth(1_300_000, 81))
    pos = c["chr_start"] + 1000 + np.arange(SW_BIG_FEATURES) * 100
    feats = [(f"feature:{c['id']}:{j + 1}", int(p), int(p)) for j, p in enumerate(pos)]
    return dict(ctgs=[c], feats=[feats], rgs=[[]], actions=("gc",))
