"""Inputs on which the f32 rounding order decides what `gams sw` and `gams peak` print, shared by test_sw_knife_cpu.py
and test_gpu_sw_knife.py.

Every float of sw.hip goes through round4, and at the parameters of the rest of the suite round4 swallows any last-ulp
difference: tile values are multiples of 1e-4, the mean times 1e4 is an integer.  Here a strict-f32 numpy model of one
sw row (center_resize, tile counts from a prefix sum, the reference's sequential sum, sum / n, sequential sq + d * d,
sqrtf(sq / (n - 1)), the cv branches, roundf(x * 1e4) / 1e4) can be made wrong on purpose, one change at a time
(`variant=`), and for every parameter set the windows of a synthetic ctg on which such a change prints another value
are searched out: the battery.  A kernel that sums by a tree, multiplies by a reciprocal, fuses d * d into the sum or
rounds half to even then differs from the reference on rows the battery is known to hold (test_sw_knife_cpu.py asserts
how many).

The range grid does the same for the gc of an arbitrary range: every (G/C count, length) up to 4096 bases on a ctg of
2048 G and 2048 A.

Nothing here imports the GPU package.  Everything is computed once per parameter set and kept."""
import functools

import numpy as np

F = np.float32
ROW_DTYPE = np.dtype([("feature", np.uint32), ("type", np.int32), ("distance", np.int32), ("start", np.int32),
                      ("end", np.int32), ("gc_content", np.float32), ("gc_mean", np.float32), ("gc_stddev", np.float32),
                      ("gc_cv", np.float32)])       # gams_sw_row_t
FIELDS = ("gc_content", "gc_mean", "gc_stddev", "gc_cv")
VARIANTS = ("pairwise", "f64", "fma", "onepass", "halfeven", "recip")
KEEP = 8                 # kKeep of sw_kernel: flanks of at most this many tiles keep their tile values in registers
PER_VARIANT = 64         # windows kept per (variant, field)
N_RANDOM = 200

# (size, max, resize) -> bases of its ctg.  The three kKeep sets share one ctg (same size, same length).
SETS = {
    (100, 20, 500): 600_000,     # the default; 5 tiles
    (100, 5, 800): 300_000,      # 8 tiles: mean ties, kKeep exactly
    (100, 5, 700): 300_000,      # 7 tiles
    (100, 5, 900): 300_000,      # 9 tiles
    (100, 3, 1600): 150_000,      # 16 tiles
    (64, 5, 512): 100_000,        # tile values that are ties themselves
    (128, 3, 1024): 100_000,
    (32, 5, 160): 100_000,        # five tiles whose values are ties
    (7, 2, 35): 300_000,         # sd sensitive; 4 tiles (a resize of 35 gives 34 bases)
    (7, 2, 36): 300_000,         # the same at 5 tiles
}
KEEP_SETS = [(100, 5, 700), (100, 5, 800), (100, 5, 900)]
CHR_START = 1001


def tiles_of(params):
    """the tiles of an unclipped flank: a window of two or more bases is resized to 2 * (resize / 2) bases"""
    return 2 * (params[2] // 2) // params[0]


# ---- the model --------------------------------------------------------------------------------------------------
def roundf(v):
    """C's roundf (half away from zero) over f32: r = floor(|v|); r + (|v| - r >= 0.5), the sign put back.  |v| - r
    is exact in f32; np.round is half-even and floor(v + 0.5) rounds the sum first: both are wrong next to a tie"""
    v = np.asarray(v, F)
    a = np.abs(v)
    r = np.floor(a)
    return np.copysign(r + (a - r >= F(0.5)).astype(F), v)


def round4(v, halfeven=False):
    """utils.rs:135-138 with decimals = 4: roundf(x * 1e4) / 1e4 in f32"""
    y = np.asarray(v, F) * F(10000.0)
    return (np.rint(y) if halfeven else roundf(y)) / F(10000.0)


def ratio(c, n, variant=None):
    """c / n in f32 (bio's gc_content: the count over the length)"""
    c, n = np.asarray(c).astype(F), np.asarray(n).astype(F)
    if variant == "recip":
        return c * (F(1.0) / n)
    return c / n


def center_resize(ps, pe, s, e, resize):
    """window.rs:96-124 over a single-span parent [ps, pe], vectorised (center_resize_1 of sw.hip)"""
    s, e = np.asarray(s, np.int64), np.asarray(e, np.int64)
    half = (e - s + 1) // 2
    mid_l = np.where(half == 0, s, s + half - 1)
    mid_r = np.where(half == 0, s, s + half)
    hr = resize // 2
    left = np.maximum((mid_l - ps + 1) - hr + 1, 1)
    right = np.minimum((mid_r - ps + 1) + hr - 1, pe - ps + 1)
    return ps + left - 1, ps + right - 1


def windows(cs, ce, fs, fe, size, mx):
    """window.rs:3-56 for every feature: (feature, type, distance, start, end) of the rows in the reference's order
    (feature, M, L1.., R1..)"""
    fs, fe = np.asarray(fs, np.int64), np.asarray(fe, np.int64)
    nf, psize = fs.size, ce - cs + 1
    m_s, m_e = center_resize(cs, ce, fs, fe, size)
    ws, we = np.zeros((nf, 1 + 2 * mx), np.int64), np.zeros((nf, 1 + 2 * mx), np.int64)
    ok = np.zeros((nf, 1 + 2 * mx), bool)
    typ, dist = np.zeros(1 + 2 * mx, np.int32), np.zeros(1 + 2 * mx, np.int32)
    ws[:, 0], we[:, 0], ok[:, 0] = m_s, m_e, True
    for t in (1, 2):
        if t == 2:
            sw_start = (m_e - cs + 1) + 1                       # :21
            sw_end = sw_start + size - 1
        else:
            sw_end = (m_s - cs + 1) - 1                         # :24
            sw_start = sw_end - size + 1
        alive = np.ones(nf, bool)
        for d in range(1, mx + 1):
            alive = alive & (sw_start >= 1) & (sw_end <= psize)   # :30-35: the first that leaves the parent ends the side
            col = d if t == 1 else mx + d
            ws[:, col], we[:, col], ok[:, col] = cs + sw_start - 1, cs + sw_end - 1, alive
            typ[col], dist[col] = t, d
            if t == 2:
                sw_start = sw_end + 1
                sw_end = sw_start + size - 1
            else:
                sw_end = sw_start - 1
                sw_start = sw_end - size + 1
    feat = np.broadcast_to(np.arange(nf, dtype=np.uint32)[:, None], ok.shape)
    return (feat[ok], np.broadcast_to(typ, ok.shape)[ok], np.broadcast_to(dist, ok.shape)[ok], ws[ok], we[ok])


def _tile_values(ctg, size, variant):
    """round4(count / size) of the `size` bases from every offset of the ctg (kept per size and rounding)"""
    key = (size, variant if variant in ("halfeven", "recip") else None)
    if key not in ctg["tv"]:
        P = ctg["P"]
        c = P[size:] - P[:-size] if P.size > size else np.zeros(0, np.int64)
        ctg["tv"][key] = round4(ratio(c, np.full(c.shape, size), key[1]), key[1] == "halfeven")
    return ctg["tv"][key]


def _flank_stats(x, live, nt, variant):
    """mean, stddev and cv (unrounded f32) of the tile values x[i, :nt[i]], in the reference's order unless a
    variant says otherwise"""
    n, T = x.shape
    lenf = nt.astype(F)
    xz = np.where(live, x, F(0.0))
    with np.errstate(all="ignore"):
        if variant == "f64":                                    # everything in f64, cast at the end
            s = np.zeros(n, np.float64)
            for t in range(T):
                s = s + xz[:, t].astype(np.float64)
            mean = s / nt.astype(np.float64)
            sq = np.zeros(n, np.float64)
            for t in range(T):
                d = x[:, t].astype(np.float64) - mean
                sq = np.where(live[:, t], sq + d * d, sq)
            sd = np.sqrt(sq / (nt.astype(np.float64) - 1.0))
            cv = np.where((mean == 0.0) | (mean == 1.0), 0.0, np.where(mean <= 0.5, sd / mean, sd / (1.0 - mean)))
            return mean.astype(F), sd.astype(F), cv.astype(F)
        if variant == "pairwise":                               # a tree over the tiles, zeros behind the last
            w = 1
            while w < max(T, 1):
                w *= 2
            tree = np.zeros((n, w), F)
            tree[:, :T] = xz
            while tree.shape[1] > 1:
                tree = tree[:, 0::2] + tree[:, 1::2]
            s = tree[:, 0]
        else:
            s = np.zeros(n, F)
            for t in range(T):
                s = np.where(live[:, t], s + x[:, t], s)        # stat.rs:3
        mean = s / lenf                                         # stat.rs:5
        sq = np.zeros(n, F)
        if variant == "onepass":                                # sum(x^2) - n * mean^2
            for t in range(T):
                sq = sq + xz[:, t] * xz[:, t]
            sq = np.maximum(sq - lenf * (mean * mean), F(0.0))
        else:
            for t in range(T):
                d = x[:, t] - mean
                if variant == "fma":                            # d * d unrounded into the sum
                    nxt = (d.astype(np.float64) * d.astype(np.float64) + sq.astype(np.float64)).astype(F)
                else:
                    nxt = sq + d * d                            # stat.rs:12
                sq = np.where(live[:, t], nxt, sq)
        sd = np.sqrt(sq / (lenf - F(1.0)))                      # stat.rs:13
        cv = np.where((mean == F(0.0)) | (mean == F(1.0)), F(0.0),
                      np.where(mean <= F(0.5), sd / mean, sd / (F(1.0) - mean)))     # utils.rs:169-175
    assert mean.dtype == sd.dtype == cv.dtype == F
    return mean, sd, cv


def stats(ctg, ws, we, size, resize, variant=None):
    """the four printed statistics of the windows [ws, we] (chromosome coordinates) of `ctg`: f32 [n, 4] in the order
    of FIELDS.  A flank of 0 tiles gives NaN, -0, NaN, one of 1 tile its value, NaN, NaN (or cv 0 at a mean of 0 or 1)"""
    ws, we = np.asarray(ws, np.int64), np.asarray(we, np.int64)
    cs, ce, P = ctg["chr_start"], ctg["chr_end"], ctg["P"]
    he = variant == "halfeven"
    content = round4(ratio(P[we - cs + 1] - P[ws - cs], we - ws + 1, variant), he)          # utils.rs:141-162
    rs, re = center_resize(cs, ce, ws, we, resize)                                          # sw.rs:175
    nt = (re - rs + 1) // size                                                              # sliding(range, size, size)
    T = int(nt.max()) if nt.size else 0
    tv = _tile_values(ctg, size, variant)
    t = np.arange(T, dtype=np.int64)
    live = t[None, :] < nt[:, None]
    at = np.where(live, (rs - cs)[:, None] + t[None, :] * size, 0)
    x = tv[at] if tv.size else np.zeros(at.shape, F)
    mean, sd, cv = _flank_stats(x, live, nt, variant)
    return np.stack([content, round4(mean, he), round4(sd, he), round4(cv, he)], axis=1)


def rows(ctg, fs, fe, size, mx, resize, variant=None):
    """the rows of gams_gpu_sw / gams_ref_sw for the features [fs, fe] of `ctg`, as ROW_DTYPE"""
    feat, typ, dist, ws, we = windows(ctg["chr_start"], ctg["chr_end"], fs, fe, size, mx)
    st = stats(ctg, ws, we, size, resize, variant)
    out = np.zeros(feat.size, ROW_DTYPE)
    out["feature"], out["type"], out["distance"], out["start"], out["end"] = feat, typ, dist, ws, we
    for k, f in enumerate(FIELDS):
        out[f] = st[:, k]
    return out


def fmt4(v):
    """Rust's `{}` of a round4 value below 1000: m / 10^4 with its trailing zeros dropped; NaN, 0 and -0 by name"""
    v = F(v)
    if np.isnan(v):
        return "NaN"
    if v == 0:
        return "-0" if np.signbit(v) else "0"
    m = int(round(abs(float(v)) * 10000.0))
    assert 0 < m < 10_000_000 and F(m / 10000.0) == abs(v), v
    s = ("%d.%04d" % divmod(m, 10000)).rstrip("0").rstrip(".")
    return "-" + s if v < 0 else s


def text(ctg, ids, r):
    """the rows `r` as `gams sw` prints them (sw.rs:152-190, data.rs:58-83); ids[f] = the id of feature f"""
    memo, out, serial, last = {}, [], 0, -1
    for f, typ, dist, s, e, *vals in r.tolist():
        serial = serial + 1 if f == last else 1
        last = f
        fl = []
        for v, bits in zip(vals, np.array(vals, F).view(np.uint32).tolist()):
            if bits not in memo:
                memo[bits] = fmt4(v)
            fl.append(memo[bits])
        rg = "%s:%d" % (ctg["chr_id"], s) if s == e else "%s:%d-%d" % (ctg["chr_id"], s, e)
        out.append("sw:%s:%d\t%s\t%s\t%d\t%s\t\n" % (ids[f], serial, rg, "MLR"[typ], dist, "\t".join(fl)))
    return "".join(out)


def differs(a, b):
    """where two f32 arrays print another value: the bits differ and not both are NaN"""
    a, b = np.asarray(a, F), np.asarray(b, F)
    return (a.view(np.uint32) != b.view(np.uint32)) & ~(np.isnan(a) & np.isnan(b))


# ---- the ctgs ---------------------------------------------------------------------------------------------------
def make_ctg(seq, cid="ctg:I:1", chr_id="I", chr_start=CHR_START):
    seq = np.ascontiguousarray(seq, np.uint8)
    gc = (seq == ord("G")) | (seq == ord("C")) | (seq == ord("g")) | (seq == ord("c"))
    return dict(id=cid, chr_id=chr_id, chr_start=chr_start, chr_end=chr_start + seq.size - 1, seq=seq.tobytes(),
                P=np.concatenate(([0], np.cumsum(gc, dtype=np.int64))), tv={})


@functools.lru_cache(maxsize=None)
def knife_ctg(size, n, stretch):
    """n bases in blocks of size / 2 .. 4 * size bases whose G/C richness is one of 0.1 .. 0.9, with one all-G and one
    all-A/T stretch of `stretch` bases (longer than the flank) a third and two thirds in"""
    rng = np.random.default_rng(7919 * size + n)
    gc_letters, at_letters = np.frombuffer(b"GCGCgc", np.uint8), np.frombuffer(b"ATATatN", np.uint8)
    parts, have = [], 0
    marks = {}
    for name, where, letters in (("G", n // 3, b"G"), ("AT", 2 * n // 3, b"AT")):
        while have < where:
            ln = int(rng.integers(size // 2 + 1, 4 * size + 1))
            p = rng.choice(np.arange(1, 10) / 10.0)
            isgc = rng.random(ln) < p
            parts.append(np.where(isgc, gc_letters[rng.integers(0, gc_letters.size, ln)],
                                  at_letters[rng.integers(0, at_letters.size, ln)]).astype(np.uint8))
            have += ln
        marks[name] = (have, stretch)
        parts.append(np.frombuffer(letters * (stretch // len(letters) + 1), np.uint8)[:stretch])
        have += stretch
    while have < n:
        ln = int(rng.integers(size // 2 + 1, 4 * size + 1))
        p = rng.choice(np.arange(1, 10) / 10.0)
        isgc = rng.random(ln) < p
        parts.append(np.where(isgc, gc_letters[rng.integers(0, gc_letters.size, ln)],
                              at_letters[rng.integers(0, at_letters.size, ln)]).astype(np.uint8))
        have += ln
    c = make_ctg(np.concatenate(parts)[:n])
    c["stretches"] = marks                       # name -> (offset, bases)
    return c


def ctg_of(params):
    size = params[0]
    widest = max(p[2] for p in SETS if p[0] == size and SETS[p] == SETS[params])
    return knife_ctg(size, SETS[params], widest + 4 * size)


def short_ctgs(params):
    """ctgs too short for a full flank: size - 1 bases (no tile: NaN, -0, NaN), size and 2 * size - 1 bases (one tile:
    its value, NaN, and cv NaN or 0), 2 * size and 3 * size + 1 bases; all-G, all-A and mixed"""
    size = params[0]
    rng = np.random.default_rng(size)
    out, at = [], 5
    for k, n in enumerate((size - 1, size, 2 * size - 1, 2 * size, 3 * size + 1, size, size)):
        seq = np.frombuffer(b"GCATgcatNN", np.uint8)[rng.integers(0, 10, n)]
        if k == 5:
            seq = np.full(n, ord("G"), np.uint8)
        if k == 6:
            seq = np.full(n, ord("A"), np.uint8)
        out.append(make_ctg(seq, "ctg:S:%d" % (k + 1), "S", at))
        at += n + 3
    return out


def short_features(c):
    """every point of a short ctg and the ctg itself"""
    p = np.arange(c["chr_start"], c["chr_end"] + 1)
    return np.concatenate((p, [c["chr_start"]])).astype(np.int32), np.concatenate((p, [c["chr_end"]])).astype(np.int32)


# ---- the battery ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def battery(params):
    """-> (ctg, fs, fe, found).  The features of one parameter set, sorted by start: per (variant, field) the first
    PER_VARIANT windows of the ctg on which the variant prints another value than the model, each through a feature
    that has it among its rows (an M window through its point; a full window through the point whose R1 it is, or L1
    next to the ctg start); N_RANDOM features of 1 .. 3 * size bases at seeded places; every point within `resize`
    of either end of the ctg (flanks clipped to every tile count the ctg allows); points through the all-G and the
    all-A/T stretch.  found[(variant, field)] = how many such windows the whole ctg holds."""
    size, mx, resize = params
    c = ctg_of(params)
    cs, ce = c["chr_start"], c["chr_end"]
    pos = np.arange(cs, ce + 1, dtype=np.int64)
    m_s, m_e = center_resize(cs, ce, pos, pos, size)            # the M window of every point
    w_s = np.arange(cs, ce - size + 2, dtype=np.int64)          # every full window
    w_e = w_s + size - 1
    half = size // 2
    base_m, base_w = stats(c, m_s, m_e, size, resize), stats(c, w_s, w_e, size, resize)
    picks, found = [], {}
    for v in VARIANTS:
        dm = differs(base_m, stats(c, m_s, m_e, size, resize, v))
        dw = differs(base_w, stats(c, w_s, w_e, size, resize, v))
        for k, field in enumerate(FIELDS):
            ww = w_s[dw[:, k]]
            through = np.where(ww - half >= cs, ww - half, ww + size - 1 + half)
            cand = np.unique(np.concatenate((pos[dm[:, k]], through[through <= ce])))
            found[(v, field)] = int(dm[:, k].sum() + dw[:, k].sum())
            picks.append(cand[:PER_VARIANT])
    rng = np.random.default_rng(size * 31 + resize)
    rs = rng.integers(cs + 2 * size, ce - 5 * size, N_RANDOM)
    rw = rng.integers(0, 3 * size, N_RANDOM)
    ends = np.concatenate((np.arange(cs, cs + resize), np.arange(ce - resize + 1, ce + 1)))
    inside = []
    for off, n in c["stretches"].values():
        inside.append(np.arange(cs + off - size, cs + off + n + size, max(size // 3, 1)))
    points = np.unique(np.concatenate(picks + [ends] + inside))
    fs = np.concatenate((points, rs))
    fe = np.concatenate((points, rs + rw))
    order = np.lexsort((fe, fs))
    return c, fs[order].astype(np.int32), fe[order].astype(np.int32), found


def feature_ids(c, n):
    return ["feature:%s:%d" % (c["id"], k + 1) for k in range(n)]


@functools.lru_cache(maxsize=None)
def battery_rows(params, variant=None):
    c, fs, fe, _ = battery(params)
    return rows(c, fs, fe, *params, variant=variant)


def sensitivity(params, variant):
    """field -> the battery rows on which the variant prints another value than the model"""
    a, b = battery_rows(params), battery_rows(params, variant)
    return {f: int(differs(a[f], b[f]).sum()) for f in FIELDS}


# ---- the range grid ---------------------------------------------------------------------------------------------
GRID_G = 2048
GRID_VARIANTS = ("recip", "mulfirst", "halfeven", "f64")


@functools.lru_cache(maxsize=None)
def grid_ctg():
    return make_ctg(np.frombuffer(b"G" * GRID_G + b"A" * GRID_G, np.uint8), chr_start=1)


def grid_model(c, ln, variant=None):
    """round4(c / len) of utils.rs:141-162 in f32, vectorised; the variants change one step each"""
    c, ln = np.asarray(c), np.asarray(ln)
    if variant == "f64":
        y = c.astype(np.float64) / ln.astype(np.float64) * 10000.0
        r = np.floor(y)
        return ((r + (y - r >= 0.5)) / 10000.0).astype(F)
    if variant == "mulfirst":                                   # c * 1e4 / len
        return roundf(c.astype(F) * F(10000.0) / ln.astype(F)) / F(10000.0)
    return round4(ratio(c, ln, variant), variant == "halfeven")


@functools.lru_cache(maxsize=None)
def grid():
    """-> dict(c, len, start, end, gc, ties, differ): every (G/C count c, length len) with len <= 4096, c <= 2048 and
    len - c <= 2048 on grid_ctg(), where the range (2049 - c, 2048 - c + len) holds exactly c G in len bases; the
    model's answer; the indices of the exact ties (c * 1e4 / len is k + 1/2 in real arithmetic); per variant the
    indices on which it differs from the model"""
    ln, c = np.meshgrid(np.arange(1, 2 * GRID_G + 1, dtype=np.int64), np.arange(0, GRID_G + 1, dtype=np.int64), indexing="ij")
    ok = (c <= ln) & (ln - c <= GRID_G)
    ln, c = ln[ok], c[ok]
    g = dict(c=c.astype(np.int32), len=ln.astype(np.int32), start=(GRID_G + 1 - c).astype(np.int32),
             end=(GRID_G - c + ln).astype(np.int32), gc=grid_model(c, ln))
    g["ties"] = np.flatnonzero((20000 * c) % (2 * ln) == ln)
    g["differ"] = {v: np.flatnonzero(differs(g["gc"], grid_model(c, ln, v))) for v in GRID_VARIANTS}
    return g


@functools.lru_cache(maxsize=None)
def grid_edges():
    """the indices of the ties and of every pair a variant changes, ascending"""
    g = grid()
    return np.unique(np.concatenate([g["ties"]] + [g["differ"][v] for v in GRID_VARIANTS]))


def grid_peak_case():
    """-> (ctgs, data, idx): grid_ctg() as chromosome I and, with the same bases, as chromosome II; the bytes of a wave
    TSV whose lines are the ranges of grid_edges() = idx on both, ascending on I and descending on II, behind one
    sacrificial line each (read_peak drops the first located line of a ctg)"""
    g, idx = grid(), grid_edges()
    one = grid_ctg()
    two = dict(one, id="ctg:II:1", chr_id="II")
    lines = ["#range\tgc_content\tsignal", "I:10-20\t0.5\t1", "II:10-20\t0.5\t1"]
    s, e = g["start"].tolist(), g["end"].tolist()
    for k, (a, b) in enumerate(zip(idx.tolist(), idx[::-1].tolist())):
        lines.append("I:%s\t0.5\t%d" % (str(s[a]) if s[a] == e[a] else "%d-%d" % (s[a], e[a]), 1 - 2 * (k % 2)))
        lines.append("II:%s\t0.5\t%d" % (str(s[b]) if s[b] == e[b] else "%d-%d" % (s[b], e[b]), 2 * (k % 2) - 1))
    return [one, two], ("\n".join(lines) + "\n").encode(), idx


# ---- the kKeep sets against each other --------------------------------------------------------------------------
def keep_features():
    """-> (ctg, fs, fe): the ctg the sets at 7, 8 and 9 tiles share, and every point within the widest flank of either
    of its ends: the flanks of their windows are clipped by the ctg"""
    c = ctg_of(KEEP_SETS[0])
    far = max(p[2] for p in KEEP_SETS)
    p = np.concatenate((np.arange(c["chr_start"], c["chr_start"] + far), np.arange(c["chr_end"] - far + 1, c["chr_end"] + 1)))
    return c, p.astype(np.int32), p.astype(np.int32)


def keep_pairs():
    """[(params a, params b, mask over the rows of keep_features())]: the rows whose flank holds the same tiles under
    both resizes (it begins on the same base and has as many tiles)"""
    c, fs, fe = keep_features()
    cs, ce = c["chr_start"], c["chr_end"]
    size, mx = KEEP_SETS[0][:2]
    assert all(p[:2] == (size, mx) for p in KEEP_SETS)
    _, _, _, ws, we = windows(cs, ce, fs, fe, size, mx)
    out = []
    for i, a in enumerate(KEEP_SETS):
        for b in KEEP_SETS[i + 1:]:
            (sa, ea), (sb, eb) = center_resize(cs, ce, ws, we, a[2]), center_resize(cs, ce, ws, we, b[2])
            out.append((a, b, (sa == sb) & ((ea - sa + 1) // size == (eb - sb + 1) // size)))
    return out
