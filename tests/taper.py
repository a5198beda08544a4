"""The tapered tile table of the headline wave plan (size 100, step 10, lag 100), as a model and as a world.  A module,
not a test: test_wave_taper_cpu.py holds wave_taper_tails / wave_taper_width of gams_amd/csrc/wave_select.hpp against
the model and checks the world's layout, test_gpu_wave_taper.py holds gams_wave_plan_tiles against the model for the
device's own CU count and runs wave_fast_taper_kernel over the world.

The model is written from the documents, not from the C++ (include/gams_gpu_diag.h on gams_wave_plan_set_taper and
_set_taper_shape, DESIGN "tapered launches"):
  * a round of workgroup slots is 8 per CU; a launch over at least a round and a half of W = 12 tiles is tapered;
  * a tile of width W holds 256 * W - lag - 1 windows: 2,971 / 1,947 / 923 for W = 12 / 8 / 4;
  * the W = 4 tail is pct4 % of a round -- whole slots, so floor(slots * pct4 / 100) of them, a W = 4 tile each -- and
    at most 8 % of the batch's windows (whole windows: floor(T * 8 / 100)); the W = 8 tail in front of it likewise with
    pct8 %, W = 8 tiles and 17 %;
  * the tails are made of whole ctgs: a ctg is cut into W = 4 tiles when the windows from its first one to the end of
    the batch fit the W = 4 tail, into W = 8 tiles when they fit both tails together, else into W = 12 tiles.

The world is the smallest one that reaches the kernel: T = 12 * cus * 2,971 windows is the floor (91 Mb at 256 CUs),
so it is generated from fixed seeds, never committed, and built from the back (see layout)."""
from collections import namedtuple
from concurrent.futures import ThreadPoolExecutor

import numpy as np

SIZE, STEP, LAG = 100, 10, 100
PCT4, PCT8 = 25, 50                  # default shape of the two tails, % of a round
CAP4, CAP8 = 8, 17                   # and what they may take of the batch, %
SHAPES = ((0, 0), (0, 50), (100, 0), (100, 100), (1, 1))     # gams_wave_plan_set_taper_shape beyond the default
MARGIN = 5000                        # windows of the world above the floor
BODY, FILL = 50_000, 20_000          # windows of an ordinary ctg of the body / of a tail
BIG_TILES = 64                       # tile starts of one ctg take every residue against the 128-base plane load
RUN = 1200                           # bases of a homopolymer / N run: longer than the 1,110 bases of lag + 1 windows


# ---- the model ---------------------------------------------------------------------------------------------------
def tile_windows(w, lag=LAG):
    return 256 * w - lag - 1


def slots(cus):
    return 8 * max(cus, 1)


def tapered(total, cus, lag=LAG):
    """a launch over at least a round and a half of W = 12 tiles"""
    s = slots(cus)
    return total // tile_windows(12, lag) >= s + s // 2


def tails(total, cus, pct4=PCT4, pct8=PCT8, lag=LAG):
    """-> (x4, y8): the windows of the W = 4 tail and of the W = 8 tail in front of it"""
    s = slots(cus)
    x4 = min((s * pct4 // 100) * tile_windows(4, lag), total * CAP4 // 100)
    y8 = min((s * pct8 // 100) * tile_windows(8, lag), total * CAP8 // 100)
    return x4, y8


def widths(ctg_windows, cus, pct4=PCT4, pct8=PCT8, lag=LAG):
    """-> W of every ctg of the batch (4, 8 or 12)"""
    n = np.asarray(ctg_windows, np.int64)
    total = int(n.sum())
    x4, y8 = tails(total, cus, pct4, pct8, lag)
    after = total - (np.cumsum(n) - n)           # windows from the ctg's first one to the end of the batch
    return np.where(after <= x4, 4, np.where(after <= x4 + y8, 8, 12))


def table(ctg_windows, cus, pct4=PCT4, pct8=PCT8, lag=LAG, taper=True):
    """-> the tile table, one row (ctg, first window, W) per tile; taper=False: W = 12 tiles throughout, W reads 0"""
    n = np.asarray(ctg_windows, np.int64)
    w = widths(n, cus, pct4, pct8, lag) if taper else np.full(n.size, 12)
    tw = 256 * w - lag - 1
    tiles = (n + tw - 1) // tw
    ctg = np.repeat(np.arange(n.size), tiles)
    first = np.cumsum(tiles) - tiles
    w0 = (np.arange(int(tiles.sum())) - first[ctg]) * tw[ctg]
    return np.stack([ctg, w0, w[ctg] if taper else np.zeros(ctg.size, np.int64)], axis=1).astype(np.uint32)


# ---- the world ---------------------------------------------------------------------------------------------------
# counts: windows of every ctg.  w4 / w8: the ctgs (ranges) of the two tails; front: the 100-window ctg before the W = 8
# tail; big4 / big8: each tail's ctg of many tiles; body: range of the ordinary ctgs in front.
Layout = namedtuple("Layout", "cus T x4 y8 counts body front w8 w4 big8 big4")


def bases(n_win, ragged=0):
    """length of a ctg of n_win windows of 100 / 10 with `ragged` (0..9) bases beyond the last window"""
    return (n_win - 1) * STEP + SIZE + ragged


def edge_counts(w):
    """what every tail holds: the lag itself (nothing can signal), one window more, either side of one and of two of
    the region's tiles (a last tile of one window among them), either side of the W = 12 tile"""
    tw = tile_windows(w)
    return [LAG, LAG + 1, tw - 1, tw, tw + 1, 2 * tw + 1, 2970, 2971, 2972]


def _region(w, total):
    """window counts of a tail of exactly `total` windows: its big ctg, ordinary ctgs, its edge ctgs"""
    tw = tile_windows(w)
    listed = edge_counts(w)
    rest = total - sum(listed)
    assert rest >= LAG, "the tail has no room for its edge ctgs"
    # the big ctg: BIG_TILES tiles and a last tile of one window, plus what the ordinary ctgs behind it leave over;
    # a tail of fewer windows (x4 is 2 * cus W = 4 tiles: below 80 CUs) gives it all it has left
    big = BIG_TILES * tw + 1
    big = rest if rest < big + FILL else big + (rest - big) % FILL
    fill = [FILL] * ((rest - big) // FILL)
    # the edge ctgs last, the shortest at the very end: the smallest tail shapes (1 % of a round) still hold some of them
    counts = [big] + fill + sorted(listed, reverse=True)
    assert sum(counts) == total
    return counts


def layout(cus):
    """The world for a device of `cus` compute units, from the back: a W = 4 tail whose windows sum to exactly the
    default x4 (its first ctg has after == x4), a W = 8 tail of exactly y8 in front (after == x4 + y8), a ctg of `lag`
    windows in front of that (after == x4 + y8 + 100: W = 12), ordinary ctgs up to T."""
    total = slots(cus) * 3 // 2 * tile_windows(12) + MARGIN
    x4, y8 = tails(total, cus)
    c4, c8 = _region(4, x4), _region(8, y8)
    left = total - x4 - y8 - LAG
    body = [BODY] * (left // BODY)
    body[-1] += left % BODY
    counts = body + [LAG] + c8 + c4
    assert sum(counts) == total
    nb = len(body)
    w8 = range(nb + 1, nb + 1 + len(c8))
    w4 = range(w8[-1] + 1, len(counts))
    return Layout(cus, total, x4, y8, np.asarray(counts, np.int64), range(0, nb), nb, w8, w4, w8[0], w4[0])


def mixed(lay, tail):
    """the ctgs of a tail (lay.w4 or lay.w8) that are not ordinary: its big ctg, then its edge ctgs"""
    return [tail[0]] + list(tail)[-len(edge_counts(4)):]


_TEXT = np.frombuffer(b"ACGTNacgtn", np.uint8)
_ACGT = np.frombuffer(b"ACGT", np.uint8)


def ragged(k):
    return (3 * k) % 10


def sequence(lay, k, seed=20260101):
    """the bases of ctg k.  Edge ctgs and the big ctg of a tail alternate between random bytes 0..255 (lower-case g / c
    among them) and ACGTNacgtn text; the ordinary ctgs are uniform ACGT.  The big ctg carries a run of G across its
    first tile seam and a run of N across its second."""
    n = bases(int(lay.counts[k]), ragged(k))
    rng = np.random.default_rng([seed, k])
    for tail, big, w in ((lay.w8, lay.big8, 8), (lay.w4, lay.big4, 4)):
        if k in mixed(lay, tail):
            j = mixed(lay, tail).index(k)
            s = rng.integers(0, 256, n, dtype=np.uint8) if j & 1 else np.ascontiguousarray(_TEXT[rng.integers(0, 10, n)])
            if k == big:
                for seam, base in ((1, ord("G")), (2, ord("N"))):
                    mid = seam * tile_windows(w) * STEP
                    s[mid - RUN // 2:mid + RUN // 2] = base
            return s
    return np.ascontiguousarray(_ACGT[rng.integers(0, 4, n, dtype=np.uint8)])


def sequences(lay, threads=16):
    with ThreadPoolExecutor(min(threads, 16)) as ex:
        return list(ex.map(lambda k: sequence(lay, k), range(lay.counts.size)))


def ctg_dicts(seqs):
    """the ctg records the host operators take: every ctg a chromosome of its own, first coordinates that differ"""
    out = []
    for k, s in enumerate(seqs):
        start = 1 + (k % 7) * 1000
        out.append(dict(id=f"ctg:w{k}:1", chr_id=f"w{k}", chr_start=start, chr_end=start + s.size - 1, seq=s))
    return out


# ---- the oracle over the world -----------------------------------------------------------------------------------
def oracle(seqs, threshold, threads=16):
    """oracle.wave_windows over every ctg on at most 16 host threads -> (counts u32[], signals i8[]) per ctg"""
    from oracle import oracle as ora

    def one(s):
        cnt, _, sig = ora.wave_windows(s, SIZE, STEP, LAG, threshold, 1.0)
        return cnt.copy(), sig.astype(np.int8)

    with ThreadPoolExecutor(min(threads, 16)) as ex:
        return list(ex.map(one, seqs))


def peak_records(dense, dtype):
    """the peak records of oracle()'s result, in the order the library packs them (ctg, then window)"""
    idx = [np.flatnonzero(sig) for _, sig in dense]
    rec = np.zeros(sum(i.size for i in idx), dtype)
    at = 0
    for c, ((cnt, sig), i) in enumerate(zip(dense, idx)):
        part = rec[at:at + i.size]
        part["ctg"], part["window"], part["gc_count"], part["signal"] = c, i, cnt[i], sig[i]
        at += i.size
    return rec


def tile_signal_counts(dense, tiles, lag=LAG):
    """windows that signal in every tile of the table (rows of table())"""
    out = np.zeros(len(tiles), np.int64)
    for t, (c, w0, w) in enumerate(np.asarray(tiles, np.int64)):
        out[t] = np.count_nonzero(dense[c][1][w0:w0 + tile_windows(w if w else 12, lag)])
    return out
