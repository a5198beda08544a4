"""The model and the batteries of tests/sw_knife.py held to account, without a GPU: the strict-f32 numpy model of an sw
row equals the CPU twin gams_ref_sw on every row of every battery (all fields, the floats by bit pattern, NaN patterns
included) and prints the text of the oracle's sw_proc_ctg; every battery holds the rows it is for -- per (parameter
set, variant, field) at least so many rows on which the variant prints another value (the table below: conditions, not
measurements); the range grid's model equals the oracle on every tie and every pair a variant changes, and every
variant changes at least 300 pairs.  test_gpu_sw_knife.py holds the device to the same model."""
import ctypes as C

import numpy as np
import pytest

import peak_text as pt
import sw_knife as sk
from gams_amd import _lib
from oracle import oracle as ora

R = ora.ref()
SETS = list(sk.SETS)


def twin_rows(c, fs, fe, params):
    """gams_ref_sw over the features of one ctg"""
    seq = np.frombuffer(c["seq"], np.uint8)
    fs, fe = np.ascontiguousarray(fs, np.int32), np.ascontiguousarray(fe, np.int32)
    n = C.c_uint64()
    assert R.gams_ref_sw(seq.ctypes.data, seq.size, c["chr_start"], fs.ctypes.data, fe.ctypes.data, fs.size, *params, None, 0,
                         C.byref(n)) == 0
    out = np.zeros(n.value, sk.ROW_DTYPE)
    assert R.gams_ref_sw(seq.ctypes.data, seq.size, c["chr_start"], fs.ctypes.data, fe.ctypes.data, fs.size, *params,
                         out.ctypes.data, out.size, C.byref(n)) == 0 and n.value == out.size
    return out


def first_row_difference(a, b):
    """None, or how many rows of two row arrays differ and the first of them, the floats of both as hex"""
    if a.size == b.size and a.tobytes() == b.tobytes():
        return None
    if a.size != b.size:
        return "%d rows against %d" % (a.size, b.size)
    bad = np.flatnonzero((a.view(np.uint8).reshape(a.size, -1) != b.view(np.uint8).reshape(b.size, -1)).any(axis=1))
    q = int(bad[0])

    def show(r):
        head = tuple(int(r[f]) for f in ("feature", "type", "distance", "start", "end"))
        return head + tuple("%s=%08x" % (f, int(np.array(r[f], np.float32).view(np.uint32))) for f in sk.FIELDS)

    return "%d of %d rows differ, the first is row %d: %s against %s" % (bad.size, a.size, q, show(a[q]), show(b[q]))


def oracle_text(c, fs, fe, params):
    feats = list(zip(sk.feature_ids(c, len(fs)), np.asarray(fs).tolist(), np.asarray(fe).tolist()))
    return ora.sw_proc_ctg(c["chr_id"], c["chr_start"], c["chr_end"], c["seq"], feats, *params)


def test_row_layout_and_roundf():
    """the model's rows are gams_sw_row_t; its roundf is C's on both sides of every half and on the halves themselves"""
    assert sk.ROW_DTYPE == _lib.SW_ROW_DTYPE
    half = (np.arange(0, 4000, dtype=np.float32) + np.float32(0.5))
    v = np.concatenate((half, np.nextafter(half, np.float32(0)), np.nextafter(half, np.float32(1e9)),
                        np.random.default_rng(1).uniform(0, 12000, 4000).astype(np.float32), [np.float32(8388607.5)]))
    v = np.concatenate((v, -v)).astype(np.float32)
    want = np.array([ora.round_(float(x), 0) for x in v], np.float32)
    assert np.array_equal(sk.roundf(v).view(np.uint32), want.view(np.uint32))
    assert int((np.round(v) != want).sum()) > 1000                         # np.round is the wrong function
    # the printed form of a round4 value is Rust's
    for x in (0.0, -0.0, float("nan"), 1.0, 0.5, 0.0001, 0.1235, 0.07, 12.3406, 999.9999):
        assert sk.fmt4(np.float32(x)) == ora.fmt_f32(np.float32(x)), x


@pytest.mark.parametrize("params", SETS)
def test_model_equals_the_twin_and_the_oracle_text(params):
    c, fs, fe, _ = sk.battery(params)
    got, want = sk.battery_rows(params), twin_rows(c, fs, fe, params)
    assert first_row_difference(got, want) is None, first_row_difference(got, want)
    assert got.size > 3000 and fs.size > 600
    assert sk.text(c, sk.feature_ids(c, fs.size), got) == oracle_text(c, fs, fe, params)


@pytest.mark.parametrize("params", SETS)
def test_model_equals_the_twin_on_short_ctgs(params):
    """flanks of no tile (NaN, -0, NaN) and of one tile (its value, NaN and a cv of NaN or 0), bit for bit"""
    seen = set()
    for c in sk.short_ctgs(params):
        fs, fe = sk.short_features(c)
        got, want = sk.rows(c, fs, fe, *params), twin_rows(c, fs, fe, params)
        assert first_row_difference(got, want) is None, (c["id"], first_row_difference(got, want))
        assert sk.text(c, sk.feature_ids(c, fs.size), got) == oracle_text(c, fs, fe, params)
        for r in got:
            seen.add(tuple(sk.fmt4(r[f]) for f in sk.FIELDS[1:]))
    assert ("NaN", "-0", "NaN") in seen                                   # no tile
    assert ("1", "NaN", "0") in seen and ("0", "NaN", "0") in seen        # one tile, all G and all A
    assert any(m not in ("NaN", "0", "1") and s == "NaN" and v == "NaN" for m, s, v in seen)


@pytest.mark.parametrize("params", SETS)
def test_battery_holds_what_it_is_built_for(params):
    size, mx, resize = params
    c, fs, fe, _ = sk.battery(params)
    cs, ce = c["chr_start"], c["chr_end"]
    r = sk.battery_rows(params)
    points = fs[fs == fe]
    assert set(range(cs, cs + resize)) <= set(points.tolist()) and set(range(ce - resize + 1, ce + 1)) <= set(points.tolist())
    assert int((fe > fs).sum()) >= sk.N_RANDOM // 2
    rs, re = sk.center_resize(cs, ce, r["start"], r["end"], resize)
    nt = (re - rs + 1) // size
    full = sk.tiles_of(params)
    lowest = (resize // 2 + size // 2) // size                             # the flank of the M window of the first base
    assert set(range(lowest + 1, full + 1)) <= set(np.unique(nt).tolist()) and nt.max() == full
    assert int((nt == full).sum()) > 1000
    # every row type at every distance, and the stretches: a mean of exactly 1 and of exactly 0, where cv is 0
    assert set(zip(r["type"].tolist(), r["distance"].tolist())) == {(0, 0)} | {(t, d) for t in (1, 2) for d in range(1, mx + 1)}
    for name, mean in (("G", 1.0), ("AT", 0.0)):
        off, n = c["stretches"][name]
        assert n > resize + 2 * size
        inside = (r["start"] >= cs + off + resize // 2) & (r["end"] < cs + off + n - resize // 2)
        assert inside.sum() > 10 and (r["gc_mean"][inside] == mean).all() and (r["gc_content"][inside] == mean).all()
        assert (r["gc_cv"][inside] == 0).all() and (r["gc_stddev"][inside] == 0).all()
    assert ((r["gc_mean"] > 0.5) & (r["gc_cv"] > 0)).sum() > 100 and ((r["gc_mean"] <= 0.5) & (r["gc_cv"] > 0)).sum() > 100


# (set) -> variant -> field -> the least number of battery rows on which the variant prints another value.  16
# wherever the search over the set's ctg reaches that many; behind `#` what it found when this was written, and the
# lower figure itself where it found fewer than 16.  recip (c * (1 / size)) reaches no row of any set: nobody may rely
# on the batteries for it -- the range grid below is what catches a reciprocal.
M, S, V, G = "gc_mean", "gc_stddev", "gc_cv", "gc_content"
SENSITIVITY = {
    (100, 20, 500): {"pairwise": {V: 16, S: 16},                    # 79, 16
                     "f64": {V: 16, S: 16},                         # 134, 83
                     "fma": {V: 16, S: 16},                         # 51, 66
                     "onepass": {V: 16, S: 16},                     # 528, 228
                     "halfeven": {V: 16, S: 16}},                   # 94, 73
    (100, 5, 800): {"pairwise": {M: 16, V: 16, S: 6},               # 1430, 73, 6
                    "f64": {M: 16, V: 16, S: 14},                   # 1282, 96, 14
                    "fma": {V: 16, S: 6},                           # 34, 6
                    "onepass": {V: 16, S: 16},                      # 183, 98
                    "halfeven": {M: 16, V: 16, S: 14}},             # 2400, 77, 14
    (100, 5, 700): {"pairwise": {V: 16, S: 16},                     # 82, 18
                    "f64": {V: 16, S: 16},                          # 157, 61
                    "fma": {V: 16, S: 16},                          # 28, 16
                    "onepass": {V: 16, S: 16},                      # 213, 123
                    "halfeven": {V: 16, S: 16}},                    # 66, 30
    (100, 5, 900): {"pairwise": {M: 16, V: 16, S: 4},               # 135, 84, 4
                    "f64": {M: 16, V: 16, S: 16},                   # 90, 96, 35
                    "fma": {V: 16, S: 16},                          # 57, 18
                    "onepass": {V: 16, S: 16},                      # 206, 126
                    "halfeven": {M: 16, V: 16, S: 16}},             # 99, 69, 54
    (100, 3, 1600): {"pairwise": {M: 16, V: 16, S: 16},             # 963, 72, 18
                     "f64": {M: 16, V: 16, S: 16},                  # 969, 99, 20
                     "fma": {V: 16, S: 12},                         # 34, 12
                     "onepass": {V: 16, S: 16},                     # 167, 77
                     "halfeven": {M: 16, V: 16, S: 16}},            # 1194, 78, 22
    (64, 5, 512): {"pairwise": {M: 16, V: 16},                      # 294, 41
                   "f64": {M: 16, V: 16, S: 4},                     # 256, 78, 4
                   "fma": {V: 16, S: 11},                           # 24, 11
                   "onepass": {V: 16, S: 16},                       # 164, 82
                   "halfeven": {G: 16, M: 16, S: 16, V: 16}},       # 1730, 2552, 1255, 3725
    (128, 3, 1024): {"pairwise": {M: 16, V: 16, S: 4},              # 322, 44, 4
                     "f64": {M: 16, V: 16, S: 6},                   # 230, 73, 6
                     "fma": {V: 16, S: 4},                          # 18, 4
                     "onepass": {V: 16, S: 16},                     # 163, 70
                     "halfeven": {G: 16, M: 16, S: 16, V: 16}},     # 863, 1366, 1285, 2696
    (32, 5, 160): {"pairwise": {V: 8},                              # 8
                   "f64": {V: 16, S: 6},                            # 42, 6
                   "fma": {V: 10, S: 8},                            # 10, 8
                   "onepass": {V: 16, S: 16},                       # 159, 104
                   "halfeven": {G: 16, M: 16, S: 16, V: 16}},       # 1677, 1865, 1510, 3458
    # 34 bases: 4 tiles.  A tree over 4 tiles moves the mean of 105 rows and the printed stddev of none of the 600,000
    # windows of the ctg; at 5 tiles (the next set) it does
    (7, 2, 35): {"pairwise": {M: 16, S: 0},                         # 105, 0
                 "f64": {M: 16, S: 16},                             # 140, 113
                 "fma": {S: 16},                                    # 64
                 "onepass": {S: 16, V: 16},                         # 265, 90
                 "halfeven": {M: 16, S: 16}},                       # 307, 164
    (7, 2, 36): {"pairwise": {S: 16},                               # 68
                 "f64": {S: 16, V: 8},                              # 72, 8
                 "fma": {S: 16, V: 8},                              # 72, 8
                 "onepass": {S: 16, V: 16},                         # 93, 76
                 "halfeven": {S: 16}},                              # 176
}


@pytest.mark.parametrize("params", SETS)
def test_sensitivity(params):
    """a kernel that computes as the variant does differs from the twin on at least this many rows of the battery"""
    table = SENSITIVITY[params]
    assert set(table) == set(sk.VARIANTS) - {"recip"}
    for variant, fields in table.items():
        got = sk.sensitivity(params, variant)
        print(params, variant, got)
        for field, least in fields.items():
            assert got[field] >= least, (params, variant, field, got[field], least)
        assert max(got[f] for f in fields) >= 8, (params, variant)
    assert sk.sensitivity(params, "recip") == dict.fromkeys(sk.FIELDS, 0)
    assert all(sk.battery(params)[3][("recip", f)] == 0 for f in sk.FIELDS)    # ... and no window of the whole ctg


def test_every_variant_is_reached_at_full_strength_somewhere():
    for variant in set(sk.VARIANTS) - {"recip"}:
        assert sum(1 for p in SETS for least in SENSITIVITY[p][variant].values() if least >= 16) >= 4, variant


def test_keep_sets_share_their_ctg_and_their_clipped_flanks():
    """the sets at 7, 8 and 9 tiles run over one ctg; where the flank of a window is clipped to the same tiles at two
    resizes, the model's rows are the same rows"""
    assert [sk.tiles_of(p) for p in sk.KEEP_SETS] == [sk.KEEP - 1, sk.KEEP, sk.KEEP + 1]
    c, fs, fe = sk.keep_features()
    assert all(sk.ctg_of(p) is c for p in sk.KEEP_SETS)
    compared = 0
    for a, b, same in sk.keep_pairs():
        ra, rb = sk.rows(c, fs, fe, *a), sk.rows(c, fs, fe, *b)
        assert ra[same].tobytes() == rb[same].tobytes()
        compared += int(same.sum())
    assert compared > 1000


# ---- the range grid -------------------------------------------------------------------------------------------------
def test_grid_counts():
    g = sk.grid()
    assert g["c"].size == 4_198_400 and g["ties"].size == 3_516
    n = {v: int(g["differ"][v].size) for v in sk.GRID_VARIANTS}
    print(n)                                                              # 490 / 325 / 2,021 / 487
    assert all(k >= 300 for k in n.values()), n
    c = sk.grid_ctg()
    P = c["P"]
    assert np.array_equal(P[g["end"]] - P[g["start"] - 1], g["c"]) and np.array_equal(g["end"] - g["start"] + 1, g["len"])
    assert g["start"].min() == 1 and g["end"].max() == 2 * sk.GRID_G
    assert 3_500 < sk.grid_edges().size < 8_000


def test_grid_model_equals_the_oracle():
    """on every exact tie, every pair a variant changes and 5,000 seeded pairs, bit for bit"""
    g, c = sk.grid(), sk.grid_ctg()
    pick = np.unique(np.concatenate((sk.grid_edges(), np.random.default_rng(5).integers(0, g["c"].size, 5000))))
    seq = np.frombuffer(c["seq"], np.uint8)
    rs, re = np.ascontiguousarray(g["start"][pick]), np.ascontiguousarray(g["end"][pick])
    want = np.zeros(pick.size, np.float32)
    assert R.gams_ref_range_gc(seq.ctypes.data, seq.size, 1, rs.ctypes.data, re.ctypes.data, pick.size, want.ctypes.data) == 0
    assert want[0] == ora.range_gc_content(seq, 1, int(rs[0]), int(re[0]))
    bad = np.flatnonzero(want.view(np.uint32) != g["gc"][pick].view(np.uint32))
    assert bad.size == 0, [(int(g["c"][pick[q]]), int(g["len"][pick[q]]), "%08x" % want[q:q + 1].view(np.uint32)[0]) for q in bad[:5]]


def test_grid_peak_input_carries_the_edges():
    """the wave TSV made of the ties and variant-changed pairs: the model of tests/peak_text.py keeps every one of them
    (all but the sacrificial first line of each ctg), and its gc column is this module's model"""
    ctgs, data, idx = sk.grid_peak_case()
    want = pt.model(ctgs, data).decode()
    rows = [r.split("\t") for r in want.split("\n")[:-1]]
    assert len(rows) == 2 * idx.size
    g = sk.grid()
    assert [c["id"] for c in ctgs] == sorted(c["id"] for c in ctgs)
    for k, in_file in enumerate((idx, idx[::-1])):                        # peak.rs:49: a stable sort by start
        order = in_file[np.argsort(g["start"][in_file], kind="stable")]
        mine = rows[k * idx.size:(k + 1) * idx.size]
        assert [r[3] for r in mine] == [sk.fmt4(v) for v in g["gc"][order]]
        assert [int(r[2]) for r in mine] == g["len"][order].tolist()
