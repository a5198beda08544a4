"""`gams sw --action count`: rg_count of every window, on the device (gams_gpu_sw_text_actions, gams_gpu_sw_count_batch
and the host operators above them).  The expected text is always the oracle's: oracle.sw_proc_ctg's rows, field 9
rewritten with oracle.lapper_count over the ctg's rgs (sorted starts, sorted stop = end + 1) at (win.min(), win.max()),
fields 5-8 blanked when gc is not among the actions (data.rs:58-83)."""
import ctypes as C
import time

import numpy as np
import pytest

import helpers
from gams_amd import _lib, engine, host, synth
from oracle import oracle as ora

pytestmark = pytest.mark.gpu

ACTION_SETS = [("gc",), ("count",), ("gc", "count"), ("gibbs",)]
NO_GROUP = 0xFFFFFFFF


@pytest.fixture(scope="module")
def eng():
    e = engine.Engine(0)
    yield e
    e.close()


def all_ctgs(s288c, piece=100000):
    ctgs = []
    for chr_id in ("I", "Mito"):
        ctgs += helpers.gen_ctgs(chr_id, s288c[chr_id], piece=piece)
    return ctgs


def bucket_features(ctgs):
    """spo11_hot.rg bucketed by ctg as the feature loader does (utils.rs:39-67, first range of a ctg dropped)"""
    idx = helpers.ctg_index(ctgs)
    buckets = {}
    for ln in helpers.read_lines("spo11_hot.rg"):
        chr_id, s, e = helpers.parse_range(ln)
        hit = [i for i in idx.get(chr_id, []) if i[0] < e and i[1] > s]
        if not hit:
            continue
        cid = hit[0][2]
        if cid in buckets:
            buckets[cid].append((s, e))
        else:
            buckets[cid] = []
    return buckets


def features_of(c, buckets):
    return [(f"feature:{c['id']}:{i + 1}", s, e) for i, (s, e) in enumerate(buckets.get(c["id"], []))]


def rgs_by_ctg(records):
    """(ctg_id, range string) records -> ctg_id -> [(start, end)]"""
    out = {}
    for cid, rg in records:
        _, s, e = helpers.parse_range(rg)
        out.setdefault(cid, []).append((s, e))
    return out


def expected(c, feats, rgs, actions, size=100, mx=20, resize=500):
    """the oracle's text for one ctg; rgs = [(start, end)] of the ctg, None = the ctg has no rg group (count 0)"""
    if not feats:
        return ""
    text = ora.sw_proc_ctg(c["chr_id"], c["chr_start"], c["chr_end"], c["seq"], feats, size, mx, resize)
    st = np.sort(np.array([s for s, _ in rgs or []], np.int64)).astype(np.uint32)
    sp = np.sort(np.array([e + 1 for _, e in rgs or []], np.int64)).astype(np.uint32)
    rows = []
    for row in text.splitlines():
        f = row.split("\t")
        assert len(f) == 9 and f[8] == ""
        if "count" in actions:
            _, ws, we = helpers.parse_range(f[1])
            f[8] = str(ora.lapper_count(st, sp, ws, we)) if rgs is not None else "0"
        if "gc" not in actions:
            f[4:8] = ["", "", "", ""]
        rows.append("\t".join(f))
    return "\n".join(rows) + "\n"


# ---- S288c goldens -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def s288c_case(eng, s288c):
    ctgs = all_ctgs(s288c)
    buckets = bucket_features(ctgs)
    recs = host.read_range(eng, ctgs, helpers.read_lines("SK1.snp.rg"))    # the rg loader, drop-first quirk included
    assert len(recs) > 1000
    return ctgs, buckets, recs, rgs_by_ctg(recs)


@pytest.mark.parametrize("actions", ACTION_SETS)
def test_s288c_goldens_every_action_set(eng, s288c_case, actions):
    """spo11_hot.rg features x SK1.snp.rg rgs on every ctg, through the single-ctg operator (rows + the array count
    entry + the host formatter) and through the batched operator (text from the device)"""
    ctgs, buckets, recs, rg_of = s288c_case
    exp_all, counted = "", 0
    for c in sorted(ctgs, key=lambda c: c["id"]):
        feats = features_of(c, buckets)
        exp = expected(c, feats, rg_of.get(c["id"], []), actions)
        got = host.sw(eng, c, feats, actions=actions, rg_records=recs) if feats else ""
        assert got == exp, (c["id"], actions)
        exp_all += exp
        if "count" in actions:
            counted += sum(int(r.split("\t")[8]) > 0 for r in exp.splitlines())
    flist = [features_of(c, buckets) for c in sorted(ctgs, key=lambda c: c["id"])]
    got = host.sw_multi([eng], sorted(ctgs, key=lambda c: c["id"]), flist, actions=actions, rg_records=recs)
    assert got == exp_all
    if "count" in actions:
        assert counted > 100                       # the SNPs do land in windows
    if actions == ("gc",):
        c = next(c for c in ctgs if features_of(c, buckets))
        feats = features_of(c, buckets)
        assert host.sw(eng, c, feats, actions=actions, rg_records=recs) == host.sw(eng, c, feats)
        assert got == host.sw_multi([eng], sorted(ctgs, key=lambda c: c["id"]), flist)


# ---- random parameters, rgs placed on the windows' edges -------------------------------------------
def placed_rgs(rng, c, feats, size, mx, resize):
    """rgs on the windows the oracle makes: first / last base, ending on the first base, spanning many windows,
    past the ctg's ends, duplicates, and random ones"""
    text = ora.sw_proc_ctg(c["chr_id"], c["chr_start"], c["chr_end"], c["seq"], feats, size, mx, resize)
    wins = [helpers.parse_range(r.split("\t")[1])[1:] for r in text.splitlines()]
    pick = rng.choice(len(wins), min(len(wins), 400), replace=False)
    rgs = []
    for k, i in enumerate(pick):
        ws, we = wins[i]
        kind = k % 5
        if kind == 0:
            rgs.append((we, we))                          # starts on the window's last base: not counted there
        elif kind == 1:
            rgs.append((ws, ws))                          # on the first base
        elif kind == 2:
            rgs.append((max(1, ws - 7), ws))              # ends on the first base
        elif kind == 3:
            rgs.append((ws, we + 6 * size))               # spans several windows
        else:
            rgs.append((ws + (we - ws) // 2, ws + (we - ws) // 2))
    rgs += [(c["chr_start"] - 50, c["chr_start"] + 10), (c["chr_end"] - 10, c["chr_end"] + 300),
            (c["chr_start"] - 1000, c["chr_end"] + 1000)]  # past the ctg's ends, and over all of it
    rgs += rgs[:30]                                       # duplicates
    for _ in range(300):
        s = int(rng.integers(c["chr_start"], c["chr_end"] + 1))
        rgs.append((s, s + int(rng.choice([0, 0, 0, 1, 50, 2000]))))
    return rgs


@pytest.mark.parametrize("size,mx,resize", [(100, 20, 500), (100, 1, 100), (50, 5, 333), (10, 40, 5000), (100, 0, 500),
                                            (200, 3, 100)])
def test_sw_count_random_features(eng, s288c, size, mx, resize):
    ctgs = helpers.gen_ctgs("I", s288c["I"], piece=100000)
    c, bare = ctgs[1], ctgs[0]                              # I:100001-230218; I:1-100000 gets features, no rgs
    rng = np.random.default_rng(size * 1000 + mx + 7)
    feats = []
    for i in range(300):
        s = int(rng.integers(c["chr_start"], c["chr_end"] + 1))
        e = min(c["chr_end"], s + int(rng.choice([0, 0, 1, 2, 99, 100, 101, 1500])))
        feats.append((f"feature:{c['id']}:{i + 1}", s, e))
    feats += [(f"feature:{c['id']}:e{k}", p, p) for k, p in enumerate(
        [c["chr_start"], c["chr_start"] + 1, c["chr_start"] + 99, c["chr_end"], c["chr_end"] - 1, c["chr_end"] - 100])]
    rgs = placed_rgs(rng, c, feats, size, mx, resize)
    recs = [(c["id"], f"I:{s}-{e}") for s, e in rgs]
    bare_feats = [(f"feature:{bare['id']}:{i + 1}", p, p) for i, p in enumerate((500, 50000, 99990))]
    for actions in (("count",), ("gc", "count")):
        got = host.sw(eng, c, feats, size, mx, resize, actions=actions, rg_records=recs)
        assert got == expected(c, feats, rgs, actions, size, mx, resize), actions
        multi = host.sw_multi([eng], [bare, c], [bare_feats, feats], size, mx, resize, actions=actions, rg_records=recs)
        exp_bare = expected(bare, bare_feats, [], actions, size, mx, resize)
        assert multi == exp_bare + got
        assert all(r.endswith("\t0") for r in exp_bare.splitlines())


# ---- batching and devices ----------------------------------------------------------------------
@pytest.mark.parametrize("n_handles", [1, 2, 4])
def test_sw_multi_handles_equal_single_handle(eng, s288c_case, n_handles):
    """handles on device 0, as the other multi tests: LPT shares of the ctgs, each handle indexing its own ctgs' rgs"""
    ctgs, buckets, recs, rg_of = s288c_case
    flist = [features_of(c, buckets) for c in ctgs]
    actions = ("gc", "count")
    single = host.sw_multi([eng], ctgs, flist, actions=actions, rg_records=recs)
    per_ctg = "".join(host.sw(eng, c, f, actions=actions, rg_records=recs) for c, f in zip(ctgs, flist) if f)
    assert single == per_ctg
    engs = [eng] + [engine.Engine(0) for _ in range(n_handles - 1)]
    try:
        got = host.sw_multi(engs, ctgs, flist, actions=actions, rg_records=recs)
        text, ms = host.sw_multi_timed(engs, ctgs, flist, actions=actions, rg_records=recs)
    finally:
        for x in engs[1:]:
            x.close()
    assert got == single and text == single
    assert ms > 0.0 and 0.0 < host.last_sw_index_ms() <= ms


# ---- the array entry and the text entry, directly ----------------------------------------------
def batch_case(s288c, seed=3):
    rng = np.random.default_rng(seed)
    ctgs = helpers.gen_ctgs("I", s288c["I"], piece=30000)[:6]
    feats, rgs = [], []
    for k, c in enumerate(ctgs):
        n = 0 if k == 2 else int(rng.integers(5, 60))
        a = rng.integers(c["chr_start"], c["chr_end"] + 1, n)
        b = np.minimum(a + rng.choice([0, 1, 50, 999], n), c["chr_end"])
        feats.append([(f"feature:{c['id']}:{j + 1}", int(x), int(y)) for j, (x, y) in enumerate(zip(a, b))])
        s = rng.integers(max(1, c["chr_start"] - 100), c["chr_end"] + 100, 800)
        rgs.append([(int(x), int(x) + int(rng.choice([0, 0, 0, 5, 300]))) for x in s])
    return ctgs, feats, rgs


def build_index(eng, rgs_per_group):
    off = np.concatenate([[0], np.cumsum([len(g) for g in rgs_per_group])]).astype(np.uint64)
    st = np.array([s for g in rgs_per_group for s, _ in g], np.int64).astype(np.uint32)
    sp = np.array([e + 1 for g in rgs_per_group for _, e in g], np.int64).astype(np.uint32)
    return engine.Index(eng, off, st, sp)


def sel_arrays(ctgs, feats, sel):
    cst = [ctgs[i]["chr_start"] for i in sel]
    foff = np.concatenate([[0], np.cumsum([len(feats[i]) for i in sel])])
    fs = [f[1] for i in sel for f in feats[i]]
    fe = [f[2] for i in sel for f in feats[i]]
    ids = [f[0] for i in sel for f in feats[i]]
    return cst, foff, fs, fe, ids


def test_count_batch_equals_the_oracle_row_by_row(eng, s288c):
    """gams_gpu_sw_count_batch (the counts the host formatter takes when the text entry refuses): one count per row
    of gams_gpu_sw_batch, groups given per selected ctg -- reordered, repeated, UINT32_MAX and a group past the end
    (no group: 0)"""
    ctgs, feats, rgs = batch_case(s288c)
    ix = build_index(eng, rgs[:5])                               # ctg 5 has no group in the index
    ss = engine.SeqSet(eng, [c["seq"] for c in ctgs])
    for sel, grp in (([0, 1, 2, 3, 4, 5], [0, 1, 2, 3, 4, NO_GROUP]), ([4, 1, 1, 0], [4, 1, 1, 0]),
                     ([3, 5], [3, 77])):
        cst, foff, fs, fe, _ = sel_arrays(ctgs, feats, sel)
        cnt, roff = engine.sw_count_batch(eng, ss, sel, cst, foff, fs, fe, 100, 20, ix, grp)
        exp = []
        for i, g in zip(sel, grp):
            text = expected(ctgs[i], feats[i], rgs[i] if g < 5 else None, ("count",))
            exp += [int(r.split("\t")[8]) for r in text.splitlines()]
        assert cnt.tolist() == exp, sel
        assert int(roff[-1]) == len(exp)
        # the rows of gams_gpu_sw_batch, in the same order
        n = C.c_uint64()
        sel_a, cst_a, foff_a = np.array(sel, np.uint32), np.array(cst, np.int32), np.array(foff, np.uint64)
        fs_a, fe_a = np.array(fs, np.int32), np.array(fe, np.int32)
        rows = np.zeros(max(len(exp), 1), _lib.SW_ROW_DTYPE)
        eng.check(eng.lib.gams_gpu_sw_batch(eng.h, ss.p, len(sel), sel_a.ctypes.data, cst_a.ctypes.data, foff_a.ctypes.data,
                                            fs_a.ctypes.data, fe_a.ctypes.data, 100, 20, 500, rows.ctypes.data, rows.size,
                                            None, C.byref(n)))
        assert n.value == len(exp)
    ss.close()
    ix.close()


def test_count_only_reads_no_sequence_byte(eng, s288c):
    """-a count on a seqset whose bytes were never uploaded gives the text of the uploaded one, and the oracle's"""
    ctgs, feats, rgs = batch_case(s288c, seed=9)
    ix = build_index(eng, rgs)
    sel = list(range(len(ctgs)))
    cst, foff, fs, fe, ids = sel_arrays(ctgs, feats, sel)
    names = [c["chr_id"] for c in ctgs]
    up = engine.SeqSet(eng, [c["seq"] for c in ctgs])
    bare = engine.SeqSet(eng, [c["seq"] for c in ctgs], upload=False)
    rc, text_bare, off_bare = engine.sw_text_actions(eng, bare, sel, names, cst, foff, fs, fe, ids, 100, 20, 500,
                                                     _lib.SW_COUNT, ix, sel)
    assert rc == _lib.OK
    rc, text_up, off_up = engine.sw_text_actions(eng, up, sel, names, cst, foff, fs, fe, ids, 100, 20, 500, _lib.SW_COUNT,
                                                 ix, sel)
    assert rc == _lib.OK
    assert text_bare == text_up and np.array_equal(off_bare, off_up)
    exp = "".join(expected(c, f, r, ("count",)) for c, f, r in zip(ctgs, feats, rgs))
    assert text_bare.decode() == exp
    cnt, _ = engine.sw_count_batch(eng, bare, sel, cst, foff, fs, fe, 100, 20, ix, sel)
    assert cnt.tolist() == [int(r.split("\t")[8]) for r in exp.splitlines()]
    # with gc the same call on the uploaded set adds the statistics and keeps the counts
    rc, text_both, _ = engine.sw_text_actions(eng, up, sel, names, cst, foff, fs, fe, ids, 100, 20, 500,
                                              _lib.SW_GC | _lib.SW_COUNT, ix, sel)
    assert rc == _lib.OK
    assert text_both.decode() == "".join(expected(c, f, r, ("gc", "count")) for c, f, r in zip(ctgs, feats, rgs))
    # no action: the four statistics and rg_count empty; the geometry alone
    rc, text_none, _ = engine.sw_text_actions(eng, bare, sel, names, cst, foff, fs, fe, ids, 100, 20, 500, 0)
    assert rc == _lib.OK
    assert text_none.decode() == "".join(expected(c, f, r, ("gibbs",)) for c, f, r in zip(ctgs, feats, rgs))
    # gams_gpu_sw_text itself is unchanged: GAMS_SW_GC without an index
    rc, text_gc, _ = engine.sw_text_actions(eng, up, sel, names, cst, foff, fs, fe, ids, 100, 20, 500, _lib.SW_GC)
    assert rc == _lib.OK
    assert text_gc.decode() == "".join(expected(c, f, r, ("gc",)) for c, f, r in zip(ctgs, feats, rgs))
    for s in (up, bare):
        s.close()
    ix.close()


def test_sw_action_errors(eng, s288c):
    ctgs, feats, rgs = batch_case(s288c)
    ix = build_index(eng, rgs)
    sel = [0, 1]
    cst, foff, fs, fe, ids = sel_arrays(ctgs, feats, sel)
    names = [ctgs[i]["chr_id"] for i in sel]
    ss = engine.SeqSet(eng, [ctgs[i]["seq"] for i in sel])
    for bad in (4, 8, 0x80000000, 7):
        rc, _, _ = engine.sw_text_actions(eng, ss, [0, 1], names, cst, foff, fs, fe, ids, 100, 20, 500, bad, ix, [0, 1])
        assert rc == _lib.EINVAL, bad
    rc, _, _ = engine.sw_text_actions(eng, ss, [0, 1], names, cst, foff, fs, fe, ids, 100, 20, 500, _lib.SW_COUNT)
    assert rc == _lib.EINVAL
    assert "GAMS_SW_COUNT" in eng.lib.gams_gpu_last_error(eng.h).decode()
    n = C.c_uint64()
    sel_a, cst_a, foff_a = np.array([0, 1], np.uint32), np.array(cst, np.int32), np.array(foff, np.uint64)
    fs_a, fe_a = np.array(fs, np.int32), np.array(fe, np.int32)
    assert eng.lib.gams_gpu_sw_count_batch(eng.h, ss.p, 2, sel_a.ctypes.data, cst_a.ctypes.data, foff_a.ctypes.data,
                                           fs_a.ctypes.data, fe_a.ctypes.data, 100, 20, None, None, None, 0, None,
                                           C.byref(n)) == _lib.EINVAL
    # the existing rules hold: a feature whose middle lies outside the ctg
    rc, _, _ = engine.sw_text_actions(eng, ss, [0], names[:1], cst[:1], [0, 1], [cst[0] - 500], [cst[0] + 10], ["f:x"],
                                      100, 20, 500, _lib.SW_COUNT, ix, [0])
    assert rc == _lib.EINVAL
    with pytest.raises(ValueError):
        host.sw(eng, ctgs[0], feats[0], actions=("gc", "peak"))
    ss.close()
    ix.close()


# ---- scale -------------------------------------------------------------------------------------
def test_atha_shaped_1e5_features_1e6_rgs(eng):
    """configs[2]-shaped chromosome (30 Mb, piece 1e6 -> 30 ctgs), 1e5 point features, 1e6 rgs (SNP-like, a few
    long): -a gc -a count against the oracle on a sample of ctgs, within a few seconds"""
    rng = np.random.default_rng(17)
    chrom = synth.chromosome(30_000_000, 9)
    ctgs = synth.gen_ctgs("9", chrom, piece=1000000)
    flist = []
    for c in ctgs:
        fs = np.sort(rng.integers(c["chr_start"], c["chr_end"] + 1, 100000 // len(ctgs)))
        flist.append([(f"feature:{c['id']}:{i + 1}", int(s), int(s)) for i, s in enumerate(fs)])
    per = 1_000_000 // len(ctgs)
    rg_of, recs = {}, []
    for c in ctgs:
        s = rng.integers(c["chr_start"], c["chr_end"] + 1, per)
        ln = np.where(rng.random(per) < 0.001, rng.integers(100, 20000, per), 0)
        e = np.minimum(s + ln, c["chr_end"])
        rg_of[c["id"]] = list(zip(s.tolist(), e.tolist()))
        recs += [(c["id"], f"9:{a}-{b}") for a, b in rg_of[c["id"]]]
    assert len(recs) >= 990_000
    t0 = time.perf_counter()
    text, ms = host.sw_multi_timed([eng], ctgs, flist, actions=("gc", "count"), rg_records=recs)
    wall = time.perf_counter() - t0
    assert ms < 10_000 and wall < 60, (ms, wall)
    assert text.count("\n") > 3_000_000
    for k in (0, len(ctgs) // 2, len(ctgs) - 1):               # the rows of the ctg's first 400 features
        c = ctgs[k]
        exp = expected(c, flist[k][:400], rg_of[c["id"]], ("gc", "count"))
        at = text.find(f"sw:{flist[k][0][0]}:1\t")
        assert at >= 0 and (at == 0 or text[at - 1] == "\n")
        assert text[at:at + len(exp)] == exp, c["id"]
