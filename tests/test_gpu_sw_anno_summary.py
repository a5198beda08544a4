"""The Prop columns of the sw summary on the device: host.sw_summary(..., anno=) / host.sw_summary_table
and gams_gpu_sw_feature_summary_anno / gams_gpu_sw_summary_batch_anno through the C ABI, against the pure-Python model of
tests/sw_anno_summary.py over TEXT: the rows of host.sw_text with one column appended by host.anno_text per set -- the
reference's `gams sw | gams anno a.json stdin | gams anno b.json stdin` --, summed as integers.  Every comparison is exact.

Which reduction a call takes: (max + 1) * (10 + n_anno) <= 2560 words reduces in LDS (max <= 212 with two sets, <= 181
with four); beyond that the workgroups add to global memory directly, the Prop words included."""
import ctypes as C

import numpy as np
import pytest

import sw_anno_summary as sas
import sw_text as swt
from gams_amd import _lib, engine, host
from test_gpu_sw_summary import Acc, abi_sum, same_tables
from test_gpu_sw_text import SwTables, seq_arrays
from test_gpu_text_ops import all_ctgs, read_bytes

pytestmark = pytest.mark.gpu

L = _lib.load()
GC, COUNT = _lib.SW_GC, _lib.SW_COUNT
NONE = 0xFFFFFFFF


@pytest.fixture(scope="module")
def eng():
    e = engine.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def synth(eng):
    """the three synthetic ctgs, their feature file, and the two resident sets: (prefix, AnnoSet, {chr: (lo, hi)})"""
    ctgs = sas.synth_ctgs()
    data = sas.synth_features(ctgs)
    rows = swt.model(ctgs, data)
    edges = sorted({int(sas.RANGE.match(r.split(b"\t")[1]).group(2)) for r in rows.split(b"\n")[:-1]
                    if r.split(b"\t")[0].startswith(b"sw:feature:ctg:A:1:")})
    dense, sparse = sas.dense_set(ctgs, edges), sas.sparse_set(ctgs)
    sets = [("dense", host.AnnoSet(eng, sas.runlist_json(dense)), dense), ("sparse", host.AnnoSet(eng, sas.runlist_json(sparse)), sparse)]
    yield ctgs, data, sets
    for _, aset, _ in sets:
        aset.close()


@pytest.fixture(scope="module")
def long_ctg(eng):
    """one ctg of 70 kb, 40 features, and four sets on its chromosome (spans of 100-3000 bases at four densities)"""
    ctgs = sas.one_ctg()
    data = sas.synth_features(ctgs, mx=300, seed=29, n=40)
    sets = [("s%d" % k, host.AnnoSet(eng, sas.runlist_json(sas.sparse_set(ctgs, seed=31 + k)))) for k in range(4)]
    yield ctgs, data, sets
    for _, aset in sets:
        aset.close()


def annotated(eng, ctgs, data, sets, size=100, mx=20, resize=500, actions=("gc",), **kw):
    """the model's input: host.sw_text's rows with host.anno_text's column per set (both pinned by their own tests)"""
    rows = host.sw_text(eng, ctgs, data, size=size, mx=mx, resize=resize, actions=actions, **kw)
    for s in sets:
        rows = host.anno_text(eng, ctgs, s[1], rows)
    return rows


def pairs(sets):
    return [(s[0], s[1]) for s in sets]


def test_golden_rg_file_and_the_same_set_twice(eng, s288c):
    """S288c chr I and Mito ctgs, spo11_hot.rg, intergenic.json: one set, then the same set under two prefixes"""
    ctgs = all_ctgs(s288c)
    data = read_bytes("spo11_hot.rg")
    js = read_bytes("intergenic.json")
    aset = host.AnnoSet(eng, js)
    try:
        want, model = sas.summary([annotated(eng, ctgs, data, [("intergenic", aset)])], ["intergenic"])
        got = host.sw_summary(eng, ctgs, data, anno=[("intergenic", aset)])
        assert host.last_operator_device() == 1
        assert got == want and model.rows() > 2000
        assert got.split(b"\n")[0] == b"distance\tAVG_gc_content\tAVG_gc_mean\tAVG_gc_stddev\tAVG_gc_cv\tAVG_intergenicProp\tCOUNT"
        assert any(0 < int(v) < 10000 * model.groups[k][0] for k in model.groups for v in model.groups[k][4])
        assert host.sw_summary(eng, ctgs, data, anno=[("intergenic", js)]) == want     # bytes build a set for the call
        twice = host.sw_summary(eng, ctgs, data, anno=[("a", aset), ("b", aset)])
        assert twice == sas.summary([annotated(eng, ctgs, data, [("a", aset), ("b", aset)])], ["a", "b"])[0]
        body = [ln.split(b"\t") for ln in twice.split(b"\n")[1:-1]]
        assert len(body) == 21 and all(ln[5] == ln[6] for ln in body)
        assert [ln[5] for ln in body] == [ln.split(b"\t")[5] for ln in got.split(b"\n")[1:-1]]
    finally:
        aset.close()


@pytest.mark.parametrize("size,mx,resize", [(100, 20, 500), (32, 20, 160), (100, 0, 500)])
def test_synthetic_sets(eng, synth, size, mx, resize):
    ctgs, data, sets = synth
    rows = annotated(eng, ctgs, data, sets, size, mx, resize)
    want, model = sas.summary([rows], ["dense", "sparse"])
    got = host.sw_summary(eng, ctgs, data, size=size, mx=mx, resize=resize, anno=pairs(sets))
    assert host.last_operator_device() == 1
    assert got == want
    tab = host.sw_summary_table(eng, ctgs, data, size=size, mx=mx, resize=resize, anno=pairs(sets))
    assert tab["prop"].dtype == np.uint64 and np.array_equal(tab["prop"], model.prop(mx))
    assert same_tables(tab, model.arrays(mx)) and got.count(b"\n") == mx + 2
    q = [(r.split(b"\t")[0], sas.prop_units(r.split(b"\t")[9]), sas.prop_units(r.split(b"\t")[10])) for r in rows.split(b"\n")[:-1]]
    assert all(a == 10000 for i, a, _ in q if i.startswith(b"sw:feature:ctg:A:2:"))      # the span over the whole ctg
    assert all(b == 0 for i, _, b in q if i.startswith(b"sw:feature:ctg:B:1:"))          # the absent chromosome
    assert any(a == 0 for i, a, _ in q if i.startswith(b"sw:feature:ctg:A:1:"))          # the stretch with no span
    if size == 32:                                              # props of k / 32: rows whose q is the even side of a tie
        full = [a for (i, a, _), r in zip(q, rows.split(b"\n")) if b"-" in r.split(b"\t")[1] and
                int(r.split(b"\t")[1].split(b"-")[1]) - int(r.split(b"\t")[1].split(b":")[1].split(b"-")[0]) == 31]
        assert any(a in set(sas.tie_units(32).values()) for a in full)
    # the device's cover equals the oracle's on these rows: the model's second source
    assert sas.annotate(sas.annotate(host.sw_text(eng, ctgs, data, size=size, mx=mx, resize=resize), ctgs, sets[0][2]),
                        ctgs, sets[1][2]) == rows


@pytest.mark.parametrize("n_sets,mx", [(2, 300),               # 301 groups: the global path carries Prop words
                                       (4, 181), (4, 182),     # four sets: the last max in LDS, the first beyond it
                                       (1, 231), (1, 232)])
def test_lds_threshold_and_global_path(eng, long_ctg, n_sets, mx):
    ctgs, data, sets = long_ctg
    use = sets[:n_sets]
    want, model = sas.summary([annotated(eng, ctgs, data, use, mx=mx)], [p for p, _ in use])
    got = host.sw_summary(eng, ctgs, data, mx=mx, anno=use)
    assert host.last_operator_device() == 1
    assert got == want and got.count(b"\n") == mx + 2
    assert np.array_equal(host.sw_summary_table(eng, ctgs, data, mx=mx, anno=use)["prop"], model.prop(mx))
    assert all(int(model.prop(mx)[0, :, a].sum()) > 0 for a in range(n_sets))


@pytest.fixture(scope="module")
def rg(eng, synth):
    ctgs = synth[0]
    lines = [ln.decode() for ln in sas.synth_features(ctgs, seed=41, n=900).split(b"\n")[:-1]]
    return "\n".join(lines).encode(), host.read_range(eng, ctgs, lines)


@pytest.mark.parametrize("actions", [("count",), ("gc", "count"), ("gibbs",)])
def test_actions(eng, synth, rg, actions):
    """the Prop columns do not depend on the action mask; count-only and gibbs read no sequence byte"""
    ctgs, data, sets = synth
    kw = dict(rg_data=rg[0]) if "count" in actions else {}
    want, model = sas.summary([annotated(eng, ctgs, data, sets, actions=actions, **kw)], ["dense", "sparse"], actions=actions)
    head = ([b"distance"] + ([b"AVG_gc_content", b"AVG_gc_mean", b"AVG_gc_stddev", b"AVG_gc_cv"] if "gc" in actions else []) +
            [b"AVG_denseProp", b"AVG_sparseProp"] + ([b"AVG_rg_count"] if "count" in actions else []) + [b"COUNT"])
    assert want.split(b"\n")[0].split(b"\t") == head
    got = host.sw_summary(eng, ctgs, data, actions=actions, anno=pairs(sets), **kw)
    assert got == want and host.last_operator_device() == 1
    if "count" in actions:
        assert any(g[3] for g in model.groups.values())
    if "gc" not in actions:
        bare = [{k: v for k, v in c.items() if k != "seq"} for c in ctgs]
        assert host.sw_summary(eng, bare, data, actions=actions, anno=pairs(sets), **kw) == want
        gc_tab = host.sw_summary_table(eng, ctgs, data, anno=pairs(sets))
        assert np.array_equal(host.sw_summary_table(eng, bare, data, actions=actions, anno=pairs(sets), **kw)["prop"], gc_tab["prop"])


def test_tags_slots_and_repeatability(eng, synth):
    ctgs, a_data, sets = synth
    b_data, a2_data = sas.synth_features(ctgs, seed=43, n=90), sas.synth_features(ctgs, seed=47, n=45)
    files, tags = [a_data, b_data, a2_data], ["hot", "cold", "hot"]
    texts = [annotated(eng, ctgs, d, sets) for d in files]
    want, model = sas.summary(texts, ["dense", "sparse"], [b"hot", b"cold", b"hot"])
    got = host.sw_summary(eng, ctgs, files, tags=tags, anno=pairs(sets))
    assert got == want and host.last_operator_device() == 1
    assert got.startswith(b"tag\tdistance\t") and [ln.split(b"\t")[0] for ln in got.split(b"\n")[1:-1]] == [b"cold"] * 21 + [b"hot"] * 21
    tab = host.sw_summary_table(eng, ctgs, files, tags=tags, anno=pairs(sets))
    assert tab["tags"] == [b"cold", b"hot"] and np.array_equal(tab["prop"], model.prop(20, [b"hot", b"cold", b"hot"]))
    assert host.sw_summary(eng, ctgs, files, tags=tags, anno=pairs(sets)) == got        # two calls, the same bytes
    # a resident seqset in another order than the ctgs
    seqs = seq_arrays(ctgs)
    perm = [2, 0, 1]
    ss = engine.SeqSet(eng, [seqs[perm.index(k)] for k in range(3)])
    try:
        moved = [dict(c, slot=perm[i]) for i, c in enumerate(ctgs)]
        assert host.sw_summary(eng, moved, files, tags=tags, seqset=ss, anno=pairs(sets)) == want
        assert host.last_operator_device() == 1
    finally:
        ss.close()


def test_no_change_without_sets(eng, synth):
    ctgs, data, sets = synth
    plain = host.sw_summary(eng, ctgs, data)
    assert plain == host.sw_summary(eng, ctgs, data, anno=None) == host.sw_summary(eng, ctgs, data, anno=[])
    assert b"Prop" not in plain
    assert "prop" not in host.sw_summary_table(eng, ctgs, data)
    assert host.sw_summary_table(eng, ctgs, data, anno=[])["prop"].shape == (1, 21, 0)
    # the ten words are the same with and without sets
    assert same_tables(host.sw_summary_table(eng, ctgs, data, anno=pairs(sets)), host.sw_summary_table(eng, ctgs, data))


def test_ctg_ids_anno_would_not_find_are_refused(eng, synth):
    ctgs, data, sets = synth
    odd = [dict(c, id=c["id"].replace("ctg:B:1", "ctg:B-x:1")) for c in ctgs]
    assert host.sw_summary(eng, odd, data).count(b"\n") == 22      # without sets nothing changes
    with pytest.raises(ValueError):
        host.sw_summary(eng, odd, data, anno=pairs(sets))
    with pytest.raises(ValueError):
        host.sw_summary(eng, ctgs, data, anno=pairs(sets) * 3)      # six sets
    with pytest.raises(ValueError):
        host.sw_summary(eng, ctgs, data, anno=[("x", {"A": "1-5"})])


def test_host_fallback_carries_the_sets(eng, synth, rg):
    """a byte the loader refuses: the rows come from gams_gpu_sw_batch and the Prop units from gams_gpu_cover"""
    ctgs, data, sets = synth
    hi = data + b"nonsense \xc3\xa9\n"
    for actions, kw in ((("gc",), {}), (("gc", "count"), dict(rg_data=rg[0])), (("count",), dict(rg_data=rg[0]))):
        want = sas.summary([annotated(eng, ctgs, data, sets, actions=actions, **kw)], ["dense", "sparse"], actions=actions)[0]
        assert host.sw_summary(eng, ctgs, hi, actions=actions, anno=pairs(sets), **kw) == want
        assert host.last_operator_device() == 0
    both = host.sw_summary(eng, ctgs, [data, hi], tags=["t", "t"], anno=pairs(sets))
    assert both == host.sw_summary(eng, ctgs, [data, data], tags=["t", "t"], anno=pairs(sets))


# ---- the C ABI ----------------------------------------------------------------------------------------------------------
class AnnoAcc(Acc):
    """a gams_sw_summary_t made for n_anno sets"""

    def __init__(self, eng, n_anno, mx=20, n_tags=1, actions=GC, size=100, resize=500):
        self.eng, self.mx, self.n_tags, self.n_anno = eng, mx, n_tags, n_anno
        self.p = C.c_void_p()
        rc = L.gams_sw_summary_create_anno(eng.h, mx, n_tags, actions, size, resize, n_anno, C.byref(self.p))
        assert rc == 0, L.gams_gpu_last_error(eng.h)

    def read_prop(self):
        a = np.full(self.n_tags * (self.mx + 1) * max(self.n_anno, 1), 77, np.uint64)
        assert L.gams_sw_summary_read_anno(self.eng.h, self.p, a.ctypes.data) == 0
        return a.reshape(self.n_tags, self.mx + 1, -1)[:, :, :self.n_anno]

    def everything(self):
        w = self.read()
        return np.concatenate([w[k].ravel() for k in ("count", "sum", "nan", "rg_count")] + [self.read_prop().ravel()])


def set_args(sets, order):
    """(n, the array of gams_spans_t*, the array of set_group columns, what must outlive the call)"""
    cols = [np.array([s.names.index(c["chr_id"]) if c["chr_id"] in s.names else NONE for c in order], np.uint32) for s in sets]
    sp = (C.c_void_p * max(len(sets), 1))(*[s._sp for s in sets])
    cp = (C.c_void_p * max(len(sets), 1))(*[c.ctypes.data for c in cols])
    return len(sets), sp, cp, cols


def abi_sum_anno(eng, T, ss, data, acc, n, sp, cp, tag=0, size=100, mx=20, resize=500, actions=GC):
    nf, rows = C.c_uint64(), C.c_uint64()
    rc = L.gams_gpu_sw_feature_summary_anno(eng.h, None if ss is None else ss.p, T.ix, T.chr, T.ids, T.slot.ctypes.data,
                                            T.cs.ctypes.data, T.ce.ctypes.data, data, len(data), size, mx, resize, actions,
                                            None, None, acc.p, tag, n, sp, cp, C.byref(nf), C.byref(rows))
    return rc, nf.value, rows.value


def test_abi_entries_reset_and_error_paths(eng, synth):
    ctgs, data, named = synth
    sets = [s[1] for s in named]
    model = sas.summary([annotated(eng, ctgs, data, named)], ["dense", "sparse"])[1]
    ss = engine.SeqSet(eng, seq_arrays(ctgs))
    T = SwTables(eng, ctgs)
    acc, arr, plain, four = AnnoAcc(eng, 2, n_tags=2), AnnoAcc(eng, 2), Acc(eng), AnnoAcc(eng, 4)
    try:
        n, sp, cp, keep = set_args(sets, T.order)
        rc, nf, rows = abi_sum_anno(eng, T, ss, data, acc, n, sp, cp, tag=1)
        assert rc == 0, L.gams_gpu_last_error(eng.h)
        assert rows == model.rows() and np.array_equal(acc.read_prop()[1], model.prop(20)[0]) and not acc.read_prop()[0].any()
        before = acc.everything()
        # every refusal leaves all words, Prop words included, as they were
        assert abi_sum_anno(eng, T, ss, data, acc, 1, sp, cp)[0] == _lib.EINVAL               # made for two sets
        assert abi_sum_anno(eng, T, ss, data, acc, 0, None, None)[0] == _lib.EINVAL
        assert abi_sum(eng, T, ss, data, acc)[0] == _lib.EINVAL                               # the entry without sets
        assert abi_sum_anno(eng, T, ss, data, acc, 5, sp, cp)[0] == _lib.EINVAL               # beyond GAMS_SW_SUMMARY_MAX_ANNO
        null_set = (C.c_void_p * 2)(sets[0]._sp, None)
        assert abi_sum_anno(eng, T, ss, data, acc, 2, null_set, cp)[0] == _lib.EINVAL
        null_col = (C.c_void_p * 2)(keep[0].ctypes.data, None)
        assert abi_sum_anno(eng, T, ss, data, acc, 2, sp, null_col)[0] == _lib.EINVAL
        assert abi_sum_anno(eng, T, ss, data, acc, 2, None, cp)[0] == _lib.EINVAL
        assert abi_sum_anno(eng, T, ss, data, acc, n, sp, cp, tag=2)[0] == _lib.EINVAL
        assert abi_sum_anno(eng, T, ss, data, acc, n, sp, cp, mx=19)[0] == _lib.EINVAL
        assert abi_sum_anno(eng, T, ss, data + b"nonsense \xc3\xa9\n", acc, n, sp, cp)[0] == _lib.EUNSUPPORTED
        assert abi_sum_anno(eng, T, ss, data, plain, n, sp, cp)[0] == _lib.EINVAL             # an accumulator without sets
        assert np.array_equal(acc.everything(), before) and not plain.read()["count"].any()
        p = C.c_void_p()
        assert L.gams_sw_summary_create_anno(eng.h, 20, 1, GC, 100, 500, 5, C.byref(p)) == _lib.EINVAL and not p.value
        # a second call adds the same again; reset zeroes the Prop words too
        assert abi_sum_anno(eng, T, ss, data, acc, n, sp, cp, tag=1)[0] == 0
        assert np.array_equal(acc.everything(), 2 * before)
        acc.reset()
        assert not acc.everything().any()
        assert abi_sum_anno(eng, T, ss, data, acc, n, sp, cp, tag=1) == (0, nf, rows) and np.array_equal(acc.everything(), before)
        # four sets at once: the two sets, each twice
        n4, sp4, cp4, keep4 = set_args(sets + sets, T.order)
        assert abi_sum_anno(eng, T, ss, data, four, n4, sp4, cp4)[0] == 0
        p4 = four.read_prop()[0]
        assert np.array_equal(p4[:, :2], model.prop(20)[0]) and np.array_equal(p4[:, 2:], model.prop(20)[0])
        # gams_gpu_sw_summary_batch_anno over the model's features as arrays
        feats = swt.features(ctgs, data)
        sel = [i for i in range(len(ctgs)) if feats[i]]
        index = np.array(sel, np.uint32)
        cs = np.array([ctgs[i]["chr_start"] for i in sel], np.int32)
        off = np.cumsum([0] + [len(feats[i]) for i in sel]).astype(np.uint64)
        fs = np.array([f[1] for i in sel for f in feats[i]], np.int32)
        fe = np.array([f[2] for i in sel for f in feats[i]], np.int32)
        nb, spb, cpb, keepb = set_args(sets, [ctgs[i] for i in sel])
        n_rows = C.c_uint64()

        def batch(a, n_, sp_, cp_, entry=L.gams_gpu_sw_summary_batch_anno):
            args = [eng.h, ss.p, len(sel), index.ctypes.data, cs.ctypes.data, off.ctypes.data, fs.ctypes.data, fe.ctypes.data,
                    100, 20, 500, GC, None, None, a.p, 0]
            if entry is L.gams_gpu_sw_summary_batch_anno:
                args += [n_, sp_, cp_]
            return entry(*args, C.byref(n_rows))

        assert batch(arr, nb, spb, cpb) == 0, L.gams_gpu_last_error(eng.h)
        assert n_rows.value == rows and np.array_equal(arr.read_prop(), model.prop(20))
        assert same_tables(arr.read(), {k: v[1:2] for k, v in acc.read().items()})
        kept = arr.everything()
        assert batch(arr, 1, spb, cpb) == _lib.EINVAL and batch(arr, 2, null_set, cpb) == _lib.EINVAL
        assert batch(arr, 2, spb, null_col) == _lib.EINVAL and batch(arr, 5, spb, cpb) == _lib.EINVAL
        assert batch(arr, 0, None, None, entry=L.gams_gpu_sw_summary_batch) == _lib.EINVAL    # the existing entry refuses it
        assert batch(plain, nb, spb, cpb) == _lib.EINVAL
        assert np.array_equal(arr.everything(), kept)
        assert batch(plain, 0, None, None) == 0 and int(plain.read()["count"].sum()) == rows   # n_anno 0: the entry without sets
    finally:
        for a in (acc, arr, plain, four):
            a.close()
        T.close()
        ss.close()
