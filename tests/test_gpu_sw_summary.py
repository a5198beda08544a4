"""The sw summary on the device: gams_gpu_sw_feature_summary / gams_gpu_sw_summary_batch through the C ABI and
host.sw_summary / host.sw_summary_table above them, against the pure-Python model of tests/sw_summary.py over the text of
the rows (tests/sw_text.py's model, host.sw_text and host.sw_multi).  All sums are integers: every comparison is exact.

Which reduction a parameter set takes (a workgroup keeps max + 1 <= 256 distances, 20 KiB, in LDS):
every case here but `size=10, mx=2000` has at most 41 distances and reduces in LDS; mx=2000 has 2001 groups and adds to
global memory directly."""
import ctypes as C

import numpy as np
import pytest

import sw_summary as sws
import sw_text as swt
from gams_amd import _lib, engine, host
from test_gpu_sw_text import SwTables, abi_sw, multi, seq_arrays
from test_gpu_text_ops import all_ctgs, read_bytes

pytestmark = pytest.mark.gpu

L = _lib.load()
GC, COUNT = _lib.SW_GC, _lib.SW_COUNT
STAGES = 10                # lines parse locate first keep offsets order | gather geometry rows


@pytest.fixture(scope="module")
def eng():
    e = engine.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def synth():
    """the synthetic ctgs, the bytes of their feature file (about 4000 lines), the model's features and its rows"""
    ctgs = swt.synth_ctgs()
    data = swt.synth_data(swt.synth_lines(ctgs))
    return ctgs, data, swt.features(ctgs, data), swt.model(ctgs, data)


@pytest.fixture(scope="module")
def small(synth):
    """the same ctgs under a file of 600 lines with the same edge lines, and one of 40 for the 2001-distance case"""
    ctgs = synth[0]
    return (swt.synth_data(swt.synth_lines(ctgs, seed=37, n=600)), swt.synth_data(swt.synth_lines(ctgs, seed=41, n=40)))


@pytest.fixture(scope="module")
def rg(eng, synth):
    """an rg file over the same ctgs (no tab in a line) and the rg: records read_range makes of its lines"""
    ctgs = synth[0]
    lines = [ln for ln in swt.synth_lines(ctgs, seed=31, n=1500) if "\t" not in ln]
    return "\n".join(lines).encode(), host.read_range(eng, ctgs, lines)


class Acc:
    """a gams_sw_summary_t"""

    def __init__(self, eng, mx=20, n_tags=1, actions=GC, size=100, resize=500):
        self.eng, self.mx, self.n_tags = eng, mx, n_tags
        self.p = C.c_void_p()
        rc = L.gams_sw_summary_create(eng.h, mx, n_tags, actions, size, resize, C.byref(self.p))
        assert rc == 0, L.gams_gpu_last_error(eng.h)

    def read(self):
        n = self.n_tags * (self.mx + 1)
        a = [np.full(k * n, 77, np.uint64) for k in (1, 4, 4, 1)]
        assert L.gams_sw_summary_read(self.eng.h, self.p, *[x.ctypes.data for x in a]) == 0
        sh = (self.n_tags, self.mx + 1)
        return dict(count=a[0].reshape(sh), sum=a[1].reshape(sh + (4,)), nan=a[2].reshape(sh + (4,)), rg_count=a[3].reshape(sh))

    def reset(self):
        assert L.gams_sw_summary_reset(self.eng.h, self.p) == 0

    def close(self):
        L.gams_sw_summary_destroy(self.eng.h, self.p)


def abi_sum(eng, T, ss, data, acc, tag=0, size=100, mx=20, resize=500, actions=GC, rg=True):
    """(rc, n_features, n_rows) of gams_gpu_sw_feature_summary"""
    nf, rows = C.c_uint64(), C.c_uint64()
    count = bool(actions & COUNT) and rg
    rc = L.gams_gpu_sw_feature_summary(eng.h, None if ss is None else ss.p, T.ix, T.chr, T.ids, T.slot.ctypes.data,
                                       T.cs.ctypes.data, T.ce.ctypes.data, data, len(data), size, mx, resize, actions,
                                       T.rg_ix if count else None, T.rg_group.ctypes.data if count else None, acc.p, tag,
                                       C.byref(nf), C.byref(rows))
    return rc, nf.value, rows.value


def same_tables(a, b):
    return all(np.array_equal(np.asarray(a[k], np.uint64), np.asarray(b[k], np.uint64)) for k in ("count", "sum", "nan", "rg_count"))


def test_main_case(eng, synth):
    """about 1.6e5 rows in hundreds of workgroups; 41 slots a feature do not divide 256: features straddle the seams"""
    ctgs, data, feats, rows_text = synth
    want, model = sws.summary([rows_text])
    got = host.sw_summary(eng, ctgs, data)
    assert host.last_operator_device() == 1
    assert got == want
    assert got.count(b"\n") == 22 and model.rows() > 100000
    tab = host.sw_summary_table(eng, ctgs, data)
    assert tab["tags"] is None and same_tables(tab, model.arrays(20))
    ss = engine.SeqSet(eng, seq_arrays(ctgs))
    T = SwTables(eng, ctgs)
    try:
        rc, _, _, nf, n_rows = abi_sw(eng, T, ss, data)
        assert rc == 0 and int(tab["count"].sum()) == n_rows == model.rows()
    finally:
        T.close()
        ss.close()
    assert got == sws.summary([host.sw_text(eng, ctgs, data)])[0]


def test_golden_rg_file(eng, s288c):
    ctgs = all_ctgs(s288c)
    data = read_bytes("spo11_hot.rg")
    want, model = sws.summary([swt.model(ctgs, data)])
    assert host.sw_summary(eng, ctgs, data) == want and host.last_operator_device() == 1
    assert same_tables(host.sw_summary_table(eng, ctgs, data), model.arrays(20))
    assert want == sws.summary([host.sw_text(eng, ctgs, data)])[0] and model.rows() > 2000


@pytest.mark.parametrize("size,mx,resize,which", [(100, 0, 500, 0),        # one group (LDS)
                                                  (10, 2000, 500, 1),      # 2001 groups: the global path
                                                  (100, 20, 100, 0),       # one flank tile: stddev and cv are NaN
                                                  (100, 20, 50, 0),        # no tile: the mean is NaN too, stddev is -0
                                                  (50, 5, 333, 0)])
def test_parameters(eng, synth, small, size, mx, resize, which):
    ctgs = synth[0]
    data = small[which]
    want, model = sws.summary([swt.model(ctgs, data, size, mx, resize)])
    got = host.sw_summary(eng, ctgs, data, size=size, mx=mx, resize=resize)
    assert host.last_operator_device() == 1
    assert got == want
    assert same_tables(host.sw_summary_table(eng, ctgs, data, size=size, mx=mx, resize=resize), model.arrays(mx))
    lines = [ln.split(b"\t") for ln in got.split(b"\n")[1:-1]]
    if mx == 0:
        assert len(lines) == 1 and lines[0][0] == b"0"
    if mx == 2000:
        assert len(lines) > 257 and model.rows() > 20000
    if resize == 100:                                          # (an M window cut short at a ctg's edge has no tile at all)
        assert all(ln[3] == b"nan" and ln[4] == b"nan" for ln in lines)
        assert all(ln[2] != b"nan" for ln in lines if ln[0] != b"0") and len(lines) == 21
    if resize == 50:
        # no tile: mean = 0 / 0 and cv are NaN; the deviation is sqrt(0 / (0 - 1)) = sqrt(-0) = -0 (stat.rs:13), which the
        # rows print as "-0" and the table counts as 0
        assert b"\t-0\t" in swt.model(ctgs, data, size, mx, resize)
        assert all(ln[1] != b"nan" and ln[2] == b"nan" and ln[3] == b"0" and ln[4] == b"nan" for ln in lines)


def test_single_feature_and_no_kept_line(eng, synth):
    ctgs = synth[0]
    one = b"I:100-200\nI:5000-5100\n"                          # the first located line of the ctg is dropped
    want, model = sws.summary([swt.model(ctgs, one)])
    assert host.sw_summary(eng, ctgs, one) == want and model.groups[(None, 0)][0] == 1
    for empty in (b"", b"# ranges\nI:5-9\n"):
        assert host.sw_summary(eng, ctgs, empty) == sws.Table().header(False)
        assert host.last_operator_device() == 1
        assert not host.sw_summary_table(eng, ctgs, empty)["count"].any()
    assert host.sw_summary(eng, ctgs, []) == sws.Table().header(False)      # no file at all


def test_exact_tie_rounds_to_even(eng, synth):
    """two M rows whose gc_content m add up to an odd number: S / COUNT lies exactly between two integers"""
    ctgs = synth[0]
    data = sws.tie_data(ctgs, lambda d: swt.model(ctgs, d))
    want, model = sws.summary([swt.model(ctgs, data)])
    assert (None, 0, 0) in sws.ties(model)
    assert host.sw_summary(eng, ctgs, data) == want and host.last_operator_device() == 1


@pytest.mark.parametrize("actions", [("count",), ("gc", "count")])
def test_actions(eng, synth, rg, actions):
    ctgs, data, feats, _ = synth
    rg_data, rg_records = rg
    rows_text = multi(eng, ctgs, feats, actions=actions, rg_records=rg_records)
    want, model = sws.summary([rows_text], actions=actions)
    assert want.split(b"\n")[0].split(b"\t") == ([b"distance"] + ([b"AVG_gc_content", b"AVG_gc_mean", b"AVG_gc_stddev",
                                                  b"AVG_gc_cv"] if "gc" in actions else []) + [b"AVG_rg_count", b"COUNT"])
    assert any(g[3] for g in model.groups.values())
    for kw in (dict(rg_records=rg_records), dict(rg_data=rg_data), dict(rg_data=[rg_data])):
        assert host.sw_summary(eng, ctgs, data, actions=actions, **kw) == want and host.last_operator_device() == 1
    assert same_tables(host.sw_summary_table(eng, ctgs, data, actions=actions, rg_data=rg_data), model.arrays(20))
    if actions == ("count",):                                  # no sequence is read: the ctgs need not carry one
        bare = [{k: v for k, v in c.items() if k != "seq"} for c in ctgs]
        assert host.sw_summary(eng, bare, data, actions=actions, rg_data=rg_data) == want


def test_tags(eng, synth, small):
    ctgs, a_data, _, a_rows = synth
    b_data, a2_data = small
    b_rows, a2_rows = swt.model(ctgs, b_data), swt.model(ctgs, a2_data)
    files, tags = [a_data, b_data, a2_data], ["hot", "cold", "hot"]
    want, model = sws.summary([a_rows, b_rows, a2_rows], [b"hot", b"cold", b"hot"])
    got = host.sw_summary(eng, ctgs, files, tags=tags)
    assert got == want and host.last_operator_device() == 1
    body = got.split(b"\n")[1:-1]
    assert got.startswith(b"tag\tdistance\t") and [ln.split(b"\t")[0] for ln in body] == [b"cold"] * 21 + [b"hot"] * 21
    tab = host.sw_summary_table(eng, ctgs, files, tags=tags)
    assert tab["tags"] == [b"cold", b"hot"] and same_tables(tab, model.arrays(20, [b"hot", b"cold", b"hot"]))
    ta, tb, ta2 = (host.sw_summary_table(eng, ctgs, d) for d in files)
    for k in ("count", "sum", "nan", "rg_count"):
        assert np.array_equal(tab[k][1], ta[k][0] + ta2[k][0]) and np.array_equal(tab[k][0], tb[k][0])
    # drop-first is per file: two files are not their concatenation
    joined = host.sw_summary_table(eng, ctgs, a_data + b"\n" + a2_data)
    assert int(joined["count"].sum()) > int(tab["count"][1].sum())
    # untagged, several files fall into one slot
    assert same_tables(host.sw_summary_table(eng, ctgs, [a_data, a2_data]), {k: tab[k][1:2] for k in tab if k != "tags"})


def test_paths_and_repeatability(eng, synth):
    ctgs, data, _, rows_text = synth
    want = sws.summary([rows_text])[0]
    seqs = seq_arrays(ctgs)
    perm = [3, 0, 5, 1, 4, 2]                                  # the seqset in another order than the ctgs
    ss = engine.SeqSet(eng, [seqs[perm.index(k)] for k in range(6)])
    T = SwTables(eng, ctgs, perm)
    acc = Acc(eng)
    try:
        moved = [dict(c, slot=perm[i]) for i, c in enumerate(ctgs)]
        assert host.sw_summary(eng, moved, data, seqset=ss) == want and host.last_operator_device() == 1
        assert host.sw_summary(eng, ctgs, data) == want
        assert host.sw_summary(eng, moved, data, seqset=ss) == want
        rc, nf, rows = abi_sum(eng, T, ss, data, acc)
        assert rc == 0, L.gams_gpu_last_error(eng.h)
        first = acc.read()
        assert int(first["count"].sum()) == rows == rows_text.count(b"\n")
        ms = (C.c_float * 16)()
        n = C.c_uint32()
        assert L.gams_gpu_last_stage_ms(eng.h, ms, 16, C.byref(n)) == 0 and n.value == STAGES
        assert all(ms[k] >= 0 for k in range(STAGES))
        assert abi_sum(eng, T, ss, data, acc)[0] == 0          # a second call adds the same again
        twice = acc.read()
        assert all(np.array_equal(twice[k], 2 * first[k]) for k in first)
        acc.reset()
        assert not acc.read()["count"].any()
        assert abi_sum(eng, T, ss, data, acc) == (0, nf, rows) and same_tables(acc.read(), first)
    finally:
        acc.close()
        T.close()
        ss.close()


def test_error_paths_leave_the_accumulator_alone(eng, synth, rg):
    ctgs, data, _, _ = synth
    ss = engine.SeqSet(eng, seq_arrays(ctgs))
    T = SwTables(eng, ctgs, rg_records=rg[1])
    acc = Acc(eng, n_tags=2)
    both = Acc(eng, actions=GC | COUNT)
    try:
        assert abi_sum(eng, T, ss, b"I:100-200\nI:5000-5100\nI:7000\n", acc, tag=1)[0] == 0
        before = acc.read()
        assert before["count"][1].sum() > 0 and not before["count"][0].any()
        # located by overlap, the middle (30044) behind the end of ctg:I:1: refused when kept
        assert abi_sum(eng, T, ss, b"I:100-200\nI:29990-30099\n", acc)[0] == _lib.EINVAL
        assert b"line 2" in L.gams_gpu_last_error(eng.h)
        with pytest.raises(host.HostError) as ei:
            host.sw_summary(eng, ctgs, b"I:100-200\nI:29990-30099\n")
        assert ei.value.code == _lib.EINVAL
        assert abi_sum(eng, T, ss, data, acc, actions=4)[0] == _lib.EINVAL                 # unknown action bits
        assert abi_sum(eng, T, ss, data, both, actions=GC | COUNT, rg=False)[0] == _lib.EINVAL   # count without an index
        assert abi_sum(eng, T, ss, data, acc, tag=2)[0] == _lib.EINVAL                     # a tag slot >= n_tags
        assert abi_sum(eng, T, ss, data, acc, mx=19)[0] == _lib.EINVAL                     # made for another max
        assert abi_sum(eng, T, ss, data, acc, size=50)[0] == _lib.EINVAL
        assert abi_sum(eng, T, ss, data, acc, actions=GC | COUNT)[0] == _lib.EINVAL        # ... for other actions
        assert abi_sum(eng, T, None, data, acc)[0] == _lib.EINVAL                          # gc without a seqset
        # a byte the loader refuses: the entry says so, the operator summarises the rows of the batch entry on the host
        hi = data + b"\nnonsense \xc3\xa9\n"
        assert abi_sum(eng, T, ss, hi, acc)[0] == _lib.EUNSUPPORTED
        assert same_tables(acc.read(), before)
        assert not both.read()["count"].any()
        want = host.sw_summary(eng, ctgs, data)
        assert host.sw_summary(eng, ctgs, hi) == want and host.last_operator_device() == 0
        assert host.sw_summary(eng, ctgs, [data, hi], tags=["t", "t"]) == host.sw_summary(eng, ctgs, [data, data], tags=["t", "t"])
        with_cnt = host.sw_summary(eng, ctgs, data, actions=("gc", "count"), rg_data=rg[0])
        assert host.sw_summary(eng, ctgs, hi, actions=("gc", "count"), rg_data=rg[0]) == with_cnt
        only_cnt = host.sw_summary(eng, ctgs, data, actions=("count",), rg_data=rg[0])
        assert host.sw_summary(eng, ctgs, hi, actions=("count",), rg_data=rg[0]) == only_cnt
        assert host.last_operator_device() == 0
        for bad in (dict(n_tags=0), dict(mx=-1), dict(size=1), dict(resize=1), dict(actions=8)):
            kw = dict(mx=20, n_tags=1, actions=GC, size=100, resize=500)
            kw.update(bad)
            p = C.c_void_p()
            assert L.gams_sw_summary_create(eng.h, kw["mx"], kw["n_tags"], kw["actions"], kw["size"], kw["resize"],
                                            C.byref(p)) == _lib.EINVAL and not p.value
    finally:
        both.close()
        acc.close()
        T.close()
        ss.close()


@pytest.mark.parametrize("actions", [GC, GC | COUNT])
def test_abi_batch_on_the_models_features(eng, synth, rg, actions):
    """gams_gpu_sw_summary_batch over the model's features as arrays gives the integers of the file entry"""
    ctgs, data, feats, _ = synth
    ss = engine.SeqSet(eng, seq_arrays(ctgs))
    T = SwTables(eng, ctgs, rg_records=rg[1])
    from_file, from_arrays = Acc(eng, actions=actions), Acc(eng, actions=actions)
    try:
        rc, nf, rows = abi_sum(eng, T, ss, data, from_file, actions=actions)
        assert rc == 0, L.gams_gpu_last_error(eng.h)
        sel = [i for i in range(len(ctgs)) if feats[i]]
        index = np.array(sel, np.uint32)
        cs = np.array([ctgs[i]["chr_start"] for i in sel], np.int32)
        off = np.cumsum([0] + [len(feats[i]) for i in sel]).astype(np.uint64)
        fs = np.array([f[1] for i in sel for f in feats[i]], np.int32)
        fe = np.array([f[2] for i in sel for f in feats[i]], np.int32)
        group_of = {c["id"]: int(g) for c, g in zip(T.order, T.rg_group)}
        grp = np.array([group_of[ctgs[i]["id"]] for i in sel], np.uint32)
        n_rows = C.c_uint64()
        cnt = bool(actions & COUNT)
        rc = L.gams_gpu_sw_summary_batch(eng.h, ss.p, len(sel), index.ctypes.data, cs.ctypes.data, off.ctypes.data,
                                         fs.ctypes.data, fe.ctypes.data, 100, 20, 500, actions, T.rg_ix if cnt else None,
                                         grp.ctypes.data if cnt else None, from_arrays.p, 0, C.byref(n_rows))
        assert rc == 0, L.gams_gpu_last_error(eng.h)
        assert n_rows.value == rows and nf == int(off[-1])
        a, b = from_file.read(), from_arrays.read()
        assert same_tables(a, b) and int(a["count"].sum()) == rows
        assert bool(a["rg_count"].any()) == cnt
        rc = L.gams_gpu_sw_summary_batch(eng.h, ss.p, len(sel), index.ctypes.data, cs.ctypes.data, off.ctypes.data,
                                         fs.ctypes.data, fe.ctypes.data, 100, 20, 500, actions, T.rg_ix if cnt else None,
                                         grp.ctypes.data if cnt else None, from_arrays.p, 1, C.byref(n_rows))
        assert rc == _lib.EINVAL                               # a tag slot >= n_tags
    finally:
        from_arrays.close()
        from_file.close()
        T.close()
        ss.close()
