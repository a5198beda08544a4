"""Which code every sw entry answers a refused call with, and under which name: one table for gams_gpu_sw_batch,
gams_gpu_sw_count_batch, gams_gpu_sw_text_actions, gams_gpu_sw_summary_batch(_anno), gams_gpu_sw_feature_text,
gams_gpu_sw_feature_summary(_anno), gams_gpu_range_gc_batch and gams_sw_summary_create_anno.  Every single violation an
entry can refuse, then `max = 2^24 + 1` (GAMS_EUNSUPPORTED where the entry gets as far as asking) together with every
GAMS_EINVAL violation the entry tests before or after it: the precedence of the checks is part of what an entry returns.
No refused call launches a kernel, so the fixture is tiny: two ctgs of 3 kb, three feature lines, five rg lines, one
span set, size 100, max 2, resize 500.  A refused summary call leaves its accumulator as it was; after the table one
accepted call of every entry gives the model's rows, text or table, so the checks are no stricter than they were.

The expected codes were read off the entries' checks.  Two facts worth knowing when reading the table:
  * the batch summary entries compare the call with the accumulator before they look at the window parameters, and no
    accumulator can be made for size 1, resize 1, max -1 or max 2^24 + 1: they answer GAMS_EINVAL under "gpu_sw_summary"
    to all four, where the feature summary entries answer the bounds under their own check first and
    GAMS_EUNSUPPORTED to the max;
  * the text and summary batch entries name themselves for the action checks and "gpu_sw" for everything sw_check tests
    (a null seqset, the bounds, the selection, the max)."""
import ctypes as C

import numpy as np
import pytest

import sw_anno_summary as sas
import sw_summary as sws
import sw_text as swt
from gams_amd import _lib, engine, host
from test_gpu_sw_anno_summary import AnnoAcc
from test_gpu_sw_summary import Acc, same_tables
from test_gpu_sw_text import SwTables, seq_arrays

pytestmark = pytest.mark.gpu

L = _lib.load()
GC, COUNT = _lib.SW_GC, _lib.SW_COUNT
EINVAL, EUNSUP = _lib.EINVAL, _lib.EUNSUPPORTED
SIZE, MX, RESIZE = 100, 2, 500
BIG = (1 << 24) + 1
ROW = _lib.SW_ROW_DTYPE

SW, SW_COUNT, SW_TEXT, SW_SUM = b"gpu_sw", b"gpu_sw_count", b"gpu_sw_text", b"gpu_sw_summary"
F_TEXT, F_SUM, RANGE_GC, CREATE = b"gpu_sw_feature_text", b"gpu_sw_feature_summary", b"gpu_range_gc", b"sw_summary_create"

DATA = b"I:100-200\nI:1000-1100\nI:2000-2050\n"        # the first located line of a ctg is dropped: two features
RG_LINES = ["I:50-60", "I:950-1200", "I:1500", "I:1990-2010", "II:100-300", "II:2000-2500"]   # (the first of a ctg is dropped)
SPANS = {"I": (np.array([950, 1400, 2040], np.int64), np.array([1020, 1800, 2300], np.int64))}   # none on II


def _ptr(a):
    return None if a is None else a.ctypes.data


class Fixture:
    def __init__(self, eng):
        rng = np.random.default_rng(11)
        self.eng = eng
        self.ctgs = [dict(id="ctg:I:1", chr_id="I", chr_start=1, chr_end=3000, seq=rng.choice(np.frombuffer(b"ACGT", np.uint8), 3000).tobytes()),
                     dict(id="ctg:II:1", chr_id="II", chr_start=1, chr_end=3000, seq=rng.choice(np.frombuffer(b"ACGT", np.uint8), 3000).tobytes())]
        self.rg_records = host.read_range(eng, self.ctgs, RG_LINES)
        self.ss = engine.SeqSet(eng, seq_arrays(self.ctgs))
        self.T = SwTables(eng, self.ctgs, rg_records=self.rg_records)
        self.aset = host.AnnoSet(eng, sas.runlist_json(SPANS))
        feats = swt.features(self.ctgs, DATA)
        assert [len(f) for f in feats] == [2, 0]
        # the arrays of the batch entries: both ctgs selected, the second without a feature
        self.index = np.array([0, 1], np.uint32)
        self.cs = np.array([c["chr_start"] for c in self.ctgs], np.int32)
        self.off = np.array([0, 2, 2], np.uint64)
        self.fs = np.array([f[1] for f in feats[0]], np.int32)
        self.fe = np.array([f[2] for f in feats[0]], np.int32)
        self.ids = [f[0].encode() for f in feats[0]]
        group_of = {c["id"]: int(g) for c, g in zip(self.T.order, self.T.rg_group)}
        self.grp = np.array([group_of[c["id"]] for c in self.ctgs], np.uint32)
        # the set's group of every ctg: per selected ctg (batch) and per interval of the ctg index (feature entries)
        grp_of = lambda c: self.aset.names.index(c["chr_id"]) if c["chr_id"] in self.aset.names else 0xFFFFFFFF
        self.col_sel = np.array([grp_of(c) for c in self.ctgs], np.uint32)
        self.col_ivl = np.array([grp_of(c) for c in self.T.order], np.uint32)
        # the model: the rows' text (-a gc), and the rg ranges of every ctg for the count column
        self.rows_text = swt.model(self.ctgs, DATA, SIZE, MX, RESIZE)
        self.fields = [r.split(b"\t") for r in self.rows_text.split(b"\n")[:-1]]
        self.windows = [tuple(int(x) for x in sas.RANGE.match(f[1]).group(2, 3)) for f in self.fields]
        assert len(self.fields) == 10 and all(e > s for s, e in self.windows)

    def close(self):
        self.aset.close()
        self.T.close()
        self.ss.close()

    def rg_counts(self):
        """rg_count of every row by brute force: the rg ranges [s, e + 1) of ctg:I:1 against the window [ws, we)"""
        own = [sas.RANGE.match(r.encode()) for cid, r in self.rg_records if cid == "ctg:I:1"]
        own = [(int(m.group(2)), int(m.group(3) or m.group(2))) for m in own]
        assert len(own) >= 3 and all(s != we for s, _ in own for _, we in self.windows)    # no range begins on a window's end
        return [sum(1 for s, e in own if s < we and e + 1 > ws) for ws, we in self.windows]


@pytest.fixture(scope="module")
def eng():
    e = engine.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def fx(eng):
    f = Fixture(eng)
    yield f
    f.close()


# ---- one caller per entry: every argument a case may spoil is a keyword ---------------------------------------------------
DEFAULTS = dict(ss=True, slots=True, index=None, off=None, size=SIZE, mx=MX, resize=RESIZE, actions=GC, rg=True, groups=True,
                acc="gc", tag=0, n_anno=None, sets="ok", cols="ok", n_tags=1)


def _sets(fx, k, n_anno, batch):
    """(n_anno, gams_spans_t **, the set_group columns, what must outlive the call)"""
    if n_anno is None:
        n_anno = 1
    col = fx.col_sel if batch else fx.col_ivl
    sp = None if k["sets"] is None else (C.c_void_p * max(n_anno, 1))(*[None if k["sets"] == "null" else fx.aset._sp] * max(n_anno, 1))
    cp = None if k["cols"] is None else (C.c_void_p * max(n_anno, 1))(*[None if k["cols"] == "null" else col.ctypes.data] * max(n_anno, 1))
    return n_anno, sp, cp


def call(fx, accs, entry, **kw):
    """the code `entry` returns for the fixture's call with `kw` spoiled"""
    k = dict(DEFAULTS, **kw)
    h, T = fx.eng.h, fx.T
    ss = fx.ss.p if k["ss"] else None
    cnt = bool(k["actions"] & COUNT) or entry == "count_batch"
    index = fx.index if k["index"] is None else np.array(k["index"], np.uint32)
    off = fx.off if k["off"] is None else np.array(k["off"], np.uint64)
    acc = accs[k["acc"]].p if k["acc"] else None
    n_rows, nf = C.c_uint64(), C.c_uint64()
    sel = (h, ss, 2, index.ctypes.data, fx.cs.ctypes.data, off.ctypes.data, fx.fs.ctypes.data, fx.fe.ctypes.data)
    rg_sel = (T.rg_ix if cnt and k["rg"] else None, fx.grp.ctypes.data if cnt and k["groups"] else None)
    rg_ivl = (T.rg_ix if cnt and k["rg"] else None, T.rg_group.ctypes.data if cnt and k["groups"] else None)
    file_ = (h, ss, T.ix, T.chr, T.ids, T.slot.ctypes.data if k["slots"] else None, T.cs.ctypes.data, T.ce.ctypes.data, DATA, len(DATA))
    win = (k["size"], k["mx"], k["resize"])
    if entry == "batch":
        rows = np.zeros(16, ROW)
        return L.gams_gpu_sw_batch(*sel, *win, rows.ctypes.data, 16, None, C.byref(n_rows))
    if entry == "count_batch":
        count = np.zeros(16, np.int32)
        return L.gams_gpu_sw_count_batch(*sel[:8], k["size"], k["mx"], *rg_sel, count.ctypes.data, 16, None, C.byref(n_rows))
    if entry == "text_actions":
        chrs = (C.c_char_p * 2)(b"I", b"II")
        ids = (C.c_char_p * 2)(*fx.ids)
        text, nb, ctg_off = C.c_void_p(), C.c_uint64(), C.c_void_p()
        return L.gams_gpu_sw_text_actions(h, ss, 2, index.ctypes.data, chrs, fx.cs.ctypes.data, off.ctypes.data, fx.fs.ctypes.data,
                                          fx.fe.ctypes.data, ids, *win, k["actions"], *rg_sel, C.byref(text), C.byref(nb),
                                          C.byref(ctg_off), C.byref(n_rows))
    if entry == "summary_batch":
        return L.gams_gpu_sw_summary_batch(*sel, *win, k["actions"], *rg_sel, acc, k["tag"], C.byref(n_rows))
    if entry == "summary_batch_anno":
        n, sp, cp = _sets(fx, k, k["n_anno"], True)
        return L.gams_gpu_sw_summary_batch_anno(*sel, *win, k["actions"], *rg_sel, acc, k["tag"], n, sp, cp, C.byref(n_rows))
    if entry == "feature_text":
        text, nb = C.c_void_p(), C.c_uint64()
        toff = np.zeros(3, np.uint64)
        return L.gams_gpu_sw_feature_text(*file_, *win, k["actions"], *rg_ivl, C.byref(text), C.byref(nb), toff.ctypes.data,
                                          C.byref(nf), C.byref(n_rows))
    if entry == "feature_summary":
        return L.gams_gpu_sw_feature_summary(*file_, *win, k["actions"], *rg_ivl, acc, k["tag"], C.byref(nf), C.byref(n_rows))
    if entry == "feature_summary_anno":
        n, sp, cp = _sets(fx, k, k["n_anno"], False)
        return L.gams_gpu_sw_feature_summary_anno(*file_, *win, k["actions"], *rg_ivl, acc, k["tag"], n, sp, cp, C.byref(nf),
                                                  C.byref(n_rows))
    if entry == "range_gc_batch":
        gc = np.zeros(2, np.float32)
        return L.gams_gpu_range_gc_batch(*sel, gc.ctypes.data)
    if entry == "create_anno":
        p = C.c_void_p()
        rc = L.gams_sw_summary_create_anno(h, k["mx"], k["n_tags"], k["actions"], k["size"], k["resize"],
                                           0 if k["n_anno"] is None else k["n_anno"], C.byref(p))
        assert rc != 0 and not p.value
        return rc
    raise KeyError(entry)


# ---- the violations ---------------------------------------------------------------------------------------------------------
BITS = dict(actions=GC | 4)
NO_IX = dict(actions=GC | COUNT, rg=False, acc="both")
NO_GROUPS = dict(actions=GC | COUNT, groups=False, acc="both")
NO_SS = dict(ss=False)
NO_SLOTS = dict(slots=False)
SIZE1, MAX_NEG, RESIZE1, MAX_BIG = dict(size=1), dict(mx=-1), dict(resize=1), dict(mx=BIG)
OFF0, OFF_DEC, INDEX = dict(off=[1, 2, 2]), dict(off=[0, 2, 1]), dict(index=[0, 7])
TAG = dict(tag=1)
OTHER_MAX, OTHER_SIZE, OTHER_RESIZE, OTHER_ACTIONS = dict(mx=3), dict(size=50), dict(resize=400), dict(actions=GC | COUNT)
NULL_SET, NULL_COL, NULL_SETS, FIVE = dict(sets="null"), dict(cols="null"), dict(sets=None), dict(n_anno=5)

SELECTION = [OFF0, OFF_DEC, INDEX]
WINDOW = [SIZE1, MAX_NEG, RESIZE1]


def table():
    """[(entry, the spoiled arguments, the code, the name in front of the message)]"""
    t = []

    def add(entry, code, who, cases, also=None):
        t.extend((entry, dict(also or {}, **c), code, who) for c in cases)

    # gams_gpu_sw_batch: sw_check alone -- null, bounds, selection, then the max
    add("batch", EINVAL, SW, [NO_SS] + WINDOW + SELECTION)
    add("batch", EUNSUP, SW, [MAX_BIG])
    add("batch", EINVAL, SW, [NO_SS, SIZE1, RESIZE1] + SELECTION, MAX_BIG)
    # gams_gpu_sw_count_batch: its rg test, then sw_check (no resize of its own)
    add("count_batch", EINVAL, SW_COUNT, [dict(rg=False), dict(groups=False)])
    add("count_batch", EINVAL, SW, [NO_SS, SIZE1, MAX_NEG] + SELECTION)
    add("count_batch", EUNSUP, SW, [MAX_BIG])
    add("count_batch", EINVAL, SW_COUNT, [dict(rg=False), dict(groups=False)], MAX_BIG)
    add("count_batch", EINVAL, SW, [NO_SS, SIZE1] + SELECTION, MAX_BIG)
    # gams_gpu_sw_text_actions: the actions under its own name, then sw_check
    add("text_actions", EINVAL, SW_TEXT, [BITS, NO_IX, NO_GROUPS])
    add("text_actions", EINVAL, SW, [NO_SS] + WINDOW + SELECTION)
    add("text_actions", EUNSUP, SW, [MAX_BIG])
    add("text_actions", EINVAL, SW_TEXT, [BITS, NO_IX, NO_GROUPS], MAX_BIG)
    add("text_actions", EINVAL, SW, [NO_SS, SIZE1, RESIZE1] + SELECTION, MAX_BIG)
    # the batch summaries: the actions, the accumulator (no accumulator exists for a window out of bounds), then sw_check
    for entry, acc in (("summary_batch", "gc"), ("summary_batch_anno", "one")):
        a = dict(acc=acc)
        add(entry, EINVAL, SW_SUM, [BITS, dict(NO_IX, acc=acc), dict(NO_GROUPS, acc=acc)], a)
        add(entry, EINVAL, SW_SUM, WINDOW + [MAX_BIG, TAG, OTHER_MAX, OTHER_SIZE, OTHER_RESIZE, OTHER_ACTIONS, dict(acc=None)], a)
        add(entry, EINVAL, SW, [NO_SS] + SELECTION, a)
        add(entry, EINVAL, SW_SUM, [BITS, NO_SS, TAG, OTHER_SIZE] + SELECTION, dict(MAX_BIG, acc=acc))
    add("summary_batch", EINVAL, SW_SUM, [dict(acc="one")])                        # made for one set, called with none
    add("summary_batch_anno", EINVAL, SW_SUM, [dict(acc="gc"), dict(n_anno=0), NULL_SET, NULL_COL, NULL_SETS, FIVE], dict(acc="one"))
    add("summary_batch_anno", EINVAL, SW_SUM, [NULL_SET, NULL_COL], dict(MAX_BIG, acc="one"))
    # the feature entries: actions, gc, count, bounds, the name tables, the max -- and only then the accumulator
    for entry, who, acc in (("feature_text", F_TEXT, None), ("feature_summary", F_SUM, "gc"), ("feature_summary_anno", F_SUM, "one")):
        a = dict(acc=acc)
        first = [BITS, NO_SS, NO_SLOTS, dict(NO_IX, acc=acc), dict(NO_GROUPS, acc=acc)] + WINDOW
        add(entry, EINVAL, who, first, a)
        add(entry, EUNSUP, who, [MAX_BIG], a)
        add(entry, EINVAL, who, [c for c in first if "mx" not in c], dict(MAX_BIG, acc=acc))
        if acc:
            after = [TAG, OTHER_SIZE, OTHER_RESIZE, OTHER_ACTIONS]
            add(entry, EINVAL, who, after + [OTHER_MAX, dict(acc=None)], a)
            add(entry, EUNSUP, who, after, dict(MAX_BIG, acc=acc))
    add("feature_summary", EINVAL, F_SUM, [dict(acc="one")])
    sets = [dict(acc="gc"), dict(n_anno=0), NULL_SET, NULL_COL, NULL_SETS, FIVE]
    add("feature_summary_anno", EINVAL, F_SUM, sets, dict(acc="one"))
    add("feature_summary_anno", EUNSUP, F_SUM, sets, dict(MAX_BIG, acc="one"))
    # gams_gpu_range_gc_batch: the selection under its own name
    add("range_gc_batch", EINVAL, RANGE_GC, [NO_SS] + SELECTION)
    # gams_sw_summary_create_anno: one message for its parameters, the max among them
    add("create_anno", EINVAL, CREATE, [BITS, MAX_BIG, FIVE, dict(n_tags=0)] + WINDOW)
    add("create_anno", EINVAL, CREATE, [BITS, SIZE1, FIVE], MAX_BIG)
    return t


def test_refusals_then_accepted_calls(eng, fx):
    accs = dict(gc=Acc(eng, mx=MX), both=Acc(eng, mx=MX, actions=GC | COUNT), one=AnnoAcc(eng, 1, mx=MX))
    try:
        # something in every accumulator, so that "unchanged" says something
        assert call(fx, accs, "feature_summary", acc="gc") == 0
        assert call(fx, accs, "feature_summary", acc="both", actions=GC | COUNT) == 0
        assert call(fx, accs, "feature_summary_anno", acc="one") == 0
        before = {k: (a.everything() if isinstance(a, AnnoAcc) else np.concatenate([v.ravel() for v in a.read().values()]))
                  for k, a in accs.items()}
        assert all(b.any() for b in before.values())
        wrong = []
        cases = table()
        for entry, spoiled, code, who in cases:
            rc = call(fx, accs, entry, **spoiled)
            msg = L.gams_gpu_last_error(eng.h)
            print(entry, spoiled, "->", rc, msg)
            if rc != code or not msg.startswith(who + b": "):
                wrong.append((entry, spoiled, code, who, rc, msg))
            used = dict(DEFAULTS, **spoiled)["acc"]
            if "summary" in entry and used:
                a = accs[used]
                now = a.everything() if isinstance(a, AnnoAcc) else np.concatenate([v.ravel() for v in a.read().values()])
                assert np.array_equal(now, before[used]), (entry, spoiled)
        assert not wrong, wrong
        assert len(cases) > 200 and {c[0] for c in cases} == {"batch", "count_batch", "text_actions", "summary_batch",
                                                               "summary_batch_anno", "feature_text", "feature_summary",
                                                               "feature_summary_anno", "range_gc_batch", "create_anno"}
    finally:
        for a in accs.values():
            a.close()
    accepted(eng, fx)


def accepted(eng, fx):
    """one accepted call of every entry on the same fixture, against the model"""
    h, T = eng.h, fx.T
    n_rows, nf = C.c_uint64(), C.c_uint64()
    sel = (h, fx.ss.p, 2, fx.index.ctypes.data, fx.cs.ctypes.data, fx.off.ctypes.data, fx.fs.ctypes.data, fx.fe.ctypes.data)
    file_ = (h, fx.ss.p, T.ix, T.chr, T.ids, T.slot.ctypes.data, T.cs.ctypes.data, T.ce.ctypes.data, DATA, len(DATA))
    n = len(fx.fields)
    # the rows
    rows = np.zeros(16, ROW)
    row_off = np.zeros(3, np.uint64)
    assert L.gams_gpu_sw_batch(*sel, SIZE, MX, RESIZE, rows.ctypes.data, 16, row_off.ctypes.data, C.byref(n_rows)) == 0
    assert n_rows.value == n and row_off.tolist() == [0, n, n]
    for r, f, (ws, we) in zip(rows[:n], fx.fields, fx.windows):
        assert (r["type"], r["distance"], r["start"], r["end"]) == (b"MLR".index(f[2]), int(f[3]), ws, we)
        want = np.array([f[4 + k].decode() for k in range(4)], np.float32)
        got = np.array([r[name] for name in ("gc_content", "gc_mean", "gc_stddev", "gc_cv")], np.float32)
        assert np.array_equal(got, want, equal_nan=True), (f, got)
    assert [int(f[0].rsplit(b":", 2)[1]) - 1 for f in fx.fields] == rows["feature"][:n].tolist()
    # the counts
    count = np.full(16, -1, np.int32)
    assert L.gams_gpu_sw_count_batch(*sel, SIZE, MX, T.rg_ix, fx.grp.ctypes.data, count.ctypes.data, 16, None, C.byref(n_rows)) == 0
    want_counts = fx.rg_counts()
    assert n_rows.value == n and count[:n].tolist() == want_counts and any(want_counts) and not all(want_counts)
    # the text, from arrays and from the file's bytes
    chrs, ids = (C.c_char_p * 2)(b"I", b"II"), (C.c_char_p * 2)(*fx.ids)
    text, nb, ctg_off = C.c_void_p(), C.c_uint64(), C.c_void_p()
    assert L.gams_gpu_sw_text_actions(h, fx.ss.p, 2, fx.index.ctypes.data, chrs, fx.cs.ctypes.data, fx.off.ctypes.data,
                                      fx.fs.ctypes.data, fx.fe.ctypes.data, ids, SIZE, MX, RESIZE, GC, None, None, C.byref(text),
                                      C.byref(nb), C.byref(ctg_off), C.byref(n_rows)) == 0
    assert C.string_at(text, nb.value) == fx.rows_text and n_rows.value == n
    toff = np.zeros(3, np.uint64)
    assert L.gams_gpu_sw_feature_text(*file_, SIZE, MX, RESIZE, GC, None, None, C.byref(text), C.byref(nb), toff.ctypes.data,
                                      C.byref(nf), C.byref(n_rows)) == 0
    assert C.string_at(text, nb.value) == swt.interval_text(fx.ctgs, DATA, SIZE, MX, RESIZE) == fx.rows_text
    assert (nf.value, n_rows.value) == (2, n) and toff.tolist() == [0, len(fx.rows_text), len(fx.rows_text)]
    # the tables
    model = sws.summary([fx.rows_text])[1]
    props = sas.summary([sas.annotate(fx.rows_text, fx.ctgs, SPANS)], ["s"])[1].prop(MX)
    assert props.any()
    sp, cs_, ci_ = (C.c_void_p * 1)(fx.aset._sp), (C.c_void_p * 1)(fx.col_sel.ctypes.data), (C.c_void_p * 1)(fx.col_ivl.ctypes.data)
    for with_sets in (False, True):
        a, b = (AnnoAcc(eng, 1, mx=MX), AnnoAcc(eng, 1, mx=MX)) if with_sets else (Acc(eng, mx=MX), Acc(eng, mx=MX))
        try:
            if with_sets:
                assert L.gams_gpu_sw_summary_batch_anno(*sel, SIZE, MX, RESIZE, GC, None, None, a.p, 0, 1, sp, cs_, C.byref(n_rows)) == 0
                assert L.gams_gpu_sw_feature_summary_anno(*file_, SIZE, MX, RESIZE, GC, None, None, b.p, 0, 1, sp, ci_, C.byref(nf),
                                                          C.byref(n_rows)) == 0
                assert np.array_equal(a.read_prop(), props) and np.array_equal(b.read_prop(), props)
            else:
                assert L.gams_gpu_sw_summary_batch(*sel, SIZE, MX, RESIZE, GC, None, None, a.p, 0, C.byref(n_rows)) == 0
                assert L.gams_gpu_sw_feature_summary(*file_, SIZE, MX, RESIZE, GC, None, None, b.p, 0, C.byref(nf), C.byref(n_rows)) == 0
            assert n_rows.value == n
            assert same_tables(a.read(), model.arrays(MX)) and same_tables(b.read(), model.arrays(MX))
        finally:
            a.close()
            b.close()
    # the gc of the rows' windows as ranges of ctg:I:1
    rs = np.array([w[0] for w in fx.windows], np.int32)
    re_ = np.array([w[1] for w in fx.windows], np.int32)
    roff = np.array([0, n, n], np.uint64)
    gc = np.zeros(n, np.float32)
    assert L.gams_gpu_range_gc_batch(h, fx.ss.p, 2, fx.index.ctypes.data, fx.cs.ctypes.data, roff.ctypes.data, rs.ctypes.data,
                                     re_.ctypes.data, gc.ctypes.data) == 0
    assert np.array_equal(gc, np.array([f[4].decode() for f in fx.fields], np.float32))
    # an accumulator at the largest max there is room to ask for is the create entry's business, not refused by the check
    p = C.c_void_p()
    assert L.gams_sw_summary_create_anno(h, MX, 1, GC | COUNT, SIZE, RESIZE, 4, C.byref(p)) == 0 and p.value
    L.gams_sw_summary_destroy(h, p)
