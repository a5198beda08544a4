"""Every device entry that reads a text file, called one after another on ONE handle: the cases of tests/fuzz_text.py in
pairs (a large call of one family, then a small one of another, and the other way round; an empty or refused call in
front) and in seeded sequences of sixteen calls.  Every outcome must equal the model's, byte for byte and word for word,
whatever the calls before it left in the handle's pools, in its input buffer behind the padding and in its scratch words;
a text an entry handed out must still read the same after calls of the other entries.  Nothing is released between the
calls.  A failure prints the calls made so far (family, seed, size, rc) and where the outcome parts from the model."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import fuzz_text as ft
import runlist_text as rt
import sw_anno_summary as sas
from gams_amd import _lib, engine, host
from test_gpu_gen_text import Gen
from test_gpu_loader_text import abi_index_files, abi_loader
from test_gpu_locate_seq_text import abi_seq
from test_gpu_peak_records import abi_records
from test_gpu_peak_text import abi_peak, seq_arrays
from test_gpu_rg_text import abi_count, abi_index, abi_read_range, index_destroy
from test_gpu_runlist_text import create, destroy_set, read_set
from test_gpu_sw_anno_summary import AnnoAcc, abi_sum_anno, set_args
from test_gpu_sw_summary import Acc, abi_sum
from test_gpu_sw_text import SwTables, abi_sw
from test_gpu_text_ops import AnnoTables, abi_anno, abi_locate

pytestmark = pytest.mark.gpu

L = _lib.load()
# the entry whose text a family's call hands out, and the slot that text lives in ("valid until the next call of this
# entry"; the sw rows until the handle's next sw call, include/gams_gpu.h)
TEXT_ENTRY = dict(locate="gams_gpu_locate_text", count="gams_gpu_count_text", anno="gams_gpu_anno_text",
                  loader="gams_gpu_loader_text", peak_text="gams_gpu_peak_text", peak_records="gams_gpu_peak_records_text",
                  sw_text="gams_gpu_sw_feature_text", locate_seq="gams_gpu_locate_seq_text")
SLOT = dict(sw_summary="sw", sw_summary_anno="sw", sw_text="sw")


class World:
    """what the calls share: the handle, the seqset of the world's ctgs, the ctg index with its name tables and the rg
    index, the two span sets (as tables for anno and as resident sets for the summary)"""

    def __init__(self):
        w = ft.world()
        self.eng = e = engine.Engine(0)
        self.order = w["order"]
        self.ss = engine.SeqSet(e, seq_arrays(w["ctgs"]))
        self.T = SwTables(e, w["ctgs"], rg_records=w["rg_records"])
        assert [c["id"] for c in self.T.order] == [c["id"] for c in self.order]
        runlists = [{k: rt.runlist_of(zip(lo.tolist(), hi.tolist())) for k, (lo, hi) in s.items()} for s in w["sets"]]
        self.A = [AnnoTables(e, self.order, r) for r in runlists]
        self.sets = [host.AnnoSet(e, sas.runlist_json(s)) for s in w["sets"]]
        self.history, self.kept = [], {}

    def close(self):
        for s in self.sets:
            s.close()
        for a in self.A:
            a.close()
        self.T.close()
        self.ss.close()
        self.eng.close()


@pytest.fixture(scope="module")
def dev():
    d = World()
    yield d
    d.close()


@contextlib.contextmanager
def text_pointer(entry, seen):
    """while it is open, the family's text entry notes the (pointer, bytes) it hands out in `seen`"""
    name = TEXT_ENTRY.get(entry)
    if name is None:
        yield
        return
    fn = getattr(L, name)

    def spy(*args):
        rc = fn(*args)
        out = [a._obj for a in args if hasattr(a, "_obj")]
        k = next(i for i, o in enumerate(out) if isinstance(o, C.c_void_p))
        if rc == 0:
            seen.append((out[k].value, out[k + 1].value))
        return rc

    setattr(L, name, spy)
    try:
        yield
    finally:
        setattr(L, name, fn)


def ok(rc, **out):
    return dict(rc=rc, **out) if rc == 0 else dict(rc=rc)


def run(d, c):
    """the family's entry on the case's input -> its outcome, laid out as the model's"""
    e, p, data, eng, T, ss = c["entry"], c["params"], c["data"], d.eng, d.T, d.ss
    n = len(d.order)
    if e in ("locate", "count"):
        rc, text, rows = abi_locate(eng, T, data, count=e == "count")
        return ok(rc, text=text, n_rows=rows)
    if e == "anno":
        rc, text, rows = abi_anno(eng, d.A[p["which"]], data, header=p["header"], prefix=p["prefix"])
        return ok(rc, text=text, n_rows=rows)
    if e == "read_range":
        rc, got = abi_read_range(eng, T, data, n)
        return ok(rc, **{k: got[k].tolist() for k in ("off", "seen", "start", "end", "line")}) if rc == 0 else ok(rc)
    if e == "index":
        rc, ix, grp, kept = abi_index_files(eng, T, data, n) if p["files"] else abi_index(eng, T, data[0], n)
        if rc:
            return ok(rc)
        qg, qs, qe = p["queries"]
        counts = abi_count(eng, ix, qg, qs, qe).tolist()
        index_destroy(eng, ix)
        return ok(rc, kept=kept, grp=grp.tolist(), counts=counts)
    if e == "loader":
        rc, got = abi_loader(eng, T, data, n, p["kind"], p["tag"].encode("latin-1"), p["fmt"], p["base"])
        return ok(rc, **got) if rc == 0 else ok(rc)
    if e == "peak_text":
        rc, text, off, rows = abi_peak(eng, T, ss, data)
        return ok(rc, text=text, off=off.tolist(), n_rows=rows)
    if e == "peak_records":
        rc, text, off, nxt, rows, _ = abi_records(eng, d, data, p["fmt"], p["base"])
        return ok(rc, text=text, off=off.tolist(), next=nxt.tolist(), n_rows=rows)
    prm = {k: p[k] for k in ("size", "mx", "resize") if k in p}
    if e == "sw_text":
        rc, text, off, nf, rows = abi_sw(eng, T, ss, data, **prm)
        return ok(rc, text=text, off=off.tolist(), n_features=nf, n_rows=rows)
    if e in ("sw_summary", "sw_summary_anno"):
        k, actions = p["n_sets"], _lib.SW_GC | (_lib.SW_COUNT if p["count"] else 0)
        acc = AnnoAcc(eng, k, **prm) if k else Acc(eng, actions=actions, **prm)
        try:
            if k:
                ns, sp, cp, _keep = set_args([d.sets[j % 2] for j in range(k)], T.order)
                rc, nf, rows = abi_sum_anno(eng, T, ss, data, acc, ns, sp, cp, **prm)
            else:
                rc, nf, rows = abi_sum(eng, T, ss, data, acc, actions=actions, **prm)
            if rc:
                return ok(rc)
            words = {key: v[0].tolist() for key, v in acc.read().items()}
            if k:
                words["prop"] = acc.read_prop()[0].tolist()
            return ok(rc, n_features=nf, n_rows=rows, **words)
        finally:
            acc.close()
    if e == "runlist_text":
        rc, sp, nm, ng, ns = create(eng, data)
        if rc:
            return ok(rc)
        try:
            names, lo, hi = read_set(eng, sp, nm)
            assert ng == len(names)
            return ok(rc, names=names, n_spans=ns, lo=lo, hi=hi)
        finally:
            destroy_set(eng, sp, nm)
    if e == "gen_text":
        g = Gen(eng, data, p["piece"], p["fill"], p["min_len"])
        try:
            if g.rc:
                return ok(g.rc)
            return ok(0, chrs=g.chrs, chr_len=g.chr_len, table=g.table(), seqs=[g.seqset.download(i) for i in range(len(g.tab))])
        finally:
            g.close()
    assert e == "locate_seq"
    rc, text, rows = abi_seq(eng, T, ss, data)
    return ok(rc, text=text, n_rows=rows)


def call(d, entry, seed, size):
    """one call on the shared handle, held against the model; then every text handed out earlier by another entry"""
    c = ft.case(entry, seed, size)
    slot = SLOT.get(entry, entry)
    d.kept.pop(slot, None)
    seen = []
    with text_pointer(entry, seen):
        got = run(d, c)
    d.history.append((entry, seed, size, got["rc"]))
    diff = ft.difference(got, c["want"])
    assert diff is None, "%s\nafter the calls (family, seed, size, rc):\n%s" % (diff, "\n".join(map(repr, d.history)))
    if seen and seen[-1][1]:
        ptr, nb = seen[-1]
        d.kept[slot] = (ptr, nb, C.string_at(ptr, nb), len(d.history))
    for other, (ptr, nb, text, at) in d.kept.items():
        if other != slot:
            now = C.string_at(ptr, nb)
            assert now == text, "the text of call %d (%s) changed: %s\nafter the calls:\n%s" % (
                at, other, ft.first_difference(now, text), "\n".join(map(repr, d.history)))
    return got


# ---- pairs --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("x", ft.FAMILIES)
def test_pairs(dev, x):
    """X large then Y small, X small then Y large, and an empty (even Y) or refused (odd Y) X in front of a seam Y, for
    every family Y"""
    ix = ft.FAMILIES.index(x)
    for iy, y in enumerate(ft.FAMILIES):
        sx, sy = (ix + iy) % 4, (ix + 2 * iy + 1) % 4
        call(dev, x, sx, "large")
        call(dev, y, sy, "small")
        call(dev, x, sx, "small")
        call(dev, y, sy, "large")
        if iy % 2:
            call(dev, x, ft.REFUSED, "seam")
        else:
            call(dev, x, sx, "empty")
        call(dev, y, sy, "seam")


# ---- sequences ----------------------------------------------------------------------------------------------------------
def sequence(seed, n=16):
    rng = np.random.default_rng(seed)
    fam, cs, sz = rng.integers(0, len(ft.FAMILIES), n), rng.integers(0, 5, n), rng.integers(0, len(ft.SIZES), n)
    return [(ft.FAMILIES[f], (ft.SEEDS + (ft.REFUSED,))[s], ft.SIZES[z]) for f, s, z in zip(fam, cs, sz)]


@pytest.mark.parametrize("seed", range(12))
def test_sequence(dev, seed):
    """sixteen calls, family, case seed and size drawn independently; then the last successful one once more"""
    got, last = None, None
    for key in sequence(seed):
        out = call(dev, *key)
        if out["rc"] == 0:
            got, last = out, key
    assert last is not None
    again = call(dev, *last)
    assert ft.difference(again, got) is None


# ---- a fresh handle -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ft.FAMILIES)
def test_fresh_handle_agrees(dev, family):
    """the seam case on a new handle, and as call 17 of sequence 0 on the shared one: where only the second fails, a call
    before it left something that was read"""
    fresh = World()
    try:
        call(fresh, family, 1, "seam")
    finally:
        fresh.close()
    for key in sequence(0):
        call(dev, *key)
    call(dev, family, 1, "seam")

