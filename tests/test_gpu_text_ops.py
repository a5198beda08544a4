"""Text in, text out on the device: gams_gpu_locate_text / gams_gpu_count_text / gams_gpu_anno_text through the C ABI,
and the host operators above them (Locator::locate_text, gams::anno_text), against the existing array-path
operators fed the same lines (which are pinned to the reference's goldens by test_gpu_host.py)."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import helpers
from fuzz_text import assemble, fuzz_ranges
from gams_amd import _lib, engine, host
from test_text_ops_cpu import fmt4_exact

pytestmark = pytest.mark.gpu

L = _lib.load()


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


def rust_lines(data):
    """BufRead::lines(): split on \\n, one \\r before it dropped, a last line without \\n kept as it is"""
    segs = data.split(b"\n")
    last = segs.pop()
    out = [s[:-1] if s.endswith(b"\r") else s for s in segs]
    if last:
        out.append(last)
    return out


def first_fields(data):
    return [ln.split(b"\t")[0].decode() for ln in rust_lines(data)]


def _ok(eng, rc):
    if rc != 0:
        raise _lib.GamsError(rc, L.gams_gpu_last_error(eng.h).decode())


def _names(eng, names):
    nm = C.c_void_p()
    arr = (C.c_char_p * max(len(names), 1))(*[n.encode() for n in names])
    _ok(eng, L.gams_names_create(eng.h, len(names), arr, C.byref(nm)))
    return nm


RANGE = re.compile(r"^(?:[^.]*\.)?([\w/-]+)(?:\([^)]*\))?:(\d+)(?:[-_]+(\d+))?$")


class LocTables:
    """The ctg index, its name tables and (for --count) the rg index, laid out as Locator lays them out."""

    def __init__(self, eng, ctgs, rg_records=None):
        self.eng = eng
        by_chr = {}
        for c in ctgs:
            by_chr.setdefault(c["chr_id"], []).append(c)
        chrs = sorted(by_chr)
        ordered = [c for k in chrs for c in by_chr[k]]
        off = np.cumsum([0] + [len(by_chr[k]) for k in chrs]).astype(np.uint64)
        st = np.array([c["chr_start"] for c in ordered], np.uint32)
        sp = np.array([c["chr_end"] + 1 for c in ordered], np.uint32)
        self.ix = C.c_void_p()
        _ok(eng, L.gams_index_create(eng.h, len(chrs), off.ctypes.data, st.ctypes.data, sp.ctypes.data, C.byref(self.ix)))
        self.chr = _names(eng, chrs)
        self.ids = _names(eng, [c["id"] for c in ordered])
        self.rg_ix = None
        if rg_records is not None:
            rg_of = {c["id"]: [] for c in ctgs}
            for cid, r in rg_records:
                m = RANGE.match(r)
                s = int(m.group(2))
                rg_of.setdefault(cid, []).append((s, int(m.group(3)) if m.group(3) else s))
            keys = sorted(rg_of)
            gid = {k: g for g, k in enumerate(keys)}
            roff = np.cumsum([0] + [len(rg_of[k]) for k in keys]).astype(np.uint64)
            rs = np.array([s for k in keys for s, _ in rg_of[k]] or [0], np.uint32)
            re_ = np.array([e + 1 for k in keys for _, e in rg_of[k]] or [0], np.uint32)
            self.rg_ix = C.c_void_p()
            _ok(eng, L.gams_index_create(eng.h, len(keys), roff.ctypes.data, rs.ctypes.data, re_.ctypes.data,
                                         C.byref(self.rg_ix)))
            self.rg_group = np.array([gid[c["id"]] for c in ordered], np.uint32)

    def close(self):
        L.gams_index_destroy(self.eng.h, self.ix)
        if self.rg_ix is not None:
            L.gams_index_destroy(self.eng.h, self.rg_ix)
        L.gams_names_destroy(self.eng.h, self.chr)
        L.gams_names_destroy(self.eng.h, self.ids)


def abi_locate(eng, T, data, count=False, rg_group=None):
    """(rc, text, n_rows) of gams_gpu_locate_text / gams_gpu_count_text"""
    text, nb, rows = C.c_void_p(), C.c_uint64(), C.c_uint64()
    n = len(data)
    if isinstance(data, bytearray):
        data = (C.c_char * n).from_buffer(data)
    if count:
        g = T.rg_group if rg_group is None else rg_group
        rc = L.gams_gpu_count_text(eng.h, T.ix, T.chr, T.rg_ix, g.ctypes.data, data, n, C.byref(text),
                                   C.byref(nb), C.byref(rows))
    else:
        rc = L.gams_gpu_locate_text(eng.h, T.ix, T.chr, T.ids, data, n, C.byref(text), C.byref(nb),
                                    C.byref(rows))
    return rc, (C.string_at(text, nb.value) if rc == 0 and nb.value else b""), rows.value


class AnnoTables:
    def __init__(self, eng, ctgs, runlists):
        self.eng = eng
        chrs = sorted(runlists)
        lo, hi, off = [], [], [0]
        for k in chrs:
            for part in runlists[k].split(","):
                if part and part != "-":
                    a, _, b = part.partition("-")
                    lo.append(int(a))
                    hi.append(int(b) if b else int(a))
            off.append(len(lo))
        off = np.array(off, np.uint64)
        lo = np.array(lo or [0], np.int32)
        hi = np.array(hi or [0], np.int32)
        self.sp = C.c_void_p()
        _ok(eng, L.gams_spans_create(eng.h, len(chrs), off.ctypes.data, lo.ctypes.data, hi.ctypes.data, C.byref(self.sp)))
        self.chr = _names(eng, chrs)
        self.ids = _names(eng, [c["id"] for c in ctgs])
        self.cs = np.array([c["chr_start"] for c in ctgs], np.int32)
        self.ce = np.array([c["chr_end"] for c in ctgs], np.int32)

    def close(self):
        L.gams_spans_destroy(self.eng.h, self.sp)
        L.gams_names_destroy(self.eng.h, self.chr)
        L.gams_names_destroy(self.eng.h, self.ids)


def abi_anno(eng, T, data, header=False, prefix="", idx_id=1, idx_range=2):
    text, nb, rows = C.c_void_p(), C.c_uint64(), C.c_uint64()
    rc = L.gams_gpu_anno_text(eng.h, T.sp, T.chr, T.ids, T.cs.ctypes.data, T.ce.ctypes.data, data, len(data),
                              int(header), prefix.encode(), idx_id, idx_range, C.byref(text), C.byref(nb), C.byref(rows))
    return rc, (C.string_at(text, nb.value) if rc == 0 and nb.value else b""), rows.value


def rg_records(eng, ctgs, name):
    """the rg loader incl. its drop-first quirk (as test_gpu_host.rg_records)"""
    lines = helpers.read_lines(name)
    ids = host.find(eng, ctgs, [ln.split("\t")[0] for ln in lines])
    seen, recs = set(), []
    for ln, cid in zip(lines, ids):
        if not cid:
            continue
        if cid in seen:
            recs.append((cid, ln.split("\t")[0]))
        seen.add(cid)
    return recs


def read_bytes(name):
    with open(os.path.join(helpers.S288C, name), "rb") as fh:
        return fh.read()


# ---- goldens --------------------------------------------------------------------------------------
def test_locate_text_goldens(eng, s288c):
    ctgs = all_ctgs(s288c)
    T = LocTables(eng, ctgs)
    try:
        data = read_bytes("spo11_hot.rg")
        rc, text, rows = abi_locate(eng, T, data)
        assert rc == 0 and rows == 71 and text.count(b"\n") == 71
        assert text == host.locate(eng, ctgs, first_fields(data)).encode()
        assert host.locate_text(eng, ctgs, data) == text and host.last_operator_device() == 1
        small = b"I:1000-1100\nII:1000-1100\nMito:1000-1100"
        rc, text, rows = abi_locate(eng, T, small)
        assert rc == 0 and rows == 2
        assert text == b"I:1000-1100\tctg:I:1\nMito:1000-1100\tctg:Mito:1\n"
        rc, text, rows = abi_locate(eng, T, b"")
        assert rc == 0 and text == b"" and rows == 0
    finally:
        T.close()


def test_count_text_golden(eng, s288c):
    ctgs = all_ctgs(s288c)
    recs = rg_records(eng, ctgs, "SK1.snp.rg")
    T = LocTables(eng, ctgs, recs)
    try:
        data = b"I:1000-2000\nII:1001-2000\nMito:1000-2000\n"
        rc, text, rows = abi_locate(eng, T, data, count=True)
        assert rc == 0 and rows == 2
        assert text == b"I:1000-2000\t12\nMito:1000-2000\t0\n"
        assert host.locate_text(eng, ctgs, data, count=True, rg_records=recs) == text
        assert host.last_operator_device() == 1
    finally:
        T.close()


def test_anno_text_golden(eng, s288c):
    ctgs = all_ctgs(s288c)
    with open(os.path.join(helpers.S288C, "intergenic.json")) as fh:
        runlists = json.load(fh)
    data = read_bytes("ctg.range.tsv")
    exp = host.anno(eng, ctgs, runlists, [ln.decode() for ln in rust_lines(data)], header=True, prefix="intergenic",
                    idx_id=1, idx_range=2).encode()
    T = AnnoTables(eng, ctgs, runlists)
    try:
        rc, text, rows = abi_anno(eng, T, data, header=True, prefix="intergenic")
        assert rc == 0 and rows == 4 and text == exp
        first = text.split(b"\n")[0]
        assert first.endswith(b"\tintergenicProp") and len(first.split(b"\t")) == 8
        assert b"85779\t0.0000" in text and b"130218\t0.1072" in text
        got = host.anno_text(eng, ctgs, runlists, data, header=True, prefix="intergenic", idx_id=1, idx_range=2)
        assert got == exp and host.last_operator_device() == 1
    finally:
        T.close()


# ---- fuzz -----------------------------------------------------------------------------------------
def fuzz_ctgs(rng):
    ctgs = []
    for chr_id in ("1", "2", "3"):
        pos = 1
        for k in range(40):
            ln = int(rng.integers(5000, 60000))
            ctgs.append(dict(id=f"ctg:{chr_id}:{k + 1}", chr_id=chr_id, chr_start=pos, chr_end=pos + ln - 1, seq=b""))
            pos += ln + int(rng.integers(0, 3000))
    return ctgs


N_FUZZ = 1_000_000


def test_locate_and_count_text_fuzz(eng):
    rng = np.random.default_rng(7)
    ctgs = fuzz_ctgs(rng)
    rgs = fuzz_ranges(rng, ctgs, N_FUZZ)
    tails = rng.integers(0, 4, N_FUZZ)
    lines = [r if t == 0 else r + "\tx" * int(t) for r, t in zip(rgs, tails)]      # extra tab fields
    lines[-1] = f"{ctgs[3]['chr_id']}:{ctgs[3]['chr_start'] + 7}-{ctgs[3]['chr_start'] + 90}\r"  # kept '\r'
    data = assemble(rng, lines)
    exp = host.locate(eng, ctgs, first_fields(data)).encode()
    assert exp.endswith(b"\r\tctg:1:4\n")
    recs = []
    for c in ctgs[::2]:
        a = rng.integers(c["chr_start"], c["chr_end"] + 1, 300)
        b = np.minimum(a + rng.choice([0, 0, 5, 300], 300), c["chr_end"])
        recs += [(c["id"], f"{c['chr_id']}:{x}-{y}") for x, y in zip(a, b)]
    exp_count = host.locate(eng, ctgs, first_fields(data), count=True, rg_records=recs).encode()
    T = LocTables(eng, ctgs, recs)
    try:
        rc, text, rows = abi_locate(eng, T, data)
        assert rc == 0 and text == exp and rows == exp.count(b"\n")
        rc, text, rows = abi_locate(eng, T, data, count=True)
        assert rc == 0 and text == exp_count
        # a located ctg without an rg group: refused (the host path reports it)
        g = T.rg_group.copy()
        g[:] = np.uint32(0xFFFFFFFF)
        rc, _, _ = abi_locate(eng, T, data, count=True, rg_group=g)
        assert rc == _lib.EUNSUPPORTED
    finally:
        T.close()
    assert host.locate_text(eng, ctgs, data) == exp and host.last_operator_device() == 1
    assert host.locate_text(eng, ctgs, data, count=True, rg_records=recs) == exp_count
    assert host.last_operator_device() == 1


def fuzz_runlists(rng, ctgs):
    runlists = {}
    for chr_id in ("1", "2"):                      # chromosome 3 is not in the set
        end = max(c["chr_end"] for c in ctgs if c["chr_id"] == chr_id)
        cuts = np.sort(rng.choice(np.arange(1, end, 3), 4000, replace=False))
        runlists[chr_id] = ",".join(f"{a}-{b - 1}" if b - 1 > a else f"{a}" for a, b in zip(cuts[0::2], cuts[1::2]))
    return runlists


def test_anno_text_fuzz(eng):
    rng = np.random.default_rng(11)
    ctgs = fuzz_ctgs(rng)
    runlists = fuzz_runlists(rng, ctgs)
    rgs = fuzz_ranges(rng, ctgs, N_FUZZ)
    by_chr = {}
    for c in ctgs:
        by_chr.setdefault(c["chr_id"], []).append(c["id"])
    kind = rng.integers(0, 10, N_FUZZ)
    lines = []
    for i, (r, k) in enumerate(zip(rgs, kind)):
        m = RANGE.match(r.strip())
        chrom = m.group(1) if m else "3"
        ids = by_chr.get(chrom, by_chr["3"])
        cid = ids[i % len(ids)]
        if chrom != "3" and m and int(m.group(2)) > int(m.group(3) or m.group(2)):
            r = f"{chrom}:{m.group(2)}"                                    # no reversed range in the set
        if k == 0:
            lines.append(f"rg:{cid}:{i}\t{r}")
        elif k == 1:
            lines.append(f"x{cid.upper()}_y\t{r}" if chrom == "3" else f"x{cid}_y\t{r}")   # mixed-case CTG: off the set
        elif k == 2:
            lines.append(f"no id here\t{r}\textra")
        elif k == 3:
            lines.append(f"{cid}\tCtg:3:1\t{r}")                           # the range in field 3: invalid here
        elif k == 4 and chrom == "3":
            lines.append(f"{cid}\t3:900-10")                               # reversed, off the set: prop 0
        else:
            lines.append(f"{cid}\t{r}\t{i}")
    lines[-1] = f"{by_chr['1'][0]}\t1:10-300\r"
    data = assemble(rng, lines, allow_empty=False)
    exp = host.anno(eng, ctgs, runlists, [ln.decode() for ln in rust_lines(data)], idx_id=1, idx_range=2).encode()
    assert b"\r\t" in exp
    T = AnnoTables(eng, ctgs, runlists)
    try:
        rc, text, rows = abi_anno(eng, T, data)
        assert rc == 0 and text == exp and rows == exp.count(b"\n")
        rc, text, _ = abi_anno(eng, T, b"ID\trange\n" + data, header=True, prefix="fz")
        assert rc == 0 and text == b"ID\trange\tfzProp\n" + exp
    finally:
        T.close()
    assert host.anno_text(eng, ctgs, runlists, data) == exp and host.last_operator_device() == 1


def test_anno_text_prop4_every_fraction(eng):
    """prop = a/b for every 0 <= a <= b <= 2000: the set covers [1, 5000], the range [5001 - a, 5000 - a + b]."""
    ctgs = [dict(id="ctg:1:1", chr_id="1", chr_start=1, chr_end=1000000, seq=b"")]
    runlists = {"1": "1-5000"}
    pairs = [(a, b) for b in range(1, 2001) for a in range(b + 1)]
    data = "".join(f"ctg:1:1\t1:{5001 - a}-{5000 - a + b}\n" for a, b in pairs).encode()
    T = AnnoTables(eng, ctgs, runlists)
    try:
        rc, text, rows = abi_anno(eng, T, data)
    finally:
        T.close()
    assert rc == 0 and rows == len(pairs)
    got = [ln.rsplit(b"\t", 1)[1].decode() for ln in text.split(b"\n")[:-1]]
    a = np.array([p[0] for p in pairs], np.float32)
    b = np.array([p[1] for p in pairs], np.float32)
    props = a / b
    want = [fmt4_exact(p) for p in props]
    bad = [(pairs[i], got[i], want[i]) for i in range(len(pairs)) if got[i] != want[i]]
    assert not bad, bad[:10]


# ---- refusals and errors --------------------------------------------------------------------------
def test_refusals_fall_back(eng, s288c):
    ctgs = all_ctgs(s288c)
    T = LocTables(eng, ctgs)
    try:
        data = "I:1000-1100\tgène\nMito:1000-1100\n".encode()
        rc, _, _ = abi_locate(eng, T, data)
        assert rc == _lib.EUNSUPPORTED
        rc, _, _ = abi_locate(eng, T, b"I:1000-1100\x00\n")
        assert rc == _lib.EUNSUPPORTED
    finally:
        T.close()
    got = host.locate_text(eng, ctgs, data)
    assert got == b"I:1000-1100\tctg:I:1\nMito:1000-1100\tctg:Mito:1\n" and host.last_operator_device() == 0
    runlists = {"I": "1-5000,6000-9000"}
    data = b"ctg:I:1\tI:10-5\nctg:I:1\tI:1-100\n"
    A = AnnoTables(eng, ctgs, runlists)
    try:
        rc, _, _ = abi_anno(eng, A, data)
        assert rc == _lib.EUNSUPPORTED                                     # reversed range on a chromosome of the set
    finally:
        A.close()
    exp = host.anno(eng, ctgs, runlists, ["ctg:I:1\tI:10-5", "ctg:I:1\tI:1-100"]).encode()
    assert host.anno_text(eng, ctgs, runlists, data) == exp and host.last_operator_device() == 0


def test_anno_text_errors(eng, s288c):
    ctgs = all_ctgs(s288c)
    runlists = {"I": "1-5000"}
    A = AnnoTables(eng, ctgs, runlists)
    try:
        for data, kw in [(b"ctg:I:1\tI:1-100\nctg:I:1\n", {}),                # field 2 missing on line 2
                         (b"ctg:I:1\tI:1-100\n", dict(idx_range=3)),
                         (b"ctg:I:1\tI:1-100\n", dict(idx_id=0)),
                         (b"ctg:I:99\tI:1-100\n", {})]:                      # unknown id on a chromosome of the set
            rc, _, _ = abi_anno(eng, A, data, **kw)
            assert rc == _lib.EINVAL, (data, kw)
            with pytest.raises(host.HostError) as ei:
                host.anno_text(eng, ctgs, runlists, data, **kw)
            assert ei.value.code == _lib.EINVAL
            with pytest.raises(host.HostError) as ei:
                host.anno(eng, ctgs, runlists, [ln.decode() for ln in rust_lines(data)], **kw)
            assert ei.value.code == _lib.EINVAL
        # the id check applies on chromosomes of the set only
        rc, text, _ = abi_anno(eng, A, b"ctg:II:99\tII:1-100\n")
        assert rc == 0 and text == b"ctg:II:99\tII:1-100\t0.0000\n"
    finally:
        A.close()


def test_names_reject_duplicates(eng):
    nm = C.c_void_p()
    arr = (C.c_char_p * 3)(b"I", b"II", b"I")
    assert L.gams_names_create(eng.h, 3, arr, C.byref(nm)) == _lib.EINVAL


# ---- size -----------------------------------------------------------------------------------------
def test_locate_text_over_4gib(eng, s288c):
    """a few valid lines whose second fields are 1.1 GiB of padding: offsets past 2^32"""
    ctgs = all_ctgs(s288c)
    pad = b"x" * (1100 << 20)
    data = bytearray()
    for head, end in [(b"I:1000-1100\t", b"\n"), (b"Mito:5-50\t", b"\r\n"), (b"II:1-5\t", b"\n"),
                      (b"I:20000-20100\t", b"\n")]:
        data += head
        data += pad
        data += end
    del pad
    data += b"Mito:70000\tend"
    assert len(data) > (4 << 30)
    exp = host.locate(eng, ctgs, ["I:1000-1100", "Mito:5-50", "II:1-5", "I:20000-20100", "Mito:70000"]).encode()
    assert exp.count(b"\n") == 4
    T = LocTables(eng, ctgs)
    try:
        rc, text, rows = abi_locate(eng, T, data)
    finally:
        T.close()
    assert rc == 0 and rows == 4 and text == exp


def test_locate_text_1e7_lines(eng):
    rng = np.random.default_rng(5)
    ctgs = fuzz_ctgs(rng)
    rgs = fuzz_ranges(rng, ctgs, 1_000_000)
    chunk = ("\n".join(rgs) + "\n").encode()
    exp1 = host.locate(eng, ctgs, rgs).encode()
    data = chunk * 10
    T = LocTables(eng, ctgs)
    try:
        rc, text, rows = abi_locate(eng, T, data)
    finally:
        T.close()
    assert rc == 0 and text == exp1 * 10
    assert host.locate_text(eng, ctgs, data) == exp1 * 10 and host.last_operator_device() == 1
