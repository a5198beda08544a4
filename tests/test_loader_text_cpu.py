"""CPU checks of the loaders on the device over several files (gams_index_create_range_files, gams_gpu_loader_text,
host.loader_text, rg_data=[...]): the entries are declared, bound and exported, null arguments are refused, and a
pure-Python model of the load -- `gams rg f1 f2 ...` / `gams feature f1 f2 ...` (rg.rs:40-82, feature.rs:47-96): one
read_range per file, drop-first per file, cnt:{kind}:{ctg} carried on across files, Range::to_string() reprinted -- and
of the three row formats reproduces the reference's pinned counts on the goldens.  tests/test_gpu_loader_text.py holds
the device against this model."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import helpers
from gams_amd import _lib, host
from test_rg_text_cpu import locate_one, locator_order, model, parse_line, rust_lines

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GPU_NEW = ("gams_index_create_range_files", "gams_gpu_loader_text")
HOST_NEW = ("gams_host_loader_text", "gams_host_locate_rgs", "gams_host_locate_text_rgs", "gams_host_sw_actions_rgs",
            "gams_host_sw_multi_actions_rgs", "gams_host_sw_text_rgs")
RG, FEATURE = _lib.LOADER_RG, _lib.LOADER_FEATURE
RECORDS, TSV, RESP = _lib.LOADER_RECORDS, _lib.LOADER_TSV, _lib.LOADER_RESP


# ---- the model ------------------------------------------------------------------------------------
def range_parts(line):
    """(name, chr, strand, start, end) of a line Range::from_str accepts (gams_host.cpp, step for step), else None"""
    s = line.decode("latin-1").rstrip("\r\n ")
    colon = s.rfind(":")
    if colon <= 0 or colon + 1 >= len(s):
        return None
    head, tail = s[:colon], s[colon + 1:]
    m = re.match(r"^(\d{1,10})(?:[-_]+(\d{1,10}))?$", tail, re.A)
    if not m:
        return None
    st = int(m.group(1))
    en = int(m.group(2)) if m.group(2) else st
    if st > 0x7fffffff or en > 0x7fffffff:
        return None
    strand = name = ""
    if head.endswith(")"):
        o = head.rfind("(")
        if o < 0:
            return None
        strand, head = head[o + 1:-1], head[:o]
    dot = head.find(".")
    if dot >= 0:
        name, head = head[:dot], head[dot + 1:]
    if not head or not re.match(r"^[0-9A-Za-z_/-]+$", head):
        return None
    return name, head, strand, st, en


def canonical(parts):
    """Range::to_string()"""
    name, chr_id, strand, s, e = parts
    return (name + "." if name else "") + chr_id + (f"({strand})" if strand else "") + ":" + (str(s) if s == e else f"{s}-{e}")


def json_escape(v):
    return v.replace("\\", "\\\\").replace('"', '\\"')


def i32(v):
    return (v + 2 ** 31) % 2 ** 32 - 2 ** 31


def resp(args):
    out = b"*%d\r\n" % len(args)
    for a in args:
        out += b"$%d\r\n%s\r\n" % (len(a), a)
    return out


def record_row(kind, fmt, ctg_id, serial, parts, tag):
    """one record as text: kind RG / FEATURE, fmt RECORDS / TSV / RESP"""
    rid = f"{'feature' if kind == FEATURE else 'rg'}:{ctg_id}:{serial}"
    rng = canonical(parts)
    length = i32(parts[4] - parts[3] + 1)
    if fmt == TSV:
        row = f"{rid}\t{rng}" + (f"\t{length}\t{tag}" if kind == FEATURE else "") + "\n"
        return row.encode("latin-1")
    js = '{"id":"' + json_escape(rid) + '","range":"' + json_escape(rng) + '"'
    if kind == FEATURE:
        js += f',"length":{length},"tag":"' + json_escape(tag) + '"'
    js += "}"
    if fmt == RESP:
        return resp([b"SET", rid.encode("latin-1"), js.encode("latin-1")])
    return (rid + "\t" + js + "\n").encode("latin-1")


def model_files(ctgs, files):
    """The loader over several files.  ctgs in the order of the ctg index (locator_order).  -> dict(seen[i] = ctg i had a
    located line in any file; kept[f][i] = [(parts, line)] kept of ctg i in file f, in line order, the first located line
    of the ctg IN THAT FILE dropped; lines[f])"""
    seen = [False] * len(ctgs)
    kept, n_lines = [], []
    for data in files:
        lines = rust_lines(data)
        n_lines.append(len(lines))
        here = [False] * len(ctgs)
        buckets = [[] for _ in ctgs]
        for k, ln in enumerate(lines):
            p = range_parts(ln)
            assert (p is None) == (parse_line(ln) is None) and (p is None or (p[1], p[3], p[4]) == parse_line(ln)), ln
            if p is None:
                continue
            i = locate_one(ctgs, p[1], p[3], p[4])
            if i is None:
                continue
            if here[i]:
                buckets[i].append((p, k))
            here[i] = seen[i] = True
        kept.append(buckets)
    return dict(seen=seen, kept=kept, lines=n_lines)


def model_loader(ctgs, files, kind=RG, tag="feature", fmt=RECORDS, base=None):
    """gams_gpu_loader_text's answer: dict(rows[f][i] = the rows of file f and ctg i as bytes, text = all of them in
    (file, ctg) order, off = their n_files * n_ctg + 1 offsets, next[i] = the counter of ctg i after the load, per_file,
    n_rows)"""
    m = model_files(ctgs, files)
    nxt = list(base) if base is not None else [0] * len(ctgs)
    rows, off, text = [], [0], b""
    for f in range(len(files)):
        rows.append([])
        for i, c in enumerate(ctgs):
            out = b""
            for parts, _ in m["kept"][f][i]:
                nxt[i] += 1
                out += record_row(kind, fmt, c["id"], nxt[i], parts, tag)
            rows[f].append(out)
            text += out
            off.append(len(text))
    per_file = [sum(len(b) for b in m["kept"][f]) for f in range(len(files))]
    return dict(rows=rows, text=text, off=off, next=nxt, per_file=per_file, n_rows=sum(per_file), seen=m["seen"])


def host_order_text(ctgs, ml):
    """the model's rows in the order host.loader_text returns them: file by file, the ctgs by id"""
    by_id = sorted(range(len(ctgs)), key=lambda i: ctgs[i]["id"].encode())
    return b"".join(ml["rows"][f][i] for f in range(len(ml["rows"])) for i in by_id)


# ---- tests ----------------------------------------------------------------------------------------
def test_new_entries_are_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "gams_gpu.h")).read()
    lib = C.CDLL(_lib.SO_PATH)
    for name in GPU_NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert name in _lib.PROTOTYPES, name
        assert hasattr(lib, name), name
    for name in ("GAMS_LOADER_RG", "GAMS_LOADER_FEATURE", "GAMS_LOADER_RECORDS", "GAMS_LOADER_TSV", "GAMS_LOADER_RESP"):
        assert re.search(r"#define\s+" + name + r"\s+" + str(getattr(_lib, name[5:])) + r"\b", hdr), name
    hl = C.CDLL(host.SO_PATH)
    for name in HOST_NEW:
        assert hasattr(hl, name), name
    assert callable(host.loader_text)


def test_null_arguments_are_einval():
    lib = _lib.load()
    n, ix, text, nb = C.c_uint64(), C.c_void_p(), C.c_void_p(), C.c_uint64()
    assert lib.gams_index_create_range_files(None, None, None, 1, None, None, C.byref(ix), None, C.byref(n)) == _lib.EINVAL
    assert lib.gams_gpu_loader_text(None, None, None, None, 1, None, None, RG, None, 0, RECORDS, None, C.byref(text),
                                    C.byref(nb), None, None, None, C.byref(n)) == _lib.EINVAL


class _NoDevice:
    h = None


def test_rg_data_takes_a_list_and_still_excludes_rg_records():
    ctg = dict(id="ctg:I:1", chr_id="I", chr_start=1, chr_end=1000, seq=b"A" * 1000)
    recs = [("ctg:I:1", "I:5-8")]
    for files in ([b"I:5-8\n", b"I:9\n"], (b"I:5-8\n",)):
        assert host._one_rg_source((), files) == [bytes(f) for f in files]
        with pytest.raises(ValueError):
            host.locate(_NoDevice(), [ctg], ["I:1-10"], count=True, rg_records=recs, rg_data=files)
        with pytest.raises(ValueError):
            host.locate_text(_NoDevice(), [ctg], b"I:1-10\n", count=True, rg_records=recs, rg_data=files)
        with pytest.raises(ValueError):
            host.sw(_NoDevice(), ctg, [("feature:ctg:I:1:1", 100, 200)], actions=("gc", "count"), rg_records=recs, rg_data=files)
        with pytest.raises(ValueError):
            host.sw_multi([_NoDevice()], [ctg], [[("feature:ctg:I:1:1", 100, 200)]], actions=("count",), rg_records=recs,
                          rg_data=files)
        with pytest.raises(ValueError):
            host.sw_text(_NoDevice(), [ctg], b"I:100-200\n", actions=("count",), rg_records=recs, rg_data=files)
    assert host._one_rg_source((), b"I:5-8\n") == b"I:5-8\n" and host._one_rg_source((), None) is None
    with pytest.raises(ValueError):
        host.loader_text(_NoDevice(), [ctg], [b""], kind="peak")


def test_range_parts_and_canonical_text():
    want = {b"I:5": "I:5", b"I:5-5": "I:5", b"I:007_9 ": "I:7-9", b"I:9-5": "I:9-5", b"I(+):5-9": "I(+):5-9",
            b"I():5-9": "I:5-9", b"nm.I(-):5--9\r": "nm.I(-):5-9", b".I:5": "I:5", b'a"b\\(.I("):1': 'a"b\\(.I("):1',
            b"n(m.I:5": "n(m.I:5"}
    for ln, text in want.items():
        assert canonical(range_parts(ln)) == text, ln
    for ln in (b"", b"I", b"I:", b":5", b"I:1-100\tfoo", b"I:12345678901", b"I:2147483648", b"a.b.c:1-2", b"I(+:1-2", b"(+):5"):
        assert range_parts(ln) is None and parse_line(ln) is None, ln


def test_row_formats():
    p = range_parts(b'na"me.I(+):007_9 ')
    assert record_row(RG, RECORDS, "ctg:I:1", 12, p, "") == b'rg:ctg:I:1:12\t{"id":"rg:ctg:I:1:12","range":"na\\"me.I(+):7-9"}\n'
    assert record_row(RG, TSV, "ctg:I:1", 12, p, "") == b'rg:ctg:I:1:12\tna"me.I(+):7-9\n'
    js = b'{"id":"feature:ctg:I:1:3","range":"na\\"me.I(+):7-9","length":3,"tag":"t\\\\g"}'
    assert record_row(FEATURE, RECORDS, "ctg:I:1", 3, p, "t\\g") == b"feature:ctg:I:1:3\t" + js + b"\n"
    assert record_row(FEATURE, TSV, "ctg:I:1", 3, p, "t\\g") == b'feature:ctg:I:1:3\tna"me.I(+):7-9\t3\tt\\g\n'
    assert record_row(FEATURE, RESP, "ctg:I:1", 3, p, "t\\g") == \
        b"*3\r\n$3\r\nSET\r\n$17\r\nfeature:ctg:I:1:3\r\n$%d\r\n%s\r\n" % (len(js), js)
    assert record_row(FEATURE, TSV, "c", 1, range_parts(b"I:9-5"), "") == b"feature:c:1\tI:9-5\t-3\t\n"


def golden_ctgs(s288c):
    ctgs = []
    for chr_id in ("I", "Mito"):
        ctgs += helpers.gen_ctgs(chr_id, s288c[chr_id], piece=100000)
    return locator_order(ctgs)


def golden(name):
    with open(os.path.join(helpers.S288C, name), "rb") as fh:
        return fh.read()


def test_spo11_alone_is_69_records_numbered_from_one(s288c):
    """tests/cli.rs:235-304: 79 lines, 71 located, 69 records; the serials of a ctg are 1..n"""
    ctgs = golden_ctgs(s288c)
    ml = model_loader(ctgs, [golden("spo11_hot.rg")])
    assert ml["n_rows"] == 69 and ml["per_file"] == [69] and sum(ml["seen"]) == 2 and sum(ml["next"]) == 69
    for i, c in enumerate(ctgs):
        rows = ml["rows"][0][i].splitlines()
        assert [r.split(b"\t")[0] for r in rows] == [f"rg:{c['id']}:{k}".encode() for k in range(1, ml["next"][i] + 1)]
    # one file is the one-file model
    one = model(ctgs, golden("spo11_hot.rg"))
    assert [len(b) for b in one["buckets"]] == ml["next"]


def test_two_files_are_two_loads_not_their_concatenation(s288c):
    ctgs = golden_ctgs(s288c)
    a, b = golden("spo11_hot.rg"), golden("SK1.snp.rg")
    assert a.endswith(b"\n")
    both = model_loader(ctgs, [a, b])
    la, lb = model_loader(ctgs, [a]), model_loader(ctgs, [b])
    assert both["next"] == [x + y for x, y in zip(la["next"], lb["next"])]
    assert both["per_file"] == [la["n_rows"], lb["n_rows"]] and both["per_file"][0] == 69
    cat = model_loader(ctgs, [a + b])
    assert cat["next"] != both["next"] and cat["n_rows"] > both["n_rows"]      # the second file's first lines are kept
    # the serials of the second file continue behind the first's: the same as loading it on the first's counters
    again = model_loader(ctgs, [b], base=la["next"])
    assert again["rows"][0] == both["rows"][1] and again["next"] == both["next"]
    for fmt in (TSV, RESP):
        assert model_loader(ctgs, [a, b], FEATURE, "hot", fmt)["n_rows"] == both["n_rows"]


# ---- the fuzz inputs of tests/test_gpu_loader_text.py ----------------------------------------------
def fuzz_table(rng):
    """up to 40 ctgs over three chromosomes, gaps between them, given in an order that is not the id order"""
    ctgs = []
    n = int(rng.integers(3, 41))
    pos = {"1": 1, "2": 1, "X-a/b": 1}
    for k in range(n):
        chr_id = ("1", "2", "X-a/b")[int(rng.integers(0, 3))]
        ln = int(rng.integers(50, 5000))
        serial = sum(c["chr_id"] == chr_id for c in ctgs) + 1
        ctgs.append(dict(id=f"ctg:{chr_id}:{serial}", chr_id=chr_id, chr_start=pos[chr_id], chr_end=pos[chr_id] + ln - 1, seq=b""))
        pos[chr_id] += ln + int(rng.integers(0, 300))
    return [ctgs[i] for i in rng.permutation(n)]


def fuzz_file(rng, ctgs, n):
    """n lines: valid, malformed, on unknown chromosomes, between ctgs, a point on a ctg start; no control bytes but the
    line ends"""
    names = ("", "", "nm.", 'q"uo\\te.', "n(m.", ".")
    strands = ("", "", "(+)", "(-)", '(")', "()")
    out = []
    for _ in range(n):
        c = ctgs[int(rng.integers(0, len(ctgs)))]
        k = int(rng.integers(0, 14))
        s = max(1, c["chr_start"] + int(rng.integers(-100, 5200)))
        e = s + int(rng.choice([0, 0, 1, 10, 500, 6000]))
        head = names[int(rng.integers(0, len(names)))] + c["chr_id"] + strands[int(rng.integers(0, len(strands)))]
        if k == 0:
            out.append(f"{c['chr_id']}:{c['chr_start']}")                  # a point on a ctg start: not located
        elif k == 1:
            out.append(f"{head}:{s}__-{e} ")
        elif k == 2:
            out.append(f"chrUn:{s}-{e}")
        elif k == 3:
            out.append(f"{head}:{12345678901 if s % 2 else 3000000000}-{e}")
        elif k == 4:
            out.append(f"{c['chr_id']}-{s}-{e}")
        elif k == 5:
            out.append(f"{head}:{s}-")
        elif k == 6:
            out.append(f"{head}:{e}-{s}")                                  # reversed where e > s
        elif k == 7:
            out.append("")
        elif k == 8:
            out.append(f"{head}:00{s}")
        else:
            out.append(f"{head}:{s}-{e}" if e != s else f"{head}:{s}")
    nl = ["\r\n" if x else "\n" for x in rng.random(n) < 0.2]
    data = "".join(ln + end for ln, end in zip(out, nl))
    if n and rng.random() < 0.5:
        data = data[:-len(nl[-1])]                                         # the last line without its '\n'
    return data.encode("latin-1")


def fuzz_case(seed):
    """(ctgs, files, kind, tag, fmt, base by ctg id) of one seed: up to 4 files of up to 2,000 lines"""
    rng = np.random.default_rng(seed)
    ctgs = fuzz_table(rng)
    files = [fuzz_file(rng, ctgs, int(rng.choice([0, 1, 70, 700, 2000]))) for _ in range(int(rng.integers(1, 5)))]
    kind = (RG, FEATURE)[seed % 2]
    fmt = (RECORDS, TSV, RESP)[seed % 3]
    base = {c["id"]: int(rng.choice([0, 0, 8, 99, 12345])) for c in ctgs}
    return ctgs, files, kind, ('t"a\\g', "", "peak")[seed % 3], fmt, base


def test_fuzz_inputs_hold_no_control_bytes_and_the_model_takes_them():
    for seed in range(20):
        ctgs, files, kind, tag, fmt, base = fuzz_case(seed)
        assert len(ctgs) <= 40 and 1 <= len(files) <= 4
        for data in files:
            assert not re.search(rb"[\x00-\x09\x0b\x0c\x0e-\x1f\x80-\xff]", data)
            assert not re.search(rb"\r(?!\n)", data)                       # a '\r' only in front of a '\n'
        order = locator_order(ctgs)
        ml = model_loader(order, files, kind, tag, fmt, [base[c["id"]] for c in order])   # (asserts the two parsers agree)
        assert ml["n_rows"] == sum(ml["per_file"]) and len(ml["off"]) == len(files) * len(order) + 1
    assert any(model_loader(locator_order(c), f)["n_rows"] > 100 for c, f, *_ in map(fuzz_case, range(20)))
