"""A pure-Python model of `gams gen` over the bytes of one FASTA file, and the edge battery that the CPU reader test and
the GPU tests of gams_gpu_gen_text share.

The model restates bio::io::fasta::Reader as gen.rs:67-78 uses it (include/gams_gpu.h, gams_gpu_gen_text), then runs
helpers.gen_ctgs per record; `refusal` says what the device entry does with an input instead of answering."""
import collections

import numpy as np

import helpers

WS = b" \t\n\x0b\x0c\r"        # ASCII white space, what the reference's trim_end() drops from a line
BLK = 16384                     # bytes per workgroup of the device's passes over the input

Case = collections.namedtuple("Case", "name data piece fill min_len")


class NotFasta(ValueError):
    """the first byte is not '>' (the reference panics: Expected > at record start)"""


def lines_of(data):
    """split on b'\\n'; a last line without one counts, nothing follows a final one"""
    lines = data.split(b"\n")
    if lines[-1] == b"":
        lines.pop()
    return lines


def header_id(line):
    """the bytes behind '>' up to the first ASCII white space or the line's end"""
    n = 1
    while n < len(line) and line[n] not in WS:
        n += 1
    return line[1:n].decode("latin-1")


def records(data):
    """[(id, bases)] in file order, as the reference reads them: every sequence line trimmed of trailing white space"""
    if not data:
        return []
    if data[:1] != b">":
        raise NotFasta()
    recs = []
    for line in lines_of(data):
        if line[:1] == b">":
            recs.append([header_id(line), []])
        else:
            recs[-1][1].append(line.rstrip(WS))
    return [(name, b"".join(chunks)) for name, chunks in recs]


def refusal(data):
    """None, "EINVAL" or "EUNSUPPORTED": what gams_gpu_gen_text returns for these bytes instead of a table"""
    if not data:
        return None
    if data[:1] != b">":
        return "EINVAL"
    if any(b >= 0x80 or b == 0 for b in np.unique(np.frombuffer(data, np.uint8)).tolist()):
        return "EUNSUPPORTED"
    seen = set()
    for line in lines_of(data):
        if line[:1] == b">":
            name = header_id(line)
            if not name or name in seen:
                return "EUNSUPPORTED"
            seen.add(name)
        else:
            body = line[:-1] if line[-1:] == b"\r" else line      # one '\r' in front of the '\n' or at the input's end
            if any(c in b" \t\x0b\x0c\r" for c in body):
                return "EUNSUPPORTED"
    return None


def model(data, piece=500000, fill=50, min_len=5000):
    """-> (ctgs as helpers.gen_ctgs gives them, in record order; {chromosome: bases}).  A duplicate id continues its
    serial counter and keeps its last length (cnt:ctg:{chr} and len_of, gen.rs:78 and :133)."""
    ctgs, chr_len, serial = [], {}, {}
    for name, seq in records(data):
        chr_len[name] = len(seq)
        for c in helpers.gen_ctgs(name, seq, piece, fill, min_len):
            serial[name] = serial.get(name, 0) + 1
            c["id"] = f"ctg:{name}:{serial[name]}"
            ctgs.append(c)
    return ctgs, chr_len


def table(ctgs):
    """what the tests compare of a ctg list: (id, chr_id, chr_start, chr_end, length)"""
    return [(c["id"], c["chr_id"], c["chr_start"], c["chr_end"], c["length"]) for c in ctgs]


# ---- inputs ---------------------------------------------------------------------------------------------------------
def fold(seq, width, eol=b"\n"):
    """the lines of a sequence at one width, every one ended"""
    seq = bytes(seq)
    return b"".join(seq[i:i + width] + eol for i in range(0, len(seq), width))


def fasta(recs, width=60, eol=b"\n"):
    return b"".join(b">" + name.encode() + eol + fold(seq, width, eol) for name, seq in recs)


def bases(n, seed, nrate=0.0):
    return helpers.synth(n, seed, nrate=nrate).tobytes()


def with_runs(n, seed, runs):
    """n synthetic bases without N, then N over every (start, length) of runs"""
    a = np.frombuffer(bases(n, seed), np.uint8).copy()
    for s, k in runs:
        a[s:s + k] = ord("N")
    return a.tobytes()


def header_at(pos, name, first="a"):
    """a file whose second header line begins exactly at byte `pos` (the first record's bases fill the room in front)"""
    head = b">" + first.encode() + b"\n"
    room = pos - len(head)                       # lines of 60 bases + '\n', then one shorter line
    full, rest = divmod(room, 61)
    if rest == 0:
        full, rest = full - 1, 61
    seq = bases(full * 60 + rest - 1, 5)
    body = fold(seq[:full * 60], 60) + seq[full * 60:] + b"\n"
    assert len(head + body) == pos
    return head + body + b">" + name.encode() + b"\n" + fold(bases(500, 6), 60)


def line_cases():
    out = []
    small = dict(piece=700, fill=5, min_len=20)
    two = [("a", with_runs(2000, 1, [(0, 3), (500, 4), (900, 5), (1400, 40)])), ("b", with_runs(1500, 2, [(700, 9), (1490, 10)]))]
    for w in (1, 15, 16, 17, 60, 61, 255, 256, 257):
        out.append(Case(f"width{w}", fasta(two, w), **small))
    mixed = b">m\n" + b"".join(two[0][1][i:j] + b"\n" for i, j in ((0, 1), (1, 17), (17, 33), (33, 290), (290, 291), (291, 2000)))
    out.append(Case("mixed_widths", mixed + fasta(two[1:], 61), **small))
    out.append(Case("crlf", fasta(two, 60, b"\r\n"), **small))
    plain = fasta(two, 60)
    out.append(Case("no_final_newline", plain[:-1], **small))
    out.append(Case("final_cr", plain[:-1] + b"\r", **small))
    out.append(Case("last_header_no_newline", plain + b">tail", **small))
    blank = b">a\n\n" + fold(two[0][1][:600], 60) + b"\n\r\n\n" + fold(two[0][1][600:], 60) + b"\n\n>b\n" + fold(two[1][1], 60) + b"\n\n"
    out.append(Case("blank_lines", blank, **small))
    out.append(Case("gt_inside_line", b">a desc > more\n" + fold(two[0][1][:300], 60) + b"AC>GT\n" + fold(two[0][1][300:], 60), **small))
    out.append(Case("long_header", b">L " + b"x" * 17000 + b"\n" + fold(two[0][1], 60) + b">M\t" + b"y" * 40000 + b"\n" + fold(two[1][1], 60),
                    **small))
    out.append(Case("header_starts_after_seam", header_at(BLK, "b"), **small))
    out.append(Case("header_gt_ends_block", header_at(BLK - 1, "b"), **small))
    for name, pos in (("header_ends_on_seam", BLK - 3), ("header_newline_after_seam", BLK - 2)):   # ">b\n" ends at pos + 3
        out.append(Case(name, header_at(pos, "b"), **small))
    # '\r' as the last byte of a block and its '\n' first in the next: CRLF lines of 62 bytes behind a header of the
    # length that puts a line's '\r' there
    for name, at in (("cr_ends_block", BLK - 1), ("cr_ends_second_block", 2 * BLK - 1)):
        seq = bases(40000, 7, 2e-3)
        data = next(d for d in (fasta([("c" * n, seq)], 60, b"\r\n") for n in range(1, 63)) if d[at:at + 2] == b"\r\n")
        out.append(Case(name, data, piece=3000, fill=5, min_len=20))
    many = [(f"r{i}", bases(10, 100 + i)) for i in range(1000)]
    out.append(Case("thousand_records", fasta(many, 60), piece=700, fill=5, min_len=5))
    out.append(Case("all_geometries_one_file",
                    b"".join(fasta([(f"w{w}{n}", s) for n, s in two], w) for w in (1, 15, 16, 17, 60, 61, 255, 256, 257))
                    + fasta([("x" + n, s) for n, s in two], 60, b"\r\n") + b">e1\n>e2\n\n>last\n" + two[0][1][:77], **small))
    return out


def span_cases():
    out = []
    A = lambda n, seed=3: bases(n, seed)
    N = lambda n: b"N" * n
    # an N-run over line breaks and over the seam between the first two 16-KiB blocks of the INPUT (base i of the one
    # record lies at byte 3 + i + i // 60), one over base 4 * 4096 of the stream (a workgroup seam of the scan), one over a
    # single line break, and a single N
    at = next(i for i in range(BLK) if 3 + i + i // 60 >= BLK - 150)
    seq = with_runs(40000, 11, [(at, 300), (BLK - 200, 400), (30, 61), (20000, 1)])
    data = fasta([("s", seq)], 60)
    assert data[BLK - 150:BLK + 100].replace(b"\n", b"") == b"N" * (250 - data[BLK - 150:BLK + 100].count(b"\n"))
    assert data[BLK - 1:BLK + 1] == b"NN" and b"\n" in data[BLK - 150:BLK + 100]
    out.append(Case("n_run_over_seam", data, piece=9000, fill=50, min_len=100))
    out.append(Case("holes_fill", fasta([("h", A(6000) + N(49) + A(6000, 4) + N(50) + A(6000, 5))]), piece=500000, fill=50, min_len=5000))
    out.append(Case("spans_min_len", fasta([("m", N(60) + A(4999) + N(60) + A(5000, 4) + N(60))]), piece=500000, fill=50, min_len=5000))
    p = 1000
    out.append(Case("spans_piece", fasta([("p", N(60).join([A(p), A(p + 1, 4), A(2 * p, 5), A(2 * p + 1, 6), A(3 * p - 1, 7)]))]),
                    piece=p, fill=50, min_len=100))
    out.append(Case("all_n", fasta([("n", N(3000)), ("v", A(400))]), piece=1000, fill=5, min_len=100))
    out.append(Case("empty_records", b">e1\n>e2 nothing\n" + fasta([("v", A(400))]) + b">e3\n\n>e4", piece=1000, fill=5, min_len=100))
    # a leading N-run of k bases in records of 320 bases: the ctg begins k bases behind a multiple of 16 in the stream
    out.append(Case("lead_n", fasta([(f"k{k}", N(k) + A(320 - k, 20 + k)) for k in range(16)], 61), piece=1000, fill=5, min_len=100))
    cross = [("c1", N(10) + A(30)), ("c2", A(30, 4) + N(10))]
    out.append(Case("run_over_chromosomes_short", fasta(cross), piece=1000, fill=5, min_len=50))
    out.append(Case("run_over_chromosomes", fasta(cross), piece=1000, fill=5, min_len=20))
    out.append(Case("run_over_empty_record", b">c1\n" + A(30) + b"\n>c0\n>c2\n" + A(30, 4) + b"\n", piece=1000, fill=5, min_len=20))
    out.append(Case("ctg_255_256_257", fasta([("g", N(60).join([A(255), A(256, 4), A(257, 5), A(1, 6), A(16, 7), A(17, 8)]))]),
                    piece=1000, fill=5, min_len=1))
    return out


def size_case():
    """about 3 MB at width 60: many input blocks, and 16 * k bases, so that the stream's last 16-B unit is full"""
    n = 3_000_000
    a = helpers.synth(n, 42, nrate=1e-4)
    a[-40:] = np.frombuffer(b"ACGT" * 10, np.uint8)          # the last run reaches the end of the stream
    half = 16 * 90000
    return Case("size_3mb", fasta([("big1", a[:half].tobytes()), ("big2", a[half:].tobytes())], 60), piece=100000, fill=50, min_len=5000)


def refused_cases():
    """inputs the device refuses and the host path answers (the reference trims trailing white space of a line)"""
    s = bases(300, 9)
    return [
        Case("trailing_space", b">a\n" + s[:60] + b" \n" + s[60:120] + b"\t\n" + s[120:] + b"\n", 1000, 5, 20),
        Case("trailing_crcr", b">a\n" + s[:60] + b"\r\r\n" + s[60:] + b" \r\n", 1000, 5, 20),
        Case("trailing_vt_ff", b">a\n" + s[:60] + b"\x0b\n" + s[60:] + b"\x0c", 1000, 5, 20),
        Case("interior_tab", b">a\n" + s[:30] + b"\t" + s[30:] + b"\n", 1000, 5, 20),
        Case("interior_cr", b">a\n" + s[:30] + b"\r" + s[30:] + b"\n", 1000, 5, 20),
        Case("duplicate_id", b">a\n" + s + b"\n>b\n" + s[:100] + b"\n>a x\n" + s[:200] + b"\n", 120, 5, 20),
        Case("latin1_id", b">chr\xe9 x\n" + s + b"\n>b\xff\n" + s[:100] + b"\n", 1000, 5, 20),
        Case("empty_id", b">\n" + s + b"\n> spaced\n" + s[:100] + b"\n", 1000, 5, 20),
    ]


def battery():
    return line_cases() + span_cases()
