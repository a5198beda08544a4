"""CPU checks of `gams peak` on the device (gams_gpu_peak_text, host.peak_text): the shortest round-trip f32 formatter
of the amplitudes (gams_fmt_f32_short, csrc/text_fmt.hpp) against std::to_chars over its whole domain and over the
gc_content tables of the wave rows, which the host fills with the same formatter, the pure-Python
model (tests/peak_text.py) against the golden rows, the cases the synthetic input of the GPU test must carry, and the
loud failure without a device.  tests/test_gpu_peak_text.py checks the device against the model."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import helpers
import peak_text as pt
from gams_amd import _lib, host
from oracle import oracle as ora

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

# Every amplitude of `gams peak` is |a - b| in f32 of two round4 gc values a = fl(i / 10^4), b = fl(j / 10^4): all
# pairs 0 <= j <= i <= 10^4.  The reference text is std::to_chars' shortest digits laid out positionally (what
# gams::fmt_f32 prints and Rust's `{}`).  Prints: mismatches, then the count of values per number of significant digits.
POSITIONAL = r"""
#include "text_fmt.hpp"
#include <charconv>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
static std::string positional(float v, int *nd) {
    *nd = 0;
    if (v == 0.0f) return "0";
    char buf[64];
    auto r = std::to_chars(buf, buf + sizeof buf, v, std::chars_format::scientific);
    std::string sci(buf, r.ptr), digits;
    size_t i = 0;
    for (; i < sci.size() && sci[i] != 'e'; ++i)
        if (sci[i] != '.') digits += sci[i];
    const int ex = std::atoi(sci.c_str() + i + 1);
    *nd = (int)digits.size();
    if (ex >= 0) return digits;                       // v <= 1: "1"
    return "0." + std::string((size_t)(-ex - 1), '0') + digits;
}
"""
DRIVER = POSITIONAL + r"""
int main() {
    long bad = 0, hist[12] = {0};
    for (int i = 0; i <= 10000; ++i)
        for (int j = 0; j <= i; ++j) {
            const float v = std::fabs((float)i / 10000.0f - (float)j / 10000.0f);
            char b[64];
            const uint32_t n = gams_fmt_f32_short(v, b), n0 = gams_fmt_f32_short(v, nullptr);
            int nd;
            const std::string want = positional(v, &nd);
            if (n != n0 || std::string(b, n) != want) {
                if (bad < 10) fprintf(stderr, "%.9g: got '%s' want '%s'\n", v, std::string(b, n).c_str(), want.c_str());
                ++bad;
            }
            ++hist[nd];
        }
    printf("%ld", bad);
    for (int k = 0; k < 12; ++k) printf(" %ld", hist[k]);
    printf("\n");
    return 0;
}
"""


def test_fmt_f32_short_is_exact_over_the_amplitude_domain(tmp_path):
    exe = compile_driver(tmp_path, "fmt_main", DRIVER)
    out = subprocess.run([exe], stdout=subprocess.PIPE, text=True, check=True).stdout.split()
    bad, hist = int(out[0]), [int(x) for x in out[1:]]
    print("mismatches", bad, "values per significant digits", hist)
    assert sum(hist) == 10001 * 10002 // 2
    assert bad == 0
    assert hist[8] > 0 and hist[9] > 0 and sum(hist[10:]) == 0


# The gc_content table of the wave rows (RowTabs::fill, csrc/wave.hip): the text of the f32 k / size for every count
# 0 <= k <= size, for every size up to 2048 and the 15 largest a plan takes.  Prints: mismatches, values, the longest text,
# texts longer than 10 bytes, and -- among the sizes up to 255 -- the longest text and the first size and k that have it.
GC_DRIVER = POSITIONAL + r"""
int main() {
    long bad = 0, n = 0, longer = 0;
    unsigned longest = 0, longest255 = 0, size255 = 0, k255 = 0;
    for (int size = 1; size <= 65535; size = size == 2048 ? 65521 : size + 1)
        for (int k = 0; k <= size; ++k, ++n) {
            const float v = (float)k / (float)size;
            char b[64];
            const uint32_t len = gams_fmt_f32_short(v, b), len0 = gams_fmt_f32_short(v, nullptr);
            int nd;
            const std::string want = positional(v, &nd);
            if (len != len0 || std::string(b, len) != want) {
                if (bad < 10) fprintf(stderr, "%d/%d: got '%s' want '%s'\n", k, size, std::string(b, len).c_str(), want.c_str());
                ++bad;
            }
            if (len > longest) longest = len;
            if (len > 10u) ++longer;
            if (size <= 255 && len > longest255) longest255 = len, size255 = (unsigned)size, k255 = (unsigned)k;
        }
    printf("%ld %ld %u %ld %u %u %u\n", bad, n, longest, longer, longest255, size255, k255);
    return 0;
}
"""


def compile_driver(tmp_path, name, text):
    src = tmp_path / (name + ".cpp")
    src.write_text(text)
    exe = tmp_path / name
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "gams_amd", "csrc"),
                           str(src), "-o", str(exe)])
    return str(exe)


def test_the_gc_content_table_is_the_references_text(tmp_path):
    """gams_fmt_f32_short(k / size) against to_chars' positional form for every entry of every table of the sizes 1..2048
    and 65521..65535: no mismatch, no text beyond an entry of the table, and texts of more than 10 bytes among them.  The
    size the GPU tests take for a long gc text (text_edges.GC_LONG_SIZE) is the first up to 255 with the longest text."""
    import text_edges as te

    out = subprocess.run([compile_driver(tmp_path, "gc_main", GC_DRIVER)], stdout=subprocess.PIPE, text=True, check=True).stdout
    bad, n, longest, longer, longest255, size255, k255 = (int(x) for x in out.split())
    print("mismatches", bad, "values", n, "longest", longest, "longer than 10 bytes", longer, "up to size 255:", longest255,
          "bytes at", k255, "/", size255)
    rows_hpp = open(os.path.join(ROOT, "gams_amd", "csrc", "wave_rows.hpp")).read()
    stride = int(re.search(r"constexpr uint32_t kGcStride = (\d+);", rows_hpp).group(1))
    assert n == sum(s + 1 for s in list(range(1, 2049)) + list(range(65521, 65536))) > 3_000_000
    assert bad == 0
    assert longest <= stride - 1 and longer > 0
    assert (te.GC_LONG_SIZE, te.GC_LONG_BYTES) == (size255, longest255) and longest255 > 10
    assert len(te.gc_texts(size255)[k255]) == longest255 == max(len(t) for t in te.gc_texts(size255))


def test_fmt_f32_short_edges():
    f32 = np.float32
    for v, want in [(0.0, "0"), (1.0, "1"), (0.5, "0.5"), (2.0 ** -14, "0.000061035156"),
                    (0.0268, "0.0268"), (float(f32(0.026800007)), "0.026800007")]:
        assert host.fmt_f32_short(v) == want == host.fmt_f32(v) == ora.fmt_f32(v), v
    # a power of two has its lower neighbour half as far away as its upper one: both candidates are tried
    for e in range(0, 15):
        p = f32(2.0 ** -e)
        for v in (np.nextafter(p, f32(0)), p, np.nextafter(p, f32(2))):
            if v <= 1:
                got = host.fmt_f32_short(float(v))
                assert got == host.fmt_f32(float(v)), (e, v)
                assert f32(got) == v, (e, v)
    for v in (float("nan"), float("inf"), -0.5, 1.0000001, 2.0):
        assert host.fmt_f32_short(v) == "", v


def test_new_entry_is_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "gams_gpu.h")).read()
    assert re.search(r"\bint\s+gams_gpu_peak_text\s*\(", hdr)
    assert "gams_gpu_peak_text" in _lib.PROTOTYPES and hasattr(C.CDLL(_lib.SO_PATH), "gams_gpu_peak_text")
    hl = C.CDLL(host.SO_PATH)
    for name in ("gams_host_peak_text", "gams_host_fmt_f32_short"):
        assert hasattr(hl, name), name


class _NoDevice:
    h = None


def test_peak_text_fails_loudly_without_a_device():
    lib = _lib.load()
    text, nb, rows = C.c_void_p(), C.c_uint64(), C.c_uint64()
    data = b"I:1-10\t0.5\t1\n"
    assert lib.gams_gpu_peak_text(None, None, None, None, None, None, None, None, data, len(data), C.byref(text),
                                  C.byref(nb), None, C.byref(rows)) == _lib.EINVAL
    ctgs = [dict(id="ctg:I:1", chr_id="I", chr_start=1, chr_end=1000, seq=b"A" * 1000)]
    with pytest.raises(host.HostError):
        host.peak_text(_NoDevice(), ctgs, data)


def test_model_gives_the_golden_rows(s288c):
    """tests/S288c/I.peaks.tsv on the layout it was made with (piece 500000): the 115 rows test_command_peak expects
    from the oracle (the file is position-sorted, so sorting changes nothing)"""
    ctgs = helpers.gen_ctgs("I", s288c["I"], piece=500000)
    lines = helpers.read_lines("I.peaks.tsv")
    with open(os.path.join(helpers.S288C, "I.peaks.tsv"), "rb") as fh:
        got = pt.model(ctgs, fh.read()).decode()
    peaks = []
    for ln in lines[1:]:
        parts = ln.split("\t")
        _, s, e = helpers.parse_range(parts[0].replace("(+)", ""))
        peaks.append((s, e, parts[2]))
    c = ctgs[0]
    assert got == ora.peak_rows(c["id"], c["chr_id"], c["chr_start"], c["chr_end"], c["seq"], peaks[1:])
    rows = got.splitlines()
    assert len(rows) == 115 and rows[0].startswith("peak:ctg:I:1:1\tI:3091-3210\t120\t")
    # on the piece-100000 layout a peak leaves its ctg: the reference's panic
    many = []
    for chr_id in ("I", "Mito"):
        many += helpers.gen_ctgs(chr_id, s288c[chr_id], piece=100000)
    with open(os.path.join(helpers.S288C, "I.peaks.tsv"), "rb") as fh:
        with pytest.raises(pt.ModelError):
            pt.model(many, fh.read())


def test_model_edges():
    ctgs = [dict(id="ctg:I:1", chr_id="I", chr_start=1, chr_end=1000, seq=b"ACGT" * 250)]
    with pytest.raises(pt.ModelError):                   # a valid range without a signal column, located or not
        pt.model(ctgs, b"I:1-10\t0.5\n")
    with pytest.raises(pt.ModelError):
        pt.model(ctgs, b"II:1-10\n")
    assert pt.model(ctgs, b"") == b"" and pt.model(ctgs, b"I:5-9\t0\t1\n") == b""      # one located line: dropped
    got = pt.model(ctgs, b"I:5-9\t0\t1\nn.I(-):0021_24\t0\t-1\tx\nI:11\t0\t\n").decode().splitlines()
    assert got == ["peak:ctg:I:1:1\tI:11\t1\t1\t\t11\t0\t\t11\t0.5\t-1",
                   "peak:ctg:I:1:2\tn.I:21-24\t4\t0.5\t-1\t11\t0.5\t\t977\t0\t-1"]


def test_synthetic_input_carries_its_cases():
    """so that the GPU test cannot pass vacuously"""
    ctgs = pt.synth_ctgs()
    data = pt.synth_data(pt.synth_lines(ctgs))
    assert b"\r\n" in data and not data.endswith(b"\n")
    located, kept = pt.buckets(ctgs, data)
    by_id = {c["id"]: i for i, c in enumerate(ctgs)}
    assert located[by_id[pt.ONE_LINE]] == 1 and located[by_id[pt.TWO_LINES]] == 2
    assert max(len(b) for b in kept) > 256
    ties = sum(1 for b in kept for p, q in zip(b, b[1:]) if p[0] == q[0] and p[1] != q[1])
    assert ties >= 1
    # ties keep file order: the line numbers rise inside a run of equal starts
    assert all(p[4] < q[4] for b in kept for p, q in zip(b, b[1:]) if p[0] == q[0])
    rows = [r.split("\t") for r in pt.model(ctgs, data).decode().split("\n")[:-1]]
    assert len(rows) == sum(len(b) for b in kept) and all(len(r) == 11 for r in rows)
    assert any(int(r[5]) < 0 for r in rows) and any(int(r[8]) < 0 for r in rows)        # overlapping peaks
    assert sum(1 for r in rows for a in (r[6], r[9]) if pt.sig_digits(a) >= 8) >= 100
    assert any("-" not in r[1].split(":")[-1] for r in rows)                             # a point range: no "-end"
    assert any(r[1].startswith("nm") for r in rows)                                      # a name. prefix is kept
    assert not any("(" in r[1] for r in rows)                                            # the strand is not
    assert {r[4] for r in rows} == {"1", "-1", "", pt.LONG_SIGNAL}
    assert any(r[0].startswith("peak:" + pt.LONG_ID + ":") for r in rows) and len(pt.LONG_ID) == 40
    assert len(pt.LONG_SIGNAL) == 40
