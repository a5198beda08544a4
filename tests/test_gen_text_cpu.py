"""`gams gen` from the bytes of a FASTA file, the parts that need no GPU: the pure-Python model of tests/gen_text.py
against the golden ctg table, the host layer's FASTA reader against the model, and the new entry points' declarations."""
import ctypes as C
import gzip
import os
import re
import subprocess

import pytest

import gen_text as gt
import helpers
from gams_amd import _lib, host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEN_ABI = ("gams_gpu_gen_text", "gams_gen_counts", "gams_gen_chrs", "gams_gen_ctgs", "gams_gen_seqset", "gams_gen_destroy",
           "gams_seqset_download")


@pytest.fixture(scope="module")
def genome():
    with gzip.open(os.path.join(helpers.S288C, "genome.fa.gz"), "rb") as fh:
        return fh.read()


def test_model_reproduces_the_golden_ctg_table(genome):
    ctgs, chr_len = gt.model(genome, piece=100000)
    assert [c["id"] for c in ctgs] == ["ctg:I:1", "ctg:I:2", "ctg:Mito:1"]
    assert [c["range"] for c in ctgs] == ["I:1-100000", "I:100001-230218", "Mito:1-85779"]
    assert chr_len == {"I": 230218, "Mito": 85779}
    want = open(os.path.join(helpers.S288C, "ctg.tsv")).read().splitlines()
    rows = ["\t".join(str(c[k]) for k in ("id", "range", "chr_id", "chr_start", "chr_end")) + "\t+\t" + str(c["length"]) for c in ctgs]
    assert sorted(rows) == sorted(want[1:])
    assert gt.refusal(genome) is None
    # the model's reader is the pinned one on the golden file
    assert dict(gt.records(genome)) == helpers.load_s288c()


def test_model_refusals():
    assert gt.refusal(b"") is None and gt.model(b"") == ([], {})
    assert gt.refusal(b"ACGT\n") == "EINVAL"
    assert gt.refusal(b">a\nAC\x80GT\n") == "EUNSUPPORTED" and gt.refusal(b">a\x00\nACGT\n") == "EUNSUPPORTED"
    for case in gt.refused_cases():
        assert gt.refusal(case.data) == "EUNSUPPORTED", case.name
    for case in gt.battery():
        assert gt.refusal(case.data) is None, case.name


@pytest.mark.parametrize("case", gt.battery() + gt.refused_cases(), ids=lambda c: c.name)
def test_read_fasta_equals_the_model(case):
    assert host.read_fasta(case.data) == gt.records(case.data)


def test_read_fasta_on_the_golden_genome_and_at_the_ends(genome):
    assert host.read_fasta(genome) == gt.records(genome)
    assert host.read_fasta(b"") == []
    assert host.read_fasta(b">only") == [("only", b"")]
    assert host.read_fasta(b">a b\tc\nAC GT \n\n") == [("a", b"AC GT")]
    with pytest.raises(host.HostError) as err:
        host.read_fasta(b"ACGT\n>a\nAC\n")
    assert err.value.code == _lib.EINVAL


def test_new_entries_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "gams_gpu.h")).read()
    lib = C.CDLL(_lib.SO_PATH)
    for name in GEN_ABI:
        assert re.search(r"\b(int|void)\s+" + name + r"\s*\(", hdr), name
        assert name in _lib.PROTOTYPES, name
        assert hasattr(lib, name), name
    hl = host.load()
    for name in ("gams_host_read_fasta", "gams_host_gen_text"):
        assert hasattr(hl, name), name
    assert C.sizeof(_lib.GenParams) == 12 and _lib.GEN_CTG_DTYPE.itemsize == 16


def test_header_with_the_gen_types_compiles_as_c(tmp_path):
    src = tmp_path / "gen_abi.c"
    src.write_text(
        '#include "gams_gpu.h"\n'
        "int main(void) {\n"
        "    gams_gen_params_t p = {500000, 50, 5000};\n"
        "    gams_gen_ctg_t c = {0u, 1u, 1, 100};\n"
        "    gams_gen_t *g = 0;\n"
        "    /* no handle: the call must fail cleanly */\n"
        "    int rc = gams_gpu_gen_text(0, \">a\\nACGT\\n\", 8, &p, &g);\n"
        "    gams_gen_destroy(0, g);\n"
        "    return rc == GAMS_EINVAL && sizeof p == 12 && sizeof c == 16 ? 0 : 1;\n"
        "}\n")
    exe = tmp_path / "gen_abi"
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                           "-o", str(exe), "-L", os.path.join(ROOT, "gams_amd"), "-lgams_gpu",
                           "-Wl,-rpath," + os.path.join(ROOT, "gams_amd")])
    assert subprocess.call([str(exe)]) == 0
