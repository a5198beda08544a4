"""The indexed `seq:` members on the CPU: the host twin of the indexed writer (gams_seq_gz_host_indexed*), the layout of
its FEXTRA subfield, and the host twin of the device inflater (gams_seq_gunzip_host), which runs the decoder core the
kernels share.  Whatever is not an intact indexed member must come back FOREIGN, never as an error or a wrong answer;
the same core runs over the same members in a stand-alone program built with the address and undefined-behaviour
sanitizers."""
import gzip
import os
import shutil
import struct
import subprocess
import zlib

import numpy as np
import pytest

import seq_gz_index as gi
from gams_amd import _lib, host
from seq_gz_index import B, CHUNK, HEAD, L, damaged, gunzip_host, imember, parse_index, strip_index
from test_seq_gz_cpu import masked_dna, member

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DONE, FOREIGN = _lib.SEQ_GZ_DONE, _lib.SEQ_GZ_FOREIGN
BLOCKS = (4096, 32768)


@pytest.fixture(scope="module")
def corpus():
    """{block: [(name, input, indexed member)]}, made once"""
    return {blk: [(name, data, imember(data, blk)) for name, data in gi.case_inputs(blk)] for blk in BLOCKS}


def test_constants_agree():
    assert CHUNK in (1024, 2048, 4096) and 4096 % CHUNK == 0 and CHUNK % 16 == 0
    assert _lib.SEQ_GZ_INDEXED == 0x100 and (DONE, FOREIGN) == (0, 1)
    hdr = open(os.path.join(ROOT, "include", "gams_gpu.h")).read()
    assert "#define GAMS_SEQ_GZ_CHUNK %du" % CHUNK in hdr and "#define GAMS_SEQ_GZ_INDEXED 0x100" in hdr


@pytest.mark.parametrize("block", BLOCKS)
def test_members_inflate_and_carry_the_specified_subfield(corpus, block):
    for name, data, m in corpus[block]:
        assert gzip.decompress(m) == data, name
        d = zlib.decompressobj(31)
        assert d.decompress(m) + d.flush() == data and d.eof and d.unused_data == b"", name
        assert m[:10] == HEAD and m[3] == 4
        blk, chunk, ent, body = parse_index(m)
        assert (blk, chunk) == (block, CHUNK) and len(ent) == -(-len(data) // CHUNK), name
        assert struct.unpack("<H", m[14:16])[0] == 8 + 4 * len(ent)
        assert strip_index(m) == member(data, block), name          # body and trailer are the plain twin's, bit for bit
        assert all(a < b for a, b in zip(ent, ent[1:])) and (not ent or ent[0] == 0), name
        assert all(e < 8 * (len(m) - 8 - body) for e in ent)
    assert len(corpus[block][0][2]) == 30 + 14                      # the empty member: no entries


@pytest.mark.parametrize("block", BLOCKS)
def test_every_entry_starts_its_chunk(corpus, block):
    """a literal-only bit decoder in Python, started at each entry on its own"""
    for name, data, m in corpus[block]:
        assert gi.decode_by_entries(m) == data, name


@pytest.mark.parametrize("block", BLOCKS)
def test_host_twin_of_the_inflater_returns_the_input(corpus, block):
    for name, data, m in corpus[block]:
        assert gunzip_host(m) == (_lib.OK, DONE, data, len(data)), name
        if data:
            rc, st, _, n = gunzip_host(m, cap=len(data) - 1)        # too little room: said, nothing written behind it
            assert rc == _lib.EINVAL and n == len(data)


def test_other_chunks_and_the_default_entries():
    data = masked_dna(3 * B + 123, 9)
    assert imember(data) == imember(data, B) == imember(data, B, CHUNK)
    a = np.frombuffer(data, np.uint8)
    assert host.encode_gz_fast(data, indexed=True) == imember(data) and host.encode_gz_fast(data) == member(data)
    assert host.decode_gz_indexed(imember(data)) == data
    for chunk in (512, 1024, 2048, 4096):
        for block in (4096, 8192, 65536):
            m = imember(data, block, chunk)
            assert parse_index(m)[:2] == (block, chunk) and strip_index(m) == member(data, block)
            assert gunzip_host(m)[:3] == (_lib.OK, DONE, data)
    n = gi.C.c_uint64()
    for chunk in (0, 16, 256, 8192, 3000):
        assert L.gams_seq_gz_host_indexed_chunk(a.ctypes.data, a.size, B, chunk, None, 0, gi.C.byref(n)) == _lib.EINVAL
    # a block the decoder refuses and says so; any gzip reader still inflates the member
    m = imember(data, 131072)
    assert gzip.decompress(m) == data and gunzip_host(m)[1] == FOREIGN


def test_an_index_that_would_not_fit_is_left_out():
    """more than 16,380 chunks: the plain member, from the indexed writer, at chunk 512 to keep the input small"""
    data = masked_dna(16380 * 512 + 1, 3)
    assert imember(data, B, 512) == member(data)
    m = imember(data[:-1], B, 512)
    assert m[3] == 4 and len(parse_index(m)[2]) == 16380 and struct.unpack("<H", m[10:12])[0] == 65532


@pytest.fixture(scope="module")
def three_blocks():
    data = masked_dna(2 * B + 5000, 21)
    m, bad = damaged(data)
    return data, m, bad


def test_everything_else_is_foreign(three_blocks):
    data, m, bad = three_blocks
    assert gunzip_host(m)[:3] == (_lib.OK, DONE, data)
    for name, v in bad:
        rc, st, out, n = gunzip_host(v)
        assert (rc, st) == (_lib.OK, FOREIGN), name
    for v in (b"", b"\x1f", m[:33], m[:-1], m + b"\0", HEAD + b"\xff" * 40):
        assert gunzip_host(v)[:2] == (_lib.OK, FOREIGN)
    with pytest.raises(RuntimeError):
        host.decode_gz_indexed(bad[0][1])


def flips_of(m, count, seed):
    rng = np.random.default_rng(seed)
    body = parse_index(m)[3]
    # the header and the subfield whole, and seeded positions over the body and the trailer
    return list(range(8 * 40)) + sorted(set(int(x) for x in rng.integers(8 * 40, 8 * len(m), count)))


def zlib_of(v):
    try:
        d = zlib.decompressobj(31)
        out = d.decompress(v) + d.flush()
        return out if d.eof else None
    except zlib.error:
        return None


def flipped(m, bit):
    v = bytearray(m)
    v[bit >> 3] ^= 1 << (bit & 7)
    return bytes(v)


@pytest.fixture(scope="module")
def sweep(three_blocks):
    """the one seeded sweep over the 3-block member: [(bit, what gunzip_host says of the member with that bit flipped)],
    shared by the test below and the sanitizer program"""
    m = three_blocks[1]
    return [(bit, gunzip_host(flipped(m, bit))) for bit in flips_of(m, 1500, 99)]


def test_single_bit_flips_are_foreign_or_what_zlib_gives(three_blocks, sweep):
    data, m, _ = three_blocks
    done = 0
    for bit, (rc, st, out, n) in sweep:
        assert rc == _lib.OK and st in (DONE, FOREIGN), bit
        if st == DONE:
            done += 1
            assert out == zlib_of(flipped(m, bit)), bit
    assert done < 10                                                # (nearly every bit of a member matters)


def san_binary(tmp_path):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no g++ here")
    flags = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    # the sanitizer runtimes, probed with a program that has nothing else to fail on
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    p = subprocess.run([cxx] + flags + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    if p.returncode != 0 or subprocess.run([str(tmp_path / "probe")]).returncode != 0:
        pytest.skip("this g++ has no usable sanitizer runtime: " + (p.stderr.strip().splitlines() or ["the probe does not run"])[-1])
    exe = tmp_path / "seq_gunzip_san"
    p = subprocess.run([cxx] + flags + [os.path.join(ROOT, "tests", "seq_gunzip_san.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    return exe


def fnv1a(data):
    h = 1469598103934665603
    for b in data:
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def test_decoder_core_is_clean_under_the_sanitizers(tmp_path, corpus, three_blocks, sweep):
    """the stand-alone program (its own main, no Python in the process) over the corpus, the damaged members and the
    same sweep: it exits clean and answers what the library answered -- status, number of bases, and for DONE the hash
    of the bases"""
    exe = san_binary(tmp_path)
    data, m, bad = three_blocks
    members = [m] + [v for _, v in bad] + [mm for blk in BLOCKS for _, _, mm in corpus[blk]]
    flips = [bit for bit, _ in sweep]
    (tmp_path / "corpus.bin").write_bytes(b"".join(struct.pack("<Q", len(v)) + v for v in members))
    (tmp_path / "flips.bin").write_bytes(struct.pack("<%dQ" % len(flips), *flips))
    p = subprocess.run([str(exe), str(tmp_path / "corpus.bin"), "0", str(tmp_path / "flips.bin")], capture_output=True, text=True)
    assert p.returncode == 0 and p.stderr == "", p.stderr[-2000:]
    lines = [ln.split() for ln in p.stdout.splitlines()]
    assert len(lines) == len(members) + len(flips)
    answers = [gunzip_host(v) for v in members] + [r for _, r in sweep]
    assert sum(1 for r in answers if r[1] == DONE) >= len(members) - len(bad)
    for ln, (rc, st, out, n) in zip(lines, answers):
        assert (int(ln[0]), int(ln[1])) == (st, n)
        assert int(ln[2], 16) == (fnv1a(out) if st == DONE else 0)
