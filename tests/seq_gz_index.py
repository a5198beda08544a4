"""Shared by the tests of the indexed `seq:` members (test_seq_gz_index_cpu.py, test_gpu_seq_gunzip.py): the host twins
through ctypes, the subfield parsed in Python, a literal-only bit decoder, the input cases and the damaged members."""
import ctypes as C
import gzip
import struct

import numpy as np

from gams_amd import _lib
from test_seq_gz_cpu import fib, masked_dna, member

L = _lib.load()
B = _lib.SEQ_GZ_BLOCK
CHUNK = _lib.SEQ_GZ_CHUNK
HEAD = bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff])


def imember(data, block=B, chunk=None):
    """gams_seq_gz_host_indexed_block (chunk None) / _indexed_chunk: sized, written, nothing behind it"""
    a = np.frombuffer(bytes(data), np.uint8)
    n = C.c_uint64()
    p = a.ctypes.data if a.size else None
    call = ((lambda o, c: L.gams_seq_gz_host_indexed_block(p, a.size, block, o, c, C.byref(n))) if chunk is None else
            (lambda o, c: L.gams_seq_gz_host_indexed_chunk(p, a.size, block, chunk, o, c, C.byref(n))))
    assert call(None, 0) == _lib.OK
    size = n.value
    out = np.full(size + 8, 0xAB, np.uint8)
    assert call(out.ctypes.data, size) == _lib.OK and n.value == size
    assert np.all(out[size:] == 0xAB)
    assert call(out.ctypes.data, size - 1) == _lib.EINVAL
    return out[:size].tobytes()


def gunzip_host(m, cap=None):
    """gams_seq_gunzip_host -> (rc, status, bases, n_out); the room is ISIZE as the last four bytes give it"""
    m = bytes(m)
    isize = struct.unpack("<I", m[-4:])[0] if len(m) >= 4 else 0
    room = min(isize, 1 << 26) if cap is None else cap
    guard = 64
    out = np.full(room + guard, 0xCD, np.uint8)
    n, st = C.c_uint64(), C.c_int(-1)
    rc = L.gams_seq_gunzip_host(m, len(m), out.ctypes.data, room, C.byref(n), C.byref(st))
    assert np.all(out[room:] == 0xCD)                       # nothing behind the room given
    return rc, st.value, out[:min(n.value, room)].tobytes(), n.value


def parse_index(m):
    """(block, chunk, entries, body offset) of an indexed member"""
    assert m[:10] == HEAD
    xlen, = struct.unpack("<H", m[10:12])
    assert m[12:14] == b"GI"
    ln, = struct.unpack("<H", m[14:16])
    assert ln == xlen - 4 and (ln - 8) % 4 == 0
    block, chunk = struct.unpack("<II", m[16:24])
    ent = list(struct.unpack("<%dI" % ((ln - 8) // 4), m[24:24 + ln - 8]))
    return block, chunk, ent, 12 + xlen


def strip_index(m):
    xlen, = struct.unpack("<H", m[10:12])
    return m[:3] + b"\0" + m[4:10] + m[12 + xlen:]


class Bits:
    def __init__(self, data, at):
        self.d, self.at = data, at

    def take(self, n):
        v = 0
        for k in range(n):
            v |= ((self.d[(self.at + k) >> 3] >> ((self.at + k) & 7)) & 1) << k
        self.at += n
        return v


def canon(lengths):
    """{(length, code): symbol} of a canonical code"""
    code, out = 0, {}
    for ln in range(1, 16):
        for s, l in enumerate(lengths):
            if l == ln:
                out[(ln, code)] = s
                code += 1
        code <<= 1
    return out


def read_sym(bits, table):
    code = 0
    for ln in range(1, 16):
        code = (code << 1) | bits.take(1)
        if (ln, code) in table:
            return table[(ln, code)]
    raise AssertionError("no code")


def read_header(bits):
    """a dynamic-Huffman block header -> (bfinal, literal table)"""
    final = bits.take(1)
    assert bits.take(2) == 2
    hlit, hdist, hclen = bits.take(5) + 257, bits.take(5) + 1, bits.take(4) + 4
    assert (hlit, hdist) == (257, 1)
    order = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
    cl = [0] * 19
    for k in range(hclen):
        cl[order[k]] = bits.take(3)
    ct = canon(cl)
    lens = []
    while len(lens) < 258:
        s = read_sym(bits, ct)
        if s < 16:
            lens.append(s)
        elif s == 16:
            lens += [lens[-1]] * (3 + bits.take(2))
        elif s == 17:
            lens += [0] * (3 + bits.take(3))
        else:
            lens += [0] * (11 + bits.take(7))
    assert len(lens) == 258 and lens[257] == 0
    return final, canon(lens[:257])


def decode_by_entries(m):
    """every chunk decoded on its own from its entry: the bases, chunk by chunk"""
    block, chunk, ent, body = parse_index(m)
    isize, = struct.unpack("<I", m[-4:])
    data = m[body:]
    out, table = [], None
    for j, e in enumerate(ent):
        bits = Bits(data, e)
        if j * chunk % block == 0:
            final, table = read_header(bits)
            assert bool(final) == (j * chunk + block >= isize)
        # (elsewhere the literal code is the block's, read at the block's entry)
        n = min(chunk, isize - j * chunk)
        got = bytes(read_sym(bits, table) for _ in range(n))
        out.append(got)
        last_in_block = (j + 1) * chunk % block == 0 or j + 1 == len(ent)
        if last_in_block:
            assert read_sym(bits, table) == 256
        if j + 1 < len(ent):
            assert bits.at == ent[j + 1]
    return b"".join(out)


def case_inputs(block, chunk=CHUNK):
    """the inputs of the issue's list, as (name, bytes)"""
    f = fib(17)
    lens = [0, 1, 2, 15, 16, 17, chunk - 1, chunk, chunk + 1, 4095, 4096, 4097, 2 * 4096 + 1, block - 1, block, block + 1,
            2 * block + 1]
    out = [("dna%d" % n, masked_dna(n, 700 + k)) for k, n in enumerate(lens)]
    out += [("one", b"G" * 1000), ("all", bytes(range(256))), ("all300", bytes(range(256)) * 40),
            ("fib", b"".join(bytes([i * 3]) * c for i, c in enumerate(f))),
            ("random", np.random.default_rng(5).integers(0, 256, 2 * block + 77, dtype=np.uint8).tobytes())]
    return out


def set_entry(m, j, v):
    return m[:24 + 4 * j] + struct.pack("<I", v) + m[28 + 4 * j:]


def damaged(data, block=B):
    """(name, bytes) of values the device must not take, from one input of at least three blocks: foreign gzip, and an
    indexed member damaged one way each"""
    m = imember(data, block)
    blk, chunk, ent, body = parse_index(m)
    assert len(data) > 2 * block and len(ent) >= 4
    body_bits = 8 * (len(m) - 8 - body)
    flip = lambda buf, bit: buf[:bit >> 3] + bytes([buf[bit >> 3] ^ (1 << (bit & 7))]) + buf[(bit >> 3) + 1:]
    out = [("zlib1", gzip.compress(data, 1)),
           ("plain", member(data, block)),
           ("cut", m[:body + (len(m) - body) // 2]),
           ("entry+1", set_entry(m, 2, ent[2] + 1)),
           ("entry_beyond", set_entry(m, 3, body_bits + 100)),
           ("entries_swapped", set_entry(set_entry(m, 1, ent[2]), 2, ent[1])),
           ("btype1", flip(flip(m, 8 * body + 1), 8 * body + 2)),
           ("body_bit", flip(m, 8 * body + body_bits // 2 + 3)),
           ("crc", flip(m, 8 * (len(m) - 8))),
           ("xlen", m[:10] + struct.pack("<H", struct.unpack("<H", m[10:12])[0] + 4) + m[12:]),
           ("len", m[:14] + struct.pack("<H", struct.unpack("<H", m[14:16])[0] - 4) + m[16:])]
    return m, out
