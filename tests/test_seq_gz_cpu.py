"""The `seq:` values as literal-only gzip members, on the CPU: the length-limited code builder (gams_deflate_lengths) and
the host twin of the device entry (gams_seq_gz_host, host.encode_gz_fast).  Every member must inflate to its input under
zlib, Python's gzip and the project's own reader; its CRC-32 and ISIZE fields are checked against zlib."""
import ctypes as C
import gzip
import struct
import zlib

import numpy as np
import pytest

import helpers
from gams_amd import _lib, host

L = _lib.load()
B = _lib.SEQ_GZ_BLOCK


def lengths(freq, limit):
    f = np.asarray(freq, np.uint32)
    out = np.full(f.size, 255, np.uint8)
    rc = L.gams_deflate_lengths(f.ctypes.data, f.size, limit, out.ctypes.data)
    return rc, out


def check_code(freq, limit):
    """the properties of a result: unused symbols 0, used ones within 1..limit, complete or single-symbol"""
    rc, ln = lengths(freq, limit)
    assert rc == _lib.OK
    f = np.asarray(freq)
    used = f != 0
    assert np.all(ln[~used] == 0)
    assert np.all((ln[used] >= 1) & (ln[used] <= limit))
    if used.sum() == 1:
        assert ln[used][0] == 1
    elif used.sum() > 1:
        assert int(np.sum(1 << (limit - ln[used].astype(np.int64)))) == 1 << limit      # Kraft sum exactly 1
    return ln


def fib(n):
    f = [1, 1]
    while len(f) < n:
        f.append(f[-1] + f[-2])
    return f[:n]


def huffman_depth(freq):
    """the deepest leaf of an unrestricted Huffman tree (any tie order gives the same depth for Fibonacci weights)"""
    import heapq
    h = [(f, 0) for f in freq if f]
    heapq.heapify(h)
    while len(h) > 1:
        a, b = heapq.heappop(h), heapq.heappop(h)
        heapq.heappush(h, (a[0] + b[0], max(a[1], b[1]) + 1))
    return h[0][1]


@pytest.mark.parametrize("limit,n", [(15, 17), (15, 18), (15, 30), (15, 40), (7, 9), (7, 10), (7, 19)])
def test_fibonacci_histograms_are_limited(limit, n):
    f = fib(n)
    assert huffman_depth(f) > limit            # the unrestricted tree is too deep: the limiter has to act
    ln = check_code(f, limit)
    assert ln.max() == limit
    # a rarer symbol never has a shorter code
    order = np.argsort(np.asarray(f), kind="stable")
    assert np.all(np.diff(ln[order].astype(int)) <= 0)
    check_code(f[::-1], limit)
    check_code([0, 0] + f + [0], limit)


def test_small_and_flat_histograms():
    for limit in (15, 7):
        for n in (2, 3, 4, 5, 16, 19):
            ln = check_code([7] * n, limit)
            assert ln.max() - ln.min() <= 1            # all equal: a balanced code
        assert list(check_code([0, 5, 0], limit)) == [0, 1, 0]
        assert list(check_code([3, 0, 9], limit)) == [1, 0, 1]
        assert list(check_code([0, 0, 0], limit)) == [0, 0, 0]
    ln = check_code([1] * 257, 15)
    assert sorted(set(ln.tolist())) == [8, 9]
    check_code([1] * 128, 7)
    assert lengths([1] * 129, 7)[0] == _lib.EINVAL     # more symbols than 2^7 codes
    assert lengths([1, 1], 0)[0] == _lib.EINVAL and lengths([1, 1], 16)[0] == _lib.EINVAL
    assert lengths([1] * 289, 15)[0] == _lib.EINVAL


def test_seeded_skewed_histograms():
    rng = np.random.default_rng(20240611)
    for k in range(3000):
        limit = 15 if k % 2 else 7
        n = int(rng.integers(1, 258 if limit == 15 else 20))
        # skewed: powers of a random base, some bins emptied, values up to 2^32 - 1
        base = rng.uniform(1.0, 2.2)
        f = np.minimum(np.floor(base ** rng.uniform(0, 30, n)), 2 ** 32 - 1).astype(np.uint64)
        f[rng.random(n) < 0.2] = 0
        ln = check_code(f.astype(np.uint32), limit)
        assert np.array_equal(ln, lengths(f.astype(np.uint32), limit)[1])      # a function of the histogram alone


def test_unlimited_case_is_huffman_optimal():
    import heapq
    rng = np.random.default_rng(7)
    for _ in range(300):
        f = rng.integers(1, 1000, int(rng.integers(2, 40)))
        h = list(map(int, f))
        heapq.heapify(h)
        cost = 0
        while len(h) > 1:
            a, b = heapq.heappop(h), heapq.heappop(h)
            cost += a + b
            heapq.heappush(h, a + b)
        ln = check_code(f, 15)
        if huffman_depth(f) <= 15:
            assert int(np.sum(f * ln)) == cost


# ---- members

def member(data, block=None):
    a = np.frombuffer(bytes(data), np.uint8)
    n = C.c_uint64()
    p = a.ctypes.data if a.size else None
    call = ((lambda o, c: L.gams_seq_gz_host(p, a.size, o, c, C.byref(n))) if block is None else
            (lambda o, c: L.gams_seq_gz_host_block(p, a.size, block, o, c, C.byref(n))))
    assert call(None, 0) == _lib.OK                    # cap = 0 sizes
    size = n.value
    out = np.full(size + 8, 0xAB, np.uint8)
    assert call(out.ctypes.data, size) == _lib.OK and n.value == size
    assert np.all(out[size:] == 0xAB)                  # nothing behind the member
    if size > 1:
        assert call(out.ctypes.data, size - 1) == _lib.EINVAL and n.value == size
    return out[:size].tobytes()


def check_member(data, block=None):
    data = bytes(data)
    m = member(data, block)
    assert m[:10] == bytes([0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 0, 0xff])
    crc, isize = struct.unpack("<II", m[-8:])
    assert crc == zlib.crc32(data) and isize == len(data) % 2 ** 32
    assert zlib.decompress(m, 31) == data
    assert gzip.decompress(m) == data
    assert host.decode_gz(m) == data
    if block is None:
        assert host.encode_gz_fast(data) == m
    return m


def masked_dna(n, seed):
    """soft-masked ACGT with runs of N"""
    s = helpers.synth(n, seed, lower=0.0, nrate=0.0)
    rng = np.random.default_rng(seed + 1)
    at = 0
    while at < n:                                      # alternating stretches: upper, lower, now and then N
        run = int(rng.integers(1, 3000))
        kind = rng.random()
        if kind < 0.3:
            s[at:at + run] |= 0x20
        elif kind < 0.4:
            s[at:at + run] = ord("N")
        at += run
    return s.tobytes()


@pytest.mark.parametrize("n", [0, 1, 2, B - 1, B, B + 1, 2 * B + 1])
def test_members_of_masked_dna(n):
    m = check_member(masked_dna(n, 100 + n % 97))
    if n == 0:
        assert len(m) == 30 and m == member(b"")       # the fixed empty member
    # nine byte values and end-of-block fit a 4-bit code, and a Huffman code is no longer than that one
    assert len(m) <= n // 2 + 100 * (n // B + 1)


def test_members_of_other_bytes():
    check_member(b"G" * 1000)
    check_member(b"\x00" * (B + 5))
    check_member(bytes(range(256)))
    check_member(bytes(range(256)) * 300)
    f = fib(17)                                        # 4,180 bytes: seventeen symbols and end-of-block, a tree too deep for 15 bits
    block = b"".join(bytes([i * 3]) * c for i, c in enumerate(f))
    assert len(block) == 4180
    check_member(block)
    check_member(np.random.default_rng(5).integers(0, 256, 3 * B + 77, dtype=np.uint8).tobytes())
    # every block has a code of its own: a byte that only the second block holds
    check_member(b"A" * B + b"\xff" * 10)


def test_block_sizes_agree_with_the_default_and_decode():
    data = masked_dna(3 * B + 123, 9)
    assert member(data, B) == member(data)
    for block in (4096, 8192, 65536):
        check_member(data, block)
    n = C.c_uint64()
    for bad in (0, 100, 4097, 2 ** 24 + 4096):
        assert L.gams_seq_gz_host_block(None, 0, bad, None, 0, C.byref(n)) == _lib.EINVAL


def test_smaller_than_the_reference_encoder_on_the_golden_genome():
    """the sum of the members over the golden genome's ctgs at piece 100,000 against flate2's Compression::fast() =
    zlib level 1 (host.encode_gz): a condition, not a tuning target"""
    ours = ref = 0
    for chr_id, seq in helpers.load_s288c().items():
        for c in helpers.gen_ctgs(chr_id, seq, piece=100000):
            ours += len(check_member(c["seq"]))
            ref += len(host.encode_gz(c["seq"]))
    assert ours <= ref, (ours, ref)
