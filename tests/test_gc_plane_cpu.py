"""CPU-only: both bodies of the host G/C classifier (gams_gc_plane, gams_amd/csrc/gc_plane.cpp) against the
definition written in numpy -- bit i & 7 of plane[i >> 3] is (seq[i] & 0xDB) == 0x43, bits past n are zero."""
import numpy as np
import pytest

from gams_amd import _lib


def plane_ref(seq):
    bits = ((seq & 0xDB) == 0x43).astype(np.uint8)
    return np.packbits(bits, bitorder="little")          # pads the last byte with zero bits


def classify(seq_buf, start, n, body):
    """run one body over seq_buf[start : start + n] (any source address); returns the plane bytes and the guard
    bytes behind them"""
    lib = _lib.load()
    nb = (n + 7) // 8
    out = np.full(nb + 16, 0xA5, dtype=np.uint8)
    assert seq_buf.dtype == np.uint8 and seq_buf.flags.c_contiguous and start + n <= seq_buf.size
    rc = lib.gams_gc_plane_with(seq_buf.ctypes.data + start, n, out.ctypes.data, body)
    if rc == _lib.EUNSUPPORTED:
        pytest.skip("this CPU has no AVX2")
    assert rc == _lib.OK
    assert (out[nb:] == 0xA5).all(), "wrote past ceil(n/8) bytes"
    return out[:nb]


BODIES = [pytest.param(_lib.GC_BODY_PORTABLE, id="portable"), pytest.param(_lib.GC_BODY_AVX2, id="avx2"),
          pytest.param(_lib.GC_BODY_AUTO, id="auto")]


@pytest.mark.parametrize("body", BODIES)
def test_every_byte_value_at_every_offset(body):
    # value v at offset k of a run of 96 + 40 bases that otherwise holds no G/C ('A'), then of one that holds
    # only G/C ('G'): the one bit that differs from the background must be bit k, for every v and k
    for fill in (ord("A"), ord("G")):
        for k in range(96):
            buf = np.full((256, 136), fill, dtype=np.uint8)
            buf[np.arange(256), k] = np.arange(256, dtype=np.uint8)
            flat = np.ascontiguousarray(buf.reshape(-1))                 # rows of 136 = 17 plane bytes each
            got = classify(flat, 0, flat.size, body)
            assert np.array_equal(got, plane_ref(flat)), (fill, k)
    # and alone in a run of 96 bases, at offset k from the run's first base
    lib = _lib.load()
    gc = {0x43, 0x47, 0x63, 0x67}
    buf = np.zeros(96, dtype=np.uint8)
    out = np.zeros(12, dtype=np.uint8)
    for k in range(96):
        for v in range(256):
            buf[k] = v
            assert lib.gams_gc_plane_with(buf.ctypes.data, 96, out.ctypes.data, body) == _lib.OK
            want = np.zeros(12, dtype=np.uint8)
            if v in gc:
                want[k >> 3] = 1 << (k & 7)
            assert out.tobytes() == want.tobytes(), (k, v)
        buf[k] = 0


@pytest.mark.parametrize("body", BODIES)
def test_lengths_and_misaligned_sources(body):
    rng = np.random.default_rng(7)
    raw = rng.integers(0, 256, size=4097 + 64, dtype=np.uint8)
    text = np.frombuffer(b"ACGTNacgtn", dtype=np.uint8)[rng.integers(0, 10, size=4097 + 64)]
    lengths = list(range(0, 131)) + [255, 256, 257, 4095, 4096, 4097]
    for buf in (raw, np.ascontiguousarray(text)):
        for n in lengths:
            for start in (0, 1, 3, 7, 13, 31, 33):
                got = classify(buf, start, n, body)
                want = plane_ref(buf[start:start + n])
                assert np.array_equal(got, want), (n, start)
                if n & 7:                                               # bits past n are zero
                    assert got[-1] >> (n & 7) == 0, (n, start)


def test_default_entry_is_the_same_function():
    lib = _lib.load()
    rng = np.random.default_rng(11)
    seq = rng.integers(0, 256, size=1000, dtype=np.uint8)
    out = np.zeros(125, dtype=np.uint8)
    assert lib.gams_gc_plane(seq.ctypes.data, seq.size, out.ctypes.data) == _lib.OK
    assert np.array_equal(out, plane_ref(seq))
    assert lib.gams_gc_plane(None, 8, out.ctypes.data) == _lib.EINVAL
    assert lib.gams_gc_plane_with(seq.ctypes.data, 8, out.ctypes.data, 9) == _lib.EINVAL
