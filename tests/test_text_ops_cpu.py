"""CPU checks of the text entries (locate -f / locate --count / anno over the bytes of an input file): the
library and the host layer export them, they fail loudly without a device, and the device's integer `{:.4}`
agrees with an exact decimal rendering and with the host operator's "%.4f"."""
import ctypes as C
from decimal import ROUND_HALF_EVEN, Decimal

import numpy as np
import pytest

from gams_amd import _lib, host

GPU_TEXT = ("gams_names_create", "gams_names_destroy", "gams_gpu_locate_text", "gams_gpu_count_text",
            "gams_gpu_anno_text")
HOST_TEXT = ("gams_host_locate_text", "gams_host_anno_text", "gams_host_last_operator_device")


def fmt4_exact(p):
    """anno.rs:140 `{:.4}` of the f32 p: its exact binary value rounded half to even at four places."""
    return str(Decimal(float(np.float32(p))).quantize(Decimal("0.0001"), rounding=ROUND_HALF_EVEN))


def test_library_exports_text_entries():
    lib = C.CDLL(_lib.SO_PATH)
    for name in GPU_TEXT:
        assert hasattr(lib, name), name
        assert name in _lib.PROTOTYPES, name


def test_host_layer_exports_text_operators():
    lib = C.CDLL(host.SO_PATH)
    for name in HOST_TEXT:
        assert hasattr(lib, name), name


class _NoDevice:
    h = None


def test_text_entries_fail_loudly_without_a_device():
    lib = _lib.load()
    h = C.c_void_p()
    if lib.gams_gpu_create(0, C.byref(h)) == 0:
        lib.gams_gpu_destroy(h)
        pytest.skip("a GPU is present")
    nm = C.c_void_p()
    names = (C.c_char_p * 1)(b"I")
    assert lib.gams_names_create(None, 1, names, C.byref(nm)) == _lib.EINVAL
    text, nb, rows = C.c_void_p(), C.c_uint64(), C.c_uint64()
    data = b"I:1-10\n"
    assert lib.gams_gpu_locate_text(None, None, None, None, data, len(data), C.byref(text), C.byref(nb),
                                    C.byref(rows)) == _lib.EINVAL
    assert lib.gams_gpu_count_text(None, None, None, None, None, data, len(data), C.byref(text), C.byref(nb),
                                   C.byref(rows)) == _lib.EINVAL
    assert lib.gams_gpu_anno_text(None, None, None, None, None, None, data, len(data), 0, b"", 1, 2, C.byref(text),
                                  C.byref(nb), C.byref(rows)) == _lib.EINVAL
    ctgs = [dict(id="ctg:I:1", chr_id="I", chr_start=1, chr_end=1000, seq=b"")]
    with pytest.raises(host.HostError):
        host.locate_text(_NoDevice(), ctgs, data)
    with pytest.raises(host.HostError):
        host.locate_text(_NoDevice(), ctgs, data, count=True, rg_records=[("ctg:I:1", "I:5-8")])
    with pytest.raises(host.HostError):
        host.anno_text(_NoDevice(), ctgs, {"I": "1-100"}, b"ctg:I:1\tI:1-10\n")


def test_prop4_formatter_is_exact():
    """Every a/b with b <= 300: the integer formatter (the device's, csrc/text_fmt.hpp), Decimal's exact rounding and
    the host operator's "%.4f" of the widened f32 print the same six bytes."""
    libc = C.CDLL(None)
    buf = C.create_string_buffer(32)
    for b in range(1, 301):
        props = np.arange(0, b + 1, dtype=np.float32) / np.float32(b)      # f32 / f32, as anno.rs:139
        for p in props:
            want = fmt4_exact(p)
            assert host.fmt_prop4(float(p)) == want, (p, b)
            libc.snprintf(buf, 32, b"%.4f", C.c_double(float(p)))
            assert buf.value.decode() == want, (p, b)


def test_prop4_formatter_edges():
    for p, want in [(0.0, "0.0000"), (1.0, "1.0000"), (4.9e-5, "0.0000"), (2.0 ** -15, "0.0000"), (1e-30, "0.0000"),
                    (5.1e-5, "0.0001"), (0.5, "0.5000")]:
        assert host.fmt_prop4(p) == want == fmt4_exact(p), p
    # next to the rounding edges: the f32 neighbours of x.xxxx5 go either way, exactly
    for x in (5e-5, 0.00015, 0.12345, 0.99995):
        f = np.float32(x)
        for p in (np.nextafter(f, np.float32(0)), f, np.nextafter(f, np.float32(1))):
            assert host.fmt_prop4(float(p)) == fmt4_exact(p), p
    for p in (float("nan"), float("inf"), -0.5, 1.0000001, 2.0):
        assert host.fmt_prop4(p) == "", p
