"""CPU checks of `sw --action` (gc, count, gibbs): the names map to the GAMS_SW_* mask, the header defines the two
flags, and the library, the host layer and the binding carry the new entries."""
import ctypes as C
import os
import re

import pytest

from gams_amd import _lib, host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GPU_SW = ("gams_gpu_sw_text_actions", "gams_gpu_sw_count_batch")
HOST_SW = ("gams_host_sw_actions", "gams_host_sw_multi_actions", "gams_host_sw_multi_actions_timed",
           "gams_host_last_sw_index_ms")


def test_action_names_map_to_the_mask():
    assert host.sw_actions(("gc",)) == 1
    assert host.sw_actions("gc") == 1
    assert host.sw_actions(("count",)) == 2
    assert host.sw_actions(("gc", "count")) == 3
    assert host.sw_actions(["count", "gc", "count"]) == 3          # ArgAction::Append into a set (sw.rs:116-119)
    assert host.sw_actions(("gibbs",)) == 0                        # declared upstream, computes nothing
    assert host.sw_actions(("gibbs", "count")) == 2
    assert host.sw_actions(()) == 0


@pytest.mark.parametrize("bad", [("GC",), ("gc", "peak"), ("counts",), ("",)])
def test_unknown_action_names_are_rejected(bad):
    with pytest.raises(ValueError):
        host.sw_actions(bad)


def test_header_defines_the_action_flags():
    src = open(os.path.join(ROOT, "include", "gams_gpu.h")).read()
    flags = dict(re.findall(r"#define\s+(GAMS_SW_[A-Z]+)\s+(\d+)u", src))
    assert flags == {"GAMS_SW_GC": "1", "GAMS_SW_COUNT": "2"}
    assert (_lib.SW_GC, _lib.SW_COUNT) == (1, 2)


def test_library_exports_sw_action_entries():
    lib = C.CDLL(_lib.SO_PATH)
    for name in GPU_SW:
        assert hasattr(lib, name), name
        assert name in _lib.PROTOTYPES, name


def test_host_layer_exports_sw_action_operators():
    lib = C.CDLL(host.SO_PATH)
    for name in HOST_SW:
        assert hasattr(lib, name), name
    host.load()                                                    # argtypes bind


def test_sw_action_entries_fail_loudly_without_a_device():
    lib = _lib.load()
    h = C.c_void_p()
    if lib.gams_gpu_create(0, C.byref(h)) == 0:
        lib.gams_gpu_destroy(h)
        pytest.skip("a GPU is present")
    txt, nb, off, rows = C.c_void_p(), C.c_uint64(), C.c_void_p(), C.c_uint64()
    assert lib.gams_gpu_sw_text_actions(None, None, 0, None, None, None, None, None, None, None, 100, 20, 500, 3, None,
                                        None, C.byref(txt), C.byref(nb), C.byref(off), C.byref(rows)) == _lib.EINVAL
    assert lib.gams_gpu_sw_count_batch(None, None, 0, None, None, None, None, None, 100, 20, None, None, None, 0, None,
                                       C.byref(rows)) == _lib.EINVAL
