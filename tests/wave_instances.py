"""Every entry of the instance list of gams_amd/csrc/wave_select.hpp (WAVE_FAST_INSTANCES), with the recipe that
reaches it on a small seqset through the existing setters.  A module, not a test: test_wave_select_cpu.py holds its
names against the list itself, test_gpu_wave_select.py runs every recipe.

A new instantiation is one line in WAVE_FAST_INSTANCES and one line here."""
from collections import namedtuple

# kernel: the name gams_wave_plan_kernel_name prints on a seqset below 64 MiB (above it `false` reads `true`)
# size, step, lag: the plan's parameters; tile_windows, threads: gams_wave_plan_set_tile / _set_threads
Instance = namedtuple("Instance", "kernel size step lag tile_windows threads")


def _fast(w, size, step, lag, nth, prm):
    return Instance(f"wave_fast_kernel<{w}, {size}, {step}, {lag}, false, {nth}>", prm[0], prm[1], prm[2], 256 * w, nth)


ANY = (50, 7, 33)            # no baked form: size, step and lag are arguments
INSTANCES = (
    [_fast(w, 0, 0, 0, 256, ANY) for w in (20, 12, 8, 4)]
    # size, step and lag baked
    + [_fast(28, 100, 1, 100, nth, (100, 1, 100)) for nth in (64, 128, 256)]
    + [_fast(w, 100, 1, 100, 256, (100, 1, 100)) for w in (20, 12)]
    + [_fast(12, 100, 10, 100, nth, (100, 10, 100)) for nth in (64, 128, 256)]
    + [_fast(w, 100, 10, 100, 256, (100, 10, 100)) for w in (8, 4)]
    # size and step baked, the lag an argument
    + [_fast(w, 100, 5, 0, 256, (100, 5, 200)) for w in (4, 8, 12)]
    + [_fast(w, 100, 10, 0, 256, (100, 10, 50)) for w in (4, 8, 12)]
    + [_fast(w, 100, 20, 0, 256, (100, 20, 50)) for w in (4, 8, 12)]
    + [_fast(20, 100, 1, 0, 256, (100, 1, 200))]
    + [_fast(20, 100, 5, 0, nth, (100, 5, 200)) for nth in (64, 128, 256)]
    + [_fast(28, 100, 1, 0, nth, (100, 1, 200)) for nth in (64, 128, 256)]
)
