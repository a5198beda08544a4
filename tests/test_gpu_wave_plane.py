"""The 1-bit G/C plane of a seqset: the tiled fast wave kernels reading the plane the uploads made, and
the same plans reading the bytes, each against the CPU oracle -- peaks, counts and dense rows, bit for bit; the rule
that a pass never reads a plane that does not describe the bytes; plane-only seqsets; the host operators' goldens."""
import ctypes as C
import gzip

import numpy as np
import pytest

import helpers
from gams_amd import _lib, engine, host
from oracle import oracle as ora

pytestmark = pytest.mark.gpu

PLANE, BYTES, AUTO = _lib.WAVE_INPUT_PLANE, _lib.WAVE_INPUT_BYTES, _lib.WAVE_INPUT_AUTO
BOTH = _lib.WAVE_PEAKS | _lib.WAVE_DENSE
HEADER = "#range\tgc_content\tsignal\n"


@pytest.fixture(scope="module")
def eng():
    e = engine.Engine(0)
    yield e
    e.close()


def mixed(lengths, seed):
    """ctgs of the given lengths, alternately random bytes 0..255 and ACGTN text in both cases"""
    rng = np.random.default_rng(seed)
    text = np.frombuffer(b"ACGTNacgtn", np.uint8)
    out = []
    for k, n in enumerate(lengths):
        if k & 1:
            out.append(np.ascontiguousarray(text[rng.integers(0, 10, n)]))
        else:
            out.append(rng.integers(0, 256, n, dtype=np.uint8))
    return out


_ORACLE = {}


def oracle_of(seq, prm):
    """(counts, signals) of one ctg, computed once per (ctg bytes, parameters)"""
    key = (seq.tobytes(), prm)
    if key not in _ORACLE:
        ocnt, _, osig = ora.wave_windows(seq, *prm)
        _ORACLE[key] = (ocnt, osig)
    return _ORACLE[key]


def check_plan(plan, seqs, prm, dense=True):
    pk = plan.peaks()
    exp = []
    for c, s in enumerate(seqs):
        ocnt, osig = oracle_of(s, prm)
        if dense:
            cnt, sig = plan.dense(c)
            assert np.array_equal(cnt, ocnt), (c, np.flatnonzero(cnt != ocnt)[:5])
            assert np.array_equal(sig.astype(np.int32), osig), (c, np.flatnonzero(sig != osig)[:5])
        idx = np.flatnonzero(osig != 0)
        exp += [(c, int(i), int(ocnt[i]), int(osig[i])) for i in idx]
    got = [(int(r["ctg"]), int(r["window"]), int(r["gc_count"]), int(r["signal"])) for r in pk]
    assert got == exp


def both_inputs(eng, seqs, prm, tile=0, threads=0, flags=BOTH, kernel=None):
    """one seqset (its plane made by gams_seqset_upload_all), the same plan reading the plane and reading the bytes"""
    ss = engine.SeqSet(eng, seqs)
    try:
        for mode in (PLANE, BYTES):
            plan = engine.WavePlan(eng, ss, *prm, flags=flags, tile_windows=tile)
            if threads:
                plan.set_threads(threads)
            plan.set_input(mode)
            if kernel:
                assert plan.kernel_name().startswith(kernel), plan.kernel_name()
            plan.run()
            assert plan.last_input() == mode
            check_plan(plan, seqs, prm, dense=bool(flags & _lib.WAVE_DENSE))
            plan.close()
        plan = engine.WavePlan(eng, ss, *prm, flags=flags, tile_windows=tile)     # the library's own choice: the plane
        plan.run()
        assert plan.last_input() == PLANE
        plan.close()
    finally:
        ss.close()


def test_short_and_ragged_ctgs_run_time_parameters(eng):
    # size 10 step 3 lag 5: every length has its 5 windows; nothing is baked
    both_inputs(eng, mixed([99, 100, 109, 110, 255, 256, 257, 4095, 4096, 4097], 1), (10, 3, 5, 2.0, 1.0),
                kernel="wave_fast_kernel<4, 0, 0, 0,")


def test_ragged_ctgs_size_and_step_baked(eng):
    # 100 / 10 with lag 2: 110 bases are the two windows the lag asks for
    both_inputs(eng, mixed([110, 255, 256, 257, 4095, 4096, 4097], 2), (100, 10, 2, 1.5, 1.0),
                kernel="wave_fast_kernel<4, 100, 10, 0,")


def test_ctg_shorter_than_size_or_lag_is_refused_like_the_reference(eng):
    for n in (99, 100, 109):                      # 0, 1, 1 windows of 100 / 10: fewer than any lag >= 2
        seqs = mixed([n, 4096], 3)
        ss = engine.SeqSet(eng, seqs)
        with pytest.raises(_lib.GamsError) as ei:
            engine.WavePlan(eng, ss, 100, 10, 2, 3.0, 1.0)
        assert ei.value.code == _lib.ESHORT
        with pytest.raises(ValueError):
            ora.wave_windows(seqs[0], 100, 10, 2, 3.0, 1.0)
        ss.close()


@pytest.mark.parametrize("tile,w,windows", [(1024, 4, 923), (3072, 12, 2971)])
def test_one_baked_tile_and_one_window_more(eng, tile, w, windows):
    # a baked tile holds 256 W - lag - 1 windows: ctgs of exactly one tile, one window more, one less, and one of several
    # tiles whose later tiles start on bases that are no multiple of 128 (tile 1 of W = 4: base 8220)
    lens = [(windows - 1) * 10 + 100, windows * 10 + 100, (windows - 2) * 10 + 100, 39990]
    both_inputs(eng, mixed(lens, 4 + w), (100, 10, 100, 3.0, 1.0), tile=tile,
                kernel=f"wave_fast_kernel<{w}, 100, 10, 100,")


def test_tile_first_base_not_on_a_plane_load(eng):
    # W = 8 and the run-time W = 4 form: the second ctg starts on byte 256 k of the buffer and has tiles whose first
    # base (tile start - lag - 1 windows) is no multiple of 128
    seqs = mixed([3001, 40000, 12345], 21)
    both_inputs(eng, seqs, (100, 10, 100, 3.0, 1.0), tile=2048, kernel="wave_fast_kernel<8, 100, 10, 100,")
    both_inputs(eng, seqs, (80, 7, 60, 2.5, 1.0), tile=1024, kernel="wave_fast_kernel<4, 0, 0, 0,")


def test_step_1_one_wave_per_tile(eng):
    # W = 28 tiles of 64 threads: 1,691 windows each
    both_inputs(eng, mixed([5000, 1790, 1791, 1792], 5), (100, 1, 100, 3.0, 1.0), tile=7168, threads=64,
                kernel="wave_fast_kernel<28, 100, 1, 100,")


@pytest.mark.parametrize("prm", [(100, 10, 50, 3.0, 1.0), (100, 10, 200, 3.0, 1.0), (100, 5, 200, 3.0, 1.0),
                                 (100, 20, 50, 3.0, 1.0)])
def test_size_and_step_baked_lag_from_the_arguments(eng, prm):
    both_inputs(eng, mixed([40000, 2090 * 2, 33333], 6), prm)


def test_run_time_parameters(eng):
    both_inputs(eng, mixed([40000, 1000, 25001], 7), (80, 7, 60, 2.5, 1.0))


def test_threshold_minus_one_overflows_the_slots_and_reruns(eng):
    # every window from `lag` on signals: the tiles' fixed slots overflow, gams_wave_peaks regrows them and runs the pass again
    both_inputs(eng, mixed([30000, 20000], 8), (100, 10, 100, -1.0, 1.0))


def test_influence_half_reads_the_dense_rows(eng):
    both_inputs(eng, mixed([30000, 12000], 9), (100, 10, 100, 3.0, 0.5))


def image_of(ss, seqs):
    """host images of the device buffer and of its G/C plane (numpy, not the library's classifier)"""
    off, nb = ss.layout()
    img = np.zeros(nb, np.uint8)
    for o, s in zip(off, seqs):
        img[int(o):int(o) + s.size] = s
    plane = np.packbits(((img & 0xDB) == 0x43).astype(np.uint8), bitorder="little")
    return off, img, plane


def test_reupload_keeps_the_plane_true(eng):
    prm = (100, 10, 100, 3.0, 1.0)
    seqs = mixed([20000, 30001, 11000], 10)
    ss = engine.SeqSet(eng, seqs)
    plan = engine.WavePlan(eng, ss, *prm, flags=BOTH)
    plan.run()
    assert plan.last_input() == PLANE
    check_plan(plan, seqs, prm)
    # one ctg again through gams_seqset_upload: bytes and plane both follow
    seqs[1] = mixed([30001], 11)[0]
    ss.upload(1, seqs[1])
    plan.run()
    assert plan.last_input() == PLANE
    check_plan(plan, seqs, prm)
    # one range through gams_seqset_upload_image: bytes without their plane -- the pass takes the bytes
    seqs[2] = mixed([11000], 12)[0]
    off, img, _ = image_of(ss, seqs)
    ss.upload_image(img, int(off[2]), int(off[2]) + seqs[2].size)
    plan.run()
    assert plan.last_input() == BYTES
    check_plan(plan, seqs, prm)
    plan.set_input(PLANE)                          # a stale plane is never read, asked for or not
    with pytest.raises(_lib.GamsError) as ei:
        plan.run()
    assert ei.value.code == _lib.ESTATE
    plan.set_input(AUTO)
    # bytes and plane of a range together: still stale (the plane of the range before is missing) ...
    off, img, pl = image_of(ss, seqs)
    ss.upload_ranges(img, pl, int(off[1]), int(off[1]) + seqs[1].size)
    plan.run()
    assert plan.last_input() == BYTES
    # ... until everything has come with its plane
    ss.upload_ranges(img, pl, 0, int(off[2]) + seqs[2].size)
    plan.run()
    assert plan.last_input() == PLANE
    check_plan(plan, seqs, prm)
    eng.sync()                                     # the images may go
    plan.close()
    ss.close()


def test_plane_only_seqset(eng):
    prm = (100, 10, 100, 3.0, 1.0)
    seqs = mixed([25000, 4097, 30000], 13)
    ss = engine.SeqSet(eng, seqs, upload=False)
    off, img, pl = image_of(ss, seqs)
    end = int(off[2]) + seqs[2].size
    mid = int(off[1])
    ss.upload_ranges(None, pl, 0, mid)             # in two pieces, as a host that follows its workers sends it
    ss.upload_ranges(None, pl, mid, end)
    plan = engine.WavePlan(eng, ss, *prm, flags=BOTH)
    plan.run()
    assert plan.last_input() == PLANE
    check_plan(plan, seqs, prm)
    plan.set_input(BYTES)
    with pytest.raises(_lib.GamsError) as ei:
        plan.run()
    assert ei.value.code == _lib.ESTATE
    plan.close()
    # whatever reads bytes refuses: a plan of the general tile kernel (16-bit counts), sw, range_gc
    gen = engine.WavePlan(eng, ss, 300, 10, 50, 3.0, 1.0, flags=BOTH)
    assert gen.kernel_name().startswith("wave_tile_kernel"), gen.kernel_name()
    with pytest.raises(_lib.GamsError) as ei:
        gen.run()
    assert ei.value.code == _lib.ESTATE
    gen.close()
    fs, fe = np.array([1000], np.int32), np.array([1200], np.int32)
    rows = np.zeros(64, _lib.SW_ROW_DTYPE)
    n = C.c_uint64()
    assert eng.lib.gams_gpu_sw(eng.h, ss.p, 0, 1, fs.ctypes.data, fe.ctypes.data, 1, 100, 20, 500, rows.ctypes.data,
                               rows.size, C.byref(n)) == _lib.ESTATE
    gc = np.zeros(1, np.float32)
    assert eng.lib.gams_gpu_range_gc(eng.h, ss.p, 0, 1, fs.ctypes.data, fe.ctypes.data, 1, gc.ctypes.data) == _lib.ESTATE
    # the bytes arrive after all: everything answers, and the plane is still true
    ss.upload_ranges(img, pl, 0, end)
    assert eng.lib.gams_gpu_range_gc(eng.h, ss.p, 0, 1, fs.ctypes.data, fe.ctypes.data, 1, gc.ctypes.data) == _lib.OK
    assert abs(float(gc[0]) - ora.range_gc_content(seqs[0], 1, 1000, 1200)) < 5e-5
    plan = engine.WavePlan(eng, ss, *prm, flags=BOTH)
    for mode in (BYTES, PLANE):
        plan.set_input(mode)
        plan.run()
        assert plan.last_input() == mode
        check_plan(plan, seqs, prm)
    eng.sync()
    plan.close()
    ss.close()


def test_host_wave_goldens_through_the_plane(eng, s288c):
    """host.wave / wave_gz upload the plane alone for these parameters: I.peaks.tsv byte for byte, the text made on the
    device, the pass fed by the plane; parameters outside the fast kernels still get their bytes"""
    want = "\n".join(helpers.read_lines("I.peaks.tsv")) + "\n"
    ctgs = helpers.gen_ctgs("I", s288c["I"], piece=500000)
    assert HEADER + host.wave(eng, ctgs, 100, 10, 100, 3.0, 1.0, 0.2) == want
    assert host.last_operator_device() == 1
    text, st = host.wave_timed(eng, ctgs, 100, 10, 100, 3.0, 1.0, 0.2)
    assert HEADER + text.decode() == want and st["plane_input"] == 1 and host.last_operator_device() == 1
    for c in ctgs:
        c["gz"] = gzip.compress(bytes(c["seq"]), 1)
    text, st = host.wave_gz(eng, ctgs, 100, 10, 100, 3.0, 1.0, 0.2, threads=4)
    assert HEADER + text.decode() == want and st["plane_input"] == 1 and host.last_operator_device() == 1
    # several ragged ctgs (more pieces than one, gaps between them), both forms against the oracle
    ragged = []
    for k, c in enumerate(helpers.gen_ctgs("I", s288c["I"], piece=30000)[:5]):
        c = dict(c)
        c["seq"] = c["seq"][:len(c["seq"]) - 7 * k]
        c["chr_end"] = c["chr_start"] + len(c["seq"]) - 1
        c["gz"] = gzip.compress(bytes(c["seq"]), 1)
        ragged.append(c)
    for kw in (dict(size=100, step=10, lag=100, threshold=3.0), dict(size=300, step=10, lag=50, threshold=2.0)):
        exp = "".join(ora.wave_proc_ctg(c["chr_id"], c["chr_start"], c["chr_end"], c["seq"], **kw) for c in ragged)
        fast = kw["size"] == 100
        text, st = host.wave_timed(eng, ragged, **kw)
        assert text.decode() == exp and st["plane_input"] == int(fast)
        text, st = host.wave_gz(eng, ragged, threads=3, **kw)
        assert text.decode() == exp and st["plane_input"] == int(fast)
