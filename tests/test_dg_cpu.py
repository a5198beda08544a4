"""The nearest-neighbour ΔG on the host: gams_dg_table and gams_dg_polymer_host -- the twin every GPU
expectation comes from -- against the strict-f32 model of tests/dg_model.py, which is written from delta_g.rs; the
reference's four known answers; and host.fmt_dg4 against "%.4f"."""
import ctypes as C

import numpy as np
import pytest

import dg_model
import helpers
from gams_amd import _lib, host
from oracle import oracle as ora


def lib_table(temp, salt):
    t = _lib.DgTable()
    rc = _lib.load().gams_dg_table(temp, salt, C.byref(t))
    return rc, np.frombuffer(bytes(t), np.float32)


def twin(table21, seq):
    t = _lib.DgTable.from_buffer_copy(np.ascontiguousarray(table21, np.float32).tobytes())
    a = np.frombuffer(bytes(seq), np.uint8)
    out = C.c_float()
    assert _lib.load().gams_dg_polymer_host(C.byref(t), a.ctypes.data if a.size else None, a.size, C.byref(out)) == _lib.OK
    return np.float32(out.value)


def same_bits(a, b):
    a, b = np.float32(a), np.float32(b)
    return (np.isnan(a) and np.isnan(b)) or a.tobytes() == b.tobytes()


def test_table():
    rc, t = lib_table(37.0, 1.0)
    assert rc == _lib.OK and t.tobytes() == dg_model.table(37.0, 1.0).tobytes()      # ln 1 = 0 in every libm
    for temp, salt in ((30.0, 0.1), (30.0, 0.5)):                                     # logf may differ in the last place
        rc, t = lib_table(temp, salt)
        assert rc == _lib.OK
        np.testing.assert_allclose(t, dg_model.table(temp, salt), rtol=1e-6, atol=0)
    for temp, salt in ((37.0, 0.0), (37.0, -1.0), (37.0, float("nan")), (float("nan"), 1.0), (float("inf"), 1.0),
                       (37.0, float("inf"))):
        assert lib_table(temp, salt)[0] == _lib.EINVAL, (temp, salt)
    assert _lib.load().gams_dg_table(37.0, 1.0, None) == _lib.EINVAL


def test_known_answers():
    for temp, salt, seq, want in dg_model.KNOWN:
        _, t = lib_table(temp, salt)
        got = twin(t, seq.encode())
        if want is None:
            assert np.isnan(got)
        else:
            assert abs(float(got) - want) < 0.001, (seq, got)                          # the reference's own bound
        d = host.DeltaG(temp, salt)
        assert (d.polymer(seq) is None) if want is None else abs(d.polymer(seq) - want) < 0.001
    t = dg_model.table()
    for seq in (b"", b"A", b"AC", b"ACG\x80", b"\xc1CGT", b"ACGU"):
        assert np.isnan(twin(t, seq)), seq
    assert not np.isnan(twin(t, b"acg"))


def test_twin_equals_the_model_bit_for_bit():
    for temp, salt in ((37.0, 1.0), (30.0, 0.1)):
        t = dg_model.table(temp, salt)
        for name, seq in dg_model.battery():
            assert same_bits(twin(t, seq), dg_model.polymer(t, seq)), name
    t = dg_model.table()
    names = dict(dg_model.battery())
    assert all(np.isnan(twin(t, names[f"bad_{w}100"])) for w in ("first", "last", "mid"))
    # the symmetry term is in, and the middle pair alone takes it out
    assert float(twin(t, names["pal100"])) - float(twin(t, names["pal_miss100"])) != 0.0
    assert same_bits(twin(t, b"GAATTC"), np.float32(dg_model.polymer(t, b"GAATT" + b"C")))
    sym = [float(twin(t, b"AT" * n)) for n in (2, 3)]
    assert abs(sym[0] - float(dg_model.polymer(t, b"ATAT"))) == 0.0


def test_ranges_on_host_threads_equal_the_twin():
    """host.dg_ranges_host (the threaded loop the measurements compare the device with) is the twin per range, ranges that
    end on a buffer's last byte included, for any thread count"""
    rng = np.random.default_rng(9)
    seqs = [np.frombuffer(dg_model.random_seq(rng, n), np.uint8).copy() for n in (1000, 37)]
    seqs[0][500] = ord("N")
    d = host.DeltaG()
    which = rng.integers(0, 2, 300).astype(np.uint32)
    ln = np.array([rng.integers(1, seqs[w].size + 1) for w in which], np.uint32)
    off = np.array([seqs[w].size - n if k % 3 == 0 else rng.integers(0, seqs[w].size - n + 1)
                    for k, (w, n) in enumerate(zip(which, ln))], np.uint64)
    exp = np.array([twin(dg_model.table(), seqs[w][o:o + n].tobytes()) for w, o, n in zip(which, off.astype(int), ln.astype(int))])
    for threads in (1, 3, 16):
        got = host.dg_ranges_host(d, seqs, which, off, ln, threads)
        assert all(same_bits(a, b) for a, b in zip(got, exp)), threads
    assert np.isnan(exp).any() and not np.isnan(exp).all()
    assert host.dg_ranges_host(d, seqs, [], [], [], 4).size == 0


def test_the_battery_has_power():
    """the same terms summed as a tree change at least half of the 100-base entries (measured with numpy's pairwise sum:
    1,946 of 2,000), so a kernel that reorders the sum cannot pass the bit-equal checks"""
    rng = np.random.default_rng(7)
    t = dg_model.table()
    seqs = [dg_model.random_seq(rng, 100) for _ in range(2000)]
    differ = sum(not same_bits(dg_model.polymer(t, s), dg_model.polymer(t, s, tree=True)) for s in seqs)
    assert differ >= 1000, differ


def test_fmt_dg4():
    cases = [0.03125, 0.09375, -1e-5, -39.270203, 123456.789, float(np.nextafter(np.float32(2 ** 20), np.float32(0))),
             -float(np.nextafter(np.float32(2 ** 20), np.float32(0))), 0.0, -0.0, 0.00005, 0.00015, 1.0, -1.0, 9.99995,
             2.0 ** -15, 2.0 ** -14, 2.0 ** -40, 1e-45, 65535.99995]
    assert host.fmt_dg4(0.03125) == "0.0312" and host.fmt_dg4(0.09375) == "0.0938"
    assert host.fmt_dg4(-1e-5) == "-0.0000" and host.fmt_dg4(-39.270203) == "-39.2702"
    rng = np.random.default_rng(11)
    bits = rng.integers(0, 2 ** 32, 10000, dtype=np.uint64).astype(np.uint32)
    vals = bits.view(np.float32)
    vals = vals[np.isfinite(vals) & (np.abs(vals) < 2 ** 20)]
    spread = (rng.standard_normal(6000) * np.array([1e-3, 1.0, 50.0, 1e3, 1e5, 3e5]).repeat(1000)).astype(np.float32)
    ties = (rng.integers(-2 ** 24, 2 ** 24, 2000) / 2.0 ** rng.integers(1, 20, 2000)).astype(np.float32)
    checked = 0
    for v in list(cases) + vals.tolist() + spread.tolist() + ties.tolist():
        v = np.float32(v)
        if abs(v) >= 2 ** 20:
            continue
        assert host.fmt_dg4(v) == "%.4f" % float(v), repr(v)
        checked += 1
    assert checked >= 10000
    for v in (2.0 ** 20, -2.0 ** 20, 1e30, float("inf"), float("nan")):
        assert host.fmt_dg4(v) == ""


def test_model_sw_text_is_well_formed(s288c):
    """the model's `sw` text with the column for one S288c ctg: ten fields a row, the tenth empty exactly where the
    model says None"""
    c = helpers.gen_ctgs("I", s288c["I"], piece=100000)[0]
    rng = np.random.default_rng(5)
    feats = [(f"feature:{c['id']}:{i + 1}", int(s), int(s) + int(rng.choice([0, 1, 40, 500])))
             for i, s in enumerate(rng.integers(c["chr_start"] + 50, c["chr_end"] - 600, 40))]
    t = dg_model.table()
    seq = bytearray(c["seq"])
    some_none = False
    for size in (100, 2):
        text = ora.sw_proc_ctg(c["chr_id"], c["chr_start"], c["chr_end"], bytes(seq), feats, size, 5, 500)
        out = dg_model.sw_text_with_dg(text, bytes(seq), c["chr_start"], t)
        assert out.count("\n") == text.count("\n") > 40
        for row, old in zip(out.splitlines(), text.splitlines()):
            f = row.split("\t")
            assert len(f) == 10 and row.startswith(old)
            _, s, e = helpers.parse_range(f[1])
            want = dg_model.polymer(t, bytes(seq[s - c["chr_start"]:e - c["chr_start"] + 1]))
            assert (f[9] == "") == bool(np.isnan(want))
            if f[9]:
                assert f[9] == "%.4f" % float(want)
            some_none |= f[9] == ""
    assert some_none                                   # size 2: every window is shorter than 3 bases
    assert host.header("sw_gibbs") == host.header("sw")[:-1] + "\tgibbs\n"
    assert host.SW_ACTIONS["gibbs"] == 0               # the action itself still has no bit
