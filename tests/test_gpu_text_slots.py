"""Every text-owning entry keeps a page-locked text of its own on the handle (include/gams_gpu.h: "valid until the next
call of this entry on the handle"): locate, locate --count, anno, peak, the loader records and locate --seq, called one
after another through the C ABI on one handle, each text read again through its kept pointer after the others ran and
after each of them regrew its buffer."""
import ctypes as C

import numpy as np
import pytest

import locate_seq_text as lst
import peak_text as pt
from gams_amd import _lib, engine, host
from test_gpu_loader_text import file_args
from test_gpu_peak_text import PeakTables, seq_arrays
from test_gpu_text_ops import AnnoTables, LocTables, rust_lines
from test_loader_text_cpu import RECORDS, RG, model_loader

pytestmark = pytest.mark.gpu

L = _lib.load()
GRANULE = 2 << 20              # the pools hand out blocks in granules of 2 MiB: a longer text takes another block


@pytest.fixture(scope="module")
def eng():
    e = engine.Engine(0)
    yield e
    e.close()


def test_six_entries_keep_their_texts_apart(eng):
    rng = np.random.default_rng(3)
    ctgs = [dict(id="ctg:1:1", chr_id="1", chr_start=1, chr_end=1000,
                 seq=np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 1000)].tobytes())]
    recs = [("ctg:1:1", "1:10-20"), ("ctg:1:1", "1:500-600")]
    runlists = {"1": "1-100,300-400"}
    # (two lines a file for the records: the first located line of a ctg in a file only opens its bucket)
    inputs = dict(locate=b"1:10-20\n1:300\n2:5-9\n1:990-1000\tx\n",
                  count=b"1:1-100\n1:15-550\n1:700-800\n",
                  anno=b"ctg:1:1\t1:50-149\nctg:1:1\t1:200-250\nctg:1:1\t1:301-400\n",
                  peak=b"#range\tgc_content\tsignal\n1:100-150\t0.5\t1\n1:400-450\t0.4\t-1\n1:200-260\t0.3\t1\n",
                  records=[b"1:5-9\n1:20-30\n", b"1:40-50\nnm.1(-):60-70\n"],
                  seq=b"1:10-20\n1:1-1000\tx\n1:5\n")
    want = dict(locate=host.locate(eng, ctgs, [ln.split(b"\t")[0].decode() for ln in rust_lines(inputs["locate"])]).encode(),
                count=host.locate(eng, ctgs, [ln.decode() for ln in rust_lines(inputs["count"])], count=True,
                                  rg_records=recs).encode(),
                anno=host.anno(eng, ctgs, runlists, [ln.decode() for ln in rust_lines(inputs["anno"])], idx_id=1,
                               idx_range=2).encode(),
                peak=pt.model(ctgs, inputs["peak"]),
                records=model_loader(ctgs, inputs["records"], RG, "", RECORDS)["text"],
                seq=lst.model(ctgs, inputs["seq"]))
    assert all(w.count(b"\n") >= 1 for w in want.values())

    ss = engine.SeqSet(eng, seq_arrays(ctgs))
    T = PeakTables(eng, ctgs)
    TC = LocTables(eng, ctgs, recs)
    A = AnnoTables(eng, ctgs, runlists)
    text, nb, rows = C.c_void_p(), C.c_uint64(), C.c_uint64()
    out = (C.byref(text), C.byref(nb), C.byref(rows))
    off = np.zeros(3, np.uint64)
    place = (T.slot.ctypes.data, T.cs.ctypes.data, T.ce.ctypes.data)

    def records(files):
        nf, ptrs, lens, _keep = file_args(files)
        return L.gams_gpu_loader_text(eng.h, T.ix, T.chr, T.ids, nf, ptrs, lens.ctypes.data, RG, b"", 0, RECORDS, None,
                                      out[0], out[1], off.ctypes.data, None, None, out[2])

    entry = dict(locate=lambda d: L.gams_gpu_locate_text(eng.h, T.ix, T.chr, T.ids, d, len(d), *out),
                 count=lambda d: L.gams_gpu_count_text(eng.h, TC.ix, TC.chr, TC.rg_ix, TC.rg_group.ctypes.data, d, len(d), *out),
                 anno=lambda d: L.gams_gpu_anno_text(eng.h, A.sp, A.chr, A.ids, A.cs.ctypes.data, A.ce.ctypes.data, d, len(d),
                                                     0, b"", 1, 2, *out),
                 peak=lambda d: L.gams_gpu_peak_text(eng.h, ss.p, T.ix, T.chr, T.ids, *place, d, len(d), out[0], out[1],
                                                     off.ctypes.data, out[2]),
                 records=records,
                 seq=lambda d: L.gams_gpu_locate_seq_text(eng.h, ss.p, T.ix, T.chr, *place, d, len(d), *out))

    def call(name, data):
        """-> (pointer, bytes) of the entry's text"""
        rc = entry[name](data)
        assert rc == 0, (name, L.gams_gpu_last_error(eng.h))
        return text.value, nb.value

    def intact(kept, but=None):
        for name, (ptr, n, w) in kept.items():
            if name != but:
                assert C.string_at(ptr, n) == w, name

    try:
        kept = {}
        for name in entry:
            ptr, n = call(name, inputs[name])
            kept[name] = (ptr, n, want[name])
        assert len({ptr for ptr, _, _ in kept.values()}) == 6
        intact(kept)
        # every entry once more with a text beyond one granule: its buffer is given back and another one taken
        for name in entry:
            times = GRANULE // len(want[name]) + 1
            data = [f * times for f in inputs[name]] if name == "records" else inputs[name] * times
            ptr, n = call(name, data)
            assert n > GRANULE and rows.value >= times
            intact(kept, but=name)
            kept[name] = (ptr, n, C.string_at(ptr, n))
        intact(kept)
    finally:
        A.close()
        TC.close()
        T.close()
        ss.close()
