"""ctypes binding of libgams_gpu.so (the C ABI in include/gams_gpu.h).

There is no CPU fallback: if the shared library is missing or a call fails, an
exception is raised.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.path.join(_HERE, "libgams_gpu.so")

OK, EINVAL, ENODEV, ENOMEM, EHIP, ESHORT, EUNSUPPORTED, ESTATE = range(8)
WAVE_PEAKS, WAVE_DENSE = 1, 2
WAVE_INPUT_AUTO, WAVE_INPUT_BYTES, WAVE_INPUT_PLANE = 0, 1, 2   # gams_wave_plan_set_input / _last_input
WAVE_BODY_AUTO, WAVE_BODY_WIDE, WAVE_BODY_NARROW = 0, 1, 2      # gams_wave_plan_set_body / _last_body
WAVE_CUT_AUTO, WAVE_CUT_TWO_WAVES, WAVE_CUT_ONE_WAVE = 0, 1, 2  # gams_wave_plan_set_cut / _last_cut
GC_BODY_AUTO, GC_BODY_PORTABLE, GC_BODY_AVX2 = 0, 1, 2          # gams_gc_plane_with
SW_GC, SW_COUNT = 1, 2          # GAMS_SW_GC / GAMS_SW_COUNT: the action set of gams_gpu_sw_text_actions
DG_STAGE_BASES = 512            # GAMS_DG_STAGE_BASES: bases per stage of the ΔG kernel (gams_gpu_diag.h)
DG_TABLE_LDS, DG_TABLE_BPERMUTE = 0, 1                # gams_gpu_dg_set_table
SW_SUMMARY_MAX_ANNO = 4         # GAMS_SW_SUMMARY_MAX_ANNO: the span sets (Prop columns) of one sw summary
SW_SUMMARY_WORDS = 10           # GAMS_SW_SUMMARY_WORDS: COUNT, four S, four NaN counters, C of a summary group
LOADER_RG, LOADER_FEATURE = 0, 1                      # gams_gpu_loader_text: kind
LOADER_RECORDS, LOADER_TSV, LOADER_RESP = 0, 1, 2     # ... and format
SEQ_GZ_BLOCK = 32768            # GAMS_SEQ_GZ_BLOCK: input bytes per deflate block of a `seq:` member
SEQ_GZ_MEMBERS = 3              # GAMS_SEQ_GZ_MEMBERS: gams_gpu_seq_gz's format beside LOADER_RESP
SEQ_GZ_INDEXED = 0x100          # GAMS_SEQ_GZ_INDEXED: ORed into either format, the members carry their chunk index
SEQ_GZ_CHUNK = 1024             # GAMS_SEQ_GZ_CHUNK: bases per index entry
SEQ_GZ_DONE, SEQ_GZ_FOREIGN = 0, 1      # gams_seqset_upload_gz / gams_seq_gunzip_host: the status of a value


class GamsError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"gams_gpu error {code}: {msg}")
        self.code = code


class WaveParams(C.Structure):
    _fields_ = [("size", C.c_int32), ("step", C.c_int32), ("lag", C.c_uint32),
                ("threshold", C.c_float), ("influence", C.c_float)]


class DgTable(C.Structure):
    """gams_dg_table_t: the 21 f32 terms of the nearest-neighbour ΔG"""
    _fields_ = [("nn", C.c_float * 16), ("init", C.c_float * 4), ("sym", C.c_float)]


class GenParams(C.Structure):
    _fields_ = [("piece", C.c_int32), ("fill", C.c_int32), ("min_len", C.c_int32)]


GEN_CTG_DTYPE = np.dtype([("chr", np.uint32), ("serial", np.uint32), ("chr_start", np.int32), ("chr_end", np.int32)])
PEAK_DTYPE = np.dtype([("ctg", np.uint32), ("window", np.uint32), ("gc_count", np.uint32),
                       ("signal", np.int32)])
SW_ROW_DTYPE = np.dtype([("feature", np.uint32), ("type", np.int32), ("distance", np.int32),
                         ("start", np.int32), ("end", np.int32), ("gc_content", np.float32),
                         ("gc_mean", np.float32), ("gc_stddev", np.float32), ("gc_cv", np.float32)])

# name -> (restype, argtypes); exactly the entry points include/gams_gpu.h and include/gams_gpu_diag.h declare
_VP = C.c_void_p
_PP = C.POINTER(C.c_void_p)
PROTOTYPES = {
    "gams_gpu_create": (C.c_int, [C.c_int, _PP]),
    "gams_gpu_destroy": (None, [_VP]),
    "gams_gpu_last_error": (C.c_char_p, [_VP]),
    "gams_gpu_device_info": (C.c_int, [_VP, C.c_char_p, C.c_size_t, C.POINTER(C.c_int32), C.POINTER(C.c_uint64)]),
    "gams_gpu_release_cached": (C.c_int, [_VP, _VP]),
    "gams_gpu_sync": (C.c_int, [_VP]),
    "gams_gpu_timer_start": (C.c_int, [_VP]),
    "gams_gpu_timer_stop": (C.c_int, [_VP, C.POINTER(C.c_float)]),
    "gams_gpu_last_kernel_ms": (C.c_int, [_VP, C.POINTER(C.c_float)]),
    "gams_gpu_last_stage_ms": (C.c_int, [_VP, _VP, C.c_uint32, C.POINTER(C.c_uint32)]),
    "gams_gpu_host_alloc": (C.c_int, [_VP, C.c_uint64, _PP]),
    "gams_gpu_host_free": (None, [_VP, _VP]),
    "gams_window_count": (C.c_int64, [C.c_int64, C.c_int32, C.c_int32]),
    "gams_seqset_create": (C.c_int, [_VP, C.c_uint32, _VP, _PP]),
    "gams_seqset_upload": (C.c_int, [_VP, _VP, C.c_uint32, _VP]),
    "gams_seqset_upload_all": (C.c_int, [_VP, _VP, _VP]),
    "gams_seqset_layout": (C.c_int, [_VP, _VP, _VP, C.POINTER(C.c_uint64)]),
    "gams_seqset_upload_image": (C.c_int, [_VP, _VP, _VP, C.c_uint64, C.c_uint64]),
    "gams_seqset_upload_ranges": (C.c_int, [_VP, _VP, _VP, _VP, C.c_uint64, C.c_uint64]),
    "gams_gc_plane": (C.c_int, [_VP, C.c_uint64, _VP]),
    "gams_gc_plane_with": (C.c_int, [_VP, C.c_uint64, _VP, C.c_int]),
    "gams_wave_plan_set_input": (C.c_int, [_VP, _VP, C.c_int]),
    "gams_wave_plan_last_input": (C.c_int, [_VP, _VP, C.POINTER(C.c_int)]),
    "gams_wave_plan_set_body": (C.c_int, [_VP, _VP, C.c_int]),
    "gams_wave_plan_last_body": (C.c_int, [_VP, _VP, C.POINTER(C.c_int)]),
    "gams_wave_plan_set_cut": (C.c_int, [_VP, _VP, C.c_int]),
    "gams_wave_plan_last_cut": (C.c_int, [_VP, _VP, C.POINTER(C.c_int)]),
    "gams_seqset_download": (C.c_int, [_VP, _VP, C.c_uint32, _VP, _VP]),
    "gams_seqset_destroy": (None, [_VP, _VP]),
    "gams_wave_plan_create": (C.c_int, [_VP, _VP, C.POINTER(WaveParams), C.c_uint32, _PP]),
    "gams_wave_plan_destroy": (None, [_VP, _VP]),
    "gams_wave_total_windows": (C.c_uint64, [_VP]),
    "gams_wave_ctg_windows": (C.c_uint32, [_VP, C.c_uint32]),
    "gams_wave_run_n": (C.c_int, [_VP, _VP, C.c_uint32]),
    "gams_wave_plan_set_depth": (C.c_int, [_VP, _VP, C.c_uint32]),
    "gams_wave_plan_select": (C.c_int, [_VP, _VP, C.c_uint32]),
    "gams_wave_plan_set_lane": (C.c_int, [_VP, _VP, C.c_uint32]),
    "gams_wave_plan_set_taper": (C.c_int, [_VP, _VP, C.c_int]),
    "gams_wave_plan_set_taper_shape": (C.c_int, [_VP, _VP, C.c_int, C.c_int]),
    "gams_wave_plan_tiles": (C.c_int, [_VP, _VP, _VP, C.c_uint64, C.POINTER(C.c_uint64)]),
    "gams_wave_plan_set_queue_threads": (C.c_int, [_VP, _VP, C.c_uint32]),
    "gams_wave_plan_kernel_name": (C.c_int, [_VP, _VP, C.c_char_p, C.c_size_t]),
    "gams_wave_plan_set_pipelined": (C.c_int, [_VP, _VP, C.c_int]),
    "gams_wave_run": (C.c_int, [_VP, _VP]),
    "gams_wave_peaks": (C.c_int, [_VP, _VP, _PP, C.POINTER(C.c_uint64)]),
    "gams_wave_rows_setup": (C.c_int, [_VP, _VP, C.POINTER(C.c_char_p), _VP, C.c_float]),
    "gams_wave_rows_begin": (C.c_int, [_VP, _VP]),
    "gams_wave_rows_end": (C.c_int, [_VP, _VP, _PP, C.POINTER(C.c_uint64), _PP]),
    "gams_wave_signal_text": (C.c_int, [_VP, _VP, C.POINTER(C.c_char_p), _VP, _PP, C.POINTER(C.c_uint64), _PP]),
    "gams_wave_dense": (C.c_int, [_VP, _VP, C.c_uint32, _VP, _VP]),
    "gams_wave_plan_set_tile": (C.c_int, [_VP, _VP, C.c_uint32]),
    "gams_wave_plan_set_threads": (C.c_int, [_VP, _VP, C.c_uint32]),
    "gams_wave_plan_settled": (C.c_int, [_VP, _VP, C.POINTER(C.c_uint32), C.POINTER(C.c_int)]),
    "gams_wave_exact_count": (C.c_int, [_VP, _VP, C.POINTER(C.c_uint64)]),
    "gams_wave_plan_set_guard": (C.c_int, [_VP, _VP, C.c_float, C.c_int]),
    "gams_wave_plan_set_stamps": (C.c_int, [_VP, _VP, C.c_int]),
    "gams_wave_stamps": (C.c_int, [_VP, _VP, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]),
    "gams_wave_stamps_raw": (C.c_int, [_VP, _VP, _VP, C.c_uint64]),
    "gams_gpu_wave": (C.c_int, [_VP, _VP, C.c_uint32, C.POINTER(WaveParams), _VP, _VP, C.POINTER(C.c_uint32)]),
    "gams_gpu_sw": (C.c_int, [_VP, _VP, C.c_uint32, C.c_int32, _VP, _VP, C.c_uint32, C.c_int32, C.c_int32,
                              C.c_int32, _VP, C.c_uint64, C.POINTER(C.c_uint64)]),
    "gams_gpu_sw_batch": (C.c_int, [_VP, _VP, C.c_uint32, _VP, _VP, _VP, _VP, _VP, C.c_int32, C.c_int32, C.c_int32,
                                    _VP, C.c_uint64, _VP, _VP]),
    "gams_gpu_sw_text": (C.c_int, [_VP, _VP, C.c_uint32, _VP, C.POINTER(C.c_char_p), _VP, _VP, _VP, _VP, C.POINTER(C.c_char_p),
                                   C.c_int32, C.c_int32, C.c_int32, _PP, C.POINTER(C.c_uint64), _PP, C.POINTER(C.c_uint64)]),
    "gams_gpu_sw_text_actions": (C.c_int, [_VP, _VP, C.c_uint32, _VP, C.POINTER(C.c_char_p), _VP, _VP, _VP, _VP,
                                           C.POINTER(C.c_char_p), C.c_int32, C.c_int32, C.c_int32, C.c_uint32, _VP, _VP,
                                           _PP, C.POINTER(C.c_uint64), _PP, C.POINTER(C.c_uint64)]),
    "gams_gpu_sw_count_batch": (C.c_int, [_VP, _VP, C.c_uint32, _VP, _VP, _VP, _VP, _VP, C.c_int32, C.c_int32, _VP, _VP,
                                          _VP, C.c_uint64, _VP, _VP]),
    "gams_gpu_range_gc": (C.c_int, [_VP, _VP, C.c_uint32, C.c_int32, _VP, _VP, C.c_uint32, _VP]),
    "gams_gpu_range_gc_batch": (C.c_int, [_VP, _VP, C.c_uint32, _VP, _VP, _VP, _VP, _VP, _VP]),
    "gams_dg_table": (C.c_int, [C.c_float, C.c_float, _VP]),
    "gams_dg_polymer_host": (C.c_int, [_VP, _VP, C.c_uint64, C.POINTER(C.c_float)]),
    "gams_gpu_range_dg_batch": (C.c_int, [_VP, _VP, C.c_uint32, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "gams_gpu_sw_dg_batch": (C.c_int, [_VP, _VP, C.c_uint32, _VP, _VP, _VP, _VP, _VP, C.c_int32, C.c_int32, _VP, _VP,
                                       C.c_uint64, _VP, _VP]),
    "gams_gpu_sw_text_dg": (C.c_int, [_VP, _VP, C.c_uint32, _VP, C.POINTER(C.c_char_p), _VP, _VP, _VP, _VP,
                                      C.POINTER(C.c_char_p), C.c_int32, C.c_int32, C.c_int32, C.c_uint32, _VP, _VP, _VP,
                                      _PP, C.POINTER(C.c_uint64), _PP, C.POINTER(C.c_uint64)]),
    "gams_gpu_dg_set_table": (C.c_int, [_VP, C.c_int]),
    "gams_index_create": (C.c_int, [_VP, C.c_uint32, _VP, _VP, _VP, _PP]),
    "gams_index_destroy": (None, [_VP, _VP]),
    "gams_gpu_count": (C.c_int, [_VP, _VP, _VP, _VP, _VP, C.c_uint64, _VP]),
    "gams_gpu_locate": (C.c_int, [_VP, _VP, _VP, _VP, _VP, C.c_uint64, _VP]),
    "gams_spans_create": (C.c_int, [_VP, C.c_uint32, _VP, _VP, _VP, _PP]),
    "gams_spans_destroy": (None, [_VP, _VP]),
    "gams_gpu_cover": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _VP, _VP, C.c_uint64, _VP]),
    "gams_spans_create_runlist_text": (C.c_int, [_VP, _VP, C.c_uint64, _PP, _PP, C.POINTER(C.c_uint32),
                                                 C.POINTER(C.c_uint64)]),
    "gams_spans_read": (C.c_int, [_VP, _VP, _VP, _VP, _VP, C.c_uint64, C.POINTER(C.c_uint64)]),
    "gams_names_create": (C.c_int, [_VP, C.c_uint32, C.POINTER(C.c_char_p), _PP]),
    "gams_names_read": (C.c_int, [_VP, _VP, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), _VP, _VP]),
    "gams_names_destroy": (None, [_VP, _VP]),
    "gams_gpu_locate_text": (C.c_int, [_VP, _VP, _VP, _VP, _VP, C.c_uint64, _PP, C.POINTER(C.c_uint64),
                                       C.POINTER(C.c_uint64)]),
    "gams_gpu_count_text": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _VP, C.c_uint64, _PP, C.POINTER(C.c_uint64),
                                      C.POINTER(C.c_uint64)]),
    "gams_gpu_anno_text": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _VP, _VP, C.c_uint64, C.c_int, C.c_char_p, C.c_uint32,
                                     C.c_uint32, _PP, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "gams_gpu_read_range_text": (C.c_int, [_VP, _VP, _VP, _VP, C.c_uint64, _VP, _VP, _VP, _VP, _VP, C.c_uint64,
                                           C.POINTER(C.c_uint64)]),
    "gams_index_create_range_text": (C.c_int, [_VP, _VP, _VP, _VP, C.c_uint64, _PP, _VP, C.POINTER(C.c_uint64)]),
    "gams_index_create_range_files": (C.c_int, [_VP, _VP, _VP, C.c_uint32, _VP, _VP, _PP, _VP, C.POINTER(C.c_uint64)]),
    "gams_gpu_loader_text": (C.c_int, [_VP, _VP, _VP, _VP, C.c_uint32, _VP, _VP, C.c_int, C.c_char_p, C.c_uint64, C.c_int, _VP,
                                       _PP, C.POINTER(C.c_uint64), _VP, _VP, _VP, C.POINTER(C.c_uint64)]),
    "gams_gpu_peak_text": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, C.c_uint64, _PP, C.POINTER(C.c_uint64), _VP,
                                     C.POINTER(C.c_uint64)]),
    "gams_gpu_peak_records_text": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, C.c_uint64, C.c_int, _VP, _PP,
                                             C.POINTER(C.c_uint64), _VP, _VP, C.POINTER(C.c_uint64)]),
    "gams_gpu_sw_feature_text": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, C.c_uint64, C.c_int32, C.c_int32,
                                           C.c_int32, C.c_uint32, _VP, _VP, _PP, C.POINTER(C.c_uint64), _VP,
                                           C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "gams_gpu_sw_feature_summary": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, C.c_uint64, C.c_int32, C.c_int32,
                                              C.c_int32, C.c_uint32, _VP, _VP, _VP, C.c_uint32, C.POINTER(C.c_uint64),
                                              C.POINTER(C.c_uint64)]),
    "gams_sw_summary_create": (C.c_int, [_VP, C.c_int32, C.c_uint32, C.c_uint32, C.c_int32, C.c_int32, _PP]),
    "gams_sw_summary_reset": (C.c_int, [_VP, _VP]),
    "gams_sw_summary_read": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _VP]),
    "gams_sw_summary_destroy": (None, [_VP, _VP]),
    "gams_gpu_sw_summary_batch": (C.c_int, [_VP, _VP, C.c_uint32, _VP, _VP, _VP, _VP, _VP, C.c_int32, C.c_int32, C.c_int32,
                                            C.c_uint32, _VP, _VP, _VP, C.c_uint32, C.POINTER(C.c_uint64)]),
    "gams_sw_summary_create_anno": (C.c_int, [_VP, C.c_int32, C.c_uint32, C.c_uint32, C.c_int32, C.c_int32, C.c_uint32, _PP]),
    "gams_sw_summary_read_anno": (C.c_int, [_VP, _VP, _VP]),
    "gams_gpu_sw_summary_batch_anno": (C.c_int, [_VP, _VP, C.c_uint32, _VP, _VP, _VP, _VP, _VP, C.c_int32, C.c_int32, C.c_int32,
                                                 C.c_uint32, _VP, _VP, _VP, C.c_uint32, C.c_uint32, _VP, _VP,
                                                 C.POINTER(C.c_uint64)]),
    "gams_gpu_sw_feature_summary_anno": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, C.c_uint64, C.c_int32, C.c_int32,
                                                   C.c_int32, C.c_uint32, _VP, _VP, _VP, C.c_uint32, C.c_uint32, _VP, _VP,
                                                   C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "gams_gpu_locate_seq_text": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, C.c_uint64, _PP, C.POINTER(C.c_uint64),
                                           C.POINTER(C.c_uint64)]),
    "gams_gpu_locate_seq_chunk": (C.c_uint32, []),
    "gams_gpu_valid_spans": (C.c_int, [_VP, _VP, C.c_uint64, C.c_int32, C.c_int32, _VP, _VP, C.c_uint64,
                                       C.POINTER(C.c_uint64)]),
    "gams_gpu_gen_text": (C.c_int, [_VP, _VP, C.c_uint64, C.POINTER(GenParams), _PP]),
    "gams_gen_counts": (C.c_int, [_VP, _VP, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]),
    "gams_gen_chrs": (C.c_int, [_VP, _VP, _VP, _VP, _VP]),
    "gams_gen_ctgs": (C.c_int, [_VP, _VP, _VP]),
    "gams_gen_seqset": (C.c_int, [_VP, _VP, _PP]),
    "gams_gen_destroy": (None, [_VP, _VP]),
    "gams_deflate_lengths": (C.c_int, [_VP, C.c_uint32, C.c_uint32, _VP]),
    "gams_seq_gz_host": (C.c_int, [_VP, C.c_uint64, _VP, C.c_uint64, C.POINTER(C.c_uint64)]),
    "gams_seq_gz_host_block": (C.c_int, [_VP, C.c_uint64, C.c_uint32, _VP, C.c_uint64, C.POINTER(C.c_uint64)]),
    "gams_gpu_seq_gz": (C.c_int, [_VP, _VP, C.c_uint32, C.c_uint32, _VP, C.c_int, _PP, C.POINTER(C.c_uint64), _VP]),
    "gams_gpu_seq_gz_set_block": (C.c_int, [_VP, C.c_uint32]),
    "gams_seq_gz_host_indexed": (C.c_int, [_VP, C.c_uint64, _VP, C.c_uint64, C.POINTER(C.c_uint64)]),
    "gams_seq_gz_host_indexed_block": (C.c_int, [_VP, C.c_uint64, C.c_uint32, _VP, C.c_uint64, C.POINTER(C.c_uint64)]),
    "gams_seq_gz_host_indexed_chunk": (C.c_int, [_VP, C.c_uint64, C.c_uint32, C.c_uint32, _VP, C.c_uint64,
                                                 C.POINTER(C.c_uint64)]),
    "gams_gpu_seq_gz_set_chunk": (C.c_int, [_VP, C.c_uint32]),
    "gams_seq_gunzip_host": (C.c_int, [_VP, C.c_uint64, _VP, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_int)]),
    "gams_seqset_upload_gz": (C.c_int, [_VP, _VP, C.c_uint32, C.c_uint32, _VP, _VP, _VP, C.POINTER(C.c_uint32)]),
}

_lib = None


def bind(path, strict=True):
    """dlopen one build of the library and bind every prototype of include/gams_gpu.h + gams_gpu_diag.h.
    strict=False (tools/ab.py comparing against an older build) skips entry points it lacks."""
    lib = C.CDLL(path)
    for name, (res, args) in PROTOTYPES.items():
        if not strict and not hasattr(lib, name):
            continue
        fn = getattr(lib, name)  # AttributeError if the .so does not export it
        fn.restype = res
        fn.argtypes = args
    return lib


def load():
    """dlopen libgams_gpu.so and bind every prototype; raises if anything is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(SO_PATH):
        raise ImportError(
            f"{SO_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
    _lib = bind(SO_PATH)
    return _lib
