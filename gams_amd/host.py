"""ctypes binding of libgams_host.so: the C++ host layer (gams_amd/host/*.cpp) that mirrors the
reference's per-ctg operators (wave/sw proc_ctg, locate, anno) on top of the C ABI."""
import ctypes as C
import os
import re

import numpy as np

from . import _lib

_HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.path.join(_HERE, "libgams_host.so")
_h = None


class HostError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"gams host error {code}: {msg}")
        self.code = code


def load():
    global _h
    if _h is not None:
        return _h
    _lib.load()
    if not os.path.exists(SO_PATH):
        raise ImportError(f"{SO_PATH} is missing: run __graft_entry__.build()")
    L = C.CDLL(SO_PATH)
    sp = C.POINTER(C.c_char_p)
    ip = C.c_void_p
    L.gams_host_last_error.restype = C.c_char_p
    L.gams_host_last_code.restype = C.c_int
    L.gams_host_free.argtypes = [C.c_void_p]
    L.gams_host_wave.restype = C.c_void_p
    L.gams_host_wave.argtypes = [C.c_void_p, C.c_uint32, sp, sp, ip, ip, C.POINTER(C.c_void_p), C.c_int32,
                                 C.c_int32, C.c_uint32, C.c_float, C.c_float, C.c_float, C.c_int]
    dp = C.POINTER(C.c_double)
    L.gams_host_wave_timed.restype = C.c_void_p
    L.gams_host_wave_timed.argtypes = [C.c_void_p, C.c_uint32, sp, sp, ip, ip, C.POINTER(C.c_void_p), C.c_int32,
                                       C.c_int32, C.c_uint32, C.c_float, C.c_float, C.c_float, C.c_int, dp,
                                       C.POINTER(C.c_uint64)]
    L.gams_host_wave_gz.restype = C.c_void_p
    L.gams_host_wave_gz.argtypes = [C.c_void_p, C.c_uint32, sp, sp, ip, ip, C.POINTER(C.c_void_p), C.c_void_p, C.c_int32,
                                    C.c_int32, C.c_uint32, C.c_float, C.c_float, C.c_float, C.c_uint32, C.c_int, dp,
                                    C.POINTER(C.c_uint64)]
    L.gams_host_decode_gz_many.restype = C.c_int
    L.gams_host_decode_gz_many.argtypes = [C.c_uint32, C.POINTER(C.c_void_p), C.c_void_p, C.POINTER(C.c_void_p), C.c_void_p,
                                           C.c_void_p, C.c_uint32]
    L.gams_host_wave_multi.restype = C.c_void_p
    L.gams_host_wave_multi.argtypes = [C.POINTER(C.c_void_p), C.c_uint32, C.c_uint32, sp, sp, ip, ip,
                                       C.POINTER(C.c_void_p), C.c_int32, C.c_int32, C.c_uint32, C.c_float,
                                       C.c_float, C.c_float, C.c_int, C.c_uint64]
    L.gams_host_sw.restype = C.c_void_p
    L.gams_host_sw.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_int32, C.c_int32, C.c_void_p, C.c_uint32,
                               sp, ip, ip, C.c_int32, C.c_int32, C.c_int32]
    L.gams_host_locate.restype = C.c_void_p
    L.gams_host_locate.argtypes = [C.c_void_p, C.c_uint32, sp, sp, ip, ip, C.c_char_p, C.c_int, C.c_char_p]
    L.gams_host_find.restype = C.c_void_p
    L.gams_host_find.argtypes = [C.c_void_p, C.c_uint32, sp, sp, ip, ip, C.c_char_p]
    L.gams_host_anno.restype = C.c_void_p
    L.gams_host_anno.argtypes = [C.c_void_p, C.c_uint32, sp, sp, ip, ip, C.c_char_p, C.c_char_p, C.c_int,
                                 C.c_char_p, C.c_uint32, C.c_uint32]
    L.gams_host_locate_seq.restype = C.c_void_p
    L.gams_host_locate_seq.argtypes = [C.c_void_p, C.c_uint32, sp, sp, ip, ip, C.c_char_p, C.c_char_p]
    L.gams_host_read_range.restype = C.c_void_p
    L.gams_host_read_range.argtypes = [C.c_void_p, C.c_uint32, sp, sp, ip, ip, C.c_char_p]
    L.gams_host_decode_gz.restype = C.c_void_p
    L.gams_host_decode_gz.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    L.gams_host_encode_gz.restype = C.c_void_p
    L.gams_host_encode_gz.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    L.gams_host_encode_gz_fast.restype = C.c_void_p
    L.gams_host_encode_gz_fast.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    L.gams_host_seq_gz.restype = C.c_void_p
    L.gams_host_seq_gz.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, sp, C.c_void_p, C.POINTER(C.c_uint64)]
    L.gams_host_seq_gz_indexed.restype = C.c_void_p
    L.gams_host_seq_gz_indexed.argtypes = L.gams_host_seq_gz.argtypes
    L.gams_host_encode_gz_indexed.restype = C.c_void_p
    L.gams_host_encode_gz_indexed.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    L.gams_host_decode_gz_indexed.restype = C.c_void_p
    L.gams_host_decode_gz_indexed.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    L.gams_host_wave_gz_device.restype = C.c_void_p
    L.gams_host_wave_gz_device.argtypes = L.gams_host_wave_gz.argtypes
    L.gams_host_seqset_upload_gz.restype = C.c_int
    L.gams_host_seqset_upload_gz.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p), C.c_void_p,
                                             C.c_void_p, C.c_uint32, C.c_void_p]
    L.gams_host_loader_records.restype = C.c_void_p
    L.gams_host_loader_records.argtypes = [C.c_void_p, C.c_uint32, sp, sp, ip, ip, C.c_char_p, C.c_char_p]
    L.gams_host_count_multi.restype = C.c_int
    L.gams_host_count_multi.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32] + [C.c_void_p] * 6 + [C.c_uint64, C.c_void_p]
    L.gams_host_cover_multi.restype = C.c_int
    L.gams_host_cover_multi.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32] + [C.c_void_p] * 8 + [C.c_uint64, C.c_void_p]
    L.gams_host_last_operator_ms.restype = C.c_double
    L.gams_host_last_operator_ms.argtypes = []
    L.gams_host_sw_multi_timed.restype = C.c_void_p
    L.gams_host_sw_multi_timed.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, sp, sp, ip, ip, C.c_void_p, C.c_char_p,
                                           C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
    L.gams_host_sw_multi.restype = C.c_void_p
    L.gams_host_sw_multi.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, sp, sp, ip, ip, C.c_void_p, C.c_char_p,
                                     C.c_int32, C.c_int32, C.c_int32]
    L.gams_host_sw_actions.restype = C.c_void_p
    L.gams_host_sw_actions.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_int32, C.c_int32, C.c_void_p, C.c_uint32,
                                       sp, ip, ip, C.c_int32, C.c_int32, C.c_int32, C.c_uint32, C.c_char_p]
    L.gams_host_sw_multi_actions.restype = C.c_void_p
    L.gams_host_sw_multi_actions.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, sp, sp, ip, ip, C.c_void_p, C.c_char_p,
                                             C.c_int32, C.c_int32, C.c_int32, C.c_uint32, C.c_char_p]
    L.gams_host_sw_multi_actions_timed.restype = C.c_void_p
    L.gams_host_sw_multi_actions_timed.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, sp, sp, ip, ip, C.c_void_p,
                                                   C.c_char_p, C.c_int32, C.c_int32, C.c_int32, C.c_uint32, C.c_char_p,
                                                   C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
    L.gams_host_last_sw_index_ms.restype = C.c_double
    L.gams_host_last_sw_index_ms.argtypes = []
    u64p = C.POINTER(C.c_uint64)
    L.gams_host_bincode_ctg_bundle.restype = C.c_void_p
    L.gams_host_bincode_ctg_bundle.argtypes = [C.c_uint32, sp, sp, ip, ip, u64p]
    L.gams_host_bincode_ctg_bundle_decode.restype = C.c_void_p
    L.gams_host_bincode_ctg_bundle_decode.argtypes = [C.c_void_p, C.c_uint64]
    L.gams_host_bincode_lapper.restype = C.c_void_p
    L.gams_host_bincode_lapper.argtypes = [C.c_uint64, C.c_void_p, C.c_void_p, sp, u64p]
    L.gams_host_bincode_lapper_decode.restype = C.c_void_p
    L.gams_host_bincode_lapper_decode.argtypes = [C.c_void_p, C.c_uint64]
    L.gams_host_resp_command.restype = C.c_void_p
    L.gams_host_resp_command.argtypes = [C.c_uint32, sp, u64p, u64p]
    L.gams_host_resp_scan_values.restype = C.c_void_p
    L.gams_host_resp_scan_values.argtypes = [C.c_char_p, u64p]
    L.gams_host_resp_parse.restype = C.c_void_p
    L.gams_host_resp_parse.argtypes = [C.c_char_p, C.c_uint64, u64p]
    L.gams_host_index_from_lappers.restype = C.c_void_p
    L.gams_host_index_from_lappers.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_char_p), u64p]
    L.gams_host_header.restype = C.c_void_p
    L.gams_host_header.argtypes = [C.c_int]
    L.gams_host_tsv_ctgs.restype = C.c_void_p
    L.gams_host_tsv_ctgs.argtypes = [C.c_uint32, sp, sp, ip, ip]
    L.gams_host_loader_tsv.restype = C.c_void_p
    L.gams_host_loader_tsv.argtypes = [C.c_void_p, C.c_uint32, sp, sp, ip, ip, C.c_char_p, C.c_char_p]
    L.gams_host_peak.restype = C.c_void_p
    L.gams_host_peak.argtypes = [C.c_void_p, C.c_uint32, sp, sp, ip, ip, C.POINTER(C.c_void_p), C.c_char_p]
    L.gams_host_locate_text.restype = C.c_void_p
    L.gams_host_locate_text.argtypes = [C.c_void_p, C.c_uint32, sp, sp, ip, ip, C.c_char_p, C.c_uint64, C.c_int,
                                        C.c_char_p, C.POINTER(C.c_uint64)]
    L.gams_host_anno_text.restype = C.c_void_p
    L.gams_host_anno_text.argtypes = [C.c_void_p, C.c_uint32, sp, sp, ip, ip, C.c_char_p, C.c_char_p, C.c_uint64,
                                      C.c_int, C.c_char_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64)]
    L.gams_host_anno_set_create.restype = C.c_void_p
    L.gams_host_anno_set_create.argtypes = [C.c_void_p, C.c_char_p, C.c_uint64]
    L.gams_host_anno_set_destroy.restype = None
    L.gams_host_anno_set_destroy.argtypes = [C.c_void_p]
    L.gams_host_anno_set_device.restype = C.c_int
    L.gams_host_anno_set_device.argtypes = [C.c_void_p]
    L.gams_host_anno_set_spans.restype = C.c_void_p
    L.gams_host_anno_set_spans.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]
    L.gams_host_anno_set_names.restype = C.c_void_p
    L.gams_host_anno_set_names.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    L.gams_host_anno_text_set.restype = C.c_void_p
    L.gams_host_anno_text_set.argtypes = [C.c_void_p, C.c_uint32, sp, sp, ip, ip, C.c_void_p, C.c_char_p, C.c_uint64,
                                          C.c_int, C.c_char_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64)]
    L.gams_host_anno_set.restype = C.c_void_p
    L.gams_host_anno_set.argtypes = [C.c_void_p, C.c_uint32, sp, sp, ip, ip, C.c_void_p, C.c_char_p, C.c_int,
                                     C.c_char_p, C.c_uint32, C.c_uint32]
    L.gams_host_read_runlist_json.restype = C.c_int
    L.gams_host_read_runlist_json.argtypes = [C.c_char_p, C.c_uint64, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64),
                                              C.POINTER(C.c_uint64)]
    L.gams_host_read_runlist_json_get.restype = None
    L.gams_host_read_runlist_json_get.argtypes = [C.c_void_p] * 5
    L.gams_host_runlist_load.restype = C.c_int64
    L.gams_host_runlist_load.argtypes = [C.c_void_p, C.c_char_p, C.c_uint64, C.c_int]
    L.gams_host_locate_rg.restype = C.c_void_p
    L.gams_host_locate_rg.argtypes = [C.c_void_p, C.c_uint32, sp, sp, ip, ip, C.c_char_p, C.c_int, C.c_char_p, C.c_uint64]
    L.gams_host_locate_text_rg.restype = C.c_void_p
    L.gams_host_locate_text_rg.argtypes = [C.c_void_p, C.c_uint32, sp, sp, ip, ip, C.c_char_p, C.c_uint64, C.c_int,
                                           C.c_char_p, C.c_uint64, C.POINTER(C.c_uint64)]
    L.gams_host_rg_load.restype = C.c_int64
    L.gams_host_rg_load.argtypes = [C.c_void_p, C.c_uint32, sp, sp, ip, ip, C.c_char_p, C.c_uint64, C.c_int]
    L.gams_host_read_range_text.restype = C.c_int
    L.gams_host_read_range_text.argtypes = [C.c_void_p, C.c_uint32, sp, sp, ip, ip, C.c_char_p, C.c_uint64,
                                            C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.gams_host_read_range_text_get.restype = None
    L.gams_host_read_range_text_get.argtypes = [C.c_void_p] * 5
    L.gams_host_sw_actions_rg.restype = C.c_void_p
    L.gams_host_sw_actions_rg.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_int32, C.c_int32, C.c_void_p, C.c_uint32,
                                          sp, ip, ip, C.c_int32, C.c_int32, C.c_int32, C.c_uint32, C.c_char_p, C.c_uint64]
    L.gams_host_sw_multi_actions_rg.restype = C.c_void_p
    L.gams_host_sw_multi_actions_rg.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, sp, sp, ip, ip, C.c_void_p, C.c_char_p,
                                                C.c_int32, C.c_int32, C.c_int32, C.c_uint32, C.c_char_p, C.c_uint64]
    vp, fl = C.POINTER(C.c_void_p), C.c_void_p        # several files: their pointers, their lengths (uint64)
    L.gams_host_locate_rgs.restype = C.c_void_p
    L.gams_host_locate_rgs.argtypes = [C.c_void_p, C.c_uint32, sp, sp, ip, ip, C.c_char_p, C.c_int, C.c_uint32, vp, fl]
    L.gams_host_locate_text_rgs.restype = C.c_void_p
    L.gams_host_locate_text_rgs.argtypes = [C.c_void_p, C.c_uint32, sp, sp, ip, ip, C.c_char_p, C.c_uint64, C.c_int,
                                            C.c_uint32, vp, fl, C.POINTER(C.c_uint64)]
    L.gams_host_sw_actions_rgs.restype = C.c_void_p
    L.gams_host_sw_actions_rgs.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_int32, C.c_int32, C.c_void_p, C.c_uint32,
                                           sp, ip, ip, C.c_int32, C.c_int32, C.c_int32, C.c_uint32, C.c_uint32, vp, fl]
    L.gams_host_sw_multi_actions_rgs.restype = C.c_void_p
    L.gams_host_sw_multi_actions_rgs.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, sp, sp, ip, ip, C.c_void_p, C.c_char_p,
                                                 C.c_int32, C.c_int32, C.c_int32, C.c_uint32, C.c_uint32, vp, fl]
    L.gams_host_sw_text_rgs.restype = C.c_void_p
    L.gams_host_sw_text_rgs.argtypes = [C.c_void_p, C.c_uint32, sp, sp, ip, ip, C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p,
                                        C.c_char_p, C.c_uint64, C.c_int32, C.c_int32, C.c_int32, C.c_uint32, C.c_uint32, vp, fl,
                                        C.POINTER(C.c_uint64)]
    L.gams_host_loader_text.restype = C.c_void_p
    L.gams_host_loader_text.argtypes = [C.c_void_p, C.c_uint32, sp, sp, ip, ip, C.c_uint32, vp, fl, C.c_int, C.c_char_p,
                                        C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]
    L.gams_host_last_operator_device.restype = C.c_int
    L.gams_host_last_operator_device.argtypes = []
    L.gams_host_fmt_prop4.restype = C.c_void_p
    L.gams_host_fmt_prop4.argtypes = [C.c_float]
    L.gams_host_fmt_dg4.restype = C.c_void_p
    L.gams_host_fmt_dg4.argtypes = [C.c_float]
    L.gams_host_sw_gibbs.restype = C.c_void_p
    L.gams_host_sw_gibbs.argtypes = [C.c_void_p, C.c_uint32, sp, sp, ip, ip, C.c_void_p, C.c_char_p, C.c_int32, C.c_int32,
                                     C.c_int32, C.c_uint32, C.c_char_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
    L.gams_host_dg_ranges.restype = C.c_int
    L.gams_host_dg_ranges.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32,
                                      C.c_void_p]
    L.gams_host_fmt_f32_short.restype = C.c_void_p
    L.gams_host_fmt_f32_short.argtypes = [C.c_float]
    L.gams_host_peak_text.restype = C.c_void_p
    L.gams_host_peak_text.argtypes = [C.c_void_p, C.c_uint32, sp, sp, ip, ip, C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p,
                                      C.c_char_p, C.c_uint64, C.POINTER(C.c_uint64)]
    L.gams_host_peak_records_text.restype = C.c_void_p
    L.gams_host_peak_records_text.argtypes = [C.c_void_p, C.c_uint32, sp, sp, ip, ip, C.POINTER(C.c_void_p), C.c_void_p,
                                              C.c_void_p, C.c_char_p, C.c_uint64, C.c_int, C.c_void_p, C.c_void_p,
                                              C.POINTER(C.c_uint64)]
    L.gams_host_peak_rows_records.restype = C.c_void_p
    L.gams_host_peak_rows_records.argtypes = [C.c_char_p, C.c_uint64, C.c_int, C.POINTER(C.c_uint64)]
    L.gams_host_fmt_f32_json.restype = C.c_void_p
    L.gams_host_fmt_f32_json.argtypes = [C.c_float]
    L.gams_host_locate_seq_text.restype = C.c_void_p
    L.gams_host_locate_seq_text.argtypes = [C.c_void_p, C.c_uint32, sp, sp, ip, ip, C.POINTER(C.c_void_p), C.c_void_p,
                                            C.c_void_p, C.c_char_p, C.c_uint64, C.POINTER(C.c_uint64)]
    L.gams_host_sw_text.restype = C.c_void_p
    L.gams_host_sw_text.argtypes = [C.c_void_p, C.c_uint32, sp, sp, ip, ip, C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p,
                                    C.c_char_p, C.c_uint64, C.c_int32, C.c_int32, C.c_int32, C.c_uint32, C.c_char_p,
                                    C.c_char_p, C.c_uint64, C.POINTER(C.c_uint64)]
    L.gams_host_sw_summary.restype = C.c_void_p
    L.gams_host_sw_summary.argtypes = [C.c_void_p, C.c_uint32, sp, sp, ip, ip, C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p,
                                       C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                       C.c_uint32, C.c_char_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.POINTER(C.c_uint64)]
    L.gams_host_sw_summary_anno.restype = C.c_void_p
    L.gams_host_sw_summary_anno.argtypes = L.gams_host_sw_summary.argtypes[:-2] + [
        C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]
    L.gams_host_sw_summarise_rows_props.restype = C.c_int
    L.gams_host_sw_summarise_rows_props.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int32, C.c_uint32, C.c_void_p,
                                                    C.c_uint32, C.c_void_p, C.c_void_p]
    L.gams_host_sw_summary_text_props.restype = C.c_void_p
    L.gams_host_sw_summary_text_props.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_int32, C.c_uint32, C.c_uint32,
                                                  C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]
    L.gams_host_prop4_units.restype = C.c_int32
    L.gams_host_prop4_units.argtypes = [C.c_float]
    L.gams_host_sw_summarise_rows.restype = C.c_int
    L.gams_host_sw_summarise_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int32, C.c_uint32, C.c_void_p]
    L.gams_host_sw_summary_text.restype = C.c_void_p
    L.gams_host_sw_summary_text.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_int32, C.c_uint32, C.POINTER(C.c_uint64)]
    L.gams_host_gen.restype = C.c_void_p
    L.gams_host_gen.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_uint64, C.c_int32, C.c_int32, C.c_int32]
    L.gams_host_read_fasta.restype = C.c_void_p
    L.gams_host_read_fasta.argtypes = [C.c_char_p, C.c_uint64, C.POINTER(C.c_uint64)]
    L.gams_host_gen_text.restype = C.c_void_p
    L.gams_host_gen_text.argtypes = [C.c_void_p, C.c_char_p, C.c_uint64, C.c_int32, C.c_int32, C.c_int32,
                                     C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
    L.gams_host_fmt_f32.restype = C.c_void_p
    L.gams_host_fmt_f32.argtypes = [C.c_float]
    L.gams_host_range_roundtrip.restype = C.c_void_p
    L.gams_host_range_roundtrip.argtypes = [C.c_char_p]
    _h = L
    return L


def _take(p):
    L = load()
    if not p:
        raise HostError(L.gams_host_last_code(), L.gams_host_last_error().decode(errors="replace"))
    s = C.string_at(p).decode()
    L.gams_host_free(p)
    return s


def _ctg_arrays(ctgs):
    n = len(ctgs)
    ids = (C.c_char_p * max(n, 1))(*[c["id"].encode() for c in ctgs])
    chrs = (C.c_char_p * max(n, 1))(*[c["chr_id"].encode() for c in ctgs])
    st = np.array([c["chr_start"] for c in ctgs], np.int32)
    en = np.array([c["chr_end"] for c in ctgs], np.int32)
    return n, ids, chrs, st, en


def wave(eng, ctgs, size=100, step=10, lag=100, threshold=3.0, influence=1.0, coverage=0.2, is_signal=False):
    """TSV rows (no header) of `gams wave` over `ctgs` (dicts with id, chr_id, chr_start, chr_end, seq)."""
    n, ids, chrs, st, en = _ctg_arrays(ctgs)
    bufs = [np.ascontiguousarray(np.frombuffer(c["seq"], np.uint8) if not isinstance(c["seq"], np.ndarray)
                                 else c["seq"]) for c in ctgs]
    seqs = (C.c_void_p * max(n, 1))(*[b.ctypes.data for b in bufs])
    return _take(load().gams_host_wave(eng.h, n, ids, chrs, st.ctypes.data, en.ctypes.data, seqs, size, step, lag,
                                       threshold, influence, coverage, int(is_signal)))


STAGE_NAMES = ("inflate_upload_ms", "upload_ms", "plan_ms", "kernel_ms", "peaks_ms", "format_ms", "total_ms",
               "inflate_threads", "peaks", "plane_input")   # plane_input: 1 if the pass read the seqset's 1-bit G/C plane


def _take_bytes(p, n):
    L = load()
    if not p:
        raise HostError(L.gams_host_last_code(), L.gams_host_last_error().decode(errors="replace"))
    b = C.string_at(p, n.value)
    L.gams_host_free(p)
    return b


def _stage_dict(st):
    d = {k: float(v) for k, v in zip(STAGE_NAMES, st)}
    d["inflate_threads"] = int(d["inflate_threads"])
    d["peaks"] = int(d["peaks"])
    d["plane_input"] = int(d["plane_input"])
    return d


def wave_timed(eng, ctgs, size=100, step=10, lag=100, threshold=3.0, influence=1.0, coverage=0.2, sync=False, is_signal=False):
    """`wave` from gunzipped host buffers -> (TSV bytes, stage clock dict of gams::WaveStages)."""
    n, ids, chrs, st, en = _ctg_arrays(ctgs)
    bufs = [np.ascontiguousarray(np.frombuffer(c["seq"], np.uint8) if not isinstance(c["seq"], np.ndarray)
                                 else c["seq"]) for c in ctgs]
    seqs = (C.c_void_p * max(n, 1))(*[b.ctypes.data for b in bufs])
    stages = (C.c_double * 10)()
    ln = C.c_uint64()
    p = load().gams_host_wave_timed(eng.h, n, ids, chrs, st.ctypes.data, en.ctypes.data, seqs, size, step, lag,
                                    threshold, influence, coverage, int(sync) | (2 if is_signal else 0), stages, C.byref(ln))
    return _take_bytes(p, ln), _stage_dict(stages)


def wave_gz(eng, ctgs, size=100, step=10, lag=100, threshold=3.0, influence=1.0, coverage=0.2, threads=0, sync=False,
            inflate="host"):
    """`wave` from the gzip'd `seq:` values (ctg dicts with id, chr_id, chr_start, chr_end, gz = bytes): `threads`
    host threads inflate one ctg at a time each into a page-locked image of the device buffer (0: 16)
    -> (TSV bytes, stage clock dict).  inflate="device": indexed members (seq_gz(..., indexed=True)) go up as they are
    and are inflated on the device (gams_seqset_upload_gz); the host threads inflate only what it does not take."""
    if inflate not in ("host", "device"):
        raise ValueError("wave_gz: inflate is 'host' or 'device'")
    n, ids, chrs, st, en = _ctg_arrays(ctgs)
    bufs = [np.frombuffer(c["gz"], np.uint8) for c in ctgs]
    blobs = (C.c_void_p * max(n, 1))(*[b.ctypes.data for b in bufs])
    lens = np.array([b.size for b in bufs], np.uint64)
    stages = (C.c_double * 10)()
    ln = C.c_uint64()
    entry = load().gams_host_wave_gz_device if inflate == "device" else load().gams_host_wave_gz
    p = entry(eng.h, n, ids, chrs, st.ctypes.data, en.ctypes.data, blobs, lens.ctypes.data, size, step,
              lag, threshold, influence, coverage, threads, int(sync), stages, C.byref(ln))
    return _take_bytes(p, ln), _stage_dict(stages)


def decode_gz_many(blobs, sizes, threads=0):
    """decode_gz of a batch of `seq:` values on `threads` host threads (0: 16); sizes[i] = room for value i
    -> list of uint8 arrays"""
    L = load()
    n = len(blobs)
    src = [np.frombuffer(b, np.uint8) for b in blobs]
    dst = [np.empty(max(int(s), 1), np.uint8) for s in sizes]
    sp_ = (C.c_void_p * max(n, 1))(*[b.ctypes.data for b in src])
    dp_ = (C.c_void_p * max(n, 1))(*[b.ctypes.data for b in dst])
    sl = np.array([b.size for b in src], np.uint64)
    cap = np.array([int(s) for s in sizes], np.uint64)
    got = np.zeros(max(n, 1), np.uint64)
    if L.gams_host_decode_gz_many(n, sp_, sl.ctypes.data, dp_, cap.ctypes.data, got.ctypes.data, threads) != 0:
        raise HostError(L.gams_host_last_code(), L.gams_host_last_error().decode(errors="replace"))
    return [d[:int(g)] for d, g in zip(dst, got)]


def wave_multi(engines, ctgs, size=100, step=10, lag=100, threshold=3.0, influence=1.0, coverage=0.2,
               is_signal=False, batch_bytes=1 << 30):
    """`gams wave` over several handles (one per GPU): LPT-sharded ctgs, one host thread per handle."""
    n, ids, chrs, st, en = _ctg_arrays(ctgs)
    bufs = [np.ascontiguousarray(np.frombuffer(c["seq"], np.uint8) if not isinstance(c["seq"], np.ndarray)
                                 else c["seq"]) for c in ctgs]
    seqs = (C.c_void_p * max(n, 1))(*[b.ctypes.data for b in bufs])
    hs = (C.c_void_p * len(engines))(*[e.h.value for e in engines])
    return _take(load().gams_host_wave_multi(hs, len(engines), n, ids, chrs, st.ctypes.data, en.ctypes.data, seqs,
                                             size, step, lag, threshold, influence, coverage, int(is_signal),
                                             batch_bytes))


SW_ACTIONS = {"gc": _lib.SW_GC, "count": _lib.SW_COUNT, "gibbs": 0}   # sw.rs:28-32; gibbs is accepted, computes nothing


def sw_actions(names):
    """`gams sw -a NAME ...` -> the GAMS_SW_* mask; a single name may be given as a string.  ValueError for a name
    sw.rs does not declare."""
    if isinstance(names, str):
        names = (names,)
    mask = 0
    for n in names:
        if n not in SW_ACTIONS:
            raise ValueError(f"sw: unknown action {n!r} (one of {', '.join(SW_ACTIONS)})")
        mask |= SW_ACTIONS[n]
    return mask


def _rg_lines(rg_records):
    return "\n".join(f"{c}\t{r}" for c, r in rg_records).encode()


def _one_rg_source(rg_records, rg_data):
    """rg_records and rg_data (the bytes of an rg file, or a list / tuple of them: several files loaded one after
    another, as `gams rg f1 f2 ...` loads them) are two forms of one argument"""
    if rg_data is not None and len(rg_records):
        raise ValueError("rg_records and rg_data are mutually exclusive: give the rg: records or the bytes of an rg file")
    if isinstance(rg_data, (list, tuple)):
        return [bytes(d) for d in rg_data]
    return None if rg_data is None else bytes(rg_data)


def _files(datas):
    """(n, pointers, lengths, the buffers that must outlive the call) of several files' bytes"""
    bufs = [np.frombuffer(bytes(d), np.uint8) for d in datas]
    ptrs = (C.c_void_p * max(len(bufs), 1))(*[b.ctypes.data if b.size else None for b in bufs])
    lens = np.array([b.size for b in bufs], np.uint64)
    return len(bufs), ptrs, lens.ctypes.data, (bufs, lens)


def sw(eng, ctg, features, size=100, mx=20, resize=500, actions=("gc",), rg_records=(), rg_data=None):
    """features: list of (feature_id, start, end).  actions: names of `gams sw -a` (gc, count, gibbs);
    rg_records: (ctg_id, range string) of the rg: records, the idx:rg: source of `count`; or rg_data: the bytes of an
    rg file, loaded on the device against THIS ctg alone.  read_range over the whole ctg table gives a range that spans
    two ctgs to the first of them; located against one ctg it falls to that ctg, and the line drop-first swallows can
    change.  Ranges inside one ctg (the rule: SNPs, peaks) give the same counts either way; where ranges may cross
    ctgs use sw_multi with every ctg, or rg_records from read_range over the table."""
    rg_data = _one_rg_source(rg_records, rg_data)
    mask = sw_actions(actions)
    nf = len(features)
    fid = (C.c_char_p * max(nf, 1))(*[f[0].encode() for f in features])
    fs = np.array([f[1] for f in features], np.int32)
    fe = np.array([f[2] for f in features], np.int32)
    seq = np.ascontiguousarray(np.frombuffer(ctg["seq"], np.uint8) if not isinstance(ctg["seq"], np.ndarray)
                               else ctg["seq"])
    if isinstance(rg_data, list):
        nr, rp, rl, _keep = _files(rg_data)
        return _take(load().gams_host_sw_actions_rgs(eng.h, ctg["id"].encode(), ctg["chr_id"].encode(), ctg["chr_start"],
                                                     ctg["chr_end"], seq.ctypes.data, nf, fid, fs.ctypes.data,
                                                     fe.ctypes.data, size, mx, resize, mask, nr, rp, rl))
    if rg_data is not None:
        return _take(load().gams_host_sw_actions_rg(eng.h, ctg["id"].encode(), ctg["chr_id"].encode(), ctg["chr_start"],
                                                    ctg["chr_end"], seq.ctypes.data, nf, fid, fs.ctypes.data,
                                                    fe.ctypes.data, size, mx, resize, mask, rg_data, len(rg_data)))
    if mask == _lib.SW_GC and not rg_records:
        return _take(load().gams_host_sw(eng.h, ctg["id"].encode(), ctg["chr_id"].encode(), ctg["chr_start"],
                                         ctg["chr_end"], seq.ctypes.data, nf, fid, fs.ctypes.data, fe.ctypes.data,
                                         size, mx, resize))
    return _take(load().gams_host_sw_actions(eng.h, ctg["id"].encode(), ctg["chr_id"].encode(), ctg["chr_start"],
                                             ctg["chr_end"], seq.ctypes.data, nf, fid, fs.ctypes.data, fe.ctypes.data,
                                             size, mx, resize, mask, _rg_lines(rg_records)))


def locate(eng, ctgs, rgs, count=False, rg_records=(), rg_data=None):
    """rgs: list of range strings; for --count rg_records: list of (ctg_id, range string), or rg_data: the bytes of an
    rg file, loaded on the device."""
    rg_data = _one_rg_source(rg_records, rg_data)
    n, ids, chrs, st, en = _ctg_arrays(ctgs)
    if isinstance(rg_data, list):
        nr, rp, rl, _keep = _files(rg_data)
        return _take(load().gams_host_locate_rgs(eng.h, n, ids, chrs, st.ctypes.data, en.ctypes.data,
                                                 "\n".join(rgs).encode(), int(count), nr, rp, rl))
    if rg_data is not None:
        return _take(load().gams_host_locate_rg(eng.h, n, ids, chrs, st.ctypes.data, en.ctypes.data,
                                                "\n".join(rgs).encode(), int(count), rg_data, len(rg_data)))
    rg_lines = "\n".join(f"{c}\t{r}" for c, r in rg_records)
    return _take(load().gams_host_locate(eng.h, n, ids, chrs, st.ctypes.data, en.ctypes.data,
                                         "\n".join(rgs).encode(), int(count), rg_lines.encode()))


def find(eng, ctgs, rgs):
    n, ids, chrs, st, en = _ctg_arrays(ctgs)
    out = _take(load().gams_host_find(eng.h, n, ids, chrs, st.ctypes.data, en.ctypes.data, "\n".join(rgs).encode()))
    return out.split("\n")[:len(rgs)]


class AnnoSet:
    """The span set of an anno run, built once from the bytes of the runlist JSON file (gams::AnnoSet): on the device
    (gams_spans_create_runlist_text), by the host reader where the device refuses.  `device` says which route built
    it; HostError with code EINVAL where the host reader refuses the file.  Pass it as `runlists` to anno() /
    anno_text(); several input files share it."""

    def __init__(self, eng, data):
        data = bytes(data)
        self.eng = eng
        self.p = load().gams_host_anno_set_create(eng.h, data, len(data))
        if not self.p:
            _check_rc(-1)
        L = load()
        self.device = bool(L.gams_host_anno_set_device(self.p))
        ng, ns = C.c_uint32(), C.c_uint64()
        self._sp = L.gams_host_anno_set_spans(self.p, C.byref(ng), C.byref(ns))
        self.n_groups, self.n_spans = ng.value, ns.value
        out_len = C.c_uint64()
        flat = _take_bytes(L.gams_host_anno_set_names(self.p, C.byref(out_len)), out_len)
        self.names = [s.decode(errors="surrogateescape") for s in flat.split(b"\0")[:-1]]

    def spans(self):
        """{chr: (lo, hi)} of the resident set, in group order (gams_spans_read)"""
        return _read_spans(self.eng, self._sp, self.names)

    def close(self):
        if getattr(self, "p", None):
            load().gams_host_anno_set_destroy(self.p)
            self.p = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _read_spans(eng, sp, names):
    lib = _lib.load()
    ns = C.c_uint64()
    off = np.zeros(len(names) + 1, np.uint64)
    eng.check(lib.gams_spans_read(eng.h, sp, off.ctypes.data, None, None, 0, C.byref(ns)))
    lo, hi = np.zeros(max(ns.value, 1), np.int32), np.zeros(max(ns.value, 1), np.int32)
    if ns.value:
        eng.check(lib.gams_spans_read(eng.h, sp, off.ctypes.data, lo.ctypes.data, hi.ctypes.data, ns.value, C.byref(ns)))
    return {k: (lo[int(off[g]):int(off[g + 1])].copy(), hi[int(off[g]):int(off[g + 1])].copy()) for g, k in enumerate(names)}


def read_runlist_text(eng, data):
    """The runlist JSON bytes through the device entry (gams_spans_create_runlist_text) and gams_spans_read:
    {chr: (lo, hi)} as numpy arrays, in file order.  GamsError (EUNSUPPORTED) where the device refuses."""
    lib = _lib.load()
    data = bytes(data)
    sp, nm = C.c_void_p(), C.c_void_p()
    ng, ns = C.c_uint32(), C.c_uint64()
    eng.check(lib.gams_spans_create_runlist_text(eng.h, data, len(data), C.byref(sp), C.byref(nm), C.byref(ng), C.byref(ns)))
    try:
        n, nb = C.c_uint32(), C.c_uint64()
        eng.check(lib.gams_names_read(eng.h, nm, C.byref(n), C.byref(nb), None, None))
        flat = C.create_string_buffer(max(nb.value, 1))
        off = np.zeros(n.value + 1, np.uint64)
        eng.check(lib.gams_names_read(eng.h, nm, C.byref(n), C.byref(nb), flat, off.ctypes.data))
        names = [flat.raw[int(off[g]):int(off[g + 1])].decode() for g in range(n.value)]
        assert n.value == ng.value
        return _read_spans(eng, sp, names)
    finally:
        lib.gams_spans_destroy(eng.h, sp)
        lib.gams_names_destroy(eng.h, nm)


def read_runlist_json(data):
    """The host reader of a runlist JSON file (gams::read_runlist_json): {chr: (lo, hi)} as numpy arrays, in file
    order (a key that comes twice keeps its first place and its last value), every set normalised.  HostError with
    code EINVAL where the reference panics."""
    L = load()
    data = bytes(data)
    ng, ns, nb = C.c_uint32(), C.c_uint64(), C.c_uint64()
    _check_rc(L.gams_host_read_runlist_json(data, len(data), C.byref(ng), C.byref(ns), C.byref(nb)))
    names = C.create_string_buffer(max(nb.value, 1))
    noff, goff = np.zeros(ng.value + 1, np.uint64), np.zeros(ng.value + 1, np.uint64)
    lo, hi = np.zeros(max(ns.value, 1), np.int32), np.zeros(max(ns.value, 1), np.int32)
    L.gams_host_read_runlist_json_get(names, noff.ctypes.data, goff.ctypes.data, lo.ctypes.data, hi.ctypes.data)
    out = {}
    for g in range(ng.value):
        key = names.raw[int(noff[g]):int(noff[g + 1])].decode()
        out[key] = (lo[int(goff[g]):int(goff[g + 1])].copy(), hi[int(goff[g]):int(goff[g + 1])].copy())
    return out


def runlist_load(eng, data, device_route=True):
    """Builds the span set of a runlist JSON file's bytes and drops it: a timing entry.  device_route: through
    gams::AnnoSet (the device entry), else the host reader + gams_spans_create.  Returns the spans of the set;
    last_operator_ms() has the ms of the load, last_operator_device() the route that built it."""
    data = bytes(data)
    got = load().gams_host_runlist_load(eng.h, data, len(data), int(device_route))
    _check_rc(0 if got >= 0 else -1)
    return int(got)


def _anno_set(eng, runlists):
    """(the AnnoSet behind a bytes / AnnoSet `runlists` argument, whether this call owns it); (None, False) for a dict"""
    if isinstance(runlists, AnnoSet):
        return runlists, False
    if isinstance(runlists, (bytes, bytearray, memoryview)):
        return AnnoSet(eng, runlists), True
    return None, False


def anno(eng, ctgs, runlists, lines, header=False, prefix="", idx_id=1, idx_range=2):
    """runlists: dict chr -> runlist string, the bytes of the runlist JSON file, or an AnnoSet."""
    n, ids, chrs, st, en = _ctg_arrays(ctgs)
    aset, own = _anno_set(eng, runlists)
    if aset is not None:
        try:
            return _take(load().gams_host_anno_set(eng.h, n, ids, chrs, st.ctypes.data, en.ctypes.data, aset.p,
                                                   "\n".join(lines).encode(), int(header), prefix.encode(), idx_id,
                                                   idx_range))
        finally:
            if own:
                aset.close()
    rl = "\n".join(f"{k}\t{v}" for k, v in runlists.items())
    return _take(load().gams_host_anno(eng.h, n, ids, chrs, st.ctypes.data, en.ctypes.data, rl.encode(),
                                       "\n".join(lines).encode(), int(header), prefix.encode(), idx_id, idx_range))


def locate_text(eng, ctgs, data, count=False, rg_records=(), rg_data=None):
    """`locate -f` / `locate --count` over the bytes of the input file (text in, text out on the device; the array
    path where the device refuses).  Returns the rows as bytes; rg_records / rg_data as for locate()."""
    rg_data = _one_rg_source(rg_records, rg_data)
    n, ids, chrs, st, en = _ctg_arrays(ctgs)
    if isinstance(rg_data, list):
        nr, rp, rl, _keep = _files(rg_data)
        out_len = C.c_uint64()
        return _take_bytes(load().gams_host_locate_text_rgs(eng.h, n, ids, chrs, st.ctypes.data, en.ctypes.data, data,
                                                            len(data), int(count), nr, rp, rl, C.byref(out_len)), out_len)
    if rg_data is not None:
        out_len = C.c_uint64()
        return _take_bytes(load().gams_host_locate_text_rg(eng.h, n, ids, chrs, st.ctypes.data, en.ctypes.data, data,
                                                           len(data), int(count), rg_data, len(rg_data),
                                                           C.byref(out_len)), out_len)
    rg_lines = "\n".join(f"{c}\t{r}" for c, r in rg_records)
    out_len = C.c_uint64()
    return _take_bytes(load().gams_host_locate_text(eng.h, n, ids, chrs, st.ctypes.data, en.ctypes.data, data, len(data),
                                                    int(count), rg_lines.encode(), C.byref(out_len)), out_len)


def anno_text(eng, ctgs, runlists, data, header=False, prefix="", idx_id=1, idx_range=2):
    """`anno` over the bytes of one input file; runlists: dict chr -> runlist string, the bytes of the runlist JSON
    file, or an AnnoSet (one set for several input files).  Returns the rows as bytes."""
    n, ids, chrs, st, en = _ctg_arrays(ctgs)
    out_len = C.c_uint64()
    aset, own = _anno_set(eng, runlists)
    if aset is not None:
        try:
            return _take_bytes(load().gams_host_anno_text_set(eng.h, n, ids, chrs, st.ctypes.data, en.ctypes.data, aset.p,
                                                              data, len(data), int(header), prefix.encode(), idx_id,
                                                              idx_range, C.byref(out_len)), out_len)
        finally:
            if own:
                aset.close()
    rl = "\n".join(f"{k}\t{v}" for k, v in runlists.items())
    return _take_bytes(load().gams_host_anno_text(eng.h, n, ids, chrs, st.ctypes.data, en.ctypes.data, rl.encode(), data,
                                                  len(data), int(header), prefix.encode(), idx_id, idx_range,
                                                  C.byref(out_len)), out_len)


def last_operator_device():
    """1 if the last wave / wave_timed / wave_gz / locate_text / locate_seq_text / anno_text / peak_text / peak_records_text / sw_text / gen_text of this thread made its rows on the device,
    0 if it fell back to the host; after AnnoSet(...) / runlist_load: 1 if the device built the set from the bytes"""
    return int(load().gams_host_last_operator_device())


def fmt_prop4(v):
    """`{:.4}` of an anno prop as the device formats it ("" outside [0, 1])"""
    return _take(load().gams_host_fmt_prop4(v))


def gen(eng, chr_id, seq, piece=500000, fill=50, min_len=5000):
    """ctg rows (id, range, chr_id, chr_start, chr_end, chr_strand, length) of one chromosome."""
    a = np.ascontiguousarray(np.frombuffer(seq, np.uint8) if not isinstance(seq, np.ndarray) else seq)
    return _take(load().gams_host_gen(eng.h, chr_id.encode(), a.ctypes.data, a.size, piece, fill, min_len))


def read_fasta(data):
    """The records of a FASTA file's bytes as the reference's reader gives them (gams::read_fasta; no engine):
    [(id, bases)] in file order, trailing white space of every sequence line trimmed."""
    out_len = C.c_uint64()
    blob = _take_bytes(load().gams_host_read_fasta(bytes(data), len(data), C.byref(out_len)), out_len)
    head, _, seqs = blob.partition(b"\n\n") if not blob.startswith(b"\n") else (b"", b"", blob[1:])   # no record: "\n"
    recs, at = [], 0
    for row in (head.split(b"\n") if head else []):
        name, n = row.split(b"\t")
        recs.append((name.decode("latin-1"), seqs[at:at + int(n)]))
        at += int(n)
    return recs


def gen_text(eng, data, piece=500000, fill=50, min_len=5000):
    """`gams gen` over the bytes of one FASTA file, made on the device from one upload of them (the host's passes where
    the device refuses; last_operator_device says which): -> (ctgs, chr_len, seqset).  ctgs: dicts with id, chr_id,
    chr_start, chr_end, range, length, chromosomes in file order; chr_len: {chromosome: bases}; seqset: the resident
    engine.SeqSet of the ctgs' bases and G/C plane, slot k = ctgs[k]."""
    from . import engine

    out_len, ptr = C.c_uint64(), C.c_void_p()
    text = _take_bytes(load().gams_host_gen_text(eng.h, bytes(data), len(data), piece, fill, min_len, C.byref(ptr),
                                                 C.byref(out_len)), out_len).decode("latin-1")   # an id may hold any byte
    ctgs, chr_len = [], {}
    for row in text.split("\n")[:-1]:
        f = row.split("\t")
        if f[0] == "chr":
            chr_len[f[1]] = int(f[2])
        else:
            s, e = int(f[3]), int(f[4])
            ctgs.append(dict(id=f[1], chr_id=f[2], chr_start=s, chr_end=e, range=f"{f[2]}:{s}-{e}" if e != s else f"{f[2]}:{s}",
                             length=e - s + 1))
    return ctgs, chr_len, engine.SeqSet.adopt(eng, ptr.value, [c["length"] for c in ctgs])


def locate_seq(eng, ctgs, rgs):
    """`gams locate --seq`: FASTA text; ctgs carry their gunzipped sequence in c["seq"]."""
    n, ids, chrs, st, en = _ctg_arrays(ctgs)
    seq_lines = "\n".join(f"{c['id']}\t{bytes(c['seq']).decode()}" for c in ctgs)
    return _take(load().gams_host_locate_seq(eng.h, n, ids, chrs, st.ctypes.data, en.ctypes.data,
                                             "\n".join(rgs).encode(), seq_lines.encode()))


def locate_seq_text(eng, ctgs, data, seqset=None):
    """`gams locate --seq` over the bytes of a range file: the FASTA records of the located lines, as bytes, copied on
    the device out of a seqset (the host's passes where the device refuses; last_operator_device says which).  Without
    `seqset` the ctgs carry their bases in c["seq"], uploaded for the call; with a resident engine.SeqSet -- what
    gen_text returns -- its slot i holds ctgs[i] (a ctg dict may name another in c["slot"]; None: no sequence).  The
    sequence bytes are copied as they are, whatever their values."""
    n, ids, chrs, st, en = _ctg_arrays(ctgs)
    out_len = C.c_uint64()
    if seqset is None:
        bufs = [np.ascontiguousarray(np.frombuffer(c["seq"], np.uint8) if not isinstance(c["seq"], np.ndarray)
                                     else c["seq"]) for c in ctgs]
        seqs = (C.c_void_p * max(n, 1))(*[b.ctypes.data for b in bufs])
        p = load().gams_host_locate_seq_text(eng.h, n, ids, chrs, st.ctypes.data, en.ctypes.data, seqs, None, None,
                                             bytes(data), len(data), C.byref(out_len))
    else:
        slot = [c.get("slot", i) for i, c in enumerate(ctgs)]
        slots = np.array([0xffffffff if k is None else k for k in slot], np.uint32)
        p = load().gams_host_locate_seq_text(eng.h, n, ids, chrs, st.ctypes.data, en.ctypes.data, None, seqset.p,
                                             slots.ctypes.data, bytes(data), len(data), C.byref(out_len))
    return _take_bytes(p, out_len)


def read_range(eng, ctgs, lines):
    """utils.rs:39-67 incl. the drop-first-per-ctg quirk: list of (ctg_id, range string)."""
    n, ids, chrs, st, en = _ctg_arrays(ctgs)
    out = _take(load().gams_host_read_range(eng.h, n, ids, chrs, st.ctypes.data, en.ctypes.data,
                                            "\n".join(lines).encode()))
    return [tuple(r.split("\t")) for r in out.splitlines()]


def read_range_text(eng, ctgs, data):
    """read_range over the bytes of an rg file, bucketed on the device (the host's passes where the device refuses):
    dict(ids = the ctg id of every bucket in ctg-id order, empty buckets included; off = n_buckets + 1 offsets;
    start, end, line = the kept ranges of bucket k at [off[k], off[k + 1]) in file order, line the 0-based line
    number) as numpy arrays."""
    n, ids, chrs, st, en = _ctg_arrays(ctgs)
    L = load()
    nb, nk = C.c_uint64(), C.c_uint64()
    _check_rc(L.gams_host_read_range_text(eng.h, n, ids, chrs, st.ctypes.data, en.ctypes.data, bytes(data), len(data),
                                          C.byref(nb), C.byref(nk)))
    which = np.zeros(max(nb.value, 1), np.uint32)
    off = np.zeros(nb.value + 1, np.uint64)
    start, end = np.zeros(max(nk.value, 1), np.int32), np.zeros(max(nk.value, 1), np.int32)
    line = np.zeros(max(nk.value, 1), np.uint32)
    L.gams_host_read_range_text_get(which.ctypes.data, off.ctypes.data, start.ctypes.data, end.ctypes.data, line.ctypes.data)
    return dict(ids=[ctgs[i]["id"] for i in which[:nb.value]], off=off, start=start[:nk.value], end=end[:nk.value],
                line=line[:nk.value])


def rg_load(eng, ctgs, data, text_path=True):
    """Builds the rg index of an rg file's bytes over `ctgs` and drops it: a timing entry.  text_path: on the device
    (Locator::set_rg_index_text), else read_range + set_rg_index on the host's lines.  Returns the ctgs with a group;
    last_operator_ms() has the ms of the load, last_operator_device() the path that built it."""
    n, ids, chrs, st, en = _ctg_arrays(ctgs)
    got = load().gams_host_rg_load(eng.h, n, ids, chrs, st.ctypes.data, en.ctypes.data, bytes(data), len(data),
                                   int(text_path))
    _check_rc(0 if got >= 0 else -1)
    return int(got)


def decode_gz(blob):
    n = C.c_uint64()
    p = load().gams_host_decode_gz(blob, len(blob), C.byref(n))
    if not p:
        raise HostError(load().gams_host_last_code(), load().gams_host_last_error().decode(errors="replace"))
    out = C.string_at(p, n.value)
    load().gams_host_free(p)
    return out


def encode_gz(data):
    n = C.c_uint64()
    p = load().gams_host_encode_gz(data, len(data), C.byref(n))
    if not p:
        raise HostError(-1, "encode_gz failed")
    out = C.string_at(p, n.value)
    load().gams_host_free(p)
    return out


def encode_gz_fast(data, indexed=False):
    """The `seq:` value of `data` as the literal-only gzip member the device writes for the same bases
    (gams_seq_gz_host), for hosts that hold them; decode_gz and every gzip reader inflate it.  indexed: with the chunk
    index in its FEXTRA field (gams_seq_gz_host_indexed), which the device inflater needs."""
    n = C.c_uint64()
    entry = load().gams_host_encode_gz_indexed if indexed else load().gams_host_encode_gz_fast
    return _take_bytes(entry(bytes(data), len(data), C.byref(n)), n)


def decode_gz_indexed(blob):
    """An indexed member inflated by the host twin of the device inflater (gams_seq_gunzip_host: the same decoder core,
    chunk by chunk); HostError for anything that is not an intact indexed member."""
    n = C.c_uint64()
    return _take_bytes(load().gams_host_decode_gz_indexed(bytes(blob), len(blob), C.byref(n)), n)


def seqset_upload_gz(eng, seqset, blobs, first=0, threads=0):
    """Slots first .. first + len(blobs) of an engine.SeqSet from their `seq:` values (gams::seqset_upload_gz): the
    device inflates the indexed members, `threads` host threads (0: 16) whatever it does not take
    -> (values inflated on the device, on the host)."""
    n = len(blobs)
    bufs = [np.frombuffer(bytes(b), np.uint8) for b in blobs]
    ptrs = (C.c_void_p * max(n, 1))(*[b.ctypes.data if b.size else None for b in bufs])
    lens = np.array([b.size for b in bufs], np.uint64)
    slot = np.ascontiguousarray(seqset.lengths[first:first + n], np.uint32)
    if slot.size != n:
        raise ValueError("seqset_upload_gz: slots outside the seqset")
    went = np.zeros(2, np.uint32)
    _check_rc(load().gams_host_seqset_upload_gz(eng.h, seqset.p, first, n, ptrs, lens.ctypes.data, slot.ctypes.data, threads,
                                                went.ctypes.data))
    return int(went[0]), int(went[1])


def _seq_gz(eng, seqset, first, count, ids, indexed=False):
    count = len(seqset.lengths) - first if count is None else count
    off = np.zeros(max(count, 0) + 1, np.uint64)
    n = C.c_uint64()
    names = None if ids is None else (C.c_char_p * max(count, 1))(*[i.encode("latin-1") for i in ids])
    entry = load().gams_host_seq_gz_indexed if indexed else load().gams_host_seq_gz
    data = _take_bytes(entry(eng.h, seqset.p, first, count, names, off.ctypes.data, C.byref(n)), n)
    return data, off


def seq_gz(eng, seqset, first=0, count=None, indexed=False):
    """The `seq:` values of slots first .. first + count (None: to the end) of a resident engine.SeqSet, deflated on the
    device: a list of gzip members, one per slot.  indexed: each with its chunk index (GAMS_SEQ_GZ_INDEXED), the form
    SeqSet.from_gz and wave_gz(inflate="device") inflate on the device."""
    data, off = _seq_gz(eng, seqset, first, count, None, indexed)
    return [data[int(off[i]):int(off[i + 1])] for i in range(len(off) - 1)]


def seq_records(eng, seqset, ctgs, fmt="resp", indexed=False):
    """What `gams gen` stores under seq:{ctg} (redis.rs:137-140) for every ctg of gen_text's result -- slot k of
    `seqset` is ctgs[k] --, as the SET stream resp_command(["SET", "seq:" + id, member]) of every ctg, written on the
    device: FASTA bytes -> gen_text -> seq_records never brings a base back."""
    if fmt != "resp":
        raise ValueError("seq_records: fmt is 'resp'")
    if len(ctgs) != len(seqset.lengths):
        raise ValueError("seq_records: one ctg per slot of the seqset")
    return _seq_gz(eng, seqset, 0, len(ctgs), [c["id"] for c in ctgs], indexed)[0]


def loader_records(eng, ctgs, lines, tag=None):
    """(key, json) of the rg: (tag None) or feature: records `gams rg` / `gams feature` would SET."""
    n, ids, chrs, st, en = _ctg_arrays(ctgs)
    out = _take(load().gams_host_loader_records(eng.h, n, ids, chrs, st.ctypes.data, en.ctypes.data,
                                                "\n".join(lines).encode(), tag.encode() if tag is not None else None))
    return [tuple(r.split("\t", 1)) for r in out.splitlines()]


LOADER_KINDS = {"rg": _lib.LOADER_RG, "feature": _lib.LOADER_FEATURE}
LOADER_FORMATS = {"records": _lib.LOADER_RECORDS, "tsv": _lib.LOADER_TSV, "resp": _lib.LOADER_RESP}


def loader_text(eng, ctgs, files, kind="rg", tag="feature", fmt="records", serial_base=None):
    """`gams rg f1 f2 ...` (kind "rg") / `gams feature --tag TAG f1 f2 ...` (kind "feature") over the bytes of the files:
    the records the loader would SET, written on the device (the host's passes where it refuses; last_operator_device
    says which), in the reference's order: file by file, the ctgs by id, file order inside a ctg.  fmt: "records"
    ("{key}\\t{json}\\n"), "tsv" (the rows of loader_tsv without its header) or "resp" (resp_command(["SET", key, json])
    of every record).  serial_base: {ctg id: the ctg's cnt: before the load} (absent: 0).
    -> (bytes, {ctg id: the counter after the load} for every ctg, [records of every file])"""
    if kind not in LOADER_KINDS or fmt not in LOADER_FORMATS:
        raise ValueError(f"loader_text: kind is one of {list(LOADER_KINDS)}, fmt one of {list(LOADER_FORMATS)}")
    n, ids, chrs, st, en = _ctg_arrays(ctgs)
    nf, fp, fl, _keep = _files(files)
    base = np.array([(serial_base or {}).get(c["id"], 0) for c in ctgs], np.int32)
    nxt = np.zeros(max(n, 1), np.int32)
    per = np.zeros(max(nf, 1), np.uint64)
    out_len = C.c_uint64()
    text = _take_bytes(load().gams_host_loader_text(eng.h, n, ids, chrs, st.ctypes.data, en.ctypes.data, nf, fp, fl,
                                                    LOADER_KINDS[kind], tag.encode("latin-1") if isinstance(tag, str) else tag,
                                                    LOADER_FORMATS[fmt], base.ctypes.data if n else None, nxt.ctypes.data,
                                                    per.ctypes.data, C.byref(out_len)), out_len)
    return text, {c["id"]: int(v) for c, v in zip(ctgs, nxt)}, [int(v) for v in per[:nf]]


def sw_multi(engines, ctgs, features_per_ctg, size=100, mx=20, resize=500, actions=("gc",), rg_records=(), rg_data=None):
    """`gams sw` over several handles; features_per_ctg[i] = list of (id, start, end) of ctgs[i]; actions,
    rg_records and rg_data as for sw()."""
    rg_data = _one_rg_source(rg_records, rg_data)
    mask = sw_actions(actions)
    n, ids, chrs, st, en = _ctg_arrays(ctgs)
    bufs = [np.ascontiguousarray(np.frombuffer(c["seq"], np.uint8) if not isinstance(c["seq"], np.ndarray)
                                 else c["seq"]) for c in ctgs]
    seqs = (C.c_void_p * max(n, 1))(*[b.ctypes.data for b in bufs])
    hs = (C.c_void_p * len(engines))(*[e.h.value for e in engines])
    rows = "\n".join(f"{i}\t{fid}\t{s}\t{e}" for i, fl in enumerate(features_per_ctg) for fid, s, e in fl)
    if isinstance(rg_data, list):
        nr, rp, rl, _keep = _files(rg_data)
        return _take(load().gams_host_sw_multi_actions_rgs(hs, len(engines), n, ids, chrs, st.ctypes.data, en.ctypes.data,
                                                           seqs, rows.encode(), size, mx, resize, mask, nr, rp, rl))
    if rg_data is not None:
        return _take(load().gams_host_sw_multi_actions_rg(hs, len(engines), n, ids, chrs, st.ctypes.data, en.ctypes.data,
                                                          seqs, rows.encode(), size, mx, resize, mask, rg_data,
                                                          len(rg_data)))
    if mask == _lib.SW_GC and not rg_records:
        return _take(load().gams_host_sw_multi(hs, len(engines), n, ids, chrs, st.ctypes.data, en.ctypes.data, seqs,
                                               rows.encode(), size, mx, resize))
    return _take(load().gams_host_sw_multi_actions(hs, len(engines), n, ids, chrs, st.ctypes.data, en.ctypes.data, seqs,
                                                   rows.encode(), size, mx, resize, mask, _rg_lines(rg_records)))


class DeltaG:
    """The nearest-neighbour free energy of a DNA polymer (the reference's DeltaG, delta_g.rs): .table holds the 21 f32
    terms of (temp, salt) as a _lib.DgTable, made once by gams_dg_table; .polymer(seq) is DeltaG::polymer on the host
    (gams_dg_polymer_host, the twin of the device entries): a float, None for fewer than 3 bases or a byte that is none
    of ACGTacgt."""

    def __init__(self, temp=37.0, salt=1.0):
        self.temp, self.salt = float(temp), float(salt)
        self.table = _lib.DgTable()
        rc = _lib.load().gams_dg_table(self.temp, self.salt, C.byref(self.table))
        if rc != _lib.OK:
            raise ValueError(f"DeltaG: temp {temp!r} must be finite, salt {salt!r} finite and above 0")

    def polymer_f32(self, seq):
        """the f32 itself, NaN for None"""
        a = np.ascontiguousarray(np.frombuffer(seq.encode("latin-1") if isinstance(seq, str) else bytes(seq), np.uint8))
        out = C.c_float()
        rc = _lib.load().gams_dg_polymer_host(C.byref(self.table), a.ctypes.data if a.size else None, a.size, C.byref(out))
        if rc != _lib.OK:
            raise _lib.GamsError(rc, "gams_dg_polymer_host")
        return np.float32(out.value)

    def polymer(self, seq):
        v = self.polymer_f32(seq)
        return None if np.isnan(v) else float(v)


def range_dg(eng, seqset, sel, chr_start, ranges, dg=None):
    """The ΔG of chromosome ranges inside ctgs of a resident seqset, on the device (gams_gpu_range_dg_batch): sel[k] names
    a slot of the seqset, chr_start[k] its first chromosome coordinate, ranges[k] its [(start, end)] -> one f32 array
    over the concatenated ranges, NaN for None.  dg: a DeltaG (default DeltaG())."""
    from . import engine

    dg = DeltaG() if dg is None else dg
    off = np.concatenate([[0], np.cumsum([len(r) for r in ranges])]).astype(np.uint64)
    rs = np.array([r[0] for rl in ranges for r in rl], np.int32)
    re_ = np.array([r[1] for rl in ranges for r in rl], np.int32)
    rc, out = engine.range_dg_batch(eng, seqset, sel, chr_start, off, rs, re_, dg.table)
    eng.check(rc)
    return out


def dg_ranges_host(dg, seqs, which, off, length, threads=16):
    """For measurement (tools/bench_dg.py): DeltaG.polymer_f32 of the length[q] bytes at seqs[which[q]][off[q]:] for
    every q, in C++ on `threads` host threads -> f32 array.  seqs: contiguous uint8 arrays."""
    which, off = np.ascontiguousarray(which, np.uint32), np.ascontiguousarray(off, np.uint64)
    length = np.ascontiguousarray(length, np.uint32)
    ptrs = (C.c_void_p * max(len(seqs), 1))(*[s.ctypes.data for s in seqs])
    out = np.zeros(which.size, np.float32)
    _check_rc(load().gams_host_dg_ranges(C.byref(dg.table), ptrs, which.ctypes.data, off.ctypes.data, length.ctypes.data,
                                         which.size, threads, out.ctypes.data))
    return out


def fmt_dg4(v):
    """the ΔG column's text: `{:.4}` of an f32 (half to even on the exact value, "-0.0000" keeps its sign); "" for a
    value the device formatter does not cover (NaN, an infinity, 2^20 or more in size)"""
    return _take(load().gams_host_fmt_dg4(float(np.float32(v))))


def sw_gibbs(eng, ctgs, features_per_ctg, size=100, mx=20, resize=500, actions=("gc",), rg_data=None, dg=None, seqset=None):
    """sw_multi on one handle with the ΔG of every window as a tenth field (header("sw_gibbs")): the f32 of
    DeltaG.polymer over the window's bases with four decimals, empty for None.  The column is this project's own:
    upstream declares `--action gibbs` and never fills it, and actions=("gibbs",) of sw / sw_multi still prints nothing.
    dg: a DeltaG (default DeltaG()).  seqset: a resident engine.SeqSet whose slot i holds ctgs[i] (a ctg dict may name
    another in c["slot"]); without it the ctgs carry their bases in c["seq"].  actions as for sw_multi; rg_data: the bytes
    of one rg file, the idx:rg: source of `count` (None: every count is 0)."""
    if isinstance(rg_data, (list, tuple)):
        raise ValueError("sw_gibbs takes the bytes of one rg file")
    rg_data = None if rg_data is None else bytes(rg_data)
    mask = sw_actions(actions)
    dg = DeltaG() if dg is None else dg
    n, ids, chrs, st, en = _ctg_arrays(ctgs)
    rows = "\n".join(f"{i}\t{fid}\t{s}\t{e}" for i, fl in enumerate(features_per_ctg) for fid, s, e in fl)
    seqs = slots = None
    if seqset is None:
        bufs = [np.ascontiguousarray(np.frombuffer(c["seq"], np.uint8) if not isinstance(c["seq"], np.ndarray)
                                     else c["seq"]) for c in ctgs]
        seqs = (C.c_void_p * max(n, 1))(*[b.ctypes.data for b in bufs])
    else:
        slots = np.array([c.get("slot", i) for i, c in enumerate(ctgs)], np.uint32)
    return _take(load().gams_host_sw_gibbs(eng.h, n, ids, chrs, st.ctypes.data, en.ctypes.data, seqs, rows.encode(), size, mx,
                                           resize, mask, rg_data, 0 if rg_data is None else len(rg_data), C.byref(dg.table),
                                           seqset.p if seqset is not None else None,
                                           slots.ctypes.data if slots is not None else None))


def last_operator_ms():
    """ms the last locate / anno call of this thread spent inside the C++ operator (without the binding's copies)"""
    return float(load().gams_host_last_operator_ms())


def sw_multi_timed(engines, ctgs, features_per_ctg, size=100, mx=20, resize=500, actions=("gc",), rg_records=()):
    """sw_multi, returning (text, ms of the operator itself: upload + kernels + row text, without this binding's
    parsing and copies).  With actions / rg_records the ms include the rg index build; last_sw_index_ms() has it."""
    mask = sw_actions(actions)
    n, ids, chrs, st, en = _ctg_arrays(ctgs)
    bufs = [np.ascontiguousarray(np.frombuffer(c["seq"], np.uint8) if not isinstance(c["seq"], np.ndarray)
                                 else c["seq"]) for c in ctgs]
    seqs = (C.c_void_p * max(n, 1))(*[b.ctypes.data for b in bufs])
    hs = (C.c_void_p * len(engines))(*[e.h.value for e in engines])
    rows = "\n".join(f"{i}\t{fid}\t{s}\t{e}" for i, fl in enumerate(features_per_ctg) for fid, s, e in fl)
    ms = C.c_double(0.0)
    n_out = C.c_uint64(0)
    if mask == _lib.SW_GC and not rg_records:
        p = load().gams_host_sw_multi_timed(hs, len(engines), n, ids, chrs, st.ctypes.data, en.ctypes.data, seqs,
                                            rows.encode(), size, mx, resize, C.byref(ms), C.byref(n_out))
    else:
        p = load().gams_host_sw_multi_actions_timed(hs, len(engines), n, ids, chrs, st.ctypes.data, en.ctypes.data,
                                                    seqs, rows.encode(), size, mx, resize, mask, _rg_lines(rg_records),
                                                    C.byref(ms), C.byref(n_out))
    return _take_bytes(p, n_out).decode(), ms.value


def last_sw_index_ms():
    """ms the last sw_multi_timed with actions / rg_records of this thread spent building the rg index"""
    return float(load().gams_host_last_sw_index_ms())


def _check_rc(rc):
    if rc != 0:
        L = load()
        raise HostError(L.gams_host_last_code(), L.gams_host_last_error().decode(errors="replace"))


def count_multi(engines, group_off, starts, stops, q_group, qs, qe):
    """`locate --count` over several handles: groups split by LPT, queries routed to their group's device."""
    hs = (C.c_void_p * len(engines))(*[e.h.value for e in engines])
    group_off = np.ascontiguousarray(group_off, np.uint64)
    a = [np.ascontiguousarray(x, np.uint32) for x in (starts, stops, q_group, qs, qe)]
    out = np.zeros(a[2].size, np.int32)
    _check_rc(load().gams_host_count_multi(hs, len(engines), group_off.size - 1, group_off.ctypes.data,
                                           *[x.ctypes.data for x in a], a[2].size, out.ctypes.data))
    return out


def cover_multi(engines, group_off, lo, hi, q_group, clip_lo, clip_hi, qs, qe):
    """`anno` coverage over several handles (groups = chromosomes of the runlist set)."""
    hs = (C.c_void_p * len(engines))(*[e.h.value for e in engines])
    group_off = np.ascontiguousarray(group_off, np.uint64)
    lo, hi = np.ascontiguousarray(lo, np.int32), np.ascontiguousarray(hi, np.int32)
    q_group = np.ascontiguousarray(q_group, np.uint32)
    b = [np.ascontiguousarray(x, np.int32) for x in (clip_lo, clip_hi, qs, qe)]
    out = np.zeros(q_group.size, np.float32)
    _check_rc(load().gams_host_cover_multi(hs, len(engines), group_off.size - 1, group_off.ctypes.data, lo.ctypes.data,
                                           hi.ctypes.data, q_group.ctypes.data, *[x.ctypes.data for x in b],
                                           q_group.size, out.ctypes.data))
    return out


def merge_windows(windows, chr_start, size, step, coverage):
    """merge_ints (wave.rs:217-252) of ascending window indices: (component min, component max, has-an-edge)"""
    L = load()
    w = np.ascontiguousarray(windows, np.uint32)
    cmin, cmax = np.zeros(w.size, np.int64), np.zeros(w.size, np.int64)
    ing = np.zeros(w.size, np.int8)
    L.gams_host_merge_windows.restype = None
    L.gams_host_merge_windows.argtypes = [C.c_void_p, C.c_uint64, C.c_int32, C.c_int32, C.c_int32, C.c_float,
                                          C.c_void_p, C.c_void_p, C.c_void_p]
    L.gams_host_merge_windows(w.ctypes.data, w.size, chr_start, size, step, coverage, cmin.ctypes.data,
                              cmax.ctypes.data, ing.ctypes.data)
    return cmin, cmax, ing.astype(bool)


def ctg_json_roundtrip(json_text):
    """parse a `ctg:` JSON record (redis.rs:132-135) and write it back the way serde_json does (:127-130)"""
    L = load()
    L.gams_host_ctg_json_roundtrip.restype = C.c_void_p
    L.gams_host_ctg_json_roundtrip.argtypes = [C.c_char_p]
    return _take(L.gams_host_ctg_json_roundtrip(json_text.encode()))


def header(command):
    """the header line `gams wave` / `gams sw` print before the rows; "sw_gibbs": the sw header with the ΔG column"""
    return _take(load().gams_host_header({"wave": 0, "sw_gibbs": 2}.get(command, 1)))


def tsv_ctgs(ctgs):
    """`gams tsv -s "ctg:*"` for these ctgs (tsv.rs:31-71)."""
    n, ids, chrs, st, en = _ctg_arrays(ctgs)
    return _take(load().gams_host_tsv_ctgs(n, ids, chrs, st.ctypes.data, en.ctypes.data))


def loader_tsv(eng, ctgs, lines, tag=None):
    """`gams tsv -s "rg:*"` / `"feature:*"` of what the loaders would have stored."""
    n, ids, chrs, st, en = _ctg_arrays(ctgs)
    return _take(load().gams_host_loader_tsv(eng.h, n, ids, chrs, st.ctypes.data, en.ctypes.data,
                                             "\n".join(lines).encode(), tag.encode() if tag is not None else None))


def peak(eng, ctgs, lines):
    """`gams peak` over the rows of a wave TSV: TSV of the Peak fields (data.rs:30-43)."""
    n, ids, chrs, st, en = _ctg_arrays(ctgs)
    bufs = [np.ascontiguousarray(np.frombuffer(c["seq"], np.uint8) if not isinstance(c["seq"], np.ndarray)
                                 else c["seq"]) for c in ctgs]
    seqs = (C.c_void_p * max(n, 1))(*[b.ctypes.data for b in bufs])
    return _take(load().gams_host_peak(eng.h, n, ids, chrs, st.ctypes.data, en.ctypes.data, seqs,
                                       "\n".join(lines).encode()))


def peak_text(eng, ctgs, data, seqset=None):
    """`gams peak` over the bytes of a wave TSV, made on the device from the bytes to the rows (the host's passes where
    the device refuses): the rows of peak() with every ctg's peaks sorted by start, as bytes.  Without `seqset` the
    ctgs carry their bases in c["seq"], uploaded for the call; with a resident engine.SeqSet its slot i holds
    ctgs[i] (a ctg dict may name another in c["slot"]; None: no sequence)."""
    n, ids, chrs, st, en = _ctg_arrays(ctgs)
    out_len = C.c_uint64()
    if seqset is None:
        bufs = [np.ascontiguousarray(np.frombuffer(c["seq"], np.uint8) if not isinstance(c["seq"], np.ndarray)
                                     else c["seq"]) for c in ctgs]
        seqs = (C.c_void_p * max(n, 1))(*[b.ctypes.data for b in bufs])
        p = load().gams_host_peak_text(eng.h, n, ids, chrs, st.ctypes.data, en.ctypes.data, seqs, None, None, bytes(data),
                                       len(data), C.byref(out_len))
    else:
        slot = [c.get("slot", i) for i, c in enumerate(ctgs)]
        slots = np.array([0xffffffff if k is None else k for k in slot], np.uint32)
        p = load().gams_host_peak_text(eng.h, n, ids, chrs, st.ctypes.data, en.ctypes.data, None, seqset.p,
                                       slots.ctypes.data, bytes(data), len(data), C.byref(out_len))
    return _take_bytes(p, out_len)


def peak_records_text(eng, ctgs, data, fmt="records", serial_base=None, seqset=None):
    """What `gams peak` stores over the bytes of a wave TSV: the Peak record of every kept peak, written on the device (the
    host's passes where it refuses; last_operator_device says which), the ctgs in id order.  fmt: "tsv" (the rows of
    peak_text), "records" ("{id}\\t{json}\\n") or "resp" (resp_command(["SET", id, json]) of every record).  serial_base:
    {ctg id: cnt:peak:{ctg} before the load} (absent: 0); the serials of a ctg continue behind it.  ctgs and seqset as for
    peak_text.  -> (bytes, {ctg id: the counter after the load} for every ctg)"""
    if fmt not in LOADER_FORMATS:
        raise ValueError(f"peak_records_text: fmt is one of {list(LOADER_FORMATS)}")
    n, ids, chrs, st, en = _ctg_arrays(ctgs)
    base = np.array([(serial_base or {}).get(c["id"], 0) for c in ctgs], np.int32)
    nxt = np.zeros(max(n, 1), np.int32)
    out_len = C.c_uint64()
    if seqset is None:
        bufs = [np.ascontiguousarray(np.frombuffer(c["seq"], np.uint8) if not isinstance(c["seq"], np.ndarray)
                                     else c["seq"]) for c in ctgs]
        seqs, ss, slots = (C.c_void_p * max(n, 1))(*[b.ctypes.data for b in bufs]), None, None
    else:
        slot = [c.get("slot", i) for i, c in enumerate(ctgs)]
        slot = np.array([0xffffffff if k is None else k for k in slot], np.uint32)
        seqs, ss, slots = None, seqset.p, slot.ctypes.data
    p = load().gams_host_peak_records_text(eng.h, n, ids, chrs, st.ctypes.data, en.ctypes.data, seqs, ss, slots, bytes(data),
                                           len(data), LOADER_FORMATS[fmt], base.ctypes.data if n else None, nxt.ctypes.data,
                                           C.byref(out_len))
    return _take_bytes(p, out_len), {c["id"]: int(v) for c, v in zip(ctgs, nxt)}


def peak_rows_records(rows, fmt="records"):
    """The host formatter behind peak_records_text's host route, over rows peak_text printed (ids as they stand): the
    same records in fmt, as bytes."""
    if fmt not in LOADER_FORMATS:
        raise ValueError(f"peak_rows_records: fmt is one of {list(LOADER_FORMATS)}")
    out_len = C.c_uint64()
    return _take_bytes(load().gams_host_peak_rows_records(bytes(rows), len(rows), LOADER_FORMATS[fmt], C.byref(out_len)), out_len)


def sw_text(eng, ctgs, data, size=100, mx=20, resize=500, actions=("gc",), rg_records=(), rg_data=None, seqset=None):
    """`gams sw` over the bytes of a feature (range) file, made on the device from the bytes to the rows (the host's
    passes where the device refuses; last_operator_device says which): the features are the kept lines of every ctg in
    file order, "feature:{ctg_id}:{k}" from 1, as `gams feature` stores them; the rows of sw_multi over them, the ctgs
    in id order, as bytes.  Without `seqset` the ctgs carry their bases in c["seq"], uploaded for the call (not needed
    without the gc action); with a resident engine.SeqSet its slot i holds ctgs[i] (a ctg dict may name another in
    c["slot"]; None: no sequence).  actions, rg_records, rg_data as for sw_multi."""
    rg_data = _one_rg_source(rg_records, rg_data)
    mask = sw_actions(actions)
    n, ids, chrs, st, en = _ctg_arrays(ctgs)
    out_len = C.c_uint64()
    rg_lines = _rg_lines(rg_records) if (mask & _lib.SW_COUNT) and rg_data is None else None
    entry = load().gams_host_sw_text
    tail = (bytes(data), len(data), size, mx, resize, mask, rg_lines, rg_data, 0 if rg_data is None else len(rg_data),
            C.byref(out_len))
    if isinstance(rg_data, list):
        nr, rp, rl, _keep = _files(rg_data)
        entry = load().gams_host_sw_text_rgs
        tail = (bytes(data), len(data), size, mx, resize, mask, nr, rp, rl, C.byref(out_len))
    if seqset is None:
        seqs = None
        if mask & _lib.SW_GC:
            bufs = [np.ascontiguousarray(np.frombuffer(c["seq"], np.uint8) if not isinstance(c["seq"], np.ndarray)
                                         else c["seq"]) for c in ctgs]
            seqs = (C.c_void_p * max(n, 1))(*[b.ctypes.data for b in bufs])
        p = entry(eng.h, n, ids, chrs, st.ctypes.data, en.ctypes.data, seqs, None, None, *tail)
    else:
        slot = [c.get("slot", i) for i, c in enumerate(ctgs)]
        slots = np.array([0xffffffff if k is None else k for k in slot], np.uint32)
        p = entry(eng.h, n, ids, chrs, st.ctypes.data, en.ctypes.data, None, seqset.p, slots.ctypes.data, *tail)
    return _take_bytes(p, out_len)


_CTG_ID_ANNO = re.compile(r"ctg:[A-Za-z0-9_]+:[0-9]+", re.IGNORECASE)


def _sw_summary_call(eng, ctgs, data, tags, size, mx, resize, actions, rg_records, rg_data, seqset, anno=None):
    """-> (text, the distinct tags in byte order or None, the table's words as [slots, mx + 1, SW_SUMMARY_WORDS], the Prop
    sums as [slots, mx + 1, n_anno] or None without anno)"""
    cols = list(anno) if anno else []
    if len(cols) > _lib.SW_SUMMARY_MAX_ANNO:
        raise ValueError("sw_summary: at most %d span sets" % _lib.SW_SUMMARY_MAX_ANNO)
    if cols:
        for c in ctgs:                                         # utils.rs:118-129 must find the id whole in a row's id
            if not _CTG_ID_ANNO.fullmatch(c["id"]):
                raise ValueError("sw_summary: `gams anno` would not find the ctg id %r in its rows" % (c["id"],))
    owned = []
    try:
        sets = []
        for prefix, rl in cols:
            aset, own = _anno_set(eng, rl)
            if aset is None:
                raise ValueError("sw_summary: anno takes (prefix, AnnoSet or the bytes of the runlist JSON)")
            if own:
                owned.append(aset)
            sets.append(aset)
        prefixes = [p.encode("latin-1") if isinstance(p, str) else bytes(p) for p, _ in cols]
        if any(b"\0" in p for p in prefixes):
            raise ValueError("sw_summary: a prefix holds a NUL")
        return _sw_summary_call_sets(eng, ctgs, data, tags, size, mx, resize, actions, rg_records, rg_data, seqset,
                                     prefixes, sets, anno is not None)
    finally:
        for aset in owned:
            aset.close()


def _sw_summary_call_sets(eng, ctgs, data, tags, size, mx, resize, actions, rg_records, rg_data, seqset, prefixes, sets,
                          with_prop):
    rg_data = _one_rg_source(rg_records, rg_data)
    mask = sw_actions(actions)
    n, ids, chrs, st, en = _ctg_arrays(ctgs)
    datas = list(data) if isinstance(data, (list, tuple)) else [data]
    if tags is not None:
        if isinstance(tags, (str, bytes)) or len(tags) != len(datas):
            raise ValueError("sw_summary: tags is None or one tag per file")
        tags = [t.encode("latin-1") if isinstance(t, str) else bytes(t) for t in tags]
        if any(b"\0" in t for t in tags):
            raise ValueError("sw_summary: a tag holds a NUL")
    nf, fp, fl, _keep = _files(datas)
    tagp = None if tags is None else (C.c_char_p * max(nf, 1))(*tags)
    slots_of = None if tags is None else sorted(set(tags))
    rg_lines = _rg_lines(rg_records) if (mask & _lib.SW_COUNT) and rg_data is None else None
    nr, rp, rl, _keep_rg = _files(rg_data if isinstance(rg_data, list) else ([] if rg_data is None else [rg_data]))
    table = np.zeros((1 if tags is None else len(slots_of), mx + 1, _lib.SW_SUMMARY_WORDS), np.uint64)
    out_len = C.c_uint64()
    na = len(sets)
    prop = np.zeros((table.shape[0], mx + 1, na), np.uint64) if with_prop else None
    prep = (C.c_char_p * max(na, 1))(*prefixes)
    setp = (C.c_void_p * max(na, 1))(*[a.p for a in sets])
    tail = (nf, fp, fl, tagp, size, mx, resize, mask, rg_lines, nr, rp, rl, na, prep, setp, table.ctypes.data,
            prop.ctypes.data if na else None, C.byref(out_len))
    if seqset is None:
        seqs = None
        if mask & _lib.SW_GC:
            bufs = [np.ascontiguousarray(np.frombuffer(c["seq"], np.uint8) if not isinstance(c["seq"], np.ndarray)
                                         else c["seq"]) for c in ctgs]
            seqs = (C.c_void_p * max(n, 1))(*[b.ctypes.data for b in bufs])
        p = load().gams_host_sw_summary_anno(eng.h, n, ids, chrs, st.ctypes.data, en.ctypes.data, seqs, None, None, *tail)
    else:
        slot = [c.get("slot", i) for i, c in enumerate(ctgs)]
        slots = np.array([0xffffffff if k is None else k for k in slot], np.uint32)
        p = load().gams_host_sw_summary_anno(eng.h, n, ids, chrs, st.ctypes.data, en.ctypes.data, None, seqset.p,
                                             slots.ctypes.data, *tail)
    return _take_bytes(p, out_len), slots_of, table, prop


def _sw_summary_arrays(slots_of, table, prop=None):
    out = {"tags": slots_of, "count": table[:, :, 0].copy(), "sum": table[:, :, 1:5].copy(), "nan": table[:, :, 5:9].copy(),
           "rg_count": table[:, :, 9].copy()}
    if prop is not None:
        out["prop"] = prop
    return out


def sw_summary(eng, ctgs, data, tags=None, size=100, mx=20, resize=500, actions=("gc",), rg_records=(), rg_data=None,
               seqset=None, anno=None):
    """The table the rows of sw_text are loaded for (fsw-distance.tera.sql; with tags fsw-distance-tag.tera.sql), reduced
    on the device -- no row leaves it (the host's passes for a file the device refuses; last_operator_device says
    whether every file took the device's route).  data: one feature file's bytes or a list of them, each read as sw_text
    reads it (drop-first is per file); tags: None or one string per file.  Returns the text as bytes: a header, then one
    line per distance with rows -- per (tag, distance), ordered by tag bytes, then distance --: the averages of
    gc_content, gc_mean, gc_stddev and gc_cv (with the gc action), of rg_count (with count) and COUNT, the rows.  An
    average is the exact sum of the printed values over COUNT, rounded to 4 places, ties to even, trailing zeros dropped;
    `nan` where a row's value is NaN.  seqset, the per-ctg slot, actions, rg_records and rg_data as for sw_text.
    anno: None, or a list of up to four (prefix, AnnoSet | the bytes of a runlist JSON file; bytes build a set for the
    call): one column AVG_{prefix}Prop per set behind AVG_gc_cv -- what `gams anno set.json stdin -H` adds to every row
    before the table is made (fsw-distance-tag.tera.sql's cdsProp, repeatsProp), joined with the rows on the device.  The
    columns do not depend on the actions.  ValueError for a ctg id `gams anno` would not find whole in a row's id."""
    return _sw_summary_call(eng, ctgs, data, tags, size, mx, resize, actions, rg_records, rg_data, seqset, anno)[0]


def sw_summary_table(eng, ctgs, data, tags=None, size=100, mx=20, resize=500, actions=("gc",), rg_records=(), rg_data=None,
                     seqset=None, anno=None):
    """sw_summary's raw integers: {"tags": the distinct tags in byte order (None without tags), "count": [slots, mx + 1],
    "sum": [slots, mx + 1, 4] (the sums of m, a statistic being m / 10^4, for gc_content, gc_mean, gc_stddev, gc_cv),
    "nan": [slots, mx + 1, 4] (the rows whose statistic is NaN, left out of the sums), "rg_count": [slots, mx + 1]},
    uint64, one slot without tags; with anno (as for sw_summary) also "prop": [slots, mx + 1, n_anno], the sums of q, a
    row's prop being printed as q / 10^4"""
    _, slots_of, table, prop = _sw_summary_call(eng, ctgs, data, tags, size, mx, resize, actions, rg_records, rg_data, seqset,
                                                anno)
    return _sw_summary_arrays(slots_of, table, prop)


def sw_summarise_rows(rows, counts=None, mx=20, actions=("gc",), table=False, props=None, prefixes=None):
    """The host's summariser over rows of _lib.SW_ROW_DTYPE (and their rg counts, int32, with the count action): the text
    of sw_summary without tags, or with table=True the integers as sw_summary_table gives them.  props: None, or one
    column of Prop units per set (uint32, one entry per row, at most 10000), printed under prefixes.  No engine."""
    L = load()
    mask = sw_actions(actions)
    rows = np.ascontiguousarray(rows, _lib.SW_ROW_DTYPE)
    cnt = None if counts is None else np.ascontiguousarray(counts, np.int32)
    if cnt is not None and cnt.size != rows.size:
        raise ValueError("sw_summarise_rows: one count per row")
    words = np.zeros((1, mx + 1, _lib.SW_SUMMARY_WORDS), np.uint64)
    if props is None:
        if prefixes:
            raise ValueError("sw_summarise_rows: prefixes without props")
        _check_rc(L.gams_host_sw_summarise_rows(rows.ctypes.data, None if cnt is None else cnt.ctypes.data, rows.size, mx,
                                                mask, words.ctypes.data))
        if table:
            return _sw_summary_arrays(None, words)
        out_len = C.c_uint64()
        return _take_bytes(L.gams_host_sw_summary_text(words.ctypes.data, 1, None, mx, mask, C.byref(out_len)), out_len)
    cols = [np.ascontiguousarray(p, np.uint32) for p in props]
    if any(c.size != rows.size for c in cols) or len(prefixes or ()) != len(cols):
        raise ValueError("sw_summarise_rows: one unit per row in every column of props, one prefix per column")
    pre = [p.encode("latin-1") if isinstance(p, str) else bytes(p) for p in prefixes]
    colp = (C.c_void_p * max(len(cols), 1))(*[c.ctypes.data if c.size else None for c in cols])
    prep = (C.c_char_p * max(len(cols), 1))(*pre)
    prop = np.zeros((1, mx + 1, len(cols)), np.uint64)
    if not rows.size:                                          # (an empty column has no address to give)
        colp = (C.c_void_p * max(len(cols), 1))(*[prop.ctypes.data] * len(cols))
    _check_rc(L.gams_host_sw_summarise_rows_props(rows.ctypes.data, None if cnt is None else cnt.ctypes.data, rows.size, mx,
                                                  mask, words.ctypes.data, len(cols), colp, prop.ctypes.data))
    if table:
        return _sw_summary_arrays(None, words, prop)
    out_len = C.c_uint64()
    return _take_bytes(L.gams_host_sw_summary_text_props(words.ctypes.data, 1, None, mx, mask, len(cols), prep, prop.ctypes.data,
                                                         C.byref(out_len)), out_len)


def prop4_units(p):
    """The integer q of an anno prop in [0, 1]: `{:.4}` prints q / 10^4 (the expression the device shares between
    anno_text and the sw summary's Prop sums).  HostError (EINVAL) outside [0, 1]."""
    q = load().gams_host_prop4_units(p)
    _check_rc(0 if q >= 0 else -1)
    return int(q)


def fmt_f32_short(v):
    """`{}` of an f32 in [0, 1] as the device formats a peak amplitude ("" where it refuses: NaN, outside [0, 1])"""
    return _take(load().gams_host_fmt_f32_short(v))


def fmt_f32_json(v):
    """An f32 as serde_json prints it where that is positional: +0 and [1e-5, 1] (the text of fmt_f32_short, ".0" behind one
    without a point).  HostError for anything else (NaN, -0, below 1e-5, above 1)."""
    return _take(load().gams_host_fmt_f32_json(v))


def fmt_f32(v):
    return _take(load().gams_host_fmt_f32(v))


def range_roundtrip(s):
    return _take(load().gams_host_range_roundtrip(s.encode()))


# ---- wire formats either side of the path (gams_wire.cpp; SURVEY 8 f-3, parity unpinned) --------
def bincode_ctg_bundle(ctgs):
    """bundle:ctg:{chr}: bincode 1.3.3 of BTreeMap<String, Ctg> (redis.rs:216-233)"""
    n, ids, chrs, st, en = _ctg_arrays(ctgs)
    ln = C.c_uint64()
    return _take_bytes(load().gams_host_bincode_ctg_bundle(n, ids, chrs, st.ctypes.data, en.ctypes.data, C.byref(ln)), ln)


def bincode_ctg_bundle_decode(blob):
    """-> the ctg.tsv text of the decoded map"""
    return _take(load().gams_host_bincode_ctg_bundle_decode(blob, len(blob)))


def bincode_lapper(starts, stops, vals=None):
    """idx:ctg:{chr} / idx:rg:{ctg}: Lapper::new(ivs) serialised (redis.rs:236-324)"""
    a = np.ascontiguousarray(starts, np.uint32)
    b = np.ascontiguousarray(stops, np.uint32)
    vp = None
    if vals is not None:
        vp = (C.c_char_p * max(len(vals), 1))(*[v.encode() for v in vals])
    ln = C.c_uint64()
    return _take_bytes(load().gams_host_bincode_lapper(a.size, a.ctypes.data, b.ctypes.data, vp, C.byref(ln)), ln)


def bincode_lapper_decode(blob):
    return _take(load().gams_host_bincode_lapper_decode(blob, len(blob)))


def resp_command(args):
    raw = [a if isinstance(a, bytes) else str(a).encode() for a in args]
    ptrs = (C.c_char_p * max(len(raw), 1))(*raw)
    lens = (C.c_uint64 * max(len(raw), 1))(*[len(a) for a in raw])
    ln = C.c_uint64()
    return _take_bytes(load().gams_host_resp_command(len(raw), ptrs, lens, C.byref(ln)), ln)


def resp_scan_values(pattern):
    ln = C.c_uint64()
    return _take_bytes(load().gams_host_resp_scan_values(pattern.encode(), C.byref(ln)), ln)


def resp_parse(buf):
    """-> (flat text of the first reply in buf, bytes consumed); consumed == 0: the reply is incomplete"""
    used = C.c_uint64()
    p = load().gams_host_resp_parse(buf, len(buf), C.byref(used))
    if not p:
        raise HostError(load().gams_host_last_code(), load().gams_host_last_error().decode(errors="replace"))
    out = C.string_at(p).decode(errors="replace")
    load().gams_host_free(p)
    return out, used.value


def index_from_lappers(eng, blobs):
    """device index (gams_index_t*, as c_void_p) over idx: blobs, one group per blob; free with gams_index_destroy"""
    ptrs = (C.c_char_p * max(len(blobs), 1))(*blobs)
    lens = (C.c_uint64 * max(len(blobs), 1))(*[len(b) for b in blobs])
    p = load().gams_host_index_from_lappers(eng.h, len(blobs), ptrs, lens)
    if not p:
        raise HostError(load().gams_host_last_code(), load().gams_host_last_error().decode(errors="replace"))
    return C.c_void_p(p)
