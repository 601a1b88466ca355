"""ctypes binding of libfalcon_hip.so (the C ABI declared in include/falcon_hip.h).

There is no CPU fallback: if the shared library is missing, or no gfx950 device is
visible, every entry point raises.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libfalcon_hip.so")

FAL_DTYPE_F32, FAL_DTYPE_F16, FAL_DTYPE_SPLIT16, FAL_OUT_F32_F16, FAL_OUT_F16_IMAGE = 0, 1, 2, 3, 4
# fal_decode_peaks: array flags and per-spectrum status bits (include/falcon_hip.h)
PEAK_F64, PEAK_ZLIB, PEAK_BIG_ENDIAN, PEAK_PAIRS = 1, 2, 4, 8
PEAK_NUMPRESS_LINEAR, PEAK_NUMPRESS_PIC, PEAK_NUMPRESS_SLOF, PEAK_NUMPRESS_MASK = 16, 32, 48, 48      # a 2-bit codec field
PEAK_STATUS = {1: "bad descriptor", 2: "bad base64", 4: "bad zlib header", 8: "bad deflate stream", 16: "more values than declared",
               32: "fewer values than declared", 64: "Adler-32 mismatch", 128: "decode buffer too small",
               256: "bad MS-Numpress stream"}
# fal_mgf_index / fal_mgf_parse: flags of a text the host reader has to read, and the per-spectrum status (include/falcon_hip.h)
MGF_FLAG_BYTES, MGF_FLAG_LINES, MGF_ST_HOST = 1, 2, 1
# fal_mgf_parse_ex / fal_mgf_headers / fal_text_rows: the optional-key bit, the key table's limits, kinds and states, the widest row
MGF_OPT_TITLE, MGF_MAX_KEYS, MGF_MAX_KEY_BYTES, TEXT_MAX_WIDTH = 1, 16, 32, 256
MGF_KEY_SPAN, MGF_KEY_INT = 0, 1
MGF_KEY_ABSENT, MGF_KEY_PRESENT, MGF_KEY_HOST = 0, 1, 2
# fal_msp_parse: the per-entry status (its flags, key kinds and key states are the MGF reader's above)
MSP_ST_HOST = 1
# fal_mgf_write: the most bytes one number takes (csrc/mgfwrite.h kMgfNumMax)
MGF_NUM_MAX = 23
FAL_EINVAL = -1
# fal_network_edges: the most peaks of one side of a scored pair (include/falcon_hip.h FAL_NET_MAX_PEAKS)
NET_MAX_PEAKS = 4096
# fal_csv_*: the most bytes one number takes (csrc/csvwrite.h kCsvNumMax), the rows the merge sort's first pass sorts per block
CSV_NUM_MAX, CSV_SORT_BLOCK = 19, 1024
# fal_records_*: the most fields of a unit, the most bytes of its literals and the field kinds (include/falcon_hip.h FAL_REC_*)
REC_MAX_FIELDS, REC_MAX_LITERALS = 32, 4096
REC_KINDS = {"i32": 0, "i64": 1, "f32": 2, "text": 3}
# fal_mzml_index / fal_mzml_parse: the same for mzML text (include/falcon_hip.h)
MZML_FLAG_STRUCT, MZML_FLAG_MARKUP, MZML_FLAG_TAGS = 1, 2, 4
MZML_ST_OK, MZML_ST_SKIP, MZML_ST_HOST = 0, 1, 2
# fal_consensus_spectra: per-cluster status bits, and the pooled peaks one workgroup sorts in LDS (include/falcon_hip.h)
CONS_FALLBACK, CONS_GLOBAL, CONS_CAPACITY, CONS_LDS_PEAKS = 1, 2, 4, 4096
STAGES = {"vectorize": 0, "build": 1, "coarse": 2, "scan": 3, "select": 4, "filter": 5, "dbscan": 6, "tail": 7,
          "kernel": 8}     # the cosine kernel's own launches (subset of "scan")


class FalconHipError(RuntimeError):
    pass


_lib: Optional[C.CDLL] = None

c_void_p, c_int, c_int64, c_uint32, c_float, c_double = C.c_void_p, C.c_int, C.c_int64, C.c_uint32, C.c_float, C.c_double
P = C.POINTER


class RecField(C.Structure):
    """include/falcon_hip.h `fal_rec_field`: one field of a record writer's unit (pointers: device memory)"""
    _fields_ = [("column", c_void_p), ("ptr", c_void_p), ("index", c_void_p), ("rows", c_int64), ("blob_bytes", c_int64),
                ("kind", C.c_int32), ("prefix", C.c_int32 * 2), ("suffix", C.c_int32 * 2)]


_SIGNATURES = {
    "fal_version": ([], c_int),
    "fal_last_error": ([], C.c_char_p),
    "fal_device_count": ([P(c_int)], c_int),
    "fal_ctx_create": ([c_int, c_void_p, c_int, P(c_void_p)], c_int),
    "fal_ctx_destroy": ([c_void_p], c_int),
    "fal_ctx_sync": ([c_void_p], c_int),
    "fal_ctx_plan": ([c_void_p, c_int64, c_int, c_int, c_int, c_int64], c_int),
    "fal_ctx_trim": ([c_void_p], c_int),
    "fal_ctx_stage_ms": ([c_void_p, c_int, P(c_float), P(c_int64)], c_int),
    "fal_ctx_enable_timing": ([c_void_p, c_int], c_int),
    "fal_ctx_counter": ([c_void_p, c_int, P(c_int64)], c_int),
    "fal_get_dim": ([c_float, c_float, c_float, P(c_uint32), P(c_float), P(c_float)], c_int),
    "fal_hash_lookup": ([c_uint32, c_uint32, c_uint32, c_void_p], c_int),
    "fal_to_vector_indices": ([c_void_p, c_void_p, c_int64, c_double, c_double, c_void_p], c_int),
    "fal_vectorize": ([c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_double, c_double,
                       c_uint32, c_uint32, c_uint32, c_int, c_int, c_void_p], c_int),
    "fal_vectorize_pair": ([c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_double, c_double,
                            c_uint32, c_uint32, c_uint32, c_int, c_void_p, c_void_p], c_int),
    "fal_vectorize_f16_image": ([c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_double, c_double,
                                 c_uint32, c_uint32, c_uint32, c_int, c_void_p, c_void_p], c_int),
    "fal_row_width": ([c_uint32, P(c_uint32)], c_int),
    "fal_vectorize_rows": ([c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_double, c_double,
                            c_uint32, c_uint32, c_uint32, c_uint32, c_int, c_int, c_void_p, c_void_p], c_int),
    "fal_window_counts": ([c_void_p, c_void_p, c_void_p, c_int, c_double, c_int64, c_void_p, c_void_p], c_int),
    "fal_window_select": ([c_void_p, c_void_p, c_int64, c_double, c_int64, c_void_p, c_int, c_void_p, c_void_p, P(c_int64)], c_int),
    "fal_precursor_splits": ([c_void_p, c_void_p, c_int64, c_double, c_int, c_int64, c_double, c_int,
                              c_void_p, c_int64, P(c_int64)], c_int),
    "fal_ivf_build": ([c_void_p, c_void_p, c_int64, c_int, c_void_p, c_int64, c_void_p, c_int, P(c_void_p)], c_int),
    "fal_ivf_build_x16": ([c_void_p, c_void_p, c_void_p, c_int64, c_int, c_void_p, c_int64, c_void_p, c_int, P(c_void_p)], c_int),
    "fal_ivf_attach_f16": ([c_void_p, c_void_p, c_int], c_int),
    "fal_ivf_attach_prefilter": ([c_void_p, c_void_p], c_int),
    "fal_ivf_attach_prefilter_ex": ([c_void_p, c_void_p, c_int], c_int),
    "fal_ivf_destroy": ([c_void_p], c_int),
    "fal_ivf_total_lists": ([c_void_p, P(c_int64)], c_int),
    "fal_ivf_export": ([c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p], c_int),
    "fal_ivf_search_topk": ([c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p], c_int),
    "fal_filter_neighbors": ([c_void_p, c_void_p, c_void_p, c_int64, c_int, c_void_p, c_void_p, c_double, c_int,
                              c_double, c_int, c_void_p, c_void_p], c_int),
    "fal_ivf_search_neighbors": ([c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_double, c_int, c_double, c_int,
                                  c_void_p, c_void_p, c_void_p], c_int),
    "fal_process_spectra": ([c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_int, c_double,
                             c_double, c_double, c_double, c_double, c_int, c_int, c_void_p, c_void_p, c_void_p,
                             c_void_p], c_int),
    "fal_rescore_neighbors": ([c_void_p, c_void_p, c_void_p, c_int64, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_double,
                               c_int], c_int),
    "fal_neighbors_to_csr": ([c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int64, c_int64, c_void_p, c_void_p, c_void_p],
                             c_int),
    "fal_neighbors_to_csr_mapped": ([c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_void_p, c_int64, c_int64, c_void_p,
                                     c_void_p, c_void_p], c_int),
    "fal_dbscan": ([c_void_p, c_void_p, c_void_p, c_int64, c_int, c_float, c_void_p, P(c_int64)], c_int),
    "fal_refine_clusters": ([c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_double, c_int, c_double,
                             P(c_int64)], c_int),
    "fal_finalize": ([c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_int, c_void_p,
                      c_void_p, P(c_int64)], c_int),
    "fal_cluster_graph": ([c_void_p, c_void_p, c_void_p, c_int64, c_int, c_float, c_void_p, c_void_p, c_double, c_int,
                           c_double, c_void_p, c_void_p, c_void_p, c_void_p, P(c_int64), P(c_int64)], c_int),
    "fal_cluster_graph_counted": ([c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_float, c_void_p, c_void_p, c_double,
                                   c_int, c_double, c_void_p, c_void_p, c_void_p, c_void_p, P(c_int64), P(c_int64)], c_int),
    "fal_cluster_graph_tiled": ([c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_float, c_void_p, c_int64, c_void_p,
                                 c_void_p, c_double, c_int, c_double, c_void_p, c_void_p, c_void_p, c_void_p, P(c_int64),
                                 P(c_int64)], c_int),
    "fal_graph_tile_limits": ([P(c_int), P(c_int)], None),
    "fal_graph_tile_capacity": ([c_int64, c_int64, P(c_int64), P(c_int64)], None),
    "fal_cluster_graph_linkage": ([c_void_p, c_void_p, c_void_p, c_int64, c_int, c_float, c_int, c_void_p, c_void_p, c_double, c_int,
                                   c_double, c_void_p, c_void_p, c_void_p, c_void_p, P(c_int64), P(c_int64)], c_int),
    "fal_linkage_cluster": ([c_void_p, c_void_p, c_void_p, c_int64, c_int, c_float, c_int, c_void_p, P(c_int64)], c_int),
    "fal_exact_edges": ([c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_double, c_int, c_double,
                         c_void_p, c_void_p, c_void_p, c_int64, P(c_int64)], c_int),
    "fal_linkage_cluster_csr": ([c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_double, c_int, c_void_p, c_void_p, c_void_p,
                                 c_void_p, c_double, c_int, c_void_p, P(c_int64)], c_int),
    "fal_cluster_exact": ([c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_double, c_int, c_double,
                           c_int, c_void_p, c_void_p, c_double, c_int, c_double, c_void_p, c_void_p, c_void_p, P(c_int64),
                           P(c_int64)], c_int),
    "fal_sort_by_precursor": ([c_void_p, c_void_p, c_int64, c_void_p, c_void_p], c_int),
    "fal_gather_f32": ([c_void_p, c_void_p, c_void_p, c_int64, c_void_p], c_int),
    "fal_decode_peaks": ([c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p,
                          c_void_p, c_void_p], c_int),
    "fal_mgf_index": ([c_void_p, c_void_p, c_int64, P(c_int64)], c_int),
    "fal_mgf_parse": ([c_void_p, c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                       c_void_p, c_void_p, c_void_p, c_void_p], c_int),
    "fal_mgf_parse_ex": ([c_void_p, c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                          c_void_p, c_void_p, c_void_p, c_void_p, c_int], c_int),
    "fal_mgf_headers": ([c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p], c_int),
    "fal_text_rows": ([c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_int64, c_int64, c_int, c_void_p, c_void_p], c_int),
    "fal_msp_index": ([c_void_p, c_void_p, c_int64, P(c_int64)], c_int),
    "fal_msp_parse": ([c_void_p, c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                       c_void_p, c_void_p], c_int),
    "fal_msp_headers": ([c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p], c_int),
    "fal_mgf_write_sizes": ([c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_void_p,
                             c_void_p, c_void_p, c_int64, c_void_p, c_void_p, P(c_int64)], c_int),
    "fal_mgf_write": ([c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_void_p,
                       c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_int64, c_void_p, c_int64, c_void_p], c_int),
    "fal_csv_order": ([c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_void_p, P(c_int64)], c_int),
    "fal_csv_write_sizes": ([c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_int64,
                             c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_void_p, c_void_p, P(c_int64)], c_int),
    "fal_csv_write": ([c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_int64,
                       c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_void_p, c_int64, c_int64, c_void_p, c_int64,
                       c_void_p], c_int),
    "fal_records_write_sizes": ([c_void_p, c_int64, c_void_p, c_int, c_void_p, c_int64, c_int, c_int, c_int, c_int, c_void_p, c_void_p,
                                 P(c_int64)], c_int),
    "fal_records_write": ([c_void_p, c_int64, c_void_p, c_int, c_void_p, c_int64, c_int, c_int, c_int, c_int, c_void_p, c_int64, c_int64,
                           c_void_p, c_int64, c_void_p], c_int),
    "fal_mzml_index": ([c_void_p, c_void_p, c_int64, P(c_int64)], c_int),
    "fal_mzml_parse": ([c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                        c_void_p, c_void_p], c_int),
    "fal_consensus_spectra": ([c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_double, c_double,
                               c_int64, c_void_p, c_void_p, c_void_p, c_void_p], c_int),
    "fal_assign_nearest": ([c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p,
                            c_void_p, c_void_p, c_int64, c_double, c_int, c_double, c_double, c_int, c_void_p, c_void_p,
                            c_void_p], c_int),
    "fal_member_scores": ([c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64,
                           c_void_p, c_double, c_void_p, c_void_p], c_int),
    "fal_cluster_summary": ([c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                             c_void_p, c_void_p, c_void_p, c_void_p, c_void_p], c_int),
    "fal_network_edges": ([c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_double, c_double, c_double,
                           c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, P(c_int64)], c_int),
    "fal_network_families": ([c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int, c_double, c_void_p, c_void_p, c_void_p,
                              P(c_int64), P(c_int64)], c_int),
    "fal_network_propagate": ([c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_int, c_double, c_void_p, c_void_p,
                               c_void_p, c_void_p, P(c_int64), P(c_int64)], c_int),
    "fal_library_search": ([c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p,
                            c_int64, c_void_p, c_void_p, c_int64, c_double, c_double, c_int, c_int, c_double, c_double, c_int, c_int,
                            c_void_p, c_void_p, c_void_p, c_void_p, c_int64, P(c_int64)], c_int),
}


def load() -> C.CDLL:
    """Load the HIP library; raise loudly when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.isfile(LIB_PATH):
        raise FalconHipError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            f"(or `make -C falcon_amd/csrc`). falcon_amd has no CPU fallback.")
    # torch bundles its own libamdhip64.so.7 (same soname as /opt/rocm's).  Whichever is loaded
    # first serves the whole process, and a process that mixes the two HIP runtimes loses its
    # device; torch owns the device memory and streams we use, so its runtime goes first.
    import torch  # noqa: F401
    lib = C.CDLL(LIB_PATH)
    for name, (args, res) in _SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError if the .so is stale
        fn.argtypes = args
        fn.restype = res
    _lib = lib
    return lib


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = load().fal_last_error().decode("utf-8", "replace")
        raise FalconHipError(f"{what or 'libfalcon_hip'} failed with code {rc}: {msg}")


def exported_symbols():
    return list(_SIGNATURES)
