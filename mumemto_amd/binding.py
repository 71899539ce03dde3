"""ctypes binding of libmumemto.so (include/mumemto.h + include/mumemto_gpu.h)."""
import ctypes as C
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = os.path.join(_HERE, "lib", "libmumemto.so")
_lib = None


class MumemtoError(RuntimeError):
    pass


def library_path():
    return _LIB


class DocView(C.Structure):
    _fields_ = [("records", C.POINTER(C.c_char_p)), ("num_records", C.c_size_t)]


class MumView(C.Structure):
    _fields_ = [("length", C.c_uint32), ("offsets", C.POINTER(C.c_int64)), ("strands", C.POINTER(C.c_uint8))]


class MemView(C.Structure):
    _fields_ = [("length", C.c_uint32), ("occurrences", C.c_size_t), ("offsets", C.POINTER(C.c_int64)),
                ("seq_ids", C.POINTER(C.c_size_t)), ("strands", C.POINTER(C.c_uint8))]


class Params(C.Structure):
    """mmt_params (include/mumemto_gpu.h)."""
    _fields_ = [("min_match_len", C.c_uint32), ("num_distinct", C.c_uint64), ("max_doc_freq", C.c_int64),
                ("max_total_freq", C.c_int64), ("use_revcomp", C.c_uint8), ("merge_metadata", C.c_uint8)]


# mmt_doc_supplier (mumemto_gpu.h): int (*)(void* user, uint64_t doc, uint8_t* dst, uint64_t len)
DOC_SUPPLIER = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64)


class Partition(C.Structure):  # mmt_partition (mumemto_gpu.h); thresh_bits 0 / 16 / 32
    _fields_ = [("n_rows", C.c_uint64), ("n_docs", C.c_uint64), ("length", C.c_void_p), ("offsets", C.c_void_p),
                ("strands", C.c_void_p), ("thresh", C.c_void_p), ("thresh_len", C.c_uint64),
                ("thresh_on_device", C.c_uint8), ("rows_on_device", C.c_uint8), ("thresh_bits", C.c_uint8)]


class StringPart(C.Structure):  # mmt_string_part (mumemto_gpu.h): host tables of a partition of the string-based merge
    _fields_ = [("n_rows", C.c_uint64), ("n_docs", C.c_uint64), ("length", C.c_void_p), ("starts", C.c_void_p),
                ("strands", C.c_void_p), ("thresh", C.c_void_p), ("thresh_rev", C.c_void_p), ("thresh_len", C.c_uint64)]


class StringRecords(C.Structure):  # mmt_string_records (mumemto_gpu.h)
    _fields_ = [("n_collections", C.c_uint64), ("begin", C.c_void_p), ("length", C.c_void_p)]


class DevicePartition:
    """One partition's MUM rows and anchor thresholds as HBM addresses (what the multi-GPU exchange
    produces): length u32[n_rows], offsets i64[n_rows, n_docs], strands u8[n_rows, n_docs],
    thresh i16/u16[thresh_len].  `keepalive` holds whatever owns the memory."""

    def __init__(self, n_rows, n_docs, length_ptr, offsets_ptr, strands_ptr, thresh_ptr, thresh_len, keepalive=None,
                 thresh_bits=16):
        self.thresh_bits = int(thresh_bits)
        self.n_rows, self.n_docs = int(n_rows), int(n_docs)
        self.length_ptr, self.offsets_ptr, self.strands_ptr = int(length_ptr), int(offsets_ptr), int(strands_ptr)
        self.thresh_ptr, self.thresh_len = int(thresh_ptr), int(thresh_len)
        self.keepalive = keepalive


C_ABI_SYMBOLS = [
    "mumemto_last_error", "mumemto_mum", "mumemto_mem", "num_docs", "doc_record_offsets", "record_lengths",
    "num_mums", "mum_at", "mum_free", "num_docs_mem", "doc_record_offsets_mem", "record_lengths_mem", "num_mems",
    "mem_at", "mem_free",
]
GPU_ABI_SYMBOLS = [
    "mmt_last_error", "mmt_engine_create", "mmt_engine_destroy", "mmt_engine_set_input_device",
    "mmt_engine_set_input_host", "mmt_engine_run", "mmt_num_rows", "mmt_num_docs", "mmt_rows_mum", "mmt_num_occ",
    "mmt_rows_mem", "mmt_output_text", "mmt_output_bumbl", "mmt_thresh_len", "mmt_copy_thresh", "mmt_thresh_device",
    "mmt_text_length", "mmt_copy_text", "mmt_copy_sa", "mmt_copy_lcp", "mmt_copy_bwt", "mmt_num_candidates",
    "mmt_copy_candidates", "mmt_stage_ms", "mmt_column_bytes", "mmt_anchor_merge", "mmt_merged_rows",
    "mmt_merged_docs", "mmt_merged_get", "mmt_merged_sort_like_direct", "mmt_merged_text", "mmt_merged_free",
    "mmt_engine_set_producer", "mmt_abi_version", "mmt_engine_set_row_tap", "mmt_text_sink_digest", "mmt_kmer_in_share", "mmt_row_tap_counts", "mmt_row_tap_get", "mmt_kmer_positions", "mmt_producer_used", "mmt_producer_expanded", "mmt_producer_stats", "mmt_engine_parse_only", "mmt_pfp_counts", "mmt_pfp_run_refined", "mmt_pfp_copy_dict",
    "mmt_pfp_copy_parse", "mmt_pfp_stage_ms", "mmt_engine_run_partitioned", "mmt_partitions_used",
    "mmt_copy_merged_thresh", "mmt_rows_mum_device", "mmt_merged_device", "mmt_engine_set_text_host",
    "mmt_engine_set_stream_host", "mmt_is_wide", "mmt_scan_ranges", "mmt_copy_sa64", "mmt_engine_set_stream_host40",
    "mmt_device_memory", "mmt_engine_run_files", "mmt_anchor_merge_min_len", "mmt_pool_trim", "mmt_pool_set_reserve",
    "mmt_engine_set_scan_shard", "mmt_merged_from_rows", "mmt_anchor_merge_by_ranges", "mmt_dist_merge_ranges", "mmt_fold_slice_bounds", "mmt_comm_unique_id", "mmt_comm_create", "mmt_comm_destroy", "mmt_comm_loopback", "mmt_comm_selftest", "mmt_dist_merge",
    "mmt_dist_gather_text", "mmt_merged_write_text", "mmt_sort_pieces", "mmt_engine_keep_columns", "mmt_columns_kept",
    "mmt_comm_verify_stats", "mmt_exchange_digest", "mmt_exchange_digest_host", "mmt_stream_stats", "mmt_engine_release_columns", "mmt_copy_thresh32", "mmt_thresh_device32", "mmt_engine_set_text_sink",
    "mmt_engine_run_supplied", "mmt_merged_from_rows_device", "mmt_merged_collinear", "mmt_merged_blocks",
    "mmt_merged_blocks_device", "mmt_merged_collinear_stats", "mmt_merged_set_blocks", "mmt_merged_inversions",
    "mmt_merged_inversion_calls", "mmt_merged_inversion_calls_device", "mmt_merged_inversion_stats",
    "mmt_merged_coverage", "mmt_merged_coverage_runs", "mmt_merged_coverage_runs_device", "mmt_merged_coverage_stats",
    "mmt_merged_bed", "mmt_merged_bed_records", "mmt_merged_bed_records_device", "mmt_merged_bed_text",
    "mmt_merged_bed_write_text", "mmt_merged_bed_stats",
    "mmt_merged_label", "mmt_merged_label_cells", "mmt_merged_label_cells_device", "mmt_merged_label_text",
    "mmt_merged_label_write_text", "mmt_merged_label_stats",
    "mmt_string_fold", "mmt_merged_string_thresh", "mmt_merged_string_thresh_device", "mmt_merged_string_thresh_len",
    "mmt_merged_string_fold_stats",
    "mmt_density_create", "mmt_density_free", "mmt_density_add_rows", "mmt_density_add_engine", "mmt_density_finish",
    "mmt_density_shape", "mmt_density_bins", "mmt_density_bins_device", "mmt_density_stats",
]


def load_library():
    """Loads libmumemto.so; raises if it has not been built (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_LIB):
        raise MumemtoError("libmumemto.so is not built (%s): run `python -m mumemto_amd.build`; "
                           "mumemto_amd has no CPU fallback" % _LIB)
    if not os.environ.get("MUMEMTO_NO_TORCH"):
        # PyTorch-ROCm ships its own libamdhip64 under the same soname.  If torch is (or will be)
        # in this process it must be loaded first, so that both share ONE HIP runtime and device
        # pointers / streams can be exchanged; loading ours first leaves torch without devices.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
    L = C.CDLL(_LIB)
    L.mumemto_last_error.restype = C.c_char_p
    L.mmt_last_error.restype = C.c_char_p
    L.mumemto_mum.argtypes = [C.POINTER(DocView), C.c_size_t, C.c_uint32, C.c_uint8, C.c_size_t, C.c_uint8,
                              C.POINTER(C.c_void_p)]
    L.mumemto_mem.argtypes = [C.POINTER(DocView), C.c_size_t, C.c_uint32, C.c_uint8, C.c_size_t, C.c_size_t,
                              C.c_size_t, C.c_uint8, C.POINTER(C.c_void_p)]
    for f in ("num_docs", "num_mums", "num_docs_mem", "num_mems"):
        getattr(L, f).restype = C.c_size_t
        getattr(L, f).argtypes = [C.c_void_p]
    for f in ("doc_record_offsets", "record_lengths", "doc_record_offsets_mem", "record_lengths_mem"):
        getattr(L, f).restype = C.POINTER(C.c_size_t)
        getattr(L, f).argtypes = [C.c_void_p]
    L.mum_at.restype = MumView
    L.mum_at.argtypes = [C.c_void_p, C.c_size_t]
    L.mem_at.restype = MemView
    L.mem_at.argtypes = [C.c_void_p, C.c_size_t]
    L.mum_free.argtypes = [C.c_void_p]
    L.mem_free.argtypes = [C.c_void_p]

    L.mmt_engine_create.argtypes = [C.c_int, C.c_void_p, C.POINTER(C.c_void_p)]
    L.mmt_engine_destroy.argtypes = [C.c_void_p]
    L.mmt_engine_set_input_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    L.mmt_engine_set_input_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    L.mmt_engine_set_text_host.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_size_t, C.c_int]
    L.mmt_engine_set_stream_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p,
                                             C.c_size_t, C.c_int]
    L.mmt_engine_run.argtypes = [C.c_void_p, C.POINTER(Params)]
    for f in ("mmt_num_rows", "mmt_num_docs", "mmt_num_occ", "mmt_thresh_len", "mmt_num_candidates",
              "mmt_merged_rows", "mmt_merged_docs"):
        getattr(L, f).restype = C.c_size_t
        getattr(L, f).argtypes = [C.c_void_p]
    L.mmt_text_length.restype = C.c_uint64
    L.mmt_text_length.argtypes = [C.c_void_p]
    L.mmt_rows_mum.argtypes = [C.c_void_p] * 4
    L.mmt_rows_mem.argtypes = [C.c_void_p] * 6
    L.mmt_output_text.restype = C.c_void_p
    L.mmt_output_text.argtypes = [C.c_void_p, C.POINTER(C.c_size_t)]
    L.mmt_output_bumbl.restype = C.c_void_p
    L.mmt_output_bumbl.argtypes = [C.c_void_p, C.POINTER(C.c_size_t)]
    L.mmt_copy_thresh.argtypes = [C.c_void_p, C.c_void_p]
    L.mmt_thresh_device.restype = C.c_void_p
    L.mmt_thresh_device.argtypes = [C.c_void_p]
    for f in ("mmt_copy_text", "mmt_copy_sa", "mmt_copy_lcp", "mmt_copy_bwt", "mmt_copy_candidates"):
        getattr(L, f).argtypes = [C.c_void_p, C.c_void_p]
    L.mmt_copy_sa64.argtypes = [C.c_void_p, C.c_void_p]
    L.mmt_is_wide.argtypes = [C.c_void_p]
    L.mmt_scan_ranges.restype = C.c_size_t
    L.mmt_scan_ranges.argtypes = [C.c_void_p]
    L.mmt_device_memory.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    L.mmt_engine_set_stream_host40.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64,
                                               C.c_void_p, C.c_size_t, C.c_int]
    L.mmt_stage_ms.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
    L.mmt_column_bytes.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
    L.mmt_engine_set_producer.argtypes = [C.c_void_p, C.c_int, C.c_uint32, C.c_uint32]
    L.mmt_producer_used.argtypes = [C.c_void_p]
    L.mmt_producer_expanded.argtypes = [C.c_void_p]
    L.mmt_producer_stats.argtypes = [C.c_void_p, C.c_void_p]
    L.mmt_text_sink_digest.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    L.mmt_kmer_in_share.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    L.mmt_engine_set_row_tap.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t]
    L.mmt_row_tap_counts.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    L.mmt_row_tap_get.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.mmt_kmer_positions.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.c_uint64,
                                     C.POINTER(C.c_uint64)]
    L.mmt_engine_parse_only.argtypes = [C.c_void_p, C.c_uint8, C.c_uint32, C.c_uint32]
    L.mmt_pfp_counts.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    L.mmt_pool_set_reserve.argtypes = [C.c_ulonglong]
    L.mmt_pool_set_reserve.restype = None
    L.mmt_pfp_run_refined.argtypes = [C.c_void_p]
    L.mmt_pfp_run_refined.restype = C.c_longlong
    L.mmt_pfp_copy_dict.argtypes = [C.c_void_p, C.c_void_p]
    L.mmt_pfp_copy_parse.argtypes = [C.c_void_p, C.c_void_p]
    L.mmt_pfp_stage_ms.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
    L.mmt_engine_run_supplied.argtypes = [C.c_void_p, DOC_SUPPLIER, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(Params)]
    L.mmt_engine_run_partitioned.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(Params),
                                             C.c_uint64]
    L.mmt_engine_run_files.argtypes = [C.c_void_p, C.POINTER(C.c_char_p), C.c_size_t, C.POINTER(Params), C.c_char_p,
                                       C.c_uint64, C.POINTER(C.c_double)]
    L.mmt_merged_from_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p,
                                       C.c_size_t, C.POINTER(C.c_void_p)]
    L.mmt_merged_from_rows_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t,
                                              C.POINTER(C.c_void_p)]
    L.mmt_merged_collinear.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_int64, C.POINTER(C.c_uint64)]
    L.mmt_merged_blocks.argtypes = [C.c_void_p, C.c_void_p]
    L.mmt_merged_blocks_device.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
    L.mmt_merged_collinear_stats.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
    L.mmt_merged_set_blocks.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]
    L.mmt_merged_inversions.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_uint64)]
    L.mmt_merged_inversion_calls.argtypes = [C.c_void_p, C.c_void_p]
    L.mmt_merged_inversion_calls_device.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    L.mmt_merged_inversion_stats.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
    L.mmt_merged_coverage.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]
    L.mmt_merged_coverage_runs.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.mmt_merged_coverage_runs_device.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
    L.mmt_merged_coverage_stats.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
    L.mmt_merged_bed.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64,
                                 C.POINTER(C.c_uint64)]
    L.mmt_merged_bed_records.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.mmt_merged_bed_records_device.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
    L.mmt_merged_bed_text.restype = C.c_void_p
    L.mmt_merged_bed_text.argtypes = [C.c_void_p, C.c_int64, C.POINTER(C.c_size_t)]
    L.mmt_merged_bed_write_text.argtypes = [C.c_void_p, C.c_int64, C.c_char_p]
    L.mmt_merged_bed_stats.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
    L.mmt_merged_label.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                   C.POINTER(C.c_uint64)]
    L.mmt_merged_label_cells.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.mmt_merged_label_cells_device.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
    L.mmt_merged_label_text.restype = C.c_void_p
    L.mmt_merged_label_text.argtypes = [C.c_void_p, C.POINTER(C.c_size_t)]
    L.mmt_merged_label_write_text.argtypes = [C.c_void_p, C.c_char_p]
    L.mmt_merged_label_stats.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
    L.mmt_merged_sequences.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.POINTER(C.c_uint64)]
    L.mmt_engine_text_packed.argtypes = [C.c_void_p]
    L.mmt_merged_sequences_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int64, C.c_int, C.c_int,
                                            C.POINTER(C.c_uint64)]
    L.mmt_merged_sequences_file.argtypes = [C.c_void_p, C.c_void_p, C.c_char_p, C.c_int64, C.c_int, C.c_int,
                                            C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.mmt_merged_sequences_offsets.argtypes = [C.c_void_p, C.c_void_p]
    L.mmt_merged_sequences_offsets_device.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    L.mmt_merged_sequences_text.restype = C.c_void_p
    L.mmt_merged_sequences_text.argtypes = [C.c_void_p, C.POINTER(C.c_size_t)]
    L.mmt_merged_sequences_write_text.argtypes = [C.c_void_p, C.c_char_p]
    L.mmt_merged_sequences_stats.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
    L.mmt_string_fold.argtypes = [C.c_void_p, C.POINTER(StringPart), C.c_size_t, C.POINTER(StringPart), C.POINTER(StringRecords),
                                  C.POINTER(C.c_void_p)]
    L.mmt_merged_string_thresh_len.restype = C.c_uint64
    L.mmt_merged_string_thresh_len.argtypes = [C.c_void_p]
    L.mmt_merged_string_thresh.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.mmt_merged_string_thresh_device.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
    L.mmt_merged_string_fold_stats.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
    L.mmt_density_create.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint64, C.POINTER(C.c_void_p)]
    L.mmt_density_free.argtypes = [C.c_void_p]
    L.mmt_density_free.restype = None
    L.mmt_density_add_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    L.mmt_density_add_engine.argtypes = [C.c_void_p, C.c_void_p]
    L.mmt_density_finish.argtypes = [C.c_void_p]
    L.mmt_density_shape.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    L.mmt_density_bins.argtypes = [C.c_void_p, C.c_void_p]
    L.mmt_density_bins_device.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    L.mmt_density_stats.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
    L.mmt_comm_unique_id.argtypes = [C.c_void_p]
    L.mmt_comm_create.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_void_p)]
    L.mmt_comm_destroy.argtypes = [C.c_void_p]
    L.mmt_comm_loopback.argtypes = [C.c_void_p, C.c_void_p]
    L.mmt_comm_selftest.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p]
    L.mmt_comm_verify_stats.argtypes = [C.c_void_p, C.c_void_p]
    L.mmt_exchange_digest.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint64, C.c_void_p]
    L.mmt_exchange_digest_host.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint64, C.c_void_p]
    L.mmt_dist_merge.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p)]
    L.mmt_dist_gather_text.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
    L.mmt_partitions_used.restype = C.c_size_t
    L.mmt_partitions_used.argtypes = [C.c_void_p]
    L.mmt_copy_merged_thresh.argtypes = [C.c_void_p, C.c_void_p]
    L.mmt_anchor_merge.argtypes = [C.c_void_p, C.POINTER(Partition), C.c_size_t, C.POINTER(C.c_void_p)]
    L.mmt_anchor_merge_by_ranges.argtypes = [C.c_void_p, C.POINTER(Partition), C.c_size_t, C.c_int, C.c_uint32,
                                             C.POINTER(C.c_void_p)]
    L.mmt_dist_merge_ranges.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p)]
    L.mmt_fold_slice_bounds.argtypes = [C.c_uint64, C.c_int, C.c_int, C.c_size_t, C.c_uint32, C.POINTER(C.c_uint64)]
    L.mmt_anchor_merge_min_len.argtypes = [C.c_void_p, C.POINTER(Partition), C.c_size_t, C.c_uint32,
                                           C.POINTER(C.c_void_p)]
    L.mmt_merged_get.argtypes = [C.c_void_p] * 5
    L.mmt_merged_device.argtypes = [C.c_void_p] + [C.POINTER(C.c_void_p)] * 4
    L.mmt_rows_mum_device.argtypes = [C.c_void_p] + [C.POINTER(C.c_void_p)] * 3
    L.mmt_merged_sort_like_direct.argtypes = [C.c_void_p, C.c_void_p]
    L.mmt_merged_write_text.argtypes = [C.c_void_p, C.c_char_p]
    L.mmt_engine_keep_columns.argtypes = [C.c_void_p, C.c_int]
    L.mmt_columns_kept.argtypes = [C.c_void_p]
    L.mmt_stream_stats.argtypes = [C.c_void_p, C.c_void_p]
    L.mmt_sort_pieces.restype = C.c_size_t
    L.mmt_sort_pieces.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    L.mmt_merged_text.restype = C.c_void_p
    L.mmt_merged_text.argtypes = [C.c_void_p, C.POINTER(C.c_size_t)]
    L.mmt_merged_free.argtypes = [C.c_void_p]
    L.mmt_engine_release_columns.argtypes = [C.c_void_p, C.c_int]
    L.mmt_engine_set_text_sink.argtypes = [C.c_void_p, C.c_char_p]
    L.mmt_copy_thresh32.argtypes = [C.c_void_p, C.c_void_p]
    L.mmt_thresh_device32.restype = C.c_void_p
    L.mmt_thresh_device32.argtypes = [C.c_void_p]
    _lib = L
    return L


def _bytes_at(ptr, n):
    """n bytes at ptr as `bytes`; ctypes.string_at takes a C int, a MEM-mode output can exceed 2 GiB"""
    if not n:
        return b""
    step = 1 << 30
    if n <= step:
        return C.string_at(ptr, n)
    base = C.cast(ptr, C.c_void_p).value
    return b"".join(C.string_at(base + o, min(step, n - o)) for o in range(0, n, step))


def _check(rc, gpu=True):
    if rc != 0:
        L = load_library()
        msg = (L.mmt_last_error() if gpu else L.mumemto_last_error()) or b""
        raise MumemtoError("libmumemto rc=%d: %s" % (rc, msg.decode(errors="replace")))


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _doc_views(sequences):
    views = (DocView * max(len(sequences), 1))()
    keep = []
    for i, doc in enumerate(sequences):
        recs = [r if isinstance(r, bytes) else r.encode() for r in doc]
        arr = (C.c_char_p * max(len(recs), 1))(*recs)
        keep.append(arr)
        views[i].records = arr
        views[i].num_records = len(recs)
    return views, keep


# ---- drop-in API (mirror of mumemto_library/mumemto_api.hpp:29-57) --------------
def mumemto_mum(sequences, min_match_len=20, use_revcomp=True, num_distinct=0, use_gsacak=False):
    """Multi-MUMs of `sequences` (list of docs, each a list of record strings).
    Returns dict(lengths=u32[n], offsets=i64[n,N] (-1 absent), strands=u8[n,N] (1='+'),
    record_lengths=list of per-doc record lengths) -- through the C ABI of mumemto.h."""
    L = load_library()
    views, keep = _doc_views(sequences)
    out = C.c_void_p()
    rc = L.mumemto_mum(views, len(sequences), min_match_len, int(bool(use_revcomp)), num_distinct,
                       int(bool(use_gsacak)), C.byref(out))
    _check(rc, gpu=False)
    try:
        n, N = L.num_mums(out), L.num_docs(out)
        lengths = np.zeros(n, np.uint32)
        offsets = np.zeros((n, N), np.int64)
        strands = np.zeros((n, N), np.uint8)
        for i in range(n):
            v = L.mum_at(out, i)
            lengths[i] = v.length
            offsets[i] = np.ctypeslib.as_array(v.offsets, shape=(N,))
            strands[i] = np.ctypeslib.as_array(v.strands, shape=(N,))
        dro = L.doc_record_offsets(out)
        rl = L.record_lengths(out)
        rec = [[rl[k] for k in range(dro[d], dro[d + 1])] for d in range(N)]
        return dict(lengths=lengths, offsets=offsets, strands=strands, record_lengths=rec)
    finally:
        L.mum_free(out)


def mumemto_mem(sequences, min_match_len=20, use_revcomp=True, num_distinct=0, max_total_freq=0, max_doc_freq=2,
                use_gsacak=False):
    """Multi-MEMs; returns a list of dict(length, offsets, seq_ids, strands) + record_lengths."""
    L = load_library()
    views, keep = _doc_views(sequences)
    out = C.c_void_p()
    rc = L.mumemto_mem(views, len(sequences), min_match_len, int(bool(use_revcomp)), num_distinct, max_total_freq,
                       max_doc_freq, int(bool(use_gsacak)), C.byref(out))
    _check(rc, gpu=False)
    try:
        n, N = L.num_mems(out), L.num_docs_mem(out)
        mems = []
        for i in range(n):
            v = L.mem_at(out, i)
            k = v.occurrences
            mems.append(dict(length=int(v.length),
                             offsets=np.ctypeslib.as_array(v.offsets, shape=(k,)).copy(),
                             seq_ids=np.ctypeslib.as_array(v.seq_ids, shape=(k,)).astype(np.int64),
                             strands=np.ctypeslib.as_array(v.strands, shape=(k,)).copy()))
        dro = L.doc_record_offsets_mem(out)
        rl = L.record_lengths_mem(out)
        rec = [[rl[k] for k in range(dro[d], dro[d + 1])] for d in range(N)]
        return dict(mems=mems, record_lengths=rec)
    finally:
        L.mem_free(out)


# ---- device-resident engine ----------------------------------------------------------
class Engine:
    """One GPU's hot path (include/mumemto_gpu.h)."""

    def __init__(self, device=0, stream=None):
        self.L = load_library()
        h = C.c_void_p()
        _check(self.L.mmt_engine_create(device, C.c_void_p(stream) if stream else None, C.byref(h)))
        self.h = h
        self.device = device
        self._keep = None

    def close(self):
        if getattr(self, "h", None):
            self.L.mmt_engine_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_docs(self, docs):
        """docs: list of docs, each a list of record bytes (host memory)."""
        lens = np.array([sum(len(r) for r in d) for d in docs], dtype=np.uint64)
        flat = b"".join(b"".join(d) for d in docs)
        bases = np.frombuffer(flat, dtype=np.uint8) if flat else np.zeros(1, np.uint8)
        _check(self.L.mmt_engine_set_input_host(self.h, _p(bases), _p(lens), len(docs)))

    def set_input_device(self, dev_ptr, doc_len, keepalive=None):
        """dev_ptr: address of the concatenated bases in HBM (e.g. tensor.data_ptr())."""
        lens = np.ascontiguousarray(doc_len, dtype=np.uint64)
        self._keep = keepalive
        _check(self.L.mmt_engine_set_input_device(self.h, C.c_void_p(dev_ptr), _p(lens), len(lens)))

    def set_text(self, text, doc_len, use_revcomp=True):
        """Hand over the text T itself (bytes; UPPER(F) '$' [revcomp '$'] per document): the `-p` checkpoint."""
        t = np.frombuffer(bytes(text), np.uint8) if len(text) else np.zeros(1, np.uint8)
        lens = np.ascontiguousarray(doc_len, np.uint64)
        _check(self.L.mmt_engine_set_text_host(self.h, _p(t), C.c_uint64(len(text)), _p(lens), len(lens), int(use_revcomp)))

    def set_stream(self, sa, lcp, bwt, doc_len, use_revcomp=True):
        """Hand over SA / LCP / BWT of the real suffixes (possibly a prefix of the stream): the `-a` checkpoint."""
        sa = np.ascontiguousarray(sa, np.uint32); lcp = np.ascontiguousarray(lcp, np.uint32)
        bwt = np.ascontiguousarray(bwt, np.uint8); lens = np.ascontiguousarray(doc_len, np.uint64)
        _check(self.L.mmt_engine_set_stream_host(self.h, _p(sa), _p(lcp), _p(bwt), C.c_uint64(len(sa)), _p(lens), len(lens),
                                                 int(use_revcomp)))

    def set_stream40(self, sa, lcp, bwt, doc_len, use_revcomp=True):
        """set_stream for suffix-array entries of up to 40 bits (sa: int64), over a text of any length."""
        sa = np.ascontiguousarray(sa, np.uint64)
        if len(sa) and int(sa.max()) >> 40:
            raise ValueError("suffix-array entry beyond 40 bits")
        lo = np.ascontiguousarray(sa & 0xffffffff, np.uint32)
        hi = np.ascontiguousarray(sa >> 32, np.uint8)
        lcp = np.ascontiguousarray(lcp, np.uint32)
        bwt = np.ascontiguousarray(bwt, np.uint8); lens = np.ascontiguousarray(doc_len, np.uint64)
        _check(self.L.mmt_engine_set_stream_host40(self.h, _p(lo), _p(hi), _p(lcp), _p(bwt), C.c_uint64(len(lo)), _p(lens),
                                                   len(lens), int(use_revcomp)))

    def run(self, min_match_len=20, num_distinct=0, max_doc_freq=1, max_total_freq=0, use_revcomp=True,
            merge_metadata=False):
        p = Params(min_match_len, num_distinct, max_doc_freq, max_total_freq, int(use_revcomp), int(merge_metadata))
        _check(self.L.mmt_engine_run(self.h, C.byref(p)))

    def run_partitioned(self, docs, max_text_chars=0, min_match_len=20, use_revcomp=True, num_distinct=0,
                        max_doc_freq=1, max_total_freq=0, flat=None, merge_metadata=False):
        """Host-resident docs of any size: one suffix array when the text fits the device (40-bit positions beyond
        2^32 characters), otherwise anchor partitions + merge (strict multi-MUMs only).  `flat` = (uint8 array of
        the concatenated bases, uint64 array of document lengths) skips the Python-side concatenation."""
        if flat is not None:
            bases, lens = flat
            lens = np.ascontiguousarray(lens, dtype=np.uint64)
        else:
            lens = np.array([sum(len(r) for r in d) for d in docs], dtype=np.uint64)
            joined = b"".join(b"".join(d) for d in docs)
            bases = np.frombuffer(joined, dtype=np.uint8) if joined else np.zeros(1, np.uint8)
        p = Params(min_match_len, num_distinct, max_doc_freq, max_total_freq, int(use_revcomp), int(merge_metadata))
        _check(self.L.mmt_engine_run_partitioned(self.h, _p(bases), _p(lens), len(lens), C.byref(p), max_text_chars))
        return int(self.L.mmt_partitions_used(self.h))

    def run_supplied(self, lens, supplier, min_match_len=20, use_revcomp=True, num_distinct=0, max_doc_freq=1,
                     max_total_freq=0, merge_metadata=False):
        """The documents supplied one at a time: `supplier(d, dst)` writes the bases of document d into the uint8 array dst
        (len = lens[d], page-locked memory of the engine).  For collections that do not fit the host as bytes; always one
        text (mmt_engine_run_supplied)."""
        lens = np.ascontiguousarray(lens, dtype=np.uint64)
        failure = []

        def _fill(_user, d, dst, n):
            try:
                supplier(int(d), np.ctypeslib.as_array(C.cast(dst, C.POINTER(C.c_uint8)), shape=(int(n),)))
                return 0
            except BaseException as exc:                       # (an exception must not unwind through the C frames)
                failure.append(exc)
                return 1
        cb = DOC_SUPPLIER(_fill)
        p = Params(min_match_len, num_distinct, max_doc_freq, max_total_freq, int(use_revcomp), int(merge_metadata))
        rc = self.L.mmt_engine_run_supplied(self.h, cb, None, _p(lens), len(lens), C.byref(p))
        if failure:
            raise failure[0]
        _check(rc)
        return 1

    def run_files(self, paths, out_prefix=None, min_match_len=20, num_distinct=0, max_doc_freq=1, max_total_freq=0,
                  use_revcomp=True, merge_metadata=False, max_text_chars=0):
        """FASTA files (one document each) -> PREFIX.mums | .mems + PREFIX.lengths, in-process: the unit of work of
        the reference's build_main.  Returns {"read", "run", "write", "total"} seconds."""
        arr = (C.c_char_p * len(paths))(*[os.fsencode(p) for p in paths])
        p = Params(min_match_len, num_distinct, max_doc_freq, max_total_freq, int(use_revcomp), int(merge_metadata))
        sec = (C.c_double * 4)()
        _check(self.L.mmt_engine_run_files(self.h, arr, len(paths), C.byref(p),
                                           os.fsencode(out_prefix) if out_prefix else None, max_text_chars, sec))
        return dict(zip(["read", "run", "write", "total"], map(float, sec)))

    def set_text_sink(self, path):
        """PREFIX.mums / .mems of the next runs straight to `path` while a run goes on (None: off).  A run over a text that fills
        the device keeps nothing else of its rows (mumemto_gpu.h)."""
        _check(self.L.mmt_engine_set_text_sink(self.h, os.fsencode(path) if path else None))

    def release_columns(self, keep_anchor_ranks=False):
        """Text, windows and sort scratch of the last run back to the device heap; keep_anchor_ranks: rows folded later can
        still be put into direct-run order (anchor_merge(sort_like_direct=True))."""
        _check(self.L.mmt_engine_release_columns(self.h, int(keep_anchor_ranks)))

    def merged_thresholds(self, anchor_len):
        out = np.zeros(anchor_len + 1, np.uint16)
        _check(self.L.mmt_copy_merged_thresh(self.h, _p(out)))
        return out

    def set_producer(self, kind="auto", w=0, p=0):
        """kind: 'auto' | 'direct' (reference -g path) | 'pfp' (reference default path) | 'guided' (the parse without the
        suffix array of its dictionary: collections with little redundancy, chosen automatically when needed)."""
        _check(self.L.mmt_engine_set_producer(self.h, {"auto": 0, "direct": 1, "pfp": 2, "guided": 3, "expand": 4}[kind], w, p))

    def producer_used(self):
        return {1: "direct", 2: "pfp", 3: "guided"}.get(self.L.mmt_producer_used(self.h), "?")

    def text_sink_digest(self):
        """(bytes, digest) of what the last run's text sink wrote (sink "/dev/null", or MMT_SINK_DIGEST set)"""
        out = (C.c_uint64 * 2)()
        _check(self.L.mmt_text_sink_digest(self.h, out))
        return int(out[0]), int(out[1])

    def kmer_in_share(self, kmer):
        """True when the suffixes beginning with kmer belong to the share of the stream the last (sharded, bucket-wise) run produced"""
        km = np.frombuffer(bytes(kmer), np.uint8).copy()
        r = self.L.mmt_kmer_in_share(self.h, _p(km), len(km))
        if r < 0:
            raise MumemtoError("the bucket-wise producer did not run")
        return bool(r)

    def set_row_tap(self, kmers, max_rows=1 << 16, max_occ=1 << 24):
        """kmers: list of equal-length byte strings (<= 16 characters), or [] to switch the tap off: the next runs copy every
        accepted interval whose match begins with one of them (length + all its text positions) before its window goes"""
        kmers = [bytes(k) for k in kmers]
        k = len(kmers[0]) if kmers else 0
        assert all(len(x) == k for x in kmers)
        flat = np.frombuffer(b"".join(kmers), np.uint8).copy() if kmers else np.zeros(1, np.uint8)
        _check(self.L.mmt_engine_set_row_tap(self.h, _p(flat), len(kmers), k, max_rows, max_occ))

    def row_tap(self):
        """(length[rows], occ_start[rows + 1], sa[entries]) of the rows the last run tapped, in no particular order"""
        c = (C.c_uint64 * 2)()
        _check(self.L.mmt_row_tap_counts(self.h, c))
        rows, occ = int(c[0]), int(c[1])
        length = np.zeros(max(rows, 1), np.uint32); start = np.zeros(rows + 1, np.uint64); sa = np.zeros(max(occ, 1), np.uint64)
        _check(self.L.mmt_row_tap_get(self.h, _p(length), _p(start), _p(sa)))
        return length[:rows], start, sa[:occ]

    def kmer_positions(self, kmers, cap=1 << 22):
        """(positions ascending, index of the k-mer each begins with) over the text resident on the device"""
        kmers = [bytes(k) for k in kmers]
        k = len(kmers[0])
        flat = np.frombuffer(b"".join(kmers), np.uint8).copy()
        pos = np.zeros(cap, np.uint64); which = np.zeros(cap, np.uint32)
        found = C.c_uint64(0)
        _check(self.L.mmt_kmer_positions(self.h, _p(flat), len(kmers), k, _p(pos), _p(which), cap, C.byref(found)))
        if found.value > cap:
            raise MumemtoError("%d positions begin with those k-mers: more than the %d asked for" % (found.value, cap))
        return pos[:found.value], which[:found.value]

    def producer_stats(self):
        """bucket-wise producer, last run: slices of run bins (assembly gaps), passes over the text, batches, staged"""
        out = (C.c_uint64 * 4)()
        _check(self.L.mmt_producer_stats(self.h, out))
        return {"run_slices": int(out[0]), "text_passes": int(out[1]), "batches": int(out[2]), "staged": bool(out[3])}

    def producer_expanded(self):
        """the bucket-wise producer sorted one representative per (distinct phrase, offset) and the emitter expanded them"""
        return bool(self.L.mmt_producer_expanded(self.h))

    def parse_only(self, use_revcomp=True, w=10, p=100):
        """Text layout + prefix-free parse; returns (dict bytes, parse u32[]) as the reference's -P writes them."""
        _check(self.L.mmt_engine_parse_only(self.h, int(use_revcomp), w, p))
        c = self.pfp_counts()
        d = np.zeros(max(c["dict_len"], 1), np.uint8)
        q = np.zeros(max(c["phrases"], 1), np.uint32)
        _check(self.L.mmt_pfp_copy_dict(self.h, _p(d)))
        _check(self.L.mmt_pfp_copy_parse(self.h, _p(q)))
        return d[: c["dict_len"]].tobytes(), q[: c["phrases"]]

    def pfp_counts(self):
        out = (C.c_uint64 * 8)()
        _check(self.L.mmt_pfp_counts(self.h, out))
        d = dict(zip(["phrases", "distinct", "dict_len", "groups", "rounds_dict", "rounds_parse", "entries",
                      "oversized_groups"], map(int, out)))
        d["run_refined"] = int(self.L.mmt_pfp_run_refined(self.h))
        return d

    def pfp_stage_ms(self):
        out = (C.c_float * 8)()
        _check(self.L.mmt_pfp_stage_ms(self.h, out))
        return list(out)

    # results
    def output_text(self):
        n = C.c_size_t()
        ptr = self.L.mmt_output_text(self.h, C.byref(n))
        return _bytes_at(ptr, n.value)

    def output_size(self):
        """Bytes of the last run's .mums / .mems output; brings them into page-locked host memory (no Python copy)."""
        n = C.c_size_t()
        self.L.mmt_output_text(self.h, C.byref(n))
        return n.value

    def output_bumbl(self):
        n = C.c_size_t()
        ptr = self.L.mmt_output_bumbl(self.h, C.byref(n))
        return _bytes_at(ptr, n.value)

    def rows_mum(self):
        n, N = self.L.mmt_num_rows(self.h), self.L.mmt_num_docs(self.h)
        length = np.zeros(max(n, 1), np.uint32)
        off = np.zeros((max(n, 1), N), np.int64)
        st = np.zeros((max(n, 1), N), np.uint8)
        _check(self.L.mmt_rows_mum(self.h, _p(length), _p(off), _p(st)))
        return length[:n], off[:n], st[:n]

    def rows_mum_device(self):
        """(n_rows, n_docs, length_ptr, offsets_ptr, strands_ptr): the MUM rows of the last run in HBM,
        valid until the next run."""
        a, b, c = C.c_void_p(), C.c_void_p(), C.c_void_p()
        _check(self.L.mmt_rows_mum_device(self.h, C.byref(a), C.byref(b), C.byref(c)))
        return (self.L.mmt_num_rows(self.h), self.L.mmt_num_docs(self.h), a.value or 0, b.value or 0, c.value or 0)

    def rows_mem(self):
        n, t = self.L.mmt_num_rows(self.h), self.L.mmt_num_occ(self.h)
        length = np.zeros(max(n, 1), np.uint32)
        occ = np.zeros(n + 1, np.uint64)
        off = np.zeros(max(t, 1), np.int64)
        ids = np.zeros(max(t, 1), np.uint64)
        st = np.zeros(max(t, 1), np.uint8)
        _check(self.L.mmt_rows_mem(self.h, _p(length), _p(occ), _p(off), _p(ids), _p(st)))
        return length[:n], occ, off[:t], ids[:t], st[:t]

    def thresholds(self):
        n = self.L.mmt_thresh_len(self.h)
        out = np.zeros(max(n, 1), np.uint16)
        if n:
            _check(self.L.mmt_copy_thresh(self.h, _p(out)))
        return out[:n]

    def thresholds32(self):
        """The engine's own threshold column: 32 bits, never saturated (what the fold and the exchange carry)."""
        n = self.L.mmt_thresh_len(self.h)
        out = np.zeros(max(n, 1), np.uint32)
        if n:
            _check(self.L.mmt_copy_thresh32(self.h, _p(out)))
        return out[:n]

    def thresh_device_ptr(self):
        """16-bit form (saturated at 65535 like PREFIX.athresh), made from the 32-bit column on the first call."""
        return self.L.mmt_thresh_device(self.h)

    def thresh_device_ptr32(self):
        return self.L.mmt_thresh_device32(self.h)

    # stage introspection
    def text_length(self):
        return int(self.L.mmt_text_length(self.h))

    def _copy(self, fn, dtype):
        n = self.text_length()
        out = np.zeros(max(n, 1), dtype)
        _check(fn(self.h, _p(out)))
        return out[:n]

    def text(self):
        return self._copy(self.L.mmt_copy_text, np.uint8)

    def sa(self):
        """Suffix array of the last run (uint32 for narrow runs, uint64 when positions need 40 bits)."""
        if self.is_wide():
            return self._copy(self.L.mmt_copy_sa64, np.uint64)
        return self._copy(self.L.mmt_copy_sa, np.uint32)

    def set_scan_shard(self, index, count):
        """This engine produces, scans and drops share `index` of `count` of the stream (multi-GPU runs of the modes
        without a partition merge); the ranks' outputs concatenate to the single-GPU output."""
        _check(self.L.mmt_engine_set_scan_shard(self.h, C.c_uint32(index), C.c_uint32(count)))

    def keep_columns(self, on=True):
        """The columns of the stream exist one window at a time; on=True also copies every window into whole columns, so
        that sa() / lcp() / bwt() work after the run (default: only for texts below 2^26 characters)."""
        _check(self.L.mmt_engine_keep_columns(self.h, C.c_int(1 if on is True else (0 if on is False else int(on)))))

    def columns_kept(self):
        return bool(self.L.mmt_columns_kept(self.h))

    def stream_stats(self):
        """Of the last run: entries of the stream this engine produced, high-water mark of its window buffers (bytes),
        windows, bytes of the suffix-array entries kept with accepted rows."""
        out = (C.c_uint64 * 4)()
        _check(self.L.mmt_stream_stats(self.h, out))
        return {"entries": int(out[0]), "window_bytes": int(out[1]), "windows": int(out[2]), "row_entry_bytes": int(out[3])}

    def sort_pieces(self):
        """[(first suffix-array entry, number of entries)] per rank of the last (sharded) run."""
        k = self.L.mmt_sort_pieces(self.h, None, None, 0)
        first, count = np.zeros(max(k, 1), np.uint64), np.zeros(max(k, 1), np.uint64)
        self.L.mmt_sort_pieces(self.h, _p(first), _p(count), k)
        return [(int(first[i]), int(count[i])) for i in range(k)]

    def is_wide(self):
        return bool(self.L.mmt_is_wide(self.h))

    def scan_ranges(self):
        return int(self.L.mmt_scan_ranges(self.h))

    def device_memory(self):
        """Device heap of this engine's GPU: bytes mapped, live, peak, and seconds spent mapping."""
        out = (C.c_uint64 * 4)()
        _check(self.L.mmt_device_memory(self.h, out))
        return {"mapped": int(out[0]), "live": int(out[1]), "peak": int(out[2]), "map_seconds": out[3] / 1e6}

    def lcp(self):
        return self._copy(self.L.mmt_copy_lcp, np.uint32)

    def bwt(self):
        return self._copy(self.L.mmt_copy_bwt, np.uint8)

    def candidates(self):
        n = self.L.mmt_num_candidates(self.h)
        out = np.zeros((max(n, 1), 4), np.uint32)
        if n:
            _check(self.L.mmt_copy_candidates(self.h, _p(out)))
        return out[:n]

    def stage_ms(self):
        out = (C.c_float * 8)()
        _check(self.L.mmt_stage_ms(self.h, out))
        return list(out)

    def column_bytes(self):
        out = (C.c_uint32 * 3)()
        _check(self.L.mmt_column_bytes(self.h, out))
        return list(out)

    # anchor merge
    def anchor_merge(self, parts, sort_like_direct=False, want_rows=True, min_len=20, text_file=None, slices=0, want_text=True):
        """parts: list of DevicePartition, or of (length u32[n], offsets i64[n,nd], strands u8[n,nd], thresh)
        where thresh is a numpy u16 array (host) or a device address paired as (ptr, length).
        want_rows=False returns only the PREFIX.mums bytes (no D2H of the tables); text_file: the library writes them
        there itself and the result carries no "text"."""
        arr = (Partition * len(parts))()
        keep = []
        for i, part in enumerate(parts):
            if isinstance(part, DevicePartition):
                arr[i] = Partition(part.n_rows, part.n_docs, part.length_ptr, part.offsets_ptr, part.strands_ptr,
                                   part.thresh_ptr, part.thresh_len, 1, 1, part.thresh_bits)
                keep.append(part)
                continue
            length, off, st, th = part
            length = np.ascontiguousarray(length, np.uint32)
            off = np.ascontiguousarray(off, np.int64)
            st = np.ascontiguousarray(st, np.uint8)
            if off.ndim != 2:
                off, st = off.reshape(len(length), -1), st.reshape(len(length), -1)
            if isinstance(th, tuple):       # (device address, entries[, bits])
                tptr, tlen, on_dev = th[0], th[1], 1
                bits = th[2] if len(th) > 2 else 16
            else:                           # uint16: the PREFIX.athresh width; uint32: the engine's own (thresholds32)
                bits = 32 if getattr(th, "dtype", None) == np.uint32 else 16
                th = np.ascontiguousarray(th, np.uint32 if bits == 32 else np.uint16)
                tptr, tlen, on_dev = _p(th).value, len(th), 0
            keep += [length, off, st, th]
            arr[i] = Partition(len(length), off.shape[1], _p(length).value, _p(off).value, _p(st).value, tptr, tlen,
                               on_dev, 0, bits)
        m = C.c_void_p()
        if slices:      # the same table as `slices` independent slices of the anchor (what `slices` ranks fold at once)
            _check(self.L.mmt_anchor_merge_by_ranges(self.h, arr, len(parts), int(slices), C.c_uint32(min_len), C.byref(m)))
        else:
            _check(self.L.mmt_anchor_merge_min_len(self.h, arr, len(parts), C.c_uint32(min_len), C.byref(m)))
        try:
            if sort_like_direct:
                _check(self.L.mmt_merged_sort_like_direct(self.h, m))
            n, nd = self.L.mmt_merged_rows(m), self.L.mmt_merged_docs(m)
            if text_file is not None:
                _check(self.L.mmt_merged_write_text(m, os.fsencode(text_file)))
                text = None
            elif not want_text:
                text = None
            else:
                k = C.c_size_t()
                ptr = self.L.mmt_merged_text(m, C.byref(k))
                if not ptr and n:
                    raise MumemtoError(self.L.mmt_last_error().decode())
                text = _bytes_at(ptr, k.value)
            if not want_rows:
                return dict(text=text, n_rows=n, n_docs=nd)
            length = np.zeros(max(n, 1), np.uint32)
            off = np.zeros((max(n, 1), nd), np.int64)
            st = np.zeros((max(n, 1), nd), np.uint8)
            th = np.zeros(int(arr[0].thresh_len), np.uint16)
            _check(self.L.mmt_merged_get(m, _p(length), _p(off), _p(st), _p(th)))
            return dict(lengths=length[:n], offsets=off[:n], strands=st[:n], thresh=th, text=text, n_rows=n, n_docs=nd)
        finally:
            self.L.mmt_merged_free(m)


def _engine_rows_in_direct_order(self, length, offsets, strands, thresh=None):
    """Rows folded elsewhere (mumemto_amd.dist.fold_by_ranges) -> re-sorted into the order of a direct run by this
    engine's anchor suffix ranks -> PREFIX.mums bytes."""
    length = np.ascontiguousarray(length, np.uint32)
    offsets = np.ascontiguousarray(offsets, np.int64).reshape(len(length), -1)
    strands = np.ascontiguousarray(strands, np.uint8).reshape(len(length), -1)
    th = np.ascontiguousarray(thresh, np.uint16) if thresh is not None else np.zeros(1, np.uint16)
    m = C.c_void_p()
    _check(self.L.mmt_merged_from_rows(self.h, _p(length), _p(offsets), _p(strands), len(length), offsets.shape[1], _p(th),
                                       len(th) if thresh is not None else 0, C.byref(m)))
    try:
        _check(self.L.mmt_merged_sort_like_direct(self.h, m))
        k = C.c_size_t()
        ptr = self.L.mmt_merged_text(m, C.byref(k))
        if not ptr and len(length):
            raise MumemtoError(self.L.mmt_last_error().decode())
        return _bytes_at(ptr, k.value)
    finally:
        self.L.mmt_merged_free(m)


Engine.rows_in_direct_order = _engine_rows_in_direct_order


class Merged:
    """A row table in the HBM of an engine's GPU (mmt_merged of mumemto_gpu.h): the result of a fold, or rows handed over
    with Merged.from_rows / Merged.from_device.  collinear() computes the collinear blocks of its rows on the device,
    inversions() the inversion calls over them, coverage() the share of every sequence its rows cover, bed() the blocks and
    rows as BED intervals in contig coordinates, label() every start as (contig, offset inside it), sequences() the rows' bases
    as a multi-FASTA."""

    def __init__(self, engine, handle):
        self.engine, self.L, self.h = engine, engine.L, handle

    @classmethod
    def from_rows(cls, engine, lengths, starts, strands):
        """host arrays: lengths u32 [n], starts i64 [n, N] (-1 = absent), strands bool / u8 [n, N] (1 = '+')"""
        lengths = np.ascontiguousarray(lengths, np.uint32)
        starts = np.ascontiguousarray(starts, np.int64)
        if starts.ndim != 2:
            starts = starts.reshape(len(lengths), -1)
        strands = np.ascontiguousarray(np.asarray(strands).astype(np.uint8)).reshape(starts.shape)
        m = C.c_void_p()
        _check(engine.L.mmt_merged_from_rows(engine.h, _p(lengths), _p(starts), _p(strands), len(lengths), starts.shape[1],
                                             None, 0, C.byref(m)))
        return cls(engine, m)

    @classmethod
    def from_device(cls, engine, n_rows, n_docs, length_ptr, offsets_ptr, strands_ptr):
        """tables already in the engine's HBM, e.g. Merged.from_device(eng, *eng.rows_mum_device()); they are copied"""
        m = C.c_void_p()
        _check(engine.L.mmt_merged_from_rows_device(engine.h, C.c_void_p(length_ptr), C.c_void_p(offsets_ptr),
                                                    C.c_void_p(strands_ptr), int(n_rows), int(n_docs), C.byref(m)))
        return cls(engine, m)

    @classmethod
    def from_partitions(cls, engine, parts, min_len=20):
        """the anchor fold of partitions, kept as a handle (Engine.anchor_merge copies the result out and frees it): parts are
        DevicePartition objects or (length u32 [n], offsets i64 [n, nd], strands u8 [n, nd], thresh u16 / u32) host tuples"""
        arr = (Partition * len(parts))()
        keep = []
        for i, part in enumerate(parts):
            if isinstance(part, DevicePartition):
                arr[i] = Partition(part.n_rows, part.n_docs, part.length_ptr, part.offsets_ptr, part.strands_ptr,
                                   part.thresh_ptr, part.thresh_len, 1, 1, part.thresh_bits)
                continue
            length = np.ascontiguousarray(part[0], np.uint32)
            off = np.ascontiguousarray(part[1], np.int64).reshape(len(length), -1)
            st = np.ascontiguousarray(part[2], np.uint8).reshape(off.shape)
            bits = 32 if part[3].dtype == np.uint32 else 16
            th = np.ascontiguousarray(part[3], np.uint32 if bits == 32 else np.uint16)
            keep += [length, off, st, th]
            arr[i] = Partition(len(length), off.shape[1], _p(length).value, _p(off).value, _p(st).value, _p(th).value,
                               len(th), 0, 0, bits)
        m = C.c_void_p()
        _check(engine.L.mmt_anchor_merge_min_len(engine.h, arr, len(parts), C.c_uint32(min_len), C.byref(m)))
        return cls(engine, m)

    @classmethod
    def string_fold(cls, engine, parts, mom, mom_records):
        """the last step of the string-based merge on the device, with the inputs of merge_mums.string_merge: parts = per
        partition (lengths u32 [n], starts i64 [n, c], strands [n, c], thresh u16 [T], thresh_rev u16 [T]), rows in the order
        of their first column; mom = (lengths, starts [m, S], strands [m, S]) of the MUMs of MUMs; mom_records = per
        collection the record lengths of mom's .lengths file.  The handle carries the merged rows and string_thresh()."""
        keep = []

        def table(rows, thresh=None, thresh_rev=None):
            length = np.ascontiguousarray(rows[0], np.uint32)
            starts = np.ascontiguousarray(rows[1], np.int64)
            if starts.ndim != 2:
                starts = starts.reshape(len(length), -1)
            strands = np.ascontiguousarray(np.asarray(rows[2]).astype(np.uint8)).reshape(starts.shape)
            th = np.ascontiguousarray(thresh if thresh is not None else [], np.uint16)
            th_rev = np.ascontiguousarray(thresh_rev if thresh_rev is not None else [], np.uint16)
            if len(th) != len(th_rev):
                raise MumemtoError("string fold: thresh and thresh_rev of a partition differ in length (%d, %d)" % (len(th), len(th_rev)))
            keep.extend([length, starts, strands, th, th_rev])
            return StringPart(len(length), starts.shape[1], _p(length).value, _p(starts).value, _p(strands).value, _p(th).value,
                              _p(th_rev).value, len(th))

        arr = (StringPart * max(len(parts), 1))()
        for i, part in enumerate(parts):
            arr[i] = table(part[:3], part[3], part[4])
        mom_part = table(mom)
        begin = np.zeros(len(mom_records) + 1, np.uint64)
        begin[1:] = np.cumsum([len(r) for r in mom_records], dtype=np.uint64)
        flat = np.ascontiguousarray(np.concatenate([np.asarray(r, np.int64).ravel() for r in mom_records] + [np.zeros(1, np.int64)]))
        records = StringRecords(len(mom_records), _p(begin).value, _p(flat).value)
        m = C.c_void_p()
        _check(engine.L.mmt_string_fold(engine.h, arr, len(parts), C.byref(mom_part), C.byref(records), C.byref(m)))
        return cls(engine, m)

    def string_thresh(self):
        """(thresh u16, thresh_rev u16) of a string_fold: the positions of the rows in their order, a 0 behind every row"""
        n = int(self.L.mmt_merged_string_thresh_len(self.h))
        th, th_rev = np.zeros(max(n, 1), np.uint16), np.zeros(max(n, 1), np.uint16)
        _check(self.L.mmt_merged_string_thresh(self.h, _p(th), _p(th_rev)))
        return th[:n], th_rev[:n]

    def string_thresh_device(self):
        """(HBM address of thresh, of thresh_rev, entries of either); owned by the handle"""
        a, b = C.c_void_p(), C.c_void_p()
        _check(self.L.mmt_merged_string_thresh_device(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value, int(self.L.mmt_merged_string_thresh_len(self.h))

    def string_fold_stats(self):
        st = (C.c_double * 8)()
        _check(self.L.mmt_merged_string_fold_stats(self.h, st))
        d = {k: float(st[i]) for i, k in enumerate(["split_ms", "locate_ms", "assemble_ms", "thresholds_ms"])}
        d.update(pieces=int(st[4]), dropped_short=int(st[5]), dropped_thresh=int(st[6]), rows=int(st[7]))
        return d

    def close(self):
        if getattr(self, "h", None):
            self.L.mmt_merged_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def n_rows(self):
        return int(self.L.mmt_merged_rows(self.h))

    @property
    def n_docs(self):
        return int(self.L.mmt_merged_docs(self.h))

    def rows(self):
        """(lengths u32 [n], starts i64 [n, N], strands u8 [n, N]) copied to the host"""
        n, nd = self.n_rows, self.n_docs
        length = np.zeros(max(n, 1), np.uint32)
        off = np.zeros((max(n, 1), nd), np.int64)
        st = np.zeros((max(n, 1), nd), np.uint8)
        _check(self.L.mmt_merged_get(self.h, _p(length), _p(off), _p(st), None))
        return length[:n], off[:n], st[:n]

    def collinear(self, max_break=1000, min_singleton_length=None):
        """Collinear blocks as the reference's `mumemto collinear` finds them: (n_blocks, 2) uint32, first and last row of
        every block.  The table becomes the filtered (no partial rows), sorted (by column 0) one the rows refer to, and
        text() / write_text() carry the block of every row as a fourth field from here on."""
        k = C.c_uint64()
        single = -1 if min_singleton_length is None else int(min_singleton_length)
        _check(self.L.mmt_merged_collinear(self.engine.h, self.h, C.c_uint32(int(max_break)), C.c_int64(single), C.byref(k)))
        return self.blocks()

    def blocks(self):
        st = (C.c_double * 12)()
        _check(self.L.mmt_merged_collinear_stats(self.h, st))
        lr = np.zeros((int(st[11]), 2), np.uint32)
        _check(self.L.mmt_merged_blocks(self.h, _p(lr) if len(lr) else None))
        return lr

    def blocks_device(self):
        """(address of the u32 [n_blocks, 2] block list, address of the u32 [n_rows] block of every row) in HBM"""
        a, b = C.c_void_p(), C.c_void_p()
        _check(self.L.mmt_merged_blocks_device(self.h, C.byref(a), C.byref(b)))
        return a.value or 0, b.value or 0

    def collinear_stats(self):
        st = (C.c_double * 12)()
        _check(self.L.mmt_merged_collinear_stats(self.h, st))
        names = ["filter_sort_ms", "extract_ms", "sort_ms", "adjacency_ms", "blocks_ms"]
        d = {k: float(st[i]) for i, k in enumerate(names)}
        d.update(rows_in=int(st[5]), rows_kept=int(st[6]), cols_sorted=int(st[7]), cols_ascending=int(st[8]),
                 batches=int(st[9]), table_sorted=bool(st[10]), n_blocks=int(st[11]))
        return d

    def set_blocks(self, blocks):
        """Attach a block list read from a file, (n_blocks, 2) first and last rows, as if collinear() had found it.  The table
        must hold full rows only, in ascending order of column 0; a list that is not ascending and disjoint is refused."""
        lr = np.ascontiguousarray(blocks, np.uint32).reshape(-1, 2)
        _check(self.L.mmt_merged_set_blocks(self.engine.h, self.h, _p(lr) if len(lr) else None, len(lr)))

    def inversions(self, max_length=None):
        """Inversion calls as the reference's `mumemto inversion` finds them, over the blocks of collinear() or set_blocks():
        int64 [k, 5] = (column, start, end, ref_start, ref_end) in ascending order of (column, position of the run)."""
        k = C.c_uint64()
        limit = -1 if max_length is None else int(max_length)
        _check(self.L.mmt_merged_inversions(self.engine.h, self.h, C.c_int64(limit), C.byref(k)))
        calls = np.zeros((int(k.value), 5), np.int64)
        _check(self.L.mmt_merged_inversion_calls(self.h, _p(calls) if len(calls) else None))
        return calls

    def inversion_calls_device(self):
        """address of the int64 [n_calls, 5] calls in HBM"""
        a = C.c_void_p()
        _check(self.L.mmt_merged_inversion_calls_device(self.h, C.byref(a)))
        return a.value or 0

    def inversion_stats(self):
        st = (C.c_double * 8)()
        _check(self.L.mmt_merged_inversion_stats(self.h, st))
        d = {k: float(st[i]) for i, k in enumerate(["gather_ms", "sort_ms", "runs_ms"])}
        d.update(n_blocks=int(st[3]), cols_sorted=int(st[4]), cols_ascending=int(st[5]), runs=int(st[6]), calls=int(st[7]))
        return d

    def coverage(self, seq_lengths, seq_idx=None, min_length=0):
        """Positions of every sequence covered by the multi-MUMs of the table, as the reference's `mumemto coverage` counts
        them: uint64 [n_docs].  seq_lengths: the length of every sequence; seq_idx: one column (the others stay 0), None:
        all of them; min_length: rows shorter than this take no part.  The table is only read."""
        lens = np.ascontiguousarray(seq_lengths, np.int64).reshape(-1)
        if len(lens) != self.n_docs:
            raise MumemtoError("coverage: %d sequence lengths for a table of %d columns" % (len(lens), self.n_docs))
        covered = np.zeros(self.n_docs, np.uint64)
        idx = -1 if seq_idx is None else int(seq_idx)
        if seq_idx is not None and idx < 0:
            idx = -2                                        # (-1 means "all" to the library; a negative index is refused there)
        _check(self.L.mmt_merged_coverage(self.engine.h, self.h, _p(lens) if len(lens) else None, C.c_int64(idx),
                                          C.c_int64(int(min_length)), _p(covered) if len(covered) else None))
        return covered

    def coverage_runs(self):
        """(run_begin uint64 [n_docs + 1], runs int64 [n, 2]) of the last coverage(): the maximal covered stretches of column
        c, half-open (begin, end) and ascending, are runs[run_begin[c]:run_begin[c + 1]]"""
        run_begin = np.zeros(self.n_docs + 1, np.uint64)
        _check(self.L.mmt_merged_coverage_runs(self.h, _p(run_begin), None))
        runs = np.zeros((int(run_begin[-1]), 2), np.int64)
        if len(runs):
            _check(self.L.mmt_merged_coverage_runs(self.h, None, _p(runs)))
        return run_begin, runs

    def coverage_runs_device(self):
        """(address of the u64 [n_docs + 1] run offsets, address of the int64 [n, 2] runs) in HBM"""
        a, b = C.c_void_p(), C.c_void_p()
        _check(self.L.mmt_merged_coverage_runs_device(self.h, C.byref(a), C.byref(b)))
        return a.value or 0, b.value or 0

    def coverage_stats(self):
        st = (C.c_double * 8)()
        _check(self.L.mmt_merged_coverage_stats(self.h, st))
        d = {k: float(st[i]) for i, k in enumerate(["extract_ms", "sort_ms", "scan_ms", "runs_ms"])}
        d.update(cols_sorted=int(st[4]), cols_ascending=int(st[5]), batches=int(st[6]), runs=int(st[7]))
        return d

    def bed(self, contigs, seq_idx=None, min_singleton_length=100):
        """BED records of the table as the reference's `mumemto bed` makes them, with the departures of mum_to_bed.py's
        docstring: one per collinear block and per free row of at least min_singleton_length (every such row with a start in
        the column when no blocks are attached).  contigs: (names, lengths), each one list per sequence in file order, as
        mumsio.read_contigs returns them; seq_idx: one column, None: all of them.  Returns the number of records; the table
        is only read."""
        begin, lens, name_begin, blob = contig_tables(contigs)
        if len(begin) != self.n_docs + 1:
            raise MumemtoError("bed: contigs of %d sequences for a table of %d columns" % (len(begin) - 1, self.n_docs))
        idx = -1 if seq_idx is None else int(seq_idx)
        if seq_idx is not None and idx < 0:
            idx = -2                                        # (-1 means "all" to the library; a negative index is refused there)
        k = C.c_uint64()
        names = np.frombuffer(blob, np.uint8) if blob else np.zeros(1, np.uint8)
        _check(self.L.mmt_merged_bed(self.engine.h, self.h, _p(begin), _p(lens), _p(name_begin), _p(names), C.c_int64(idx),
                                     C.c_int64(int(min_singleton_length)), C.byref(k)))
        return int(k.value)

    def bed_records(self):
        """(record_begin uint64 [n_docs + 1], records int64 [n, 5]) of the last bed(): the records of column c are
        records[record_begin[c]:record_begin[c + 1]] = (contig within the column, rel_start, rel_end, name, strand), name =
        the block, or -1 - i for row i of the column"""
        record_begin = np.zeros(self.n_docs + 1, np.uint64)
        _check(self.L.mmt_merged_bed_records(self.h, _p(record_begin), None))
        records = np.zeros((int(record_begin[-1]), 5), np.int64)
        if len(records):
            _check(self.L.mmt_merged_bed_records(self.h, None, _p(records)))
        return record_begin, records

    def bed_records_device(self):
        """(address of the u64 [n_docs + 1] record offsets, address of the int64 [n, 5] records) in HBM"""
        a, b = C.c_void_p(), C.c_void_p()
        _check(self.L.mmt_merged_bed_records_device(self.h, C.byref(a), C.byref(b)))
        return a.value or 0, b.value or 0

    def bed_text(self, col):
        """the BED lines of column col of the last bed(), formatted on the device"""
        k = C.c_size_t()
        ptr = self.L.mmt_merged_bed_text(self.h, C.c_int64(int(col)), C.byref(k))
        if not ptr:
            raise MumemtoError("libmumemto: %s" % self.L.mmt_last_error().decode(errors="replace"))
        return _bytes_at(ptr, k.value)

    def write_bed(self, col, path):
        _check(self.L.mmt_merged_bed_write_text(self.h, C.c_int64(int(col)), os.fsencode(path)))

    def bed_stats(self):
        st = (C.c_double * 8)()
        _check(self.L.mmt_merged_bed_stats(self.h, st))
        d = {k: float(st[i]) for i, k in enumerate(["select_ms", "gather_ms", "lookup_ms", "text_ms"])}
        d.update(records=int(st[4]), clamped=int(st[5]), batches=int(st[6]), text_bytes=int(st[7]))
        return d

    def label(self, contigs, names=False):
        """Every start of the table as (contig, offset inside that contig), as the reference's `mumemto label` gives them, with
        the departures of get_sequence_info.py's docstring.  contigs: (names, lengths), each one list per sequence in file
        order, as mumsio.read_contigs returns them; names: the text carries the contig names instead of their numbers.
        Returns the length of the text; the table is only read."""
        begin, lens, name_begin, blob = contig_tables(contigs, check_names=False)
        if len(begin) != self.n_docs + 1:
            raise MumemtoError("label: contigs of %d sequences for a table of %d columns" % (len(begin) - 1, self.n_docs))
        k = C.c_uint64()
        blob = np.frombuffer(blob, np.uint8) if blob else np.zeros(1, np.uint8)
        _check(self.L.mmt_merged_label(self.engine.h, self.h, _p(begin), _p(lens), _p(name_begin), _p(blob),
                                       C.c_int(1 if names else 0), C.byref(k)))
        return int(k.value)

    def label_cells(self):
        """(contig uint32 [n, N], rel int64 [n, N]) of the last label(); an absent cell is (0, -1)"""
        n, nd = self.n_rows, self.n_docs
        contig = np.zeros((n, nd), np.uint32)
        rel = np.zeros((n, nd), np.int64)
        _check(self.L.mmt_merged_label_cells(self.h, _p(contig) if contig.size else None, _p(rel) if rel.size else None))
        return contig, rel

    def label_cells_device(self):
        """(address of the u32 [n, N] contigs, address of the int64 [n, N] offsets) in HBM"""
        a, b = C.c_void_p(), C.c_void_p()
        _check(self.L.mmt_merged_label_cells_device(self.h, C.byref(a), C.byref(b)))
        return a.value or 0, b.value or 0

    def label_text(self):
        """the labelled lines of the last label(), formatted on the device, with the blocks attached now"""
        k = C.c_size_t()
        ptr = self.L.mmt_merged_label_text(self.h, C.byref(k))
        if not ptr:
            raise MumemtoError("libmumemto: %s" % self.L.mmt_last_error().decode(errors="replace"))
        return _bytes_at(ptr, k.value)

    def write_label(self, path):
        _check(self.L.mmt_merged_label_write_text(self.h, os.fsencode(path)))

    def label_stats(self):
        st = (C.c_double * 8)()
        _check(self.L.mmt_merged_label_stats(self.h, st))
        d = {k: float(st[i]) for i, k in enumerate(["lookup_ms", "measure_ms", "write_ms", "copy_ms"])}
        d.update(cells=int(st[4]), absent=int(st[5]), hbm_columns=int(st[6]), text_bytes=int(st[7]))
        return d

    def sequences(self, col, source=None, dialect="python", terminator=True):
        """Measures the multi-FASTA of the rows' bases in column col: record i is `>mum_<i>`, the bases of row i, `#` with
        terminator.  source: None -- the engine's own text after a run (the table's columns are its documents); bytes, a
        bytearray or a uint8 array -- the bases of document col; a str or os.PathLike -- a FASTA file of it, plain or gzip.
        dialect: "binary" (the reference's extract_mums binary: bytes as they are, strands ignored, every record ends in a
        newline, partial rows and starts beyond the end refused) or "python" (its extract_mums.py: upper case, rows on '-'
        reverse-complemented, records joined by newlines, such rows empty).  Returns the length of the text; the table is
        only read."""
        self.sequences_doc_bases = None                    # (set by a FASTA path alone)
        d = SEQ_DIALECTS.get(dialect, dialect)
        if d not in (0, 1):
            raise MumemtoError("sequences: unknown dialect %r (binary or python)" % (dialect,))
        k = C.c_uint64()
        col, term = C.c_int64(int(col)), C.c_int(1 if terminator else 0)
        if source is None:
            _check(self.L.mmt_merged_sequences(self.engine.h, self.h, col, d, term, C.byref(k)))
        elif isinstance(source, (str, os.PathLike)):
            nb = C.c_uint64()
            _check(self.L.mmt_merged_sequences_file(self.engine.h, self.h, os.fsencode(source), col, d, term, C.byref(nb),
                                                    C.byref(k)))
            self.sequences_doc_bases = int(nb.value)       # the bases the file held
        else:
            bases = np.frombuffer(source, np.uint8) if isinstance(source, (bytes, bytearray, memoryview)) else \
                np.ascontiguousarray(source, np.uint8)
            _check(self.L.mmt_merged_sequences_host(self.engine.h, self.h, _p(bases) if len(bases) else None, len(bases), col, d,
                                                    term, C.byref(k)))
        return int(k.value)

    def sequences_offsets(self):
        """uint64 [n_rows + 1]: record i of the last sequences() is bytes [offsets[i], offsets[i + 1]) of the text"""
        out = np.zeros(self.n_rows + 1, np.uint64)
        _check(self.L.mmt_merged_sequences_offsets(self.h, _p(out)))
        return out

    def sequences_offsets_device(self):
        """address of the u64 [n_rows + 1] record offsets in HBM"""
        a = C.c_void_p()
        _check(self.L.mmt_merged_sequences_offsets_device(self.h, C.byref(a)))
        return a.value or 0

    def sequences_text(self):
        """the multi-FASTA of the last sequences(), formatted on the device"""
        k = C.c_size_t()
        ptr = self.L.mmt_merged_sequences_text(self.h, C.byref(k))
        if not ptr:
            raise MumemtoError("libmumemto: %s" % self.L.mmt_last_error().decode(errors="replace"))
        return _bytes_at(ptr, k.value)

    def write_sequences(self, path):
        _check(self.L.mmt_merged_sequences_write_text(self.h, os.fsencode(path)))

    def sequences_stats(self):
        st = (C.c_double * 8)()
        _check(self.L.mmt_merged_sequences_stats(self.h, st))
        d = dict(measure_ms=float(st[0]), format_ms=float(st[1]))
        d.update(records=int(st[2]), bases=int(st[3]), clipped=int(st[4]), empty=int(st[5]), text_bytes=int(st[6]),
                 pieces=int(st[7]))
        return d

    def text(self):
        k = C.c_size_t()
        ptr = self.L.mmt_merged_text(self.h, C.byref(k))
        if not ptr and self.n_rows:
            raise MumemtoError(self.L.mmt_last_error().decode())
        return _bytes_at(ptr, k.value)

    def write_text(self, path):
        _check(self.L.mmt_merged_write_text(self.h, os.fsencode(path)))


SEQ_DIALECTS = {"binary": 0, "python": 1}


def _engine_text_packed(self):
    """the layout of the resident text: True = two bits per base, False = a byte per base, None = no text is held"""
    r = self.L.mmt_engine_text_packed(self.h)
    return None if r < 0 else bool(r)


Engine.text_packed = _engine_text_packed


def _engine_mum_sequences(self, col, dialect="python", terminator=True):
    """the multi-FASTA of the MUM rows of this engine's last run in document col, read from the rows and the text where they
    lie in HBM (Merged.sequences with the resident source)"""
    with Merged.from_device(self, *self.rows_mum_device()) as m:
        m.sequences(col, None, dialect, terminator)
        return m.sequences_text()


Engine.mum_sequences = _engine_mum_sequences


def collinear_blocks(lengths, starts, strands, max_break=1000, min_singleton_length=None, device=0):
    """Rows on the host -> ((lengths, starts, strands) of the filtered, sorted table, blocks u32 [n_blocks, 2])."""
    eng = Engine(device)
    try:
        with Merged.from_rows(eng, lengths, starts, strands) as m:
            blocks = m.collinear(max_break, min_singleton_length)
            length, off, st = m.rows()
            return (length, off, st.astype(bool)), blocks
    finally:
        eng.close()


def find_inversions(lengths, starts, strands, max_block_gap=1000, max_length=None, device=0):
    """Rows on the host -> inversion calls int64 [k, 5] = (column, start, end, ref_start, ref_end): the collinear blocks of the
    filtered, sorted table (no singletons), then the calls over them, all on the device."""
    eng = Engine(device)
    try:
        with Merged.from_rows(eng, lengths, starts, strands) as m:
            m.collinear(max_block_gap, None)
            return m.inversions(max_length)
    finally:
        eng.close()


def mum_coverage(lengths, starts, strands, seq_lengths, seq_idx=None, min_length=0, device=0):
    """Rows on the host -> (covered uint64 [n_docs], run_begin uint64 [n_docs + 1], runs int64 [n, 2]): the positions of
    every sequence (or of seq_idx alone) that the rows of at least min_length cover, and the covered stretches themselves."""
    eng = Engine(device)
    try:
        with Merged.from_rows(eng, lengths, starts, strands) as m:
            covered = m.coverage(seq_lengths, seq_idx, min_length)
            return (covered,) + m.coverage_runs()
    finally:
        eng.close()


class Density:
    """The MEM density of the sequences in the HBM of an engine's GPU (mmt_density of mumemto_gpu.h): how many multi-MEM
    occurrences cover each position, summed over bins of bin_width positions -- with bin_width 1 the array of the reference's
    mem_density.py.  Rows are added from host batches (add_rows) or from the engine's last MEM-mode run where they lie
    (add_engine), any number of times; finish() makes the table, bins() reads it, and adding goes on afterwards."""

    def __init__(self, engine, seq_lengths, bin_width=1):
        self.engine, self.L = engine, engine.L
        lens = np.ascontiguousarray(seq_lengths, np.int64).ravel()
        if int(bin_width) < 0:
            raise MumemtoError("mem density: a negative bin width (%d)" % int(bin_width))
        h = C.c_void_p()
        _check(self.L.mmt_density_create(engine.h, _p(lens), len(lens), int(bin_width), C.byref(h)))
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.L.mmt_density_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def shape(self):
        """(num, nbins, size, the bin width in use)"""
        out = (C.c_uint64 * 4)()
        _check(self.L.mmt_density_shape(self.h, out))
        return tuple(int(v) for v in out)

    def add_rows(self, lengths, occ_start, starts, docs):
        """a batch of whole rows: lengths u32 [n], occ_start u64 [n + 1] from 0, starts i64 and docs u64 [occ_start[n]]"""
        lengths = np.ascontiguousarray(lengths, np.uint32)
        occ_start = np.ascontiguousarray(occ_start, np.uint64)
        starts = np.ascontiguousarray(starts, np.int64)
        docs = np.ascontiguousarray(docs, np.uint64)
        if len(occ_start) != len(lengths) + 1:
            raise MumemtoError("mem density: occ_start has %d entries for %d rows (one more is needed)" % (len(occ_start), len(lengths)))
        if len(starts) != len(docs) or len(starts) < int(occ_start[-1]):
            raise MumemtoError("mem density: %d starts and %d documents for %d occurrences" % (len(starts), len(docs), int(occ_start[-1])))
        _check(self.L.mmt_density_add_rows(self.h, _p(lengths), _p(occ_start), _p(starts), _p(docs), len(lengths)))

    def add_engine(self, engine=None):
        """the MEM rows of the last run of `engine` (default: the engine the tables live on), read in HBM"""
        _check(self.L.mmt_density_add_engine(self.h, (engine or self.engine).h))

    def finish(self):
        _check(self.L.mmt_density_finish(self.h))

    def bins(self):
        """uint64 [num, nbins]: the depth summed over every bin, after finish()"""
        num, nbins = self.shape[:2]
        out = np.zeros((num, nbins), np.uint64)
        _check(self.L.mmt_density_bins(self.h, _p(out)))
        return out

    def bins_device(self):
        """(HBM address of the uint64 [num, nbins] table, num, nbins); owned by the handle, rewritten by the next finish()"""
        a = C.c_void_p()
        _check(self.L.mmt_density_bins_device(self.h, C.byref(a)))
        return (a.value,) + self.shape[:2]

    def stats(self):
        st = (C.c_double * 8)()
        _check(self.L.mmt_density_stats(self.h, st))
        d = dict(add_ms=float(st[0]), finish_ms=float(st[1]))
        d.update(occurrences=int(st[2]), cut=int(st[3]), empty=int(st[4]), negative=int(st[5]), nbins=int(st[6]), bin_width=int(st[7]))
        return d


def _engine_mem_density(self, seq_lengths, bin_width=1):
    """uint64 [n_docs, nbins]: the density of the MEM rows of this engine's last run, from where they lie in HBM"""
    with Density(self, seq_lengths, bin_width) as d:
        d.add_engine()
        d.finish()
        return d.bins()


Engine.mem_density = _engine_mem_density


def mem_density(lengths, occ_start, starts, docs, seq_lengths, bin_width=1, device=0):
    """MEM rows on the host (the arrays of Engine.rows_mem, or a batch of mumsio.read_mems) -> uint64 [num, nbins]: the number
    of occurrences that cover each position of each sequence, summed over bins of bin_width positions."""
    eng = Engine(device)
    try:
        with Density(eng, seq_lengths, bin_width) as d:
            d.add_rows(lengths, occ_start, starts, docs)
            d.finish()
            return d.bins()
    finally:
        eng.close()


def contig_tables(contigs, check_names=True):
    """(names, lengths), one list per sequence -> the four tables of mmt_merged_bed: contig_begin u64 [n_seqs + 1], contig_len
    i64 and name_begin u64 [n_contigs + 1] over all contigs, and the names as one byte blob; check_names=False leaves the
    judgement of the names to the library (mmt_merged_label looks at them only when it prints them)"""
    names, lengths = contigs
    if len(names) != len(lengths) or any(len(a) != len(b) for a, b in zip(names, lengths)):
        raise MumemtoError("bed: names and lengths of the contigs do not match")
    begin = np.zeros(len(names) + 1, np.uint64)
    begin[1:] = np.cumsum([len(x) for x in names], dtype=np.uint64)
    flat = [n if isinstance(n, bytes) else str(n).encode() for seq in names for n in seq]
    for n in flat if check_names else ():
        if b"\t" in n or b"\n" in n:
            raise MumemtoError("bed: the contig name %r contains a tab or a newline" % n)
    name_begin = np.zeros(len(flat) + 1, np.uint64)
    name_begin[1:] = np.cumsum([len(n) for n in flat], dtype=np.uint64)
    lens = np.ascontiguousarray([int(v) for seq in lengths for v in seq] + [0], np.int64)
    return begin, lens, name_begin, b"".join(flat)


def mum_to_bed(lengths, starts, strands, contigs, blocks=None, seq_idx=None, min_singleton_length=100, max_block_gap=None,
               device=0):
    """Rows on the host -> (record_begin uint64 [n_docs + 1], records int64 [n, 5], texts): the BED records of every sequence
    (or of seq_idx alone) and their lines, {column: bytes}.  blocks: a block list (n_blocks, 2) for rows that are the
    filtered, sorted table; max_block_gap: compute the blocks first, as collinear_blocks does; neither: every row of at least
    min_singleton_length that has a start in the column."""
    eng = Engine(device)
    try:
        with Merged.from_rows(eng, lengths, starts, strands) as m:
            if blocks is not None:
                m.set_blocks(blocks)
            elif max_block_gap is not None:
                m.collinear(max_block_gap, None)
            m.bed(contigs, seq_idx, min_singleton_length)
            cols = range(m.n_docs) if seq_idx is None else [int(seq_idx)]
            return m.bed_records() + ({c: m.bed_text(c) for c in cols},)
    finally:
        eng.close()


def get_sequence_info(lengths, starts, strands, contigs, blocks=None, names=False, device=0):
    """Rows on the host -> (contig uint32 [n, N], rel int64 [n, N], text): every start as (contig, offset inside that contig) and
    the six-field lines of `mumemto label`.  blocks: a block list (n_blocks, 2) for rows that are the filtered, sorted table
    (field 4 is then the row's block or `-`, `*` without); names: field 5 holds the contig names."""
    eng = Engine(device)
    try:
        with Merged.from_rows(eng, lengths, starts, strands) as m:
            if blocks is not None:
                m.set_blocks(blocks)
            m.label(contigs, names)
            return m.label_cells() + (m.label_text(),)
    finally:
        eng.close()


def extract_mums(lengths, starts, strands, source, col=0, dialect="python", terminator=True, path=None, device=0):
    """Rows on the host and the bases of document col (bytes, a uint8 array or a FASTA path) -> the multi-FASTA of the rows'
    sequences as bytes, or with path written to that file (and None returned); dialects as in Merged.sequences"""
    eng = Engine(device)
    try:
        with Merged.from_rows(eng, lengths, starts, strands) as m:
            m.sequences(col, source, dialect, terminator)
            if path is None:
                return m.sequences_text()
            m.write_sequences(path)
    finally:
        eng.close()


def string_merge_device(parts, mom, mom_records, device=0):
    """merge_mums.string_merge on the device: the same inputs, the same five results (lengths u32, starts i64, strands bool,
    thresh u16, thresh_rev u16)"""
    eng = Engine(device)
    try:
        with Merged.string_fold(eng, parts, mom, mom_records) as m:
            length, starts, strands = m.rows()
            return (length, starts, strands.astype(bool)) + m.string_thresh()
    finally:
        eng.close()


class Comm:
    """The C-ABI multi-GPU exchange (RCCL, one process per GPU): mmt_comm_* / mmt_dist_* of mumemto_gpu.h.
    Rank 0 calls Comm.unique_id() and hands the 128 bytes to the other ranks out of band; Comm(engine, rank, world, id)
    is collective, and so are merge() and gather_text()."""

    @staticmethod
    def unique_id():
        L = load_library()
        buf = (C.c_uint8 * 128)()
        _check(L.mmt_comm_unique_id(buf))
        return bytes(buf)

    def __init__(self, engine, rank, world, unique_id):
        self.L, self.engine, self.rank, self.world = engine.L, engine, rank, world
        buf = (C.c_uint8 * 128).from_buffer_copy(unique_id)
        h = C.c_void_p()
        _check(self.L.mmt_comm_create(engine.h, rank, world, buf, C.byref(h)))
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.L.mmt_comm_destroy(self.h)
            self.h = None

    def merge(self, min_len=20, by_ranges=False, text_file=None):
        """Strict multi-MUMs: exchange + fold + re-sort.  Rank 0 gets {"text", "n_rows", "n_docs"}, the others None.
        by_ranges: every rank folds its slice of the anchor (automatic from four ranks on; rank 0 decides for everybody).
        text_file: rank 0's library writes PREFIX.mums there itself (in pieces; no Python copy) and "text" is None."""
        m = C.c_void_p()
        f = self.L.mmt_dist_merge_ranges if by_ranges else self.L.mmt_dist_merge
        _check(f(self.h, self.engine.h, C.c_uint32(min_len), C.byref(m)))
        if not m:
            return None
        try:
            n = self.L.mmt_merged_rows(m)
            if text_file is not None:
                _check(self.L.mmt_merged_write_text(m, os.fsencode(text_file)))
                return dict(text=None, n_rows=n, n_docs=self.L.mmt_merged_docs(m))
            k = C.c_size_t()
            ptr = self.L.mmt_merged_text(m, C.byref(k))
            if not ptr and n:
                raise MumemtoError(self.L.mmt_last_error().decode())
            return dict(text=_bytes_at(ptr, k.value), n_rows=n, n_docs=self.L.mmt_merged_docs(m))
        finally:
            self.L.mmt_merged_free(m)

    def loopback(self):
        """The exchange's messages with this rank as its own peer (mmt_comm_loopback): the engine's last run (merge metadata on)
        supplies row tables and thresholds; returns bytes, pieces, the largest piece, mismatching elements, seconds."""
        out = (C.c_uint64 * 8)()
        _check(self.L.mmt_comm_loopback(self.h, out))
        return {"bytes": int(out[0]), "pieces": int(out[1]), "largest_piece_bytes": int(out[2]), "different": int(out[3]),
                "seconds": int(out[4]) / 1e6, "rows": int(out[5]), "cells": int(out[6]), "thresholds": int(out[7])}

    def selftest(self, elements, width=4):
        """One message of that many elements of `width` bytes to this rank itself, in the exchange's pieces (mmt_comm_selftest)."""
        out = (C.c_uint64 * 4)()
        _check(self.L.mmt_comm_selftest(self.h, int(elements), int(width), out))
        return {"different": int(out[0]), "pieces": int(out[1]), "largest_piece_bytes": int(out[2]), "seconds": int(out[3]) / 1e6}

    TABLES = ("lengths", "offsets", "strands", "thresholds", "text", "digests")

    def verify_stats(self):
        """The verification of the exchange since this communicator was created (mmt_comm_verify_stats): messages, pieces and
        bytes digested (sent + received), pieces that arrived different, seconds in the digest kernels, and the first mismatch
        as {"peer", "table", "piece"} or None."""
        out = (C.c_uint64 * 8)()
        _check(self.L.mmt_comm_verify_stats(self.h, out))
        none = int(out[5]) == 2 ** 64 - 1
        first = None if none else {"peer": int(out[5]), "table": self.TABLES[int(out[6])], "piece": int(out[7])}
        return {"messages": int(out[0]), "pieces": int(out[1]), "bytes": int(out[2]), "mismatches": int(out[3]),
                "digest_seconds": int(out[4]) / 1e6, "first_mismatch": first}

    def gather_text(self):
        """Sharded modes (Engine.set_scan_shard): the whole output on rank 0, b"" elsewhere."""
        ptr, k = C.c_void_p(), C.c_size_t()
        _check(self.L.mmt_dist_gather_text(self.h, C.byref(ptr), C.byref(k)))
        return _bytes_at(ptr.value, k.value) if k.value else b""


def exchange_digest(array, piece_elements, skip_elements=0):
    """The exchange's digest kernel by itself (mmt_exchange_digest): the numpy array (uint8, uint32, int64 or uint64) is copied
    into a fresh device allocation and digested from `skip_elements` elements into it, in pieces of `piece_elements`.
    Returns uint64[pieces, 2]: the sum word and the xor word of every piece (an empty range is one piece of two zeros)."""
    import numpy as np
    L = load_library()
    a = np.ascontiguousarray(array)
    if a.ndim != 1 or a.dtype.itemsize not in (1, 4, 8) or a.dtype.kind not in "ui":
        raise MumemtoError("exchange_digest: a one-dimensional integer array of 1, 4 or 8 bytes an element")
    skip, piece = int(skip_elements), int(piece_elements)
    if piece < 1 or not 0 <= skip <= a.size:
        raise MumemtoError("exchange_digest: piece_elements >= 1 and 0 <= skip_elements <= len(array)")
    n = a.size - skip
    out = np.zeros((max(1, -(-n // piece)), 2), np.uint64)
    _check(L.mmt_exchange_digest_host(a.ctypes.data, a.size, a.dtype.itemsize, skip, piece, out.ctypes.data))
    return out
