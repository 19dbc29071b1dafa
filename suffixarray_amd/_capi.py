"""ctypes binding of the C ABI in include/sa_hip.h (libsa_hip.so, built in-tree by build.py).

This is the only way Python reaches the device code: no torch types cross the boundary, device
pointers travel as integers.  There is NO CPU fallback -- if the library is missing or no HIP
device is usable, calls raise.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SA_HIP_LIB", os.path.join(_HERE, "libsa_hip.so"))   # SA_HIP_LIB: A/B builds in tools/

PAIR_DTYPE = np.dtype([("first", "<u4"), ("second", "<u4")])
SPAN_DTYPE = np.dtype([("first", "<u4"), ("count", "<u4"), ("length", "<u4"), ("ended", "<u4")])            # sa_hip_token_span
NEXT_DTYPE = np.dtype([("written", "<u4"), ("covered", "<u4"), ("total", "<u4"), ("reserved", "<u4")])      # sa_hip_token_next
LOCATE_DTYPE = np.dtype([("written", "<u4"), ("count", "<u4")])                                            # sa_hip_token_locate
DOCS_DTYPE = np.dtype([("written", "<u4"), ("examined", "<u4"), ("distinct", "<u4"), ("count", "<u4")])     # sa_hip_token_docs
ALL_DTYPE = np.dtype([("written", "<u4"), ("examined", "<u4"), ("matched", "<u4"), ("candidates", "<u4"), ("driver", "<u4"),
                      ("count", "<u4"), ("reserved", "<u4", (2,))])                                           # sa_hip_token_all
MATCH_HEAD_DTYPE = np.dtype([("written", "<u4"), ("maximal", "<u4"), ("longest", "<u4"), ("covered", "<u4")])  # sa_hip_token_match_head
SCORE_DTYPE = np.dtype([("length", "<u4"), ("context_count", "<u4"), ("token_count", "<u4"), ("first", "<u4")])  # sa_hip_token_score
SCORE_HEAD_DTYPE = np.dtype([("scored", "<u4"), ("seen", "<u4"), ("certain", "<u4"), ("longest", "<u4"),
                             ("length_sum", "<u8")])                                                       # sa_hip_token_score_head
TOP_DTYPE = np.dtype([("written", "<u4"), ("distinct", "<u4"), ("covered", "<u4"), ("total", "<u4")])       # sa_hip_token_top
TOKEN_ALL_MAX = 16                                                                                         # SA_HIP_TOKEN_ALL_MAX
CNF_DTYPE = np.dtype([("written", "<u4"), ("matched", "<u4"), ("candidates", "<u4"), ("duplicates", "<u4"), ("driver", "<u4"),
                      ("literals", "<u4"), ("examined", "<u8"), ("count", "<u8"), ("reserved", "<u8")])      # sa_hip_token_cnf
TOKEN_CNF_MAX_CLAUSES = 16                                                                                 # SA_HIP_TOKEN_CNF_MAX_CLAUSES
TOKEN_CNF_MAX_LITERALS = 64                                                                                # SA_HIP_TOKEN_CNF_MAX_LITERALS
SHARDS_NEXT_DTYPE = np.dtype([("written", "<u4"), ("length", "<u4"), ("covered", "<u8"), ("total", "<u8")])  # sa_hip_token_shards_next
SHARDS_MATCH_DTYPE = np.dtype([("length", "<u4"), ("shards", "<u4"), ("count", "<u8")])                      # sa_hip_token_shards_match
SHARDS_SCORE_DTYPE = np.dtype([("length", "<u4"), ("shards", "<u4"), ("context_count", "<u8"),
                               ("token_count", "<u8")])                                                    # sa_hip_token_shards_score
SHARDS_TOP_DTYPE = np.dtype([("written", "<u4"), ("distinct", "<u4"), ("length", "<u4"), ("shards", "<u4"), ("covered", "<u8"),
                             ("total", "<u8")])                                                            # sa_hip_token_shards_top
SHARDS_LOCATE_DTYPE = np.dtype([("written", "<u4"), ("reserved", "<u4"), ("count", "<u8")])                  # sa_hip_token_shards_locate
SHARDS_DOCS_DTYPE = np.dtype([("written", "<u4"), ("reserved", "<u4"), ("examined", "<u8"), ("distinct", "<u8"),
                              ("count", "<u8")])                                                            # sa_hip_token_shards_docs
SHARDS_ALL_DTYPE = np.dtype([("written", "<u4"), ("driver", "<u4"), ("examined", "<u8"), ("matched", "<u8"), ("candidates", "<u8"),
                             ("count", "<u8")])                                                             # sa_hip_token_shards_all
SHARDS_ALL_PAIR_DTYPE = np.dtype([("written", "<u4"), ("examined", "<u4"), ("matched", "<u4"), ("candidates", "<u4")])   # heads_dev of all_merge_device
SHARDS_ALL_PLAN_DTYPE = np.dtype([("driver", "<u4"), ("reserved", "<u4"), ("count", "<u8")])                  # plan_dev of all_merge_device
SHARDS_MAX = 64
UINT32_MAX = 0xFFFFFFFF

# every symbol include/sa_hip.h declares (tests check the library exports all of them)
EXPORTS = [
    "sa_hip_libsais", "sa_hip_libsais_omp", "sa_hip_libsais64", "sa_hip_libsais64_omp",
    "sa_hip_libsais64_device", "sa_hip_sufcheck64_device", "sa_hip_index_deep_keys",
    "sa_hip_libsais_plcp", "sa_hip_libsais_plcp_omp", "sa_hip_libsais_lcp", "sa_hip_libsais_lcp_omp",
    "sa_hip_libsais64_plcp", "sa_hip_libsais64_plcp_omp", "sa_hip_libsais64_lcp", "sa_hip_libsais64_lcp_omp",
    "sa_hip_plcp64_device", "sa_hip_lcp64_device", "sa_hip_index_plcp_device", "sa_hip_index_lcp_device",
    "sa_hip_libsais_bwt", "sa_hip_libsais_bwt_omp", "sa_hip_libsais_bwt_aux", "sa_hip_libsais_bwt_aux_omp",
    "sa_hip_libsais_unbwt", "sa_hip_libsais_unbwt_omp", "sa_hip_libsais_unbwt_aux", "sa_hip_libsais_unbwt_aux_omp",
    "sa_hip_libsais64_bwt", "sa_hip_libsais64_bwt_omp", "sa_hip_libsais64_bwt_aux", "sa_hip_libsais64_bwt_aux_omp",
    "sa_hip_libsais64_unbwt", "sa_hip_libsais64_unbwt_omp", "sa_hip_libsais64_unbwt_aux", "sa_hip_libsais64_unbwt_aux_omp",
    "sa_hip_bwt64_device", "sa_hip_unbwt64_device", "sa_hip_index_bwt_device",
    "sa_hip_libsais_int", "sa_hip_libsais_int_omp", "sa_hip_libsais64_long", "sa_hip_libsais64_long_omp",
    "sa_hip_libsais_plcp_int", "sa_hip_libsais_plcp_int_omp", "sa_hip_libsais_int_device", "sa_hip_libsais64_long_device",
    "sa_hip_plcp_int_device", "sa_hip_sufcheck_long_device",
    "sa_hip_token_index_build", "sa_hip_token_index_load_device", "sa_hip_token_index_destroy", "sa_hip_token_index_query_batch",
    "sa_hip_token_index_query_batch_device", "sa_hip_token_index_sync", "sa_hip_token_index_text_dev", "sa_hip_token_index_sa_dev",
    "sa_hip_token_index_get_sa_range", "sa_hip_token_index_get_dir_range", "sa_hip_token_index_get_key_range", "sa_hip_token_index_info",
    "sa_hip_token_index_spans_batch", "sa_hip_token_index_spans_batch_device", "sa_hip_token_index_next_batch_device",
    "sa_hip_token_index_next_batch", "sa_hip_token_index_next_of_spans", "sa_hip_token_index_next_info",
    "sa_hip_token_index_set_documents", "sa_hip_token_index_get_doc_range", "sa_hip_token_index_docs_info",
    "sa_hip_token_index_locate_batch_device", "sa_hip_token_index_locate_batch", "sa_hip_token_index_docs_batch_device",
    "sa_hip_token_index_docs_batch",
    "sa_hip_token_index_prepare_doc_ranks", "sa_hip_token_index_get_doc_ranks", "sa_hip_token_index_doc_ranks_info",
    "sa_hip_token_index_doc_counts_batch_device", "sa_hip_token_index_doc_counts_batch", "sa_hip_token_index_all_batch_device",
    "sa_hip_token_index_all_batch",
    "sa_hip_token_index_cnf_batch_device", "sa_hip_token_index_cnf_batch", "sa_hip_token_index_cnf_info",
    "sa_hip_token_index_match_batch_device", "sa_hip_token_index_match_docs_batch_device", "sa_hip_token_index_match_batch",
    "sa_hip_token_index_match_docs_batch", "sa_hip_token_index_match_info",
    "sa_hip_token_index_score_batch_device", "sa_hip_token_index_score_docs_batch_device", "sa_hip_token_index_score_batch",
    "sa_hip_token_index_score_info",
    "sa_hip_token_index_top_batch_device", "sa_hip_token_index_top_batch", "sa_hip_token_index_sample_batch_device",
    "sa_hip_token_index_sample_batch", "sa_hip_token_index_top_info",
    "sa_hip_token_shards_create", "sa_hip_token_shards_destroy", "sa_hip_token_shards_shard", "sa_hip_token_shards_sync",
    "sa_hip_token_shards_info", "sa_hip_token_shards_query_batch", "sa_hip_token_shards_query_batch_device",
    "sa_hip_token_shards_spans_batch", "sa_hip_token_shards_spans_batch_device", "sa_hip_token_shards_next_batch",
    "sa_hip_token_shards_next_batch_device", "sa_hip_token_shards_merge_device",
    "sa_hip_token_shards_match_batch_device", "sa_hip_token_shards_match_docs_batch_device", "sa_hip_token_shards_match_batch",
    "sa_hip_token_shards_match_docs_batch", "sa_hip_token_shards_match_info",
    "sa_hip_token_shards_score_batch_device", "sa_hip_token_shards_score_docs_batch_device", "sa_hip_token_shards_score_batch",
    "sa_hip_token_shards_score_info",
    "sa_hip_token_shards_top_batch_device", "sa_hip_token_shards_top_batch", "sa_hip_token_shards_sample_batch_device",
    "sa_hip_token_shards_sample_batch", "sa_hip_token_shards_top_info",
    "sa_hip_token_shards_set_documents", "sa_hip_token_shards_adopt_documents", "sa_hip_token_shards_doc_bases",
    "sa_hip_token_shards_docs_info", "sa_hip_token_shards_locate_batch_device", "sa_hip_token_shards_locate_batch",
    "sa_hip_token_shards_docs_batch_device", "sa_hip_token_shards_docs_batch", "sa_hip_token_shards_docs_merge_device",
    "sa_hip_token_shards_prepare_doc_ranks", "sa_hip_token_shards_doc_ranks_info", "sa_hip_token_shards_doc_counts_batch_device",
    "sa_hip_token_shards_doc_counts_batch", "sa_hip_token_shards_all_batch_device", "sa_hip_token_shards_all_batch",
    "sa_hip_token_shards_all_merge_device",
    "sa_hip_last_call_breakdown", "sa_hip_release_workspace",
    "sa_hip_construct_truncated_suffix_array", "sa_hip_get_substring_positions",
    "sa_hip_device_count", "sa_hip_index_create", "sa_hip_index_destroy", "sa_hip_index_build",
    "sa_hip_index_build_device", "sa_hip_index_build_device64", "sa_hip_index_load", "sa_hip_index_load_device", "sa_hip_index_n",
    "sa_hip_index_max_suffix_length", "sa_hip_index_text_dev", "sa_hip_index_sa_dev",
    "sa_hip_index_stream", "sa_hip_index_get_sa_u32", "sa_hip_index_get_sa_i64", "sa_hip_index_widen_device",
    "sa_hip_index_get_freq", "sa_hip_query_batch", "sa_hip_query_batch_device", "sa_hip_query_batch_device_fixed",
    "sa_hip_index_get_sa_range", "sa_hip_index_query_hits", "sa_hip_index_sync", "sa_hip_index_verify", "sa_hip_index_build_stats",
    "sa_hip_index_set_rows", "sa_hip_index_query_rows", "sa_hip_index_query_rows_batch", "sa_hip_index_rows_for_range", "sa_hip_csv_index_copy_rows", "sa_hip_index_get_text", "sa_hip_csv_index_create", "sa_hip_csv_index_adopt",
    "sa_hip_get_matching_row_spans_file", "sa_hip_csv_index_destroy", "sa_hip_csv_index_create_partitioned", "sa_hip_csv_index_free_parts", "sa_hip_csv_index_handle", "sa_hip_csv_index_num_rows", "sa_hip_csv_index_num_columns",
    "sa_hip_csv_index_column_index", "sa_hip_csv_index_column_name", "sa_hip_csv_index_row_tables",
    "sa_hip_get_substring_positions_file", "sa_hip_get_matching_records_file", "sa_hip_get_matching_records", "sa_hip_free_records",
    "sa_hip_init_suffix_array_byte_idxs", "sa_hip_free_suffix_array", "sa_hip_write_suffix_array", "sa_hip_read_suffix_array",
    "sa_hip_comm_unique_id", "sa_hip_comm_create", "sa_hip_comm_destroy", "sa_hip_comm_rank", "sa_hip_comm_size",
    "sa_hip_comm_replicate_index", "sa_hip_comm_allgather_ranges",
    "sa_hip_index_replica_layout", "sa_hip_index_replica_buffers", "sa_hip_index_replica_reserve", "sa_hip_index_replica_commit",
    "sa_hip_index_query_stats", "sa_hip_csv_extract_column", "sa_hip_csv_free", "sa_hip_synth_csv", "sa_hip_sort_pairs", "sa_hip_synth_uniform27", "sa_hip_last_error", "sa_hip_version",
]


class PairU32(C.Structure):
    _fields_ = [("first", C.c_uint32), ("second", C.c_uint32)]


class SuffixArrayStruct(C.Structure):
    """engine.h:123-130 layout (sa_hip_SuffixArray_struct)."""
    _fields_ = [("suffix_array", C.c_void_p), ("is_quoted_bitflag", C.c_void_p),
                ("global_byte_start_idx", C.c_uint64), ("global_byte_end_idx", C.c_uint64),
                ("max_suffix_length", C.c_uint32), ("n", C.c_uint32)]


class BuildStats(C.Structure):
    _fields_ = [("n", C.c_uint64), ("sigma", C.c_uint32), ("bits_per_symbol", C.c_uint32),
                ("initial_chars", C.c_uint32), ("rounds", C.c_uint32), ("chunk_rounds", C.c_uint32),
                ("doubling_rounds", C.c_uint32), ("final_depth", C.c_uint32), ("radix_passes", C.c_uint32),
                ("radix_records", C.c_uint64), ("radix_bytes", C.c_uint64), ("active_total", C.c_uint64),
                ("tiny_resolved", C.c_uint64),
                ("radix_ms", C.c_double), ("total_ms", C.c_double),
                ("pass_ms", C.c_double * 4), ("pass_bytes", C.c_uint64 * 4), ("pass_launches", C.c_uint32 * 4),
                ("text_top_pass", C.c_uint32), ("narrow_k", C.c_uint32), ("widen_ms", C.c_double),
                ("finisher_records", C.c_uint64), ("finisher_resolved", C.c_uint64), ("finisher_runs", C.c_uint32),
                ("widen_fused", C.c_uint32), ("narrow48", C.c_uint32), ("lite_flags", C.c_uint32),
                ("period_resolved", C.c_uint64), ("split_plan", C.c_uint32), ("split_max", C.c_uint32)]

    def as_dict(self):
        return {k: (list(getattr(self, k)) if k.startswith("pass_") else getattr(self, k)) for k, _ in self._fields_}


class CsvColumn(C.Structure):
    _fields_ = [("text", C.c_void_p), ("text_len", C.c_uint64), ("row_text_starts", C.c_void_p),
                ("row_file_offsets", C.c_void_p), ("num_rows", C.c_uint64), ("column_names", C.c_void_p),
                ("num_columns", C.c_uint32), ("column_index", C.c_uint32)]


class QueryStats(C.Structure):
    _fields_ = [("q", C.c_uint64), ("kernel_ms", C.c_double), ("kernel_ms_sum", C.c_double), ("launches", C.c_uint32),
                ("pad_", C.c_uint32)]


class BigStats(C.Structure):
    """sa_hip_big_stats: the 64-bit-index build (texts beyond 2^32 - 2 bytes)."""
    _fields_ = [("sigma", C.c_uint32), ("bits_per_symbol", C.c_uint32), ("initial_chars", C.c_uint32), ("sort_passes", C.c_uint32),
                ("rounds", C.c_uint32), ("pad_", C.c_uint32), ("tied_after_sort", C.c_uint64), ("tied_total", C.c_uint64),
                ("total_ms", C.c_float)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "pad_"}


class CallBreakdown(C.Structure):
    _fields_ = [("n", C.c_uint64), ("workspace_reused", C.c_uint32), ("pad_", C.c_uint32), ("total_ms", C.c_double),
                ("workspace_ms", C.c_double), ("upload_ms", C.c_double), ("build_ms", C.c_double), ("build_device_ms", C.c_double),
                ("download_ms", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "pad_"}


class LcpStats(C.Structure):
    """sa_hip_lcp_stats: device time per phase and text work of one PLCP / LCP pass."""
    _fields_ = [("n", C.c_uint64), ("tied", C.c_uint64), ("compared_positions", C.c_uint64), ("compared_bytes", C.c_uint64),
                ("wave_compares", C.c_uint64), ("split_compares", C.c_uint64), ("split_rounds", C.c_uint32), ("keys", C.c_uint32),
                ("phi_ms", C.c_double), ("wave_ms", C.c_double), ("split_ms", C.c_double), ("scan_ms", C.c_double),
                ("gather_ms", C.c_double), ("total_ms", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class BwtStats(C.Structure):
    """sa_hip_bwt_stats: device time per phase and the walks of one BWT / inverse BWT pass."""
    _fields_ = [("n", C.c_uint64), ("rulers", C.c_uint64), ("longest_walk", C.c_uint64), ("ruler_rounds", C.c_uint32),
                ("rank_rounds", C.c_uint32), ("aux_only", C.c_uint32), ("pad_", C.c_uint32), ("psi_ms", C.c_double),
                ("walk_ms", C.c_double), ("rank_ms", C.c_double), ("copy_ms", C.c_double), ("gather_ms", C.c_double),
                ("total_ms", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "pad_"}


class IntStats(C.Structure):
    """sa_hip_int_stats: the route and the work of one integer-alphabet build."""
    _fields_ = [("n", C.c_uint64), ("plan", C.c_uint32), ("sigma", C.c_uint32), ("compacted", C.c_uint32), ("bits_per_symbol", C.c_uint32),
                ("symbols_per_key", C.c_uint32), ("sort_passes", C.c_uint32), ("rounds", C.c_uint32), ("pad_", C.c_uint32),
                ("tied_after_sort", C.c_uint64), ("tied_total", C.c_uint64), ("min_symbol", C.c_int64), ("max_symbol", C.c_int64),
                ("alphabet_ms", C.c_double), ("total_ms", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "pad_"}


class TokenInfo(C.Structure):
    """sa_hip_token_info: the text, the search structures and the last search launch of a token index."""
    _fields_ = [("n", C.c_uint64), ("min_symbol", C.c_int64), ("max_symbol", C.c_int64), ("dir_entries", C.c_uint64),
                ("key_bytes", C.c_uint32), ("last_rank", C.c_uint32), ("prepare_ms", C.c_double), ("q", C.c_uint64),
                ("kernel_ms", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class TokenSpan(C.Structure):
    _fields_ = [("first", C.c_uint32), ("count", C.c_uint32), ("length", C.c_uint32), ("ended", C.c_uint32)]


class TokenNext(C.Structure):
    _fields_ = [("written", C.c_uint32), ("covered", C.c_uint32), ("total", C.c_uint32), ("reserved", C.c_uint32)]


class TokenNextInfo(C.Structure):
    """sa_hip_token_next_info: the last span and next-symbol launches of a token index."""
    _fields_ = [("q", C.c_uint64), ("spans_ms", C.c_double), ("next_ms", C.c_double), ("lane_spans", C.c_uint64),
                ("wave_spans", C.c_uint64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class TokenLocate(C.Structure):
    _fields_ = [("written", C.c_uint32), ("count", C.c_uint32)]


class TokenDocs(C.Structure):
    _fields_ = [("written", C.c_uint32), ("examined", C.c_uint32), ("distinct", C.c_uint32), ("count", C.c_uint32)]


class TokenDocsInfo(C.Structure):
    """sa_hip_token_docs_info: the documents of a token index and its last locate and documents launches."""
    _fields_ = [("documents", C.c_uint64), ("bytes", C.c_uint64), ("prepare_ms", C.c_double), ("da_ms", C.c_double),
                ("sort_ms", C.c_double), ("pv_ms", C.c_double), ("sort_passes", C.c_uint32), ("reserved", C.c_uint32),
                ("locate_q", C.c_uint64), ("locate_ms", C.c_double), ("docs_q", C.c_uint64), ("docs_ms", C.c_double),
                ("examined", C.c_uint64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class TokenAll(C.Structure):
    _fields_ = [("written", C.c_uint32), ("examined", C.c_uint32), ("matched", C.c_uint32), ("candidates", C.c_uint32),
                ("driver", C.c_uint32), ("count", C.c_uint32), ("reserved", C.c_uint32 * 2)]


class TokenDocRanksInfo(C.Structure):
    """sa_hip_token_doc_ranks_info: the rank-by-document array of a token index and its last doc_counts and all launches."""
    _fields_ = [("present", C.c_uint32), ("sort_passes", C.c_uint32), ("bytes", C.c_uint64), ("prepare_ms", C.c_double),
                ("counts_q", C.c_uint64), ("counts_ms", C.c_double), ("all_q", C.c_uint64), ("all_ms", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class TokenCnf(C.Structure):
    _fields_ = [("written", C.c_uint32), ("matched", C.c_uint32), ("candidates", C.c_uint32), ("duplicates", C.c_uint32),
                ("driver", C.c_uint32), ("literals", C.c_uint32), ("examined", C.c_uint64), ("count", C.c_uint64),
                ("reserved", C.c_uint64)]


class TokenCnfInfo(C.Structure):
    """sa_hip_token_cnf_info: the last cnf launch of a token index."""
    _fields_ = [("q", C.c_uint64), ("ms", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class TokenMatchHead(C.Structure):
    _fields_ = [("written", C.c_uint32), ("maximal", C.c_uint32), ("longest", C.c_uint32), ("covered", C.c_uint32)]


class TokenMatchInfo(C.Structure):
    """sa_hip_token_match_info: the last match and match-docs launches of a token index."""
    _fields_ = [("q", C.c_uint64), ("positions", C.c_uint64), ("match_ms", C.c_double), ("docs_ms", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class TokenScore(C.Structure):
    _fields_ = [("length", C.c_uint32), ("context_count", C.c_uint32), ("token_count", C.c_uint32), ("first", C.c_uint32)]


class TokenScoreHead(C.Structure):
    _fields_ = [("scored", C.c_uint32), ("seen", C.c_uint32), ("certain", C.c_uint32), ("longest", C.c_uint32),
                ("length_sum", C.c_uint64)]


class TokenScoreInfo(C.Structure):
    """sa_hip_token_score_info: the last match, score and score-docs launches of a token index."""
    _fields_ = [("q", C.c_uint64), ("positions", C.c_uint64), ("match_ms", C.c_double), ("score_ms", C.c_double),
                ("docs_ms", C.c_double)]

    def as_dict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


class TokenTop(C.Structure):
    _fields_ = [("written", C.c_uint32), ("distinct", C.c_uint32), ("covered", C.c_uint32), ("total", C.c_uint32)]


class TokenTopInfo(C.Structure):
    """sa_hip_token_top_info: the last span, top and sample launches of a token index."""
    _fields_ = [("q", C.c_uint64), ("spans_ms", C.c_double), ("top_ms", C.c_double), ("sample_ms", C.c_double)]

    def as_dict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


class TokenShardsNext(C.Structure):
    _fields_ = [("written", C.c_uint32), ("length", C.c_uint32), ("covered", C.c_uint64), ("total", C.c_uint64)]


class TokenShardsStats(C.Structure):
    """sa_hip_token_shards_stats: a shard set and its last ranges, spans and next-symbol launches."""
    _fields_ = [("shards", C.c_uint32), ("chunk", C.c_uint32), ("tokens", C.c_uint64), ("q", C.c_uint64), ("ranges_ms", C.c_double),
                ("spans_ms", C.c_double), ("next_ms", C.c_double), ("merge_ms", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class TokenShardsMatch(C.Structure):
    _fields_ = [("length", C.c_uint32), ("shards", C.c_uint32), ("count", C.c_uint64)]


class TokenShardsMatchStats(C.Structure):
    """sa_hip_token_shards_match_stats: the last match and match-docs launches of a shard set."""
    _fields_ = [("q", C.c_uint64), ("positions", C.c_uint64), ("match_ms", C.c_double), ("docs_ms", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class TokenShardsScore(C.Structure):
    _fields_ = [("length", C.c_uint32), ("shards", C.c_uint32), ("context_count", C.c_uint64), ("token_count", C.c_uint64)]


class TokenShardsScoreStats(C.Structure):
    """sa_hip_token_shards_score_stats: the last match, score and score-docs launches of a shard set."""
    _fields_ = [("q", C.c_uint64), ("positions", C.c_uint64), ("match_ms", C.c_double), ("score_ms", C.c_double),
                ("docs_ms", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class TokenShardsTop(C.Structure):
    _fields_ = [("written", C.c_uint32), ("distinct", C.c_uint32), ("length", C.c_uint32), ("shards", C.c_uint32),
                ("covered", C.c_uint64), ("total", C.c_uint64)]


class TokenShardsTopStats(C.Structure):
    """sa_hip_token_shards_top_stats: the last spans, top and sample launches of a shard set."""
    _fields_ = [("q", C.c_uint64), ("spans_ms", C.c_double), ("top_ms", C.c_double), ("sample_ms", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class TokenShardsLocate(C.Structure):
    _fields_ = [("written", C.c_uint32), ("reserved", C.c_uint32), ("count", C.c_uint64)]


class TokenShardsDocs(C.Structure):
    _fields_ = [("written", C.c_uint32), ("reserved", C.c_uint32), ("examined", C.c_uint64), ("distinct", C.c_uint64),
                ("count", C.c_uint64)]


class TokenShardsDocsStats(C.Structure):
    """sa_hip_token_shards_docs_stats: the documents of a shard set and its last locate, pair and merge launches."""
    _fields_ = [("documents", C.c_uint64), ("chunk", C.c_uint32), ("reserved", C.c_uint32), ("locate_q", C.c_uint64),
                ("locate_ms", C.c_double), ("pairs_q", C.c_uint64), ("pairs_ms", C.c_double), ("merge_q", C.c_uint64),
                ("merge_ms", C.c_double), ("streamed", C.c_uint64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class TokenShardsAll(C.Structure):
    _fields_ = [("written", C.c_uint32), ("driver", C.c_uint32), ("examined", C.c_uint64), ("matched", C.c_uint64),
                ("candidates", C.c_uint64), ("count", C.c_uint64)]


class TokenShardsRanksStats(C.Structure):
    """sa_hip_token_shards_ranks_stats: the rank-by-document arrays of a shard set and its last doc_counts and all calls."""
    _fields_ = [("present", C.c_uint32), ("chunk", C.c_uint32), ("bytes", C.c_uint64), ("prepare_ms", C.c_double),
                ("counts_q", C.c_uint64), ("counts_ms", C.c_double), ("plan_q", C.c_uint64), ("plan_ms", C.c_double),
                ("pairs_q", C.c_uint64), ("pairs_ms", C.c_double), ("merge_q", C.c_uint64), ("merge_ms", C.c_double),
                ("streamed", C.c_uint64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class ReplicaLayout(C.Structure):
    """sa_hip_replica_layout: what a replica must know about the index it copies (travels as bytes)."""
    _fields_ = [("n", C.c_uint64), ("max_suffix_length", C.c_uint32), ("key_bytes", C.c_uint32), ("bits_per_symbol", C.c_uint32),
                ("initial_chars", C.c_uint32), ("dir_bits", C.c_uint32), ("lo_shift", C.c_int32), ("dir_entries", C.c_uint64),
                ("code", C.c_uint16 * 256), ("freq", C.c_uint64 * 256)]


class ReplicaBuffers(C.Structure):
    _fields_ = [("text", C.c_void_p), ("sa", C.c_void_p), ("keys", C.c_void_p), ("dir", C.c_void_p),
                ("text_bytes", C.c_uint64), ("sa_bytes", C.c_uint64), ("keys_bytes", C.c_uint64), ("dir_bytes", C.c_uint64)]

    def items(self):
        """(device pointer, bytes) of every buffer that has to travel, in a fixed order"""
        return [(getattr(self, k) or 0, int(getattr(self, k + "_bytes"))) for k in ("text", "sa", "keys", "dir")]


class SaHipError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libsa_hip error {code}: {msg}")
        self.code = code


_lib = None


def lib():
    """Load libsa_hip.so (raises if it has not been built: there is no fallback path)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} not found: run `python -m suffixarray_amd.build` "
                          "(hipcc --offload-arch=gfx950); there is no CPU fallback")
    L = C.CDLL(LIB_PATH)
    vp, u64, u32, i32, i64 = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int32, C.c_int64
    L.sa_hip_libsais.restype = i32
    L.sa_hip_libsais.argtypes = [vp, vp, i32, i32, vp]
    L.sa_hip_libsais_omp.restype = i32
    L.sa_hip_libsais_omp.argtypes = [vp, vp, i32, i32, vp, i32]
    L.sa_hip_libsais64.restype = i64
    L.sa_hip_libsais64.argtypes = [vp, vp, i64, i64, vp]
    L.sa_hip_libsais64_omp.restype = i64
    L.sa_hip_libsais64_omp.argtypes = [vp, vp, i64, i64, vp, i64]
    L.sa_hip_libsais64_device.restype = C.c_int
    L.sa_hip_libsais64_device.argtypes = [vp, vp, i64, C.c_int, C.POINTER(BigStats)]
    L.sa_hip_sufcheck64_device.restype = C.c_int
    L.sa_hip_sufcheck64_device.argtypes = [vp, vp, i64, C.c_int, C.POINTER(u64)]
    for name in ("sa_hip_libsais_plcp", "sa_hip_libsais_lcp"):
        getattr(L, name).restype = i32
        getattr(L, name).argtypes = [vp, vp, vp, i32]
        getattr(L, name + "_omp").restype = i32
        getattr(L, name + "_omp").argtypes = [vp, vp, vp, i32, i32]
    for name in ("sa_hip_libsais64_plcp", "sa_hip_libsais64_lcp"):
        getattr(L, name).restype = i64
        getattr(L, name).argtypes = [vp, vp, vp, i64]
        getattr(L, name + "_omp").restype = i64
        getattr(L, name + "_omp").argtypes = [vp, vp, vp, i64, i64]
    for name in ("sa_hip_plcp64_device", "sa_hip_lcp64_device"):
        getattr(L, name).restype = C.c_int
        getattr(L, name).argtypes = [vp, vp, vp, i64, C.c_int, C.POINTER(LcpStats)]
    for bits, it in ((32, i32), (64, i64)):
        pre = "sa_hip_libsais" if bits == 32 else "sa_hip_libsais64"
        for sfx, args in (("_bwt", [vp, vp, vp, it, it, vp]), ("_bwt_aux", [vp, vp, vp, it, it, vp, it, vp]),
                          ("_unbwt", [vp, vp, vp, it, vp, it]), ("_unbwt_aux", [vp, vp, vp, it, vp, it, vp])):
            getattr(L, pre + sfx).restype = it
            getattr(L, pre + sfx).argtypes = args
            getattr(L, pre + sfx + "_omp").restype = it
            getattr(L, pre + sfx + "_omp").argtypes = args + [it]
    L.sa_hip_bwt64_device.restype = i64
    L.sa_hip_bwt64_device.argtypes = [vp, vp, vp, i64, i64, vp, C.c_int, C.POINTER(BwtStats)]
    L.sa_hip_unbwt64_device.restype = C.c_int
    L.sa_hip_unbwt64_device.argtypes = [vp, vp, i64, i64, vp, C.c_int, C.POINTER(BwtStats)]
    L.sa_hip_index_bwt_device.restype = C.c_int
    L.sa_hip_libsais_int.restype = i32
    L.sa_hip_libsais_int.argtypes = [vp, vp, i32, i32, i32]
    L.sa_hip_libsais_int_omp.restype = i32
    L.sa_hip_libsais_int_omp.argtypes = [vp, vp, i32, i32, i32, i32]
    L.sa_hip_libsais64_long.restype = i64
    L.sa_hip_libsais64_long.argtypes = [vp, vp, i64, i64, i64]
    L.sa_hip_libsais64_long_omp.restype = i64
    L.sa_hip_libsais64_long_omp.argtypes = [vp, vp, i64, i64, i64, i64]
    L.sa_hip_libsais_plcp_int.restype = i32
    L.sa_hip_libsais_plcp_int.argtypes = [vp, vp, vp, i32]
    L.sa_hip_libsais_plcp_int_omp.restype = i32
    L.sa_hip_libsais_plcp_int_omp.argtypes = [vp, vp, vp, i32, i32]
    L.sa_hip_libsais_int_device.restype = C.c_int
    L.sa_hip_libsais_int_device.argtypes = [vp, vp, i32, i32, C.c_int, C.POINTER(IntStats)]
    L.sa_hip_libsais64_long_device.restype = C.c_int
    L.sa_hip_libsais64_long_device.argtypes = [vp, vp, i64, i64, C.c_int, C.POINTER(IntStats)]
    L.sa_hip_plcp_int_device.restype = C.c_int
    L.sa_hip_plcp_int_device.argtypes = [vp, vp, vp, i32, C.c_int, C.POINTER(LcpStats)]
    L.sa_hip_sufcheck_long_device.restype = C.c_int
    L.sa_hip_sufcheck_long_device.argtypes = [vp, vp, i64, C.c_int, C.POINTER(u64)]
    L.sa_hip_index_bwt_device.argtypes = [vp, vp, i64, vp, C.POINTER(i64), C.POINTER(BwtStats)]
    for name in ("sa_hip_index_plcp_device", "sa_hip_index_lcp_device"):
        getattr(L, name).restype = C.c_int
        getattr(L, name).argtypes = [vp, vp, C.POINTER(LcpStats)]
    L.sa_hip_index_deep_keys.restype = C.c_int
    L.sa_hip_index_deep_keys.argtypes = [vp, C.c_int]
    L.sa_hip_last_call_breakdown.restype = C.c_int
    L.sa_hip_last_call_breakdown.argtypes = [C.POINTER(CallBreakdown)]
    L.sa_hip_release_workspace.restype = None
    L.sa_hip_release_workspace.argtypes = []
    L.sa_hip_construct_truncated_suffix_array.restype = C.c_int
    L.sa_hip_construct_truncated_suffix_array.argtypes = [vp, C.POINTER(SuffixArrayStruct)]
    L.sa_hip_get_substring_positions.restype = PairU32
    L.sa_hip_get_substring_positions.argtypes = [vp, C.POINTER(SuffixArrayStruct), C.c_char_p]
    L.sa_hip_device_count.restype = C.c_int
    L.sa_hip_device_count.argtypes = []
    L.sa_hip_index_create.restype = C.c_int
    L.sa_hip_index_create.argtypes = [C.POINTER(vp), u64, C.c_int]
    L.sa_hip_index_destroy.restype = None
    L.sa_hip_index_destroy.argtypes = [vp]
    L.sa_hip_index_build.restype = C.c_int
    L.sa_hip_index_build.argtypes = [vp, vp, u64, u32]
    L.sa_hip_index_build_device.restype = C.c_int
    L.sa_hip_index_build_device.argtypes = [vp, vp, u64, u32]
    L.sa_hip_index_build_device64.restype = C.c_int
    L.sa_hip_index_build_device64.argtypes = [vp, vp, u64, u32, vp]
    L.sa_hip_index_load.restype = C.c_int
    L.sa_hip_index_load.argtypes = [vp, vp, vp, u64, u32]
    L.sa_hip_index_load_device.restype = C.c_int
    L.sa_hip_index_load_device.argtypes = [vp, vp, vp, u64, u32]
    L.sa_hip_comm_unique_id.restype = C.c_int
    L.sa_hip_comm_unique_id.argtypes = [vp]
    L.sa_hip_comm_create.restype = C.c_int
    L.sa_hip_comm_create.argtypes = [C.POINTER(vp), vp, C.c_int, C.c_int, C.c_int]
    L.sa_hip_comm_destroy.restype = None
    L.sa_hip_comm_destroy.argtypes = [vp]
    L.sa_hip_comm_rank.restype = C.c_int
    L.sa_hip_comm_rank.argtypes = [vp]
    L.sa_hip_comm_size.restype = C.c_int
    L.sa_hip_comm_size.argtypes = [vp]
    L.sa_hip_comm_replicate_index.restype = C.c_int
    L.sa_hip_comm_replicate_index.argtypes = [vp, vp, C.c_int, C.POINTER(u64)]
    L.sa_hip_comm_allgather_ranges.restype = C.c_int
    L.sa_hip_comm_allgather_ranges.argtypes = [vp, vp, vp, u64, vp]
    L.sa_hip_index_replica_layout.restype = C.c_int
    L.sa_hip_index_replica_layout.argtypes = [vp, C.POINTER(ReplicaLayout)]
    L.sa_hip_index_replica_buffers.restype = C.c_int
    L.sa_hip_index_replica_buffers.argtypes = [vp, C.POINTER(ReplicaBuffers)]
    L.sa_hip_index_replica_reserve.restype = C.c_int
    L.sa_hip_index_replica_reserve.argtypes = [vp, C.POINTER(ReplicaLayout), C.POINTER(ReplicaBuffers)]
    L.sa_hip_index_replica_commit.restype = C.c_int
    L.sa_hip_index_replica_commit.argtypes = [vp]
    L.sa_hip_index_n.restype = u64
    L.sa_hip_index_n.argtypes = [vp]
    L.sa_hip_index_max_suffix_length.restype = u32
    L.sa_hip_index_max_suffix_length.argtypes = [vp]
    L.sa_hip_index_text_dev.restype = vp
    L.sa_hip_index_text_dev.argtypes = [vp]
    L.sa_hip_index_sa_dev.restype = vp
    L.sa_hip_index_sa_dev.argtypes = [vp]
    L.sa_hip_index_stream.restype = vp
    L.sa_hip_index_stream.argtypes = [vp]
    L.sa_hip_index_get_sa_u32.restype = C.c_int
    L.sa_hip_index_get_sa_u32.argtypes = [vp, vp]
    L.sa_hip_index_get_sa_i64.restype = C.c_int
    L.sa_hip_index_get_sa_i64.argtypes = [vp, vp]
    L.sa_hip_index_widen_device.restype = C.c_int
    L.sa_hip_index_widen_device.argtypes = [vp, vp]
    L.sa_hip_index_get_freq.restype = C.c_int
    L.sa_hip_index_get_freq.argtypes = [vp, vp]
    L.sa_hip_query_batch.restype = C.c_int
    L.sa_hip_query_batch.argtypes = [vp, vp, vp, u64, vp]
    L.sa_hip_query_batch_device.restype = C.c_int
    L.sa_hip_query_batch_device.argtypes = [vp, vp, vp, u64, vp]
    L.sa_hip_query_batch_device_fixed.restype = C.c_int
    L.sa_hip_query_batch_device_fixed.argtypes = [vp, vp, u64, u64, vp]
    L.sa_hip_index_get_sa_range.restype = C.c_int
    L.sa_hip_index_get_sa_range.argtypes = [vp, u64, u64, vp]
    L.sa_hip_index_query_hits.restype = C.c_int
    L.sa_hip_index_query_hits.argtypes = [vp, C.c_char_p, u64, C.c_uint32, C.POINTER(PairU32), vp, C.POINTER(C.c_uint32)]
    L.sa_hip_index_sync.restype = C.c_int
    L.sa_hip_index_sync.argtypes = [vp]
    L.sa_hip_index_verify.restype = C.c_int
    L.sa_hip_index_verify.argtypes = [vp, C.POINTER(u64)]
    L.sa_hip_index_build_stats.restype = C.c_int
    L.sa_hip_index_build_stats.argtypes = [vp, C.POINTER(BuildStats)]
    L.sa_hip_index_query_stats.restype = C.c_int
    L.sa_hip_index_query_stats.argtypes = [vp, C.POINTER(QueryStats)]
    L.sa_hip_csv_extract_column.restype = C.c_int
    L.sa_hip_csv_extract_column.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(CsvColumn)]
    L.sa_hip_csv_free.restype = None
    L.sa_hip_csv_free.argtypes = [C.POINTER(CsvColumn)]
    L.sa_hip_synth_csv.restype = C.c_int
    L.sa_hip_synth_csv.argtypes = [C.c_char_p, u64, u64]
    L.sa_hip_index_set_rows.restype = C.c_int
    L.sa_hip_index_set_rows.argtypes = [vp, vp, u64]
    L.sa_hip_index_query_rows.restype = C.c_int
    L.sa_hip_index_query_rows.argtypes = [vp, C.c_char_p, u64, u32, vp, C.POINTER(u32), C.POINTER(PairU32)]
    L.sa_hip_index_query_rows_batch.restype = C.c_int
    L.sa_hip_index_query_rows_batch.argtypes = [vp, vp, vp, u64, u32, vp, vp, vp]
    L.sa_hip_index_rows_for_range.restype = C.c_int
    L.sa_hip_index_rows_for_range.argtypes = [vp, PairU32, u32, vp, C.POINTER(u32)]
    L.sa_hip_index_get_text.restype = C.c_int
    L.sa_hip_index_get_text.argtypes = [vp, vp]
    L.sa_hip_csv_index_create.restype = C.c_int
    L.sa_hip_csv_index_create.argtypes = [C.POINTER(vp), C.c_char_p, C.c_char_p, u32, C.c_int]
    L.sa_hip_csv_index_adopt.restype = C.c_int
    L.sa_hip_csv_index_adopt.argtypes = [C.POINTER(vp), C.c_char_p, vp, vp, u64, vp, vp, u64, C.c_char_p, u32, u32, u32, C.c_int]
    L.sa_hip_csv_index_destroy.restype = None
    L.sa_hip_csv_index_destroy.argtypes = [vp]
    L.sa_hip_get_matching_row_spans_file.restype = C.c_int
    L.sa_hip_get_matching_row_spans_file.argtypes = [vp, C.c_char_p, u32, C.POINTER(C.c_char_p), C.POINTER(u32), C.POINTER(u32)]
    L.sa_hip_csv_index_create_partitioned.restype = C.c_int
    L.sa_hip_csv_index_create_partitioned.argtypes = [C.POINTER(C.POINTER(vp)), C.POINTER(u32), C.c_char_p, C.c_char_p, u32, C.c_int, u64]
    L.sa_hip_csv_index_free_parts.restype = None
    L.sa_hip_csv_index_free_parts.argtypes = [C.POINTER(vp)]
    L.sa_hip_csv_index_handle.restype = vp
    L.sa_hip_csv_index_handle.argtypes = [vp]
    L.sa_hip_csv_index_num_rows.restype = u64
    L.sa_hip_csv_index_num_rows.argtypes = [vp]
    L.sa_hip_csv_index_num_columns.restype = u32
    L.sa_hip_csv_index_num_columns.argtypes = [vp]
    L.sa_hip_csv_index_column_index.restype = u32
    L.sa_hip_csv_index_column_index.argtypes = [vp]
    L.sa_hip_csv_index_column_name.restype = C.c_char_p
    L.sa_hip_csv_index_column_name.argtypes = [vp, u32]
    L.sa_hip_csv_index_row_tables.restype = C.c_int
    L.sa_hip_csv_index_row_tables.argtypes = [vp, C.POINTER(vp), C.POINTER(vp)]
    L.sa_hip_csv_index_copy_rows.restype = C.c_int
    L.sa_hip_csv_index_copy_rows.argtypes = [vp, vp, u32, C.POINTER(vp)]
    L.sa_hip_get_substring_positions_file.restype = PairU32
    L.sa_hip_get_substring_positions_file.argtypes = [vp, C.c_char_p]
    L.sa_hip_get_matching_records_file.restype = C.c_int
    L.sa_hip_get_matching_records_file.argtypes = [vp, C.c_char_p, u32, C.POINTER(vp), C.POINTER(u32)]
    L.sa_hip_get_matching_records.restype = u32
    L.sa_hip_get_matching_records.argtypes = [vp, C.POINTER(SuffixArrayStruct), C.c_char_p, u32, C.POINTER(vp)]
    L.sa_hip_free_records.restype = None
    L.sa_hip_free_records.argtypes = [C.POINTER(vp), u32]
    L.sa_hip_init_suffix_array_byte_idxs.restype = C.c_int
    L.sa_hip_init_suffix_array_byte_idxs.argtypes = [C.POINTER(SuffixArrayStruct), u32, u64, u64, u32]
    L.sa_hip_free_suffix_array.restype = None
    L.sa_hip_free_suffix_array.argtypes = [C.POINTER(SuffixArrayStruct)]
    L.sa_hip_write_suffix_array.restype = C.c_int
    L.sa_hip_write_suffix_array.argtypes = [C.POINTER(SuffixArrayStruct), C.c_char_p, C.c_char_p]
    L.sa_hip_read_suffix_array.restype = C.c_int
    L.sa_hip_read_suffix_array.argtypes = [C.POINTER(SuffixArrayStruct), C.c_char_p]
    L.sa_hip_token_index_build.restype = C.c_int
    L.sa_hip_token_index_build.argtypes = [C.POINTER(vp), vp, i32, i32, C.c_int]
    L.sa_hip_token_index_load_device.restype = C.c_int
    L.sa_hip_token_index_load_device.argtypes = [C.POINTER(vp), vp, vp, i32, C.c_int]
    L.sa_hip_token_index_destroy.restype = None
    L.sa_hip_token_index_destroy.argtypes = [vp]
    L.sa_hip_token_index_query_batch.restype = C.c_int
    L.sa_hip_token_index_query_batch.argtypes = [vp, vp, vp, u64, vp]
    L.sa_hip_token_index_query_batch_device.restype = C.c_int
    L.sa_hip_token_index_query_batch_device.argtypes = [vp, vp, vp, u64, vp]
    L.sa_hip_token_index_sync.restype = C.c_int
    L.sa_hip_token_index_sync.argtypes = [vp]
    L.sa_hip_token_index_text_dev.restype = vp
    L.sa_hip_token_index_text_dev.argtypes = [vp]
    L.sa_hip_token_index_sa_dev.restype = vp
    L.sa_hip_token_index_sa_dev.argtypes = [vp]
    L.sa_hip_token_index_get_sa_range.restype = C.c_int
    L.sa_hip_token_index_get_sa_range.argtypes = [vp, u64, u64, vp]
    L.sa_hip_token_index_get_dir_range.restype = C.c_int
    L.sa_hip_token_index_get_dir_range.argtypes = [vp, u64, u64, vp]
    L.sa_hip_token_index_get_key_range.restype = C.c_int
    L.sa_hip_token_index_get_key_range.argtypes = [vp, u64, u64, vp]
    L.sa_hip_token_index_info.restype = C.c_int
    L.sa_hip_token_index_info.argtypes = [vp, C.POINTER(TokenInfo)]
    L.sa_hip_token_index_spans_batch.restype = C.c_int
    L.sa_hip_token_index_spans_batch.argtypes = [vp, vp, vp, u64, C.c_int, C.c_uint32, C.c_int, vp]
    L.sa_hip_token_index_spans_batch_device.restype = C.c_int
    L.sa_hip_token_index_spans_batch_device.argtypes = [vp, vp, vp, u64, C.c_int, C.c_uint32, C.c_int, vp]
    L.sa_hip_token_index_next_batch_device.restype = C.c_int
    L.sa_hip_token_index_next_batch_device.argtypes = [vp, vp, u64, C.c_uint32, vp, vp, vp]
    L.sa_hip_token_index_next_batch.restype = C.c_int
    L.sa_hip_token_index_next_batch.argtypes = [vp, vp, vp, u64, C.c_int, C.c_uint32, C.c_int, C.c_uint32, vp, vp, vp, vp]
    L.sa_hip_token_index_next_of_spans.restype = C.c_int
    L.sa_hip_token_index_next_of_spans.argtypes = [vp, vp, u64, C.c_uint32, vp, vp, vp]
    L.sa_hip_token_index_next_info.restype = C.c_int
    L.sa_hip_token_index_next_info.argtypes = [vp, C.POINTER(TokenNextInfo)]
    L.sa_hip_token_index_set_documents.restype = C.c_int
    L.sa_hip_token_index_set_documents.argtypes = [vp, vp, C.c_uint32]
    L.sa_hip_token_index_get_doc_range.restype = C.c_int
    L.sa_hip_token_index_get_doc_range.argtypes = [vp, u64, u64, vp, vp]
    L.sa_hip_token_index_docs_info.restype = C.c_int
    L.sa_hip_token_index_docs_info.argtypes = [vp, C.POINTER(TokenDocsInfo)]
    L.sa_hip_token_index_locate_batch_device.restype = C.c_int
    L.sa_hip_token_index_locate_batch_device.argtypes = [vp, vp, u64, C.c_uint32, vp, vp, vp]
    L.sa_hip_token_index_locate_batch.restype = C.c_int
    L.sa_hip_token_index_locate_batch.argtypes = [vp, vp, vp, u64, C.c_uint32, vp, vp, vp, vp]
    L.sa_hip_token_index_docs_batch_device.restype = C.c_int
    L.sa_hip_token_index_docs_batch_device.argtypes = [vp, vp, u64, C.c_uint32, C.c_uint32, vp, vp, vp]
    L.sa_hip_token_index_docs_batch.restype = C.c_int
    L.sa_hip_token_index_docs_batch.argtypes = [vp, vp, vp, u64, C.c_int, C.c_uint32, C.c_int, C.c_uint32, C.c_uint32, vp, vp, vp, vp]
    L.sa_hip_token_index_prepare_doc_ranks.restype = C.c_int
    L.sa_hip_token_index_prepare_doc_ranks.argtypes = [vp, C.c_int]
    L.sa_hip_token_index_get_doc_ranks.restype = C.c_int
    L.sa_hip_token_index_get_doc_ranks.argtypes = [vp, u64, u64, vp]
    L.sa_hip_token_index_doc_ranks_info.restype = C.c_int
    L.sa_hip_token_index_doc_ranks_info.argtypes = [vp, C.POINTER(TokenDocRanksInfo)]
    L.sa_hip_token_index_doc_counts_batch_device.restype = C.c_int
    L.sa_hip_token_index_doc_counts_batch_device.argtypes = [vp, vp, u64, C.c_uint32, vp, vp, u64, vp]
    L.sa_hip_token_index_doc_counts_batch.restype = C.c_int
    L.sa_hip_token_index_doc_counts_batch.argtypes = [vp, vp, vp, u64, C.c_int, C.c_uint32, C.c_int, C.c_uint32, vp, vp, vp, vp]
    L.sa_hip_token_index_all_batch_device.restype = C.c_int
    L.sa_hip_token_index_all_batch_device.argtypes = [vp, vp, u64, vp, u64, C.c_uint32, C.c_uint32, vp, vp, vp]
    L.sa_hip_token_index_all_batch.restype = C.c_int
    L.sa_hip_token_index_all_batch.argtypes = [vp, vp, vp, u64, vp, u64, C.c_int, C.c_uint32, C.c_int, C.c_uint32, C.c_uint32, vp, vp, vp, vp]
    L.sa_hip_token_index_cnf_batch_device.restype = C.c_int
    L.sa_hip_token_index_cnf_batch_device.argtypes = [vp, vp, u64, vp, u64, vp, vp, u64, C.c_uint32, C.c_uint32, vp, vp, vp]
    L.sa_hip_token_index_cnf_batch.restype = C.c_int
    L.sa_hip_token_index_cnf_batch.argtypes = [vp, vp, vp, u64, vp, u64, vp, vp, u64, C.c_int, C.c_uint32, C.c_int, C.c_uint32, C.c_uint32,
                                               vp, vp, vp, vp]
    L.sa_hip_token_index_cnf_info.restype = C.c_int
    L.sa_hip_token_index_cnf_info.argtypes = [vp, C.POINTER(TokenCnfInfo)]
    L.sa_hip_token_index_match_batch_device.restype = C.c_int
    L.sa_hip_token_index_match_batch_device.argtypes = [vp, vp, vp, u64, u64, C.c_uint32, vp]
    L.sa_hip_token_index_match_docs_batch_device.restype = C.c_int
    L.sa_hip_token_index_match_docs_batch_device.argtypes = [vp, vp, vp, u64, C.c_uint32, C.c_uint32, vp, vp, vp]
    L.sa_hip_token_index_match_batch.restype = C.c_int
    L.sa_hip_token_index_match_batch.argtypes = [vp, vp, vp, u64, C.c_uint32, vp]
    L.sa_hip_token_index_match_docs_batch.restype = C.c_int
    L.sa_hip_token_index_match_docs_batch.argtypes = [vp, vp, vp, u64, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp, vp]
    L.sa_hip_token_index_match_info.restype = C.c_int
    L.sa_hip_token_index_match_info.argtypes = [vp, C.POINTER(TokenMatchInfo)]
    L.sa_hip_token_index_score_batch_device.restype = C.c_int
    L.sa_hip_token_index_score_batch_device.argtypes = [vp, vp, vp, u64, u64, C.c_uint32, vp, vp]
    L.sa_hip_token_index_score_docs_batch_device.restype = C.c_int
    L.sa_hip_token_index_score_docs_batch_device.argtypes = [vp, vp, vp, u64, vp]
    L.sa_hip_token_index_score_batch.restype = C.c_int
    L.sa_hip_token_index_score_batch.argtypes = [vp, vp, vp, u64, C.c_uint32, vp, vp]
    L.sa_hip_token_index_score_info.restype = C.c_int
    L.sa_hip_token_index_score_info.argtypes = [vp, C.POINTER(TokenScoreInfo)]
    L.sa_hip_token_index_top_batch_device.restype = C.c_int
    L.sa_hip_token_index_top_batch_device.argtypes = [vp, vp, u64, C.c_uint32, C.c_uint32, vp, vp, vp]
    L.sa_hip_token_index_top_batch.restype = C.c_int
    L.sa_hip_token_index_top_batch.argtypes = [vp, vp, vp, u64, C.c_int, C.c_uint32, C.c_int, C.c_uint32, C.c_uint32, vp, vp, vp, vp]
    L.sa_hip_token_index_sample_batch_device.restype = C.c_int
    L.sa_hip_token_index_sample_batch_device.argtypes = [vp, vp, u64, vp, C.c_uint32, vp, vp]
    L.sa_hip_token_index_sample_batch.restype = C.c_int
    L.sa_hip_token_index_sample_batch.argtypes = [vp, vp, vp, u64, C.c_int, C.c_uint32, C.c_int, vp, C.c_uint32, vp, vp, vp]
    L.sa_hip_token_index_top_info.restype = C.c_int
    L.sa_hip_token_index_top_info.argtypes = [vp, C.POINTER(TokenTopInfo)]
    L.sa_hip_token_shards_create.restype = C.c_int
    L.sa_hip_token_shards_create.argtypes = [C.POINTER(vp), vp, C.c_uint32]
    L.sa_hip_token_shards_destroy.restype = None
    L.sa_hip_token_shards_destroy.argtypes = [vp]
    L.sa_hip_token_shards_shard.restype = vp
    L.sa_hip_token_shards_shard.argtypes = [vp, C.c_uint32]
    L.sa_hip_token_shards_sync.restype = C.c_int
    L.sa_hip_token_shards_sync.argtypes = [vp]
    L.sa_hip_token_shards_info.restype = C.c_int
    L.sa_hip_token_shards_info.argtypes = [vp, C.POINTER(TokenShardsStats)]
    L.sa_hip_token_shards_query_batch.restype = C.c_int
    L.sa_hip_token_shards_query_batch.argtypes = [vp, vp, vp, u64, vp, vp]
    L.sa_hip_token_shards_query_batch_device.restype = C.c_int
    L.sa_hip_token_shards_query_batch_device.argtypes = [vp, vp, vp, u64, vp, vp]
    L.sa_hip_token_shards_spans_batch.restype = C.c_int
    L.sa_hip_token_shards_spans_batch.argtypes = [vp, vp, vp, u64, C.c_int, C.c_uint32, C.c_int, vp, vp, vp]
    L.sa_hip_token_shards_spans_batch_device.restype = C.c_int
    L.sa_hip_token_shards_spans_batch_device.argtypes = [vp, vp, vp, u64, C.c_int, C.c_uint32, C.c_int, vp, vp, vp]
    L.sa_hip_token_shards_next_batch.restype = C.c_int
    L.sa_hip_token_shards_next_batch.argtypes = [vp, vp, vp, u64, C.c_int, C.c_uint32, C.c_int, C.c_uint32, vp, vp, vp, vp]
    L.sa_hip_token_shards_next_batch_device.restype = C.c_int
    L.sa_hip_token_shards_next_batch_device.argtypes = [vp, vp, u64, C.c_uint32, vp, vp, vp]
    L.sa_hip_token_shards_merge_device.restype = C.c_int
    L.sa_hip_token_shards_merge_device.argtypes = [vp, vp, vp, vp, u64, C.c_uint32, vp, vp, vp]
    L.sa_hip_token_shards_match_batch_device.restype = C.c_int
    L.sa_hip_token_shards_match_batch_device.argtypes = [vp, vp, vp, u64, u64, C.c_uint32, vp, vp]
    L.sa_hip_token_shards_match_docs_batch_device.restype = C.c_int
    L.sa_hip_token_shards_match_docs_batch_device.argtypes = [vp, vp, vp, u64, C.c_uint32, C.c_uint32, vp, vp, vp]
    L.sa_hip_token_shards_match_batch.restype = C.c_int
    L.sa_hip_token_shards_match_batch.argtypes = [vp, vp, vp, u64, C.c_uint32, vp, vp]
    L.sa_hip_token_shards_match_docs_batch.restype = C.c_int
    L.sa_hip_token_shards_match_docs_batch.argtypes = [vp, vp, vp, u64, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp, vp]
    L.sa_hip_token_shards_match_info.restype = C.c_int
    L.sa_hip_token_shards_match_info.argtypes = [vp, C.POINTER(TokenShardsMatchStats)]
    L.sa_hip_token_shards_score_batch_device.restype = C.c_int
    L.sa_hip_token_shards_score_batch_device.argtypes = [vp, vp, vp, u64, u64, C.c_uint32, vp, vp, vp]
    L.sa_hip_token_shards_score_docs_batch_device.restype = C.c_int
    L.sa_hip_token_shards_score_docs_batch_device.argtypes = [vp, vp, vp, u64, vp]
    L.sa_hip_token_shards_score_batch.restype = C.c_int
    L.sa_hip_token_shards_score_batch.argtypes = [vp, vp, vp, u64, C.c_uint32, vp, vp, vp]
    L.sa_hip_token_shards_score_info.restype = C.c_int
    L.sa_hip_token_shards_score_info.argtypes = [vp, C.POINTER(TokenShardsScoreStats)]
    L.sa_hip_token_shards_top_batch_device.restype = C.c_int
    L.sa_hip_token_shards_top_batch_device.argtypes = [vp, vp, u64, C.c_uint32, u64, vp, vp, vp]
    L.sa_hip_token_shards_top_batch.restype = C.c_int
    L.sa_hip_token_shards_top_batch.argtypes = [vp, vp, vp, u64, C.c_int, C.c_uint32, C.c_int, C.c_uint32, u64, vp, vp, vp, vp]
    L.sa_hip_token_shards_sample_batch_device.restype = C.c_int
    L.sa_hip_token_shards_sample_batch_device.argtypes = [vp, vp, u64, vp, C.c_uint32, vp, vp, vp]
    L.sa_hip_token_shards_sample_batch.restype = C.c_int
    L.sa_hip_token_shards_sample_batch.argtypes = [vp, vp, vp, u64, C.c_int, C.c_uint32, C.c_int, vp, C.c_uint32, vp, vp, vp, vp]
    L.sa_hip_token_shards_top_info.restype = C.c_int
    L.sa_hip_token_shards_top_info.argtypes = [vp, C.POINTER(TokenShardsTopStats)]
    L.sa_hip_token_shards_set_documents.restype = C.c_int
    L.sa_hip_token_shards_set_documents.argtypes = [vp, vp, vp]
    L.sa_hip_token_shards_adopt_documents.restype = C.c_int
    L.sa_hip_token_shards_adopt_documents.argtypes = [vp]
    L.sa_hip_token_shards_doc_bases.restype = C.c_int
    L.sa_hip_token_shards_doc_bases.argtypes = [vp, vp]
    L.sa_hip_token_shards_docs_info.restype = C.c_int
    L.sa_hip_token_shards_docs_info.argtypes = [vp, C.POINTER(TokenShardsDocsStats)]
    L.sa_hip_token_shards_locate_batch_device.restype = C.c_int
    L.sa_hip_token_shards_locate_batch_device.argtypes = [vp, vp, u64, C.c_uint32, vp, vp, vp]
    L.sa_hip_token_shards_locate_batch.restype = C.c_int
    L.sa_hip_token_shards_locate_batch.argtypes = [vp, vp, vp, u64, C.c_uint32, vp, vp, vp, vp]
    L.sa_hip_token_shards_docs_batch_device.restype = C.c_int
    L.sa_hip_token_shards_docs_batch_device.argtypes = [vp, vp, u64, C.c_uint32, u64, vp, vp, vp]
    L.sa_hip_token_shards_docs_batch.restype = C.c_int
    L.sa_hip_token_shards_docs_batch.argtypes = [vp, vp, vp, u64, C.c_int, C.c_uint32, C.c_int, C.c_uint32, u64, vp, vp, vp, vp]
    L.sa_hip_token_shards_docs_merge_device.restype = C.c_int
    L.sa_hip_token_shards_docs_merge_device.argtypes = [vp, vp, vp, vp, vp, u64, C.c_uint32, vp, vp, vp]
    L.sa_hip_token_shards_prepare_doc_ranks.restype = C.c_int
    L.sa_hip_token_shards_prepare_doc_ranks.argtypes = [vp, C.c_int]
    L.sa_hip_token_shards_doc_ranks_info.restype = C.c_int
    L.sa_hip_token_shards_doc_ranks_info.argtypes = [vp, C.POINTER(TokenShardsRanksStats)]
    L.sa_hip_token_shards_doc_counts_batch_device.restype = C.c_int
    L.sa_hip_token_shards_doc_counts_batch_device.argtypes = [vp, vp, u64, C.c_uint32, vp, vp, u64, vp]
    L.sa_hip_token_shards_doc_counts_batch.restype = C.c_int
    L.sa_hip_token_shards_doc_counts_batch.argtypes = [vp, vp, vp, u64, C.c_int, C.c_uint32, C.c_int, C.c_uint32, vp, vp, vp, vp]
    L.sa_hip_token_shards_all_batch_device.restype = C.c_int
    L.sa_hip_token_shards_all_batch_device.argtypes = [vp, vp, u64, vp, u64, C.c_uint32, u64, vp, vp, vp]
    L.sa_hip_token_shards_all_batch.restype = C.c_int
    L.sa_hip_token_shards_all_batch.argtypes = [vp, vp, vp, u64, vp, u64, C.c_int, C.c_uint32, C.c_int, C.c_uint32, u64, vp, vp, vp, vp]
    L.sa_hip_token_shards_all_merge_device.restype = C.c_int
    L.sa_hip_token_shards_all_merge_device.argtypes = [vp, vp, vp, vp, vp, vp, u64, C.c_uint32, vp, vp, vp]
    L.sa_hip_sort_pairs.restype = C.c_int
    L.sa_hip_sort_pairs.argtypes = [vp, vp, u64, C.c_int, C.c_int, C.c_int]
    L.sa_hip_synth_uniform27.restype = None
    L.sa_hip_synth_uniform27.argtypes = [vp, u64, u64]
    L.sa_hip_last_error.restype = C.c_char_p
    L.sa_hip_last_error.argtypes = []
    L.sa_hip_version.restype = C.c_char_p
    L.sa_hip_version.argtypes = []
    _lib = L
    return L


def check(rc):
    if rc != 0:
        raise SaHipError(rc, lib().sa_hip_last_error().decode("utf-8", "replace"))


def as_u8(a):
    if isinstance(a, (bytes, bytearray, memoryview)):
        return np.frombuffer(a, dtype=np.uint8)
    return np.ascontiguousarray(a, dtype=np.uint8)


def pack_patterns(patterns):
    """list[bytes] -> (packed uint8 array, uint64 offsets[Q+1])"""
    off = np.zeros(len(patterns) + 1, dtype=np.uint64)
    if len(patterns):
        off[1:] = np.cumsum([len(p) for p in patterns], dtype=np.uint64)
    buf = np.frombuffer(b"".join(patterns), dtype=np.uint8) if len(patterns) else np.zeros(0, np.uint8)
    return buf, off


class DeviceIndex:
    """Handle API: text + suffix array resident in HBM (sa_hip_index)."""

    def __init__(self, n_max, device=0):
        self._h = C.c_void_p()
        self._lib = lib()
        self._device = int(device)
        check(self._lib.sa_hip_index_create(C.byref(self._h), int(n_max), int(device)))

    @classmethod
    def from_handle(cls, handle, owner=None):
        """Non-owning wrapper of an existing sa_hip_index* (an integer); `owner` is kept alive with it."""
        self = cls.__new__(cls)
        self._h = C.c_void_p(int(handle))
        self._lib = lib()
        self._borrowed = True
        self._owner = owner
        return self

    def close(self):
        if getattr(self, "_borrowed", False):
            self._h = C.c_void_p()
            return
        if getattr(self, "_h", None) is not None and self._h:
            self._lib.sa_hip_index_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- construction -------------------------------------------------------------------------
    def build(self, text, max_suffix_length=0):
        t = as_u8(text)
        check(self._lib.sa_hip_index_build(self._h, t.ctypes.data if t.size else None, t.size, max_suffix_length))
        return self

    def build_device(self, text_dev_ptr, n, max_suffix_length=0):
        check(self._lib.sa_hip_index_build_device(self._h, text_dev_ptr, n, max_suffix_length))
        return self

    def build_device64(self, text_dev_ptr, n, sa64_dev_ptr, max_suffix_length=0):
        """Device build that also leaves the suffix array in libsais64 layout (int64[n]) in a device buffer."""
        check(self._lib.sa_hip_index_build_device64(self._h, text_dev_ptr, n, max_suffix_length, sa64_dev_ptr))
        return self

    def load(self, text, sa, max_suffix_length=0):
        t = as_u8(text)
        s = np.ascontiguousarray(sa, dtype=np.uint32)
        assert s.size == t.size
        check(self._lib.sa_hip_index_load(self._h, t.ctypes.data if t.size else None,
                                          s.ctypes.data if s.size else None, t.size, max_suffix_length))
        return self

    def load_device(self, text_dev_ptr, sa_dev_ptr, n, max_suffix_length=0):
        check(self._lib.sa_hip_index_load_device(self._h, text_dev_ptr, sa_dev_ptr, n, max_suffix_length))
        return self

    # -- replicas: the query structures travel as they are (no rebuilding on the receiving side) ------------
    def replica_layout(self):
        lay = ReplicaLayout()
        check(self._lib.sa_hip_index_replica_layout(self._h, C.byref(lay)))
        return lay

    def replica_buffers(self):
        """Device buffers of this (built) index: the source of a replication."""
        b = ReplicaBuffers()
        check(self._lib.sa_hip_index_replica_buffers(self._h, C.byref(b)))
        return b

    def replica_reserve(self, layout):
        """Allocate buffers for `layout`; returns where the caller has to put the data (then replica_commit)."""
        b = ReplicaBuffers()
        check(self._lib.sa_hip_index_replica_reserve(self._h, C.byref(layout), C.byref(b)))
        return b

    def replica_commit(self):
        check(self._lib.sa_hip_index_replica_commit(self._h))

    @property
    def stream(self):
        """The index's hipStream_t as an integer (torch.cuda.ExternalStream wraps it for event ordering)."""
        return self._lib.sa_hip_index_stream(self._h)

    # -- accessors ----------------------------------------------------------------------------
    @property
    def n(self):
        return int(self._lib.sa_hip_index_n(self._h))

    @property
    def max_suffix_length(self):
        return int(self._lib.sa_hip_index_max_suffix_length(self._h))

    @property
    def text_dev(self):
        return self._lib.sa_hip_index_text_dev(self._h)

    @property
    def sa_dev(self):
        return self._lib.sa_hip_index_sa_dev(self._h)

    def text(self):
        """The indexed text (n bytes) copied back to the host (CSV mode: the extracted column)."""
        out = np.empty(max(self.n, 1), dtype=np.uint8)
        check(self._lib.sa_hip_index_get_text(self._h, out.ctypes.data))
        return out[:self.n]

    def sa_u32(self):
        out = np.empty(max(self.n, 1), dtype=np.uint32)
        check(self._lib.sa_hip_index_get_sa_u32(self._h, out.ctypes.data))
        return out[:self.n]

    def sa_i64(self):
        out = np.empty(max(self.n, 1), dtype=np.int64)
        check(self._lib.sa_hip_index_get_sa_i64(self._h, out.ctypes.data))
        return out[:self.n]

    def widen_device(self, out_dev_ptr):
        """int64[n] libsais64-layout copy of the suffix array into a device buffer (asynchronous)."""
        check(self._lib.sa_hip_index_widen_device(self._h, out_dev_ptr))

    def sa_range(self, first, count):
        out = np.empty(max(count, 1), dtype=np.uint32)
        check(self._lib.sa_hip_index_get_sa_range(self._h, first, count, out.ctypes.data))
        return out[:count]

    def query_hits(self, pattern: bytes, max_hits: int = 4096):
        """One query and its first hits in one call: ((first, second), SA[first .. first + nhits))."""
        rng = PairU32()
        hits = np.empty(max(min(max_hits, 4096), 1), dtype=np.uint32)
        nh = C.c_uint32(0)
        check(self._lib.sa_hip_index_query_hits(self._h, pattern, len(pattern), min(max_hits, 4096), C.byref(rng),
                                                hits.ctypes.data, C.byref(nh)))
        return (rng.first, rng.second), hits[:nh.value]

    def freq(self):
        out = np.zeros(256, dtype=np.uint64)
        check(self._lib.sa_hip_index_get_freq(self._h, out.ctypes.data))
        return out

    def sync(self):
        check(self._lib.sa_hip_index_sync(self._h))

    # -- LCP arrays (sa_hip_index_[p]lcp_device; full suffix arrays only) ------------------------
    def plcp_device(self, out_dev_ptr, stats=False):
        """PLCP (text order) as u32[n] into a device buffer of the index's device.  Asynchronous on the index's stream;
        stats=True waits and returns the sa_hip_lcp_stats of the pass as a dict."""
        st = LcpStats() if stats else None
        check(self._lib.sa_hip_index_plcp_device(self._h, out_dev_ptr, C.byref(st) if st is not None else None))
        return st.as_dict() if st is not None else None

    def lcp_device(self, out_dev_ptr, stats=False):
        """LCP (SA order: LCP[r] = PLCP[SA[r]]) as u32[n] into a device buffer, as plcp_device."""
        st = LcpStats() if stats else None
        check(self._lib.sa_hip_index_lcp_device(self._h, out_dev_ptr, C.byref(st) if st is not None else None))
        return st.as_dict() if st is not None else None

    def lcp(self, plcp=False):
        """LCP (or, plcp=True, PLCP) of the index as a numpy uint32 array.  The device buffer comes from torch (a ROCm
        build), which is how this package's callers hold device memory; nothing but its address reaches the C ABI."""
        import torch
        n = self.n
        buf = torch.empty(max(n, 1), dtype=torch.int32, device=f"cuda:{getattr(self, '_device', 0)}")
        torch.cuda.synchronize(buf.device)
        (self.plcp_device if plcp else self.lcp_device)(buf.data_ptr())
        self.sync()
        return buf[:n].cpu().numpy().view(np.uint32)

    # -- BWT (sa_hip_index_bwt_device; full suffix arrays only) -----------------------------------
    def bwt_device(self, U_dev_ptr, r=None, I_dev_ptr=None, stats=False):
        """BWT of the index into a device buffer of n bytes (libsais conventions).  With r (a power of two >= 2) and
        I_dev_ptr ((n-1)//r + 1 uint32 entries): the aux rows.  Synchronous.  Returns the primary index, or
        (primary, stats dict) with stats=True."""
        st = BwtStats() if stats else None
        p = C.c_int64(0)
        check(self._lib.sa_hip_index_bwt_device(self._h, U_dev_ptr, int(r or 0), I_dev_ptr, C.byref(p),
                                                C.byref(st) if st is not None else None))
        return (p.value, st.as_dict()) if st is not None else p.value

    def bwt(self, r=None):
        """(U: uint8[n], primary) -- or, with r, (U, I: int64[(n-1)//r + 1]) as libsais_bwt_aux -- through device buffers
        taken from torch, as lcp() does."""
        import torch
        n = self.n
        dev = f"cuda:{getattr(self, '_device', 0)}"
        u = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)
        aux = torch.empty(max((n - 1) // r + 1, 1), dtype=torch.int32, device=dev) if r else None
        torch.cuda.synchronize(u.device)
        p = self.bwt_device(u.data_ptr(), r, aux.data_ptr() if aux is not None else None)
        U = u[:n].cpu().numpy()
        if r:
            return U, aux[:max((n - 1) // r + 1, 1)].cpu().numpy().view(np.uint32).astype(np.int64)
        return U, p

    def deep_keys(self, mode=2):
        """Second-level keys for patterns longer than the key (sa_hip_index_deep_keys): 2 = build now, 1 = large batches build
        them (default of a handle), 0 = drop and never build.  True when the index has them afterwards."""
        rc = self._lib.sa_hip_index_deep_keys(self._h, mode)
        if rc < 0:
            check(rc)
        return rc == 1

    def prepare_deep_keys(self):
        return self.deep_keys(2)

    def verify(self):
        """Number of violations of the suffix-array property found on the device (0 = verified)."""
        v = C.c_uint64(0)
        check(self._lib.sa_hip_index_verify(self._h, C.byref(v)))
        return int(v.value)

    def build_stats(self):
        st = BuildStats()
        check(self._lib.sa_hip_index_build_stats(self._h, C.byref(st)))
        return st.as_dict()

    def query_stats(self):
        st = QueryStats()
        check(self._lib.sa_hip_index_query_stats(self._h, C.byref(st)))
        return {"q": st.q, "kernel_ms": st.kernel_ms, "kernel_ms_sum": st.kernel_ms_sum, "launches": st.launches}

    # -- query ----------------------------------------------------------------------------------
    def query_batch(self, patterns):
        """patterns: list[bytes] or (packed uint8, uint64 offsets).  -> structured array (first, second)."""
        buf, off = patterns if isinstance(patterns, tuple) else pack_patterns(patterns)
        buf = np.ascontiguousarray(buf, dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.uint64)
        q = off.size - 1
        out = np.zeros(max(q, 1), dtype=PAIR_DTYPE)
        if q:
            check(self._lib.sa_hip_query_batch(self._h, buf.ctypes.data if buf.size else None, off.ctypes.data, q,
                                               out.ctypes.data))
        return out[:q]

    def set_rows(self, row_text_starts):
        r = np.ascontiguousarray(row_text_starts, dtype=np.uint64)
        check(self._lib.sa_hip_index_set_rows(self._h, r.ctypes.data if r.size else None, r.size))

    def query_rows(self, pattern: bytes, k):
        """ONE query -> (row ids in SA order of their first hit, (first, second))."""
        rows = np.empty(max(k, 1), dtype=np.uint64)
        n = C.c_uint32(0)
        rng = PairU32()
        check(self._lib.sa_hip_index_query_rows(self._h, pattern, len(pattern), k, rows.ctypes.data, C.byref(n), C.byref(rng)))
        return rows[:n.value].copy(), (rng.first, rng.second)

    def query_rows_batch(self, patterns, k):
        """A batch -> (list of row-id arrays, structured ranges): one search launch + one rows launch."""
        buf, off = patterns if isinstance(patterns, tuple) else pack_patterns(patterns)
        buf = np.ascontiguousarray(buf, dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.uint64)
        q = off.size - 1
        rows = np.empty((max(q, 1), max(k, 1)), dtype=np.uint64)
        counts = np.zeros(max(q, 1), dtype=np.uint32)
        ranges = np.zeros(max(q, 1), dtype=PAIR_DTYPE)
        if q:
            check(self._lib.sa_hip_index_query_rows_batch(self._h, buf.ctypes.data if buf.size else None, off.ctypes.data, q, k,
                                                          rows.ctypes.data, counts.ctypes.data, ranges.ctypes.data))
        return [rows[i, :counts[i]].copy() for i in range(q)], ranges[:q]

    def query_rows_batch_raw(self, patterns, k, out=None):
        """query_rows_batch without the per-query Python list: ((row_ids uint64[Q, k], counts uint32[Q]), ranges).
        out: (rows, counts, ranges) of an earlier call with the same Q and k, to be overwritten -- the C entry point fills
        caller-provided arrays (as engine.c:1326 does), and a loop that answers batch after batch keeps its arrays instead of
        mapping and unmapping Q x k x 8 bytes per call (1.28 GB at Q = 1e7, k = 16: ~60 ms of page-table work per step)."""
        buf, off = patterns if isinstance(patterns, tuple) else pack_patterns(patterns)
        buf = np.ascontiguousarray(buf, dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.uint64)
        q = off.size - 1
        if out is not None:
            rows, counts, ranges = out
            if (rows.shape != (max(q, 1), max(k, 1)) or rows.dtype != np.uint64 or counts.shape != (max(q, 1),) or counts.dtype != np.uint32
                    or ranges.shape != (max(q, 1),) or ranges.dtype != PAIR_DTYPE
                    or not (rows.flags.c_contiguous and counts.flags.c_contiguous and ranges.flags.c_contiguous)):
                raise ValueError("query_rows_batch_raw: `out` does not fit this batch")
        else:
            rows = np.empty((max(q, 1), max(k, 1)), dtype=np.uint64)
            counts = np.zeros(max(q, 1), dtype=np.uint32)
            ranges = np.zeros(max(q, 1), dtype=PAIR_DTYPE)
        if q:
            check(self._lib.sa_hip_index_query_rows_batch(self._h, buf.ctypes.data if buf.size else None, off.ctypes.data, q, k,
                                                          rows.ctypes.data, counts.ctypes.data, ranges.ctypes.data))
        return (rows[:q], counts[:q]), ranges[:q]

    def query_batch_device(self, patterns_dev_ptr, offsets_dev_ptr, q, out_dev_ptr):
        check(self._lib.sa_hip_query_batch_device(self._h, patterns_dev_ptr, offsets_dev_ptr, q, out_dev_ptr))

    def query_batch_device_fixed(self, patterns_dev_ptr, pattern_len, q, out_dev_ptr):
        """q patterns of pattern_len bytes each, packed back to back in device memory (no offsets array)."""
        check(self._lib.sa_hip_query_batch_device_fixed(self._h, patterns_dev_ptr, pattern_len, q, out_dev_ptr))


class Comm:
    """sa_hip_comm: RCCL communicator of the C ABI (one process per GPU; no torch involved)."""

    @staticmethod
    def unique_id():
        buf = C.create_string_buffer(128)
        check(lib().sa_hip_comm_unique_id(buf))
        return buf.raw

    def __init__(self, unique_id: bytes, nranks, rank, device=0):
        self._lib = lib()
        self._h = C.c_void_p()
        check(self._lib.sa_hip_comm_create(C.byref(self._h), unique_id, nranks, rank, device))

    @property
    def rank(self):
        return self._lib.sa_hip_comm_rank(self._h)

    @property
    def size(self):
        return self._lib.sa_hip_comm_size(self._h)

    def replicate_index(self, idx, root=0):
        n = C.c_uint64(0)
        check(self._lib.sa_hip_comm_replicate_index(self._h, idx._h, root, C.byref(n)))
        return int(n.value)

    def allgather_ranges(self, idx, send_dev_ptr, pairs_per_rank, recv_dev_ptr):
        check(self._lib.sa_hip_comm_allgather_ranges(self._h, idx._h, send_dev_ptr, pairs_per_rank, recv_dev_ptr))

    def close(self):
        if self._h:
            self._lib.sa_hip_comm_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


# -- libsais- / engine-compatible one-shot wrappers ----------------------------------------------

def last_call_breakdown():
    """Where the time of the last libsais-compatible one-shot call of this process went (sa_hip_call_breakdown)."""
    b = CallBreakdown()
    check(lib().sa_hip_last_call_breakdown(C.byref(b)))
    return b.as_dict()


def release_workspace():
    lib().sa_hip_release_workspace()


def libsais(text, want_freq=False):
    t = as_u8(text)
    sa = np.empty(max(t.size, 1), dtype=np.int32)
    freq = np.zeros(256, dtype=np.int32)
    rc = lib().sa_hip_libsais(t.ctypes.data, sa.ctypes.data, t.size, 0, freq.ctypes.data if want_freq else None)
    check(rc)
    return (sa[:t.size], freq) if want_freq else sa[:t.size]


def libsais64(text, want_freq=False):
    t = as_u8(text)
    sa = np.empty(max(t.size, 1), dtype=np.int64)
    freq = np.zeros(256, dtype=np.int64)
    rc = lib().sa_hip_libsais64(t.ctypes.data, sa.ctypes.data, t.size, 0, freq.ctypes.data if want_freq else None)
    check(int(rc))
    return (sa[:t.size], freq) if want_freq else sa[:t.size]


def libsais64_device(text_ptr, sa_ptr, n, device=0):
    """The 64-bit-index build (csrc/big_build.hpp) on device buffers: text_ptr = n bytes, sa_ptr = n int64 entries.  Returns its stats."""
    st = BigStats()
    check(lib().sa_hip_libsais64_device(text_ptr, sa_ptr, n, device, C.byref(st)))
    return st.as_dict()


def libsais_plcp(text, sa):
    """PLCP of (text, suffix array) through sa_hip_libsais_plcp: int32[n] in text order."""
    t = as_u8(text)
    s = np.ascontiguousarray(sa, dtype=np.int32)
    assert s.size == t.size
    out = np.empty(max(t.size, 1), dtype=np.int32)
    check(lib().sa_hip_libsais_plcp(t.ctypes.data, s.ctypes.data, out.ctypes.data, t.size))
    return out[:t.size]


def libsais_lcp(plcp, sa):
    """LCP from PLCP and the suffix array through sa_hip_libsais_lcp: int32[n] in SA order."""
    p = np.ascontiguousarray(plcp, dtype=np.int32)
    s = np.ascontiguousarray(sa, dtype=np.int32)
    assert s.size == p.size
    out = np.empty(max(p.size, 1), dtype=np.int32)
    check(lib().sa_hip_libsais_lcp(p.ctypes.data, s.ctypes.data, out.ctypes.data, p.size))
    return out[:p.size]


def libsais64_plcp(text, sa):
    t = as_u8(text)
    s = np.ascontiguousarray(sa, dtype=np.int64)
    assert s.size == t.size
    out = np.empty(max(t.size, 1), dtype=np.int64)
    check(int(lib().sa_hip_libsais64_plcp(t.ctypes.data, s.ctypes.data, out.ctypes.data, t.size)))
    return out[:t.size]


def libsais64_lcp(plcp, sa):
    p = np.ascontiguousarray(plcp, dtype=np.int64)
    s = np.ascontiguousarray(sa, dtype=np.int64)
    assert s.size == p.size
    out = np.empty(max(p.size, 1), dtype=np.int64)
    check(int(lib().sa_hip_libsais64_lcp(p.ctypes.data, s.ctypes.data, out.ctypes.data, p.size)))
    return out[:p.size]


def plcp64_device(text_ptr, sa_ptr, out_ptr, n, device=0):
    """PLCP with 64-bit indices on device buffers: text n bytes (8-byte aligned), sa / out n int64 entries.  Returns the stats."""
    st = LcpStats()
    check(lib().sa_hip_plcp64_device(text_ptr, sa_ptr, out_ptr, n, device, C.byref(st)))
    return st.as_dict()


def lcp64_device(text_ptr, sa_ptr, out_ptr, n, device=0):
    """LCP (SA order) with 64-bit indices on device buffers, as plcp64_device."""
    st = LcpStats()
    check(lib().sa_hip_lcp64_device(text_ptr, sa_ptr, out_ptr, n, device, C.byref(st)))
    return st.as_dict()


def libsais_bwt(text, r=None, freq=False, threads=0):
    """BWT through sa_hip_libsais_bwt[_aux]_omp: (U: uint8[n], primary) or, with r, (U, I: int32[(n-1)//r + 1]);
    freq=True appends the 256-bin int32 histogram."""
    return _bwt(text, r, freq, threads, 32)


def libsais64_bwt(text, r=None, freq=False, threads=0):
    """As libsais_bwt through sa_hip_libsais64_bwt[_aux]_omp (int64 I and freq)."""
    return _bwt(text, r, freq, threads, 64)


def _bwt(text, r, freq, threads, bits):
    t = as_u8(text)
    n = t.size
    it = np.int32 if bits == 32 else np.int64
    L = lib()
    pre = "sa_hip_libsais" if bits == 32 else "sa_hip_libsais64"
    U = np.empty(max(n, 1), dtype=np.uint8)
    A = np.empty(1, dtype=it)   # validated, never used
    f = np.zeros(256, dtype=it)
    fp = f.ctypes.data if freq else None
    if r:
        I = np.zeros((n - 1) // r + 1 if n else 1, dtype=it)
        rc = int(getattr(L, pre + "_bwt_aux_omp")(t.ctypes.data, U.ctypes.data, A.ctypes.data, n, 0, fp, int(r), I.ctypes.data, threads))
        check(rc)
        out = (U[:n], I)
    else:
        rc = int(getattr(L, pre + "_bwt_omp")(t.ctypes.data, U.ctypes.data, A.ctypes.data, n, 0, fp, threads))
        if rc < 0:
            check(rc)
        out = (U[:n], rc)
    return out + (f,) if freq else out


def libsais_unbwt(u, primary=None, I=None, r=None, freq=None, threads=0):
    """Inverse BWT through sa_hip_libsais_unbwt[_aux]_omp: the text as uint8[n].  Either primary, or I with r."""
    return _unbwt(u, primary, I, r, freq, threads, 32)


def libsais64_unbwt(u, primary=None, I=None, r=None, freq=None, threads=0):
    return _unbwt(u, primary, I, r, freq, threads, 64)


def _unbwt(u, primary, I, r, freq, threads, bits):
    b = as_u8(u)
    n = b.size
    it = np.int32 if bits == 32 else np.int64
    L = lib()
    pre = "sa_hip_libsais" if bits == 32 else "sa_hip_libsais64"
    out = np.empty(max(n, 1), dtype=np.uint8)
    A = np.empty(1, dtype=it)
    fp = np.ascontiguousarray(freq, dtype=it).ctypes.data if freq is not None else None
    if I is None:
        rc = int(getattr(L, pre + "_unbwt_omp")(b.ctypes.data, out.ctypes.data, A.ctypes.data, n, fp, int(primary), threads))
    else:
        Ia = np.ascontiguousarray(I, dtype=it)
        rc = int(getattr(L, pre + "_unbwt_aux_omp")(b.ctypes.data, out.ctypes.data, A.ctypes.data, n, fp, int(r), Ia.ctypes.data, threads))
    check(rc)
    return out[:n]


def bwt64_device(text_ptr, sa_ptr, u_ptr, n, r=None, I_ptr=None, device=0):
    """BWT with 64-bit indices on device buffers: (primary or 0, stats dict); I_ptr: (n-1)//r + 1 int64 entries."""
    st = BwtStats()
    rc = int(lib().sa_hip_bwt64_device(text_ptr, sa_ptr, u_ptr, n, int(r or 0), I_ptr, device, C.byref(st)))
    if rc < 0:
        check(rc)
    return rc, st.as_dict()


def unbwt64_device(u_ptr, out_ptr, n, r, I_ptr, device=0):
    """Inverse BWT with 64-bit indices on device buffers (r = n for a single primary index in I_ptr[0]).  Returns the stats."""
    st = BwtStats()
    check(lib().sa_hip_unbwt64_device(u_ptr, out_ptr, n, int(r), I_ptr, device, C.byref(st)))
    return st.as_dict()


def sufcheck64_device(text_ptr, sa_ptr, n, device=0):
    """Slots at which the int64 array on the device is not the suffix array of the text (0 = it is)."""
    v = C.c_uint64(0)
    check(lib().sa_hip_sufcheck64_device(text_ptr, sa_ptr, n, device, C.byref(v)))
    return int(v.value)


def _int_text(T, dtype):
    t = np.asarray(T)
    if t.dtype != dtype:
        if t.size and (int(t.min()) < np.iinfo(dtype).min or int(t.max()) > np.iinfo(dtype).max):
            raise ValueError("symbol does not fit %s" % np.dtype(dtype).name)
        t = t.astype(dtype)
    return np.ascontiguousarray(t)


def _int_k(t, k):
    return int(t.max()) + 1 if (k is None and t.size) else (1 if k is None else int(k))


def libsais_int(T, k=None, threads=0):
    """Suffix array of an int32 text with symbols in [0, k) through sa_hip_libsais_int_omp (k defaults to max + 1): int32[n].
    T is not modified."""
    t = _int_text(T, np.int32)
    sa = np.empty(max(t.size, 1), dtype=np.int32)
    check(int(lib().sa_hip_libsais_int_omp(t.ctypes.data, sa.ctypes.data, t.size, _int_k(t, k), 0, threads)))
    return sa[:t.size]


def libsais64_long(T, k=None, threads=0):
    """As libsais_int for int64 texts through sa_hip_libsais64_long_omp: int64[n]."""
    t = _int_text(T, np.int64)
    sa = np.empty(max(t.size, 1), dtype=np.int64)
    check(int(lib().sa_hip_libsais64_long_omp(t.ctypes.data, sa.ctypes.data, t.size, _int_k(t, k), 0, threads)))
    return sa[:t.size]


def libsais_plcp_int(T, SA):
    """PLCP of (int32 text, suffix array) through sa_hip_libsais_plcp_int: int32[n] in text order."""
    t = _int_text(T, np.int32)
    s = np.ascontiguousarray(SA, dtype=np.int32)
    assert s.size == t.size
    out = np.empty(max(t.size, 1), dtype=np.int32)
    check(int(lib().sa_hip_libsais_plcp_int(t.ctypes.data, s.ctypes.data, out.ctypes.data, t.size)))
    return out[:t.size]


def libsais_int_device(T_ptr, SA_ptr, n, k, device=0):
    """The int32 build on device buffers: T_ptr n int32 symbols in [0, k), SA_ptr n int32 entries.  Returns the stats."""
    st = IntStats()
    check(lib().sa_hip_libsais_int_device(T_ptr, SA_ptr, n, k, device, C.byref(st)))
    return st.as_dict()


def libsais64_long_device(T_ptr, SA_ptr, n, k, device=0):
    """The int64 build on device buffers: T_ptr n int64 symbols in [0, k), SA_ptr n int64 entries.  Returns the stats."""
    st = IntStats()
    check(lib().sa_hip_libsais64_long_device(T_ptr, SA_ptr, n, k, device, C.byref(st)))
    return st.as_dict()


def plcp_int_device(T_ptr, SA_ptr, out_ptr, n, device=0):
    """PLCP of an int32 text on device buffers (T, SA, out: n int32 entries each).  Returns the stats."""
    st = LcpStats()
    check(lib().sa_hip_plcp_int_device(T_ptr, SA_ptr, out_ptr, n, device, C.byref(st)))
    return st.as_dict()


def sufcheck_long_device(T_ptr, SA_ptr, n, device=0):
    """Slots at which the int64 array on the device is not the suffix array of the int64 text (0 = it is)."""
    v = C.c_uint64(0)
    check(lib().sa_hip_sufcheck_long_device(T_ptr, SA_ptr, n, device, C.byref(v)))
    return int(v.value)


def pack_ngrams(ngrams):
    """list of int sequences -> (packed int32 array, uint64 offsets[Q+1]); a symbol that does not fit int32 raises"""
    off = np.zeros(len(ngrams) + 1, dtype=np.uint64)
    if len(ngrams):
        off[1:] = np.cumsum([len(g) for g in ngrams], dtype=np.uint64)
    flat = [int(v) for g in ngrams for v in g]
    if flat and (min(flat) < -2 ** 31 or max(flat) > 2 ** 31 - 1):
        raise ValueError("pattern symbol does not fit int32")
    return np.array(flat, dtype=np.int32), off


def _ptr(a):
    """the address of an array; None for None and for an array without cells"""
    return a.ctypes.data if a is not None and a.size else None


def _rows(q, dtype, cap=None, fill=0):
    """An output of the host forms, filled: [max(q, 1)], or [max(q, 1), cap] with a cap (the library gets a row even when the batch
    is empty; the caller cuts to q).  An unsigned array takes the fill modulo its width."""
    dt = np.dtype(dtype)
    if dt.kind == "u":
        fill &= (1 << 8 * dt.itemsize) - 1
    shape = max(q, 1) if cap is None else (max(q, 1), cap)
    return np.full(shape, fill, dtype=dt) if fill else np.zeros(shape, dtype=dt)


def _range_args(first, count):
    """(first, count) of a read-back as non-negative ints (a negative one would reach the library as a huge uint64)"""
    first, count = int(first), int(count)
    if first < 0 or count < 0:
        raise ValueError("first and count are non-negative")
    return first, count


class _TokenHandle:
    """What TokenIndex and TokenShards share: the handle and its release through the library's _destroy, the packing of a host
    batch, the call of a host form and the *_info calls."""
    _destroy = None

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            getattr(self._lib, self._destroy)(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @staticmethod
    def _packed(patterns):
        buf, off = patterns if isinstance(patterns, tuple) else pack_ngrams(patterns)
        return np.ascontiguousarray(buf, dtype=np.int32), np.ascontiguousarray(off, dtype=np.uint64)

    @classmethod
    def _contexts(cls, patterns):
        """-> (packed int32, uint64 offsets, Q) of a host batch"""
        buf, off = cls._packed(patterns)
        return buf, off, max(off.size - 1, 0)

    def _call(self, q, fn, *args):
        """the host form fn on the handle; an empty batch does not reach the library"""
        if q > 0:
            check(fn(self._h, *args))

    def _info(self, fn, struct_cls):
        st = struct_cls()
        check(fn(self._h, C.byref(st)))
        return st.as_dict()


class TokenIndex(_TokenHandle):
    """Handle API of the token index (sa_hip_token_index): an int32 text, its suffix array and the n-gram search structures in
    HBM.  Results are structured (first, second) = (suffixes that sort before the pattern, occurrences)."""
    _destroy = "sa_hip_token_index_destroy"

    def __init__(self, handle):
        self._h = handle
        self._lib = lib()

    @classmethod
    def build(cls, tokens, k=None, device=0):
        """From a host text of symbols in [0, k) (k defaults to max + 1): upload, device build, search structures."""
        t = _int_text(tokens, np.int32)
        h = C.c_void_p()
        k = min(_int_k(t, k), 2 ** 31 - 1)   # (k = INT32_MAX admits the symbol 2^31 - 1 too)
        check(lib().sa_hip_token_index_build(C.byref(h), _ptr(t), t.size, k, int(device)))
        return cls(h)

    @classmethod
    def load_device(cls, text_dev_ptr, sa_dev_ptr, n, device=0):
        """Adopt n int32 symbols and their int32 suffix array from device memory (copied into the handle)."""
        h = C.c_void_p()
        check(lib().sa_hip_token_index_load_device(C.byref(h), text_dev_ptr, sa_dev_ptr, int(n), int(device)))
        return cls(h)

    def query_batch(self, patterns):
        """patterns: list of int sequences or (packed int32, uint64 offsets).  -> structured array (first, second)."""
        buf, off, q = self._contexts(patterns)
        out = _rows(q, PAIR_DTYPE)
        self._call(q, self._lib.sa_hip_token_index_query_batch, _ptr(buf), _ptr(off), q, _ptr(out))
        return out[:q]

    def query_batch_device(self, patterns_dev_ptr, offsets_dev_ptr, q, out_dev_ptr):
        """Every buffer on the device; asynchronous on the handle's stream until sync()."""
        check(self._lib.sa_hip_token_index_query_batch_device(self._h, patterns_dev_ptr, offsets_dev_ptr, q, out_dev_ptr))

    def sync(self):
        check(self._lib.sa_hip_token_index_sync(self._h))

    @property
    def text_dev(self):
        return self._lib.sa_hip_token_index_text_dev(self._h)

    @property
    def sa_dev(self):
        return self._lib.sa_hip_token_index_sa_dev(self._h)

    def sa_range(self, first, count):
        out = np.empty(max(count, 1), dtype=np.int32)
        check(self._lib.sa_hip_token_index_get_sa_range(self._h, int(first), int(count), out.ctypes.data))
        return out[:count]

    def dir_range(self, first, count):
        """-> uint32 entries [first, first + count) of the first-symbol directory; raises when the handle has none"""
        first, count = _range_args(first, count)
        out = np.empty(max(count, 1), dtype=np.uint32)
        check(self._lib.sa_hip_token_index_get_dir_range(self._h, int(first), int(count), out.ctypes.data))
        return out[:count]

    def key_range(self, first, count):
        """-> uint64 entries [first, first + count) of the key array; raises when the handle has none"""
        first, count = _range_args(first, count)
        out = np.empty(max(count, 1), dtype=np.uint64)
        check(self._lib.sa_hip_token_index_get_key_range(self._h, int(first), int(count), out.ctypes.data))
        return out[:count]

    def info(self):
        return self._info(self._lib.sa_hip_token_index_info, TokenInfo)

    def spans_batch(self, patterns, mode=0, max_length=0, need_next=True):
        """patterns as in query_batch.  mode 0: the span of every whole pattern; mode 1: of its longest suffix that occurs (with
        a next symbol when need_next), at most max_length symbols (0: no cap).  -> structured array (first, count, length, ended)."""
        buf, off, q = self._contexts(patterns)
        out = _rows(q, SPAN_DTYPE)
        self._call(q, self._lib.sa_hip_token_index_spans_batch, _ptr(buf), _ptr(off), q, int(mode), int(max_length), int(bool(need_next)), _ptr(out))
        return out[:q]

    def spans_batch_device(self, patterns_dev_ptr, offsets_dev_ptr, q, mode, max_length, need_next, spans_dev_ptr):
        """Every buffer on the device; asynchronous on the handle's stream until sync()."""
        check(self._lib.sa_hip_token_index_spans_batch_device(self._h, patterns_dev_ptr, offsets_dev_ptr, q, int(mode), int(max_length),
                                                              int(bool(need_next)), spans_dev_ptr))

    def next_batch_device(self, spans_dev_ptr, q, cap, symbols_dev_ptr, counts_dev_ptr, heads_dev_ptr):
        """Next symbols of q device spans, at most cap entries each; asynchronous on the handle's stream until sync()."""
        check(self._lib.sa_hip_token_index_next_batch_device(self._h, spans_dev_ptr, q, int(cap), symbols_dev_ptr, counts_dev_ptr,
                                                             heads_dev_ptr))

    def next_batch(self, patterns, cap=64, mode=0, max_length=0, need_next=True, fill=0):
        """Spans as in spans_batch, then their next symbols.  -> dict: spans [Q], symbols int32[Q, cap], counts uint32[Q, cap],
        heads (written, covered, total, reserved)[Q].  Cells beyond heads['written'] keep `fill`."""
        buf, off, q = self._contexts(patterns)
        cap = int(cap)
        spans, heads = _rows(q, SPAN_DTYPE), _rows(q, NEXT_DTYPE)
        sym, cnt = _rows(q, np.int32, cap, fill), _rows(q, np.uint32, cap, fill)
        self._call(q, self._lib.sa_hip_token_index_next_batch, _ptr(buf), _ptr(off), q, int(mode), int(max_length), int(bool(need_next)), cap,
                   _ptr(spans), _ptr(sym), _ptr(cnt), _ptr(heads))
        return {"spans": spans[:q], "symbols": sym[:q], "counts": cnt[:q], "heads": heads[:q]}

    def next_of_spans(self, spans, cap=64, fill=0):
        """Next symbols of host spans (a SPAN_DTYPE array, e.g. from spans_batch); a span beyond the array raises."""
        spans = np.ascontiguousarray(spans, dtype=SPAN_DTYPE)
        q, cap = spans.size, int(cap)
        sym, cnt, heads = _rows(q, np.int32, cap, fill), _rows(q, np.uint32, cap, fill), _rows(q, NEXT_DTYPE)
        self._call(q, self._lib.sa_hip_token_index_next_of_spans, _ptr(spans), q, cap, _ptr(sym), _ptr(cnt), _ptr(heads))
        return {"spans": spans, "symbols": sym[:q], "counts": cnt[:q], "heads": heads[:q]}

    def next_info(self):
        return self._info(self._lib.sa_hip_token_index_next_info, TokenNextInfo)

    def top_batch_device(self, spans_dev_ptr, q, k, budget, symbols_dev_ptr, counts_dev_ptr, heads_dev_ptr):
        """The k most frequent next symbols of q device spans (among the first `budget` ranks of each; 0: all); asynchronous on
        the handle's stream until sync()."""
        check(self._lib.sa_hip_token_index_top_batch_device(self._h, spans_dev_ptr, q, int(k), int(budget), symbols_dev_ptr, counts_dev_ptr,
                                                            heads_dev_ptr))

    def top_batch(self, patterns, k=8, mode=0, max_length=0, need_next=True, budget=0, fill=0):
        """Spans as in spans_batch, then their k (1 .. 64) most frequent next symbols.  -> dict: spans [Q], symbols int32[Q, k] and
        counts uint32[Q, k] sorted by count descending, then symbol ascending, heads (written, distinct, covered, total)[Q].
        Cells beyond heads['written'] keep `fill`."""
        buf, off, q = self._contexts(patterns)
        k = int(k)
        spans, heads = _rows(q, SPAN_DTYPE), _rows(q, TOP_DTYPE)
        sym, cnt = _rows(q, np.int32, k, fill), _rows(q, np.uint32, k, fill)
        self._call(q, self._lib.sa_hip_token_index_top_batch, _ptr(buf), _ptr(off), q, int(mode), int(max_length), int(bool(need_next)), k,
                   int(budget), _ptr(spans), _ptr(sym), _ptr(cnt), _ptr(heads))
        return {"spans": spans[:q], "symbols": sym[:q], "counts": cnt[:q], "heads": heads[:q]}

    def sample_batch_device(self, spans_dev_ptr, q, draws_dev_ptr, m, symbols_dev_ptr, ranks_dev_ptr=None):
        """m next symbols per device span, one per uint64 draw; asynchronous on the handle's stream until sync()."""
        check(self._lib.sa_hip_token_index_sample_batch_device(self._h, spans_dev_ptr, q, draws_dev_ptr, int(m), symbols_dev_ptr, ranks_dev_ptr))

    def sample_batch(self, patterns, draws, mode=1, max_length=0, need_next=True):
        """Spans as in spans_batch, then one next symbol per draw: draws uint64[Q, m] (or [Q]: m = 1), rank = first + ended +
        floor(draw * total / 2^64).  -> dict: spans [Q], symbols int32[Q, m] (-1 where nothing follows), ranks uint32[Q, m]
        (0xFFFFFFFF there)."""
        buf, off, q = self._contexts(patterns)
        draws = np.ascontiguousarray(draws, dtype=np.uint64)
        if draws.ndim == 1:
            draws = draws.reshape(-1, 1)
        if draws.ndim != 2 or draws.shape[0] != q or (q and draws.shape[1] == 0):
            raise ValueError("draws: uint64[Q, m], m >= 1")
        m = draws.shape[1]
        spans = _rows(q, SPAN_DTYPE)
        sym, ranks = _rows(q, np.int32, m), _rows(q, np.uint32, m)
        self._call(q, self._lib.sa_hip_token_index_sample_batch, _ptr(buf), _ptr(off), q, int(mode), int(max_length), int(bool(need_next)),
                   _ptr(draws), m, _ptr(spans), _ptr(sym), _ptr(ranks))
        return {"spans": spans[:q], "symbols": sym[:q], "ranks": ranks[:q]}

    def top_info(self):
        return self._info(self._lib.sa_hip_token_index_top_info, TokenTopInfo)

    def set_documents(self, starts):
        """starts: the first text position of every document (starts[0] == 0, non-decreasing, <= n); None removes the documents."""
        if starts is None:
            check(self._lib.sa_hip_token_index_set_documents(self._h, None, 0))
            return
        s = np.ascontiguousarray(starts)
        if s.ndim != 1 or s.size == 0 or s.size > 0xFFFFFFFF or (s.dtype.kind not in "iu") or int(s.min()) < 0 or int(s.max()) > 2 ** 31 - 1:
            raise ValueError("doc_starts: a non-empty 1-d sequence of text positions")
        s = s.astype(np.int32)
        check(self._lib.sa_hip_token_index_set_documents(self._h, s.ctypes.data, s.size))

    def doc_range(self, first, count):
        """-> (DA, PV) of the ranks [first, first + count): the document of every rank, and the previous rank of the same document"""
        da, pv = np.empty(max(count, 1), dtype=np.int32), np.empty(max(count, 1), dtype=np.int32)
        check(self._lib.sa_hip_token_index_get_doc_range(self._h, int(first), int(count), da.ctypes.data, pv.ctypes.data))
        return da[:count], pv[:count]

    def docs_info(self):
        return self._info(self._lib.sa_hip_token_index_docs_info, TokenDocsInfo)

    def locate_batch_device(self, spans_dev_ptr, q, cap, docs_dev_ptr, offsets_dev_ptr, heads_dev_ptr):
        """(document, offset) of the first cap occurrences of q device spans; asynchronous on the handle's stream until sync()."""
        check(self._lib.sa_hip_token_index_locate_batch_device(self._h, spans_dev_ptr, q, int(cap), docs_dev_ptr, offsets_dev_ptr,
                                                               heads_dev_ptr))

    def locate_batch(self, patterns, cap=16, fill=0):
        """The exact span of every pattern, then its first cap occurrences.  -> dict: spans [Q], docs int32[Q, cap], offsets
        int32[Q, cap], heads (written, count)[Q].  Cells beyond heads['written'] keep `fill`."""
        buf, off, q = self._contexts(patterns)
        cap = int(cap)
        spans, heads = _rows(q, SPAN_DTYPE), _rows(q, LOCATE_DTYPE)
        docs, offs = _rows(q, np.int32, cap, fill), _rows(q, np.int32, cap, fill)
        self._call(q, self._lib.sa_hip_token_index_locate_batch, _ptr(buf), _ptr(off), q, cap, _ptr(spans), _ptr(docs), _ptr(offs), _ptr(heads))
        return {"spans": spans[:q], "docs": docs[:q], "offsets": offs[:q], "heads": heads[:q]}

    def docs_batch_device(self, spans_dev_ptr, q, cap, budget, docs_dev_ptr, offsets_dev_ptr, heads_dev_ptr):
        """Distinct documents of q device spans (cap 0: counts only, docs and offsets may be None); asynchronous until sync()."""
        check(self._lib.sa_hip_token_index_docs_batch_device(self._h, spans_dev_ptr, q, int(cap), int(budget), docs_dev_ptr, offsets_dev_ptr,
                                                             heads_dev_ptr))

    def docs_batch(self, patterns, cap=16, budget=0, mode=0, max_length=0, need_next=False, fill=0):
        """Spans as in spans_batch, then their distinct documents among the first `budget` ranks (0: all).  -> dict: spans [Q], docs
        int32[Q, cap], offsets int32[Q, cap], heads (written, examined, distinct, count)[Q].  Cells beyond heads['written'] keep `fill`."""
        buf, off, q = self._contexts(patterns)
        cap = int(cap)
        spans, heads = _rows(q, SPAN_DTYPE), _rows(q, DOCS_DTYPE)
        docs, offs = _rows(q, np.int32, cap, fill), _rows(q, np.int32, cap, fill)
        self._call(q, self._lib.sa_hip_token_index_docs_batch, _ptr(buf), _ptr(off), q, int(mode), int(max_length), int(bool(need_next)), cap,
                   int(budget), _ptr(spans), _ptr(docs), _ptr(offs), _ptr(heads))
        return {"spans": spans[:q], "docs": docs[:q], "offsets": offs[:q], "heads": heads[:q]}

    def prepare_doc_ranks(self, on=True):
        """Build (or, with on=False, free) the rank-by-document array the two calls below need; a no-op when it is already there.
        Replacing or removing the documents drops it."""
        check(self._lib.sa_hip_token_index_prepare_doc_ranks(self._h, int(bool(on))))

    def doc_ranks(self, first, count):
        """-> RK[first : first + count): for every document the ranks of its suffixes, ascending, segment d at starts[d]"""
        out = np.empty(max(count, 1), dtype=np.int32)
        check(self._lib.sa_hip_token_index_get_doc_ranks(self._h, int(first), int(count), out.ctypes.data))
        return out[:count]

    def doc_ranks_info(self):
        return self._info(self._lib.sa_hip_token_index_doc_ranks_info, TokenDocRanksInfo)

    def doc_counts_batch_device(self, spans_dev_ptr, q, cap, docs_dev_ptr, written_dev_ptr, written_stride, counts_dev_ptr):
        """counts[i, j] = ranks of device span i inside document docs[i, j], j below the row's length (written_dev_ptr None: cap);
        asynchronous on the handle's stream until sync()."""
        check(self._lib.sa_hip_token_index_doc_counts_batch_device(self._h, spans_dev_ptr, q, int(cap), docs_dev_ptr, written_dev_ptr,
                                                                   int(written_stride), counts_dev_ptr))

    def doc_counts_batch(self, patterns, docs, written=None, mode=0, max_length=0, need_next=False, fill=0):
        """Spans as in spans_batch, then how often every one occurs in the documents of its row.  docs: int32[Q, cap]; written:
        uint32[Q] row lengths or None.  -> dict: spans [Q], counts uint32[Q, cap].  Cells beyond a row's length keep `fill`."""
        buf, off, q = self._contexts(patterns)
        docs = np.ascontiguousarray(docs, dtype=np.int32)
        if docs.ndim != 2 or docs.shape[0] != q:
            raise ValueError("docs: one row of document ids per pattern")
        cap = docs.shape[1]
        if written is not None:
            written = np.ascontiguousarray(written, dtype=np.uint32)
            if written.shape != (q,):
                raise ValueError("written: one row length per pattern")
        spans, counts = _rows(q, SPAN_DTYPE), _rows(q, np.uint32, cap, fill)
        self._call(q, self._lib.sa_hip_token_index_doc_counts_batch, _ptr(buf), _ptr(off), q, int(mode), int(max_length), int(bool(need_next)), cap,
                   docs.ctypes.data, _ptr(written), counts.ctypes.data, _ptr(spans))
        return {"spans": spans[:q], "counts": counts[:q]}

    def all_batch_device(self, spans_dev_ptr, s, group_offsets, cap, budget, docs_dev_ptr, offsets_dev_ptr, heads_dev_ptr):
        """Documents holding all spans of every group; group_offsets is a HOST uint64[G + 1] (copied by the call), everything else on
        the device (cap 0: counts only, docs and offsets may be None); asynchronous until sync()."""
        go = np.ascontiguousarray(group_offsets, dtype=np.uint64)
        check(self._lib.sa_hip_token_index_all_batch_device(self._h, spans_dev_ptr, int(s), go.ctypes.data, go.size - 1, int(cap), int(budget),
                                                            docs_dev_ptr, offsets_dev_ptr, heads_dev_ptr))

    def all_batch(self, patterns, group_offsets, cap=16, budget=0, mode=0, max_length=0, need_next=False, fill=0):
        """Spans as in spans_batch, cut into groups by group_offsets (uint64[G + 1]: 0 .. S, 1 .. TOKEN_ALL_MAX spans each), then the
        documents that hold every span of a group.  -> dict: spans [S], docs int32[G, cap], offsets int32[G, cap], heads (written,
        examined, matched, candidates, driver, count, reserved)[G].  Cells beyond heads['written'] keep `fill`."""
        buf, off, s = self._contexts(patterns)
        go = np.ascontiguousarray(group_offsets, dtype=np.uint64)
        g = max(go.size - 1, 0)
        cap = int(cap)
        spans, heads = _rows(s, SPAN_DTYPE), _rows(g, ALL_DTYPE)
        docs, offs = _rows(g, np.int32, cap, fill), _rows(g, np.int32, cap, fill)
        self._call(g, self._lib.sa_hip_token_index_all_batch, _ptr(buf), _ptr(off), s, go.ctypes.data, g, int(mode), int(max_length),
                   int(bool(need_next)), cap, int(budget), _ptr(spans), _ptr(docs), _ptr(offs), _ptr(heads))
        return {"spans": spans[:s], "docs": docs[:g], "offsets": offs[:g], "heads": heads[:g]}

    @staticmethod
    def _cnf_tables(clause_offsets, negated, group_offsets):
        """-> (uint64 clause offsets, uint8 negated or None, uint64 group offsets), contiguous"""
        co = np.ascontiguousarray(clause_offsets, dtype=np.uint64)
        go = np.ascontiguousarray(group_offsets, dtype=np.uint64)
        ng = None if negated is None else np.ascontiguousarray(negated, dtype=np.uint8)
        if ng is not None and ng.size != max(co.size - 1, 0):
            raise ValueError("negated: one byte per clause")
        return co, ng, go

    def cnf_batch_device(self, spans_dev_ptr, s, clause_offsets, negated, group_offsets, cap, budget, docs_dev_ptr, offsets_dev_ptr,
                         heads_dev_ptr):
        """Documents that satisfy every group's CNF query over device spans (the literals).  clause_offsets uint64[C + 1], negated
        uint8[C] or None and group_offsets uint64[G + 1] are HOST arrays (copied by the call), everything else is on the device (cap
        0: counts only, docs and offsets may be None); heads are CNF_DTYPE; asynchronous until sync()."""
        co, ng, go = self._cnf_tables(clause_offsets, negated, group_offsets)
        check(self._lib.sa_hip_token_index_cnf_batch_device(self._h, spans_dev_ptr, int(s), co.ctypes.data, max(co.size - 1, 0),
                                                            None if ng is None else ng.ctypes.data, go.ctypes.data, max(go.size - 1, 0),
                                                            int(cap), int(budget), docs_dev_ptr, offsets_dev_ptr, heads_dev_ptr))

    def cnf_batch(self, patterns, clause_offsets, negated, group_offsets, cap=16, budget=0, mode=0, max_length=0, need_next=False, fill=0):
        """Spans as in spans_batch (the literals), cut into clauses by clause_offsets (uint64[C + 1]) and the clauses into groups by
        group_offsets (uint64[G + 1]: 1 .. TOKEN_CNF_MAX_CLAUSES clauses and at most TOKEN_CNF_MAX_LITERALS literals each); negated
        uint8[C] or None marks exclusions.  -> dict: spans [S], docs int32[G, cap], offsets int32[G, cap], heads CNF_DTYPE[G].  Cells
        beyond heads['written'] keep `fill`."""
        buf, off, s = self._contexts(patterns)
        co, ng, go = self._cnf_tables(clause_offsets, negated, group_offsets)
        c, g = max(co.size - 1, 0), max(go.size - 1, 0)
        cap = int(cap)
        spans, heads = _rows(s, SPAN_DTYPE), _rows(g, CNF_DTYPE)
        docs, offs = _rows(g, np.int32, cap, fill), _rows(g, np.int32, cap, fill)
        self._call(g, self._lib.sa_hip_token_index_cnf_batch, _ptr(buf), _ptr(off), s, co.ctypes.data, c, None if ng is None else ng.ctypes.data,
                   go.ctypes.data, g, int(mode), int(max_length), int(bool(need_next)), cap, int(budget), _ptr(spans), _ptr(docs), _ptr(offs),
                   _ptr(heads))
        return {"spans": spans[:s], "docs": docs[:g], "offsets": offs[:g], "heads": heads[:g]}

    def cnf_info(self):
        return self._info(self._lib.sa_hip_token_index_cnf_info, TokenCnfInfo)

    def match_batch_device(self, patterns_dev_ptr, offsets_dev_ptr, q, total, max_length, spans_dev_ptr):
        """The match of every one of the `total` = offsets[q] positions of q device documents (max_length 0: no cap) into
        spans_dev_ptr[total]; asynchronous on the handle's stream until sync()."""
        check(self._lib.sa_hip_token_index_match_batch_device(self._h, patterns_dev_ptr, offsets_dev_ptr, q, int(total), int(max_length),
                                                              spans_dev_ptr))

    def match_docs_batch_device(self, spans_dev_ptr, offsets_dev_ptr, q, min_length, cap, positions_dev_ptr, out_spans_dev_ptr, heads_dev_ptr):
        """The maximal matches of at least min_length symbols of q device documents from the spans match_batch_device wrote (cap 0:
        heads only, positions and out_spans may be None); asynchronous until sync()."""
        check(self._lib.sa_hip_token_index_match_docs_batch_device(self._h, spans_dev_ptr, offsets_dev_ptr, q, int(min_length), int(cap),
                                                                   positions_dev_ptr, out_spans_dev_ptr, heads_dev_ptr))

    def match_batch(self, docs, max_length=0):
        """docs as the patterns of query_batch: query documents.  -> structured array (first, count, length, ended)[offsets[Q]]: for
        every position of the packed documents the longest prefix of what follows in its document (at most max_length symbols, 0: no
        cap) that the text holds."""
        buf, off, q = self._contexts(docs)
        total = int(off[q]) if q else 0
        out = _rows(total, SPAN_DTYPE)
        self._call(q, self._lib.sa_hip_token_index_match_batch, _ptr(buf), _ptr(off), q, int(max_length), _ptr(out))
        return out[:total]

    def match_docs_batch(self, docs, min_length=1, max_length=0, cap=64, fill=0):
        """Matches as in match_batch, then per document its maximal matches of at least min_length symbols.  -> dict: spans
        [offsets[Q]], positions uint32[Q, cap] (offsets inside the document), out_spans [Q, cap], heads (written, maximal, longest,
        covered)[Q].  Cells beyond heads['written'] keep `fill`."""
        buf, off, q = self._contexts(docs)
        cap = int(cap)
        total = int(off[q]) if q else 0
        spans, heads = _rows(total, SPAN_DTYPE), _rows(q, MATCH_HEAD_DTYPE)
        pos = _rows(q, np.uint32, cap, fill)
        outs = _rows(q, np.uint32, cap * 4, fill).view(SPAN_DTYPE)
        self._call(q, self._lib.sa_hip_token_index_match_docs_batch, _ptr(buf), _ptr(off), q, int(max_length), int(min_length), cap,
                   _ptr(spans), _ptr(pos), _ptr(outs), _ptr(heads))
        return {"spans": spans[:total], "positions": pos[:q], "out_spans": outs[:q], "heads": heads[:q]}

    def match_info(self):
        return self._info(self._lib.sa_hip_token_index_match_info, TokenMatchInfo)

    def score_batch_device(self, patterns_dev_ptr, offsets_dev_ptr, q, total, max_length, spans_dev_ptr, scores_dev_ptr):
        """The score of every one of the `total` = offsets[q] positions of q device documents (max_length 0: no cap) into
        scores_dev_ptr[total].  spans_dev_ptr: what match_batch_device wrote for the same batch and max_length, or None (the search
        over the context's length instead); asynchronous on the handle's stream until sync()."""
        check(self._lib.sa_hip_token_index_score_batch_device(self._h, patterns_dev_ptr, offsets_dev_ptr, q, int(total), int(max_length),
                                                              spans_dev_ptr, scores_dev_ptr))

    def score_docs_batch_device(self, scores_dev_ptr, offsets_dev_ptr, q, heads_dev_ptr):
        """The heads of q device documents from the scores score_batch_device wrote; asynchronous until sync()."""
        check(self._lib.sa_hip_token_index_score_docs_batch_device(self._h, scores_dev_ptr, offsets_dev_ptr, q, heads_dev_ptr))

    def score_batch(self, docs, max_length=0, scores=True, heads=True):
        """docs as the patterns of query_batch: query documents.  -> dict: scores (length, context_count, token_count, first)
        [offsets[Q]]: for every position of the packed documents the longest context before it in its document (at most max_length
        symbols, 0: no cap) that the text holds with a token behind it, how often, and how often followed by the token at the
        position; heads (scored, seen, certain, longest, length_sum)[Q].  scores / heads False: that output is not fetched (None)."""
        if not scores and not heads:
            raise ValueError("score_batch: scores or heads")
        buf, off, q = self._contexts(docs)
        total = int(off[q]) if q else 0
        sc = _rows(total, SCORE_DTYPE) if scores else None
        hd = _rows(q, SCORE_HEAD_DTYPE) if heads else None
        self._call(q, self._lib.sa_hip_token_index_score_batch, _ptr(buf), _ptr(off), q, int(max_length),
                   sc.ctypes.data if scores else None, hd.ctypes.data if heads else None)
        return {"scores": sc[:total] if scores else None, "heads": hd[:q] if heads else None}

    def score_info(self):
        return self._info(self._lib.sa_hip_token_index_score_info, TokenScoreInfo)


class _BorrowedTokenIndex(TokenIndex):
    """A shard of a TokenShards set: the set owns the handle, close() only lets go of it."""

    def close(self):
        self._h = C.c_void_p()


class TokenShards(_TokenHandle):
    """Handle API of a shard set (sa_hip_token_shards): S <= 64 token indexes on one device answered as one corpus.  Per-shard
    results are shard-major arrays of shape [S, Q]."""
    _destroy = "sa_hip_token_shards_destroy"

    def __init__(self, handle, shards):
        self._h = handle
        self._lib = lib()
        self.shards = int(shards)

    @classmethod
    def create(cls, indexes):
        """Adopts the TokenIndex handles: on success they belong to the set and the wrappers passed in are emptied."""
        indexes = list(indexes)
        arr = (C.c_void_p * max(len(indexes), 1))(*[t._h.value if isinstance(t._h, C.c_void_p) else t._h for t in indexes])
        h = C.c_void_p()
        check(lib().sa_hip_token_shards_create(C.byref(h), arr, len(indexes)))
        for t in indexes:
            t._h = C.c_void_p()
        return cls(h, len(indexes))

    @classmethod
    def build(cls, texts, k=None, device=0):
        """One TokenIndex.build per text, then create(); a failure closes what was built."""
        built = []
        try:
            for t in texts:
                built.append(TokenIndex.build(t, k, device))
            return cls.create(built)
        except Exception:
            for t in built:
                t.close()
            raise

    def shard(self, s):
        """The borrowed TokenIndex of shard s (valid while the set lives; do not use it while the set is being asked)."""
        h = self._lib.sa_hip_token_shards_shard(self._h, int(s))
        if not h:
            raise IndexError("no shard %d" % s)
        return _BorrowedTokenIndex(C.c_void_p(h))

    def sync(self):
        check(self._lib.sa_hip_token_shards_sync(self._h))

    def info(self):
        return self._info(self._lib.sa_hip_token_shards_info, TokenShardsStats)

    def _shard_rows(self, q, dtype):
        """a per-shard output of zeros, [S, max(q, 1)]"""
        return np.zeros((self.shards, max(q, 1)), dtype=dtype)

    def query_batch(self, patterns, per_shard=True):
        """-> (totals uint64[Q], per_shard structured (first, second)[S, Q] or None)"""
        buf, off, q = self._contexts(patterns)
        totals = _rows(q, np.uint64)
        per = self._shard_rows(q, PAIR_DTYPE) if per_shard else None
        self._call(q, self._lib.sa_hip_token_shards_query_batch, _ptr(buf), _ptr(off), q, _ptr(totals), _ptr(per))
        return totals[:q], (per[:, :q] if per_shard else None)

    def query_batch_device(self, patterns_dev_ptr, offsets_dev_ptr, q, totals_dev_ptr, per_shard_dev_ptr=None):
        """Every buffer on the device; asynchronous on the set's stream until sync()."""
        check(self._lib.sa_hip_token_shards_query_batch_device(self._h, patterns_dev_ptr, offsets_dev_ptr, q, totals_dev_ptr, per_shard_dev_ptr))

    def spans_batch(self, patterns, mode=0, max_length=0, need_next=True):
        """-> dict: length uint32[Q], totals uint64[Q], spans structured (first, count, length, ended)[S, Q]"""
        buf, off, q = self._contexts(patterns)
        length, totals, spans = _rows(q, np.uint32), _rows(q, np.uint64), self._shard_rows(q, SPAN_DTYPE)
        self._call(q, self._lib.sa_hip_token_shards_spans_batch, _ptr(buf), _ptr(off), q, int(mode), int(max_length), int(bool(need_next)),
                   _ptr(length), _ptr(totals), _ptr(spans))
        return {"length": length[:q], "totals": totals[:q], "spans": spans[:, :q]}

    def spans_batch_device(self, patterns_dev_ptr, offsets_dev_ptr, q, mode, max_length, need_next, length_dev_ptr, totals_dev_ptr, spans_dev_ptr):
        check(self._lib.sa_hip_token_shards_spans_batch_device(self._h, patterns_dev_ptr, offsets_dev_ptr, q, int(mode), int(max_length),
                                                               int(bool(need_next)), length_dev_ptr, totals_dev_ptr, spans_dev_ptr))

    def next_batch(self, patterns, cap=64, mode=0, max_length=0, need_next=True, fill=0):
        """Spans as in spans_batch, then the merged next symbols.  -> dict: spans [S, Q], symbols int32[Q, cap], counts
        uint64[Q, cap], heads (written, length, covered, total)[Q].  Cells beyond heads['written'] keep `fill`."""
        buf, off, q = self._contexts(patterns)
        cap = int(cap)
        spans, heads = self._shard_rows(q, SPAN_DTYPE), _rows(q, SHARDS_NEXT_DTYPE)
        sym, cnt = _rows(q, np.int32, cap, fill), _rows(q, np.uint64, cap, fill)
        self._call(q, self._lib.sa_hip_token_shards_next_batch, _ptr(buf), _ptr(off), q, int(mode), int(max_length), int(bool(need_next)), cap,
                   _ptr(spans), _ptr(sym), _ptr(cnt), _ptr(heads))
        return {"spans": spans[:, :q], "symbols": sym[:q], "counts": cnt[:q], "heads": heads[:q]}

    def next_batch_device(self, spans_dev_ptr, q, cap, symbols_dev_ptr, counts_dev_ptr, heads_dev_ptr):
        """Merged next symbols of q contexts from their S * q device spans; asynchronous on the set's stream until sync()."""
        check(self._lib.sa_hip_token_shards_next_batch_device(self._h, spans_dev_ptr, q, int(cap), symbols_dev_ptr, counts_dev_ptr, heads_dev_ptr))

    def merge_device(self, symbols_dev_ptr, counts_dev_ptr, heads_dev_ptr, q, cap, out_symbols_dev_ptr, out_counts_dev_ptr, out_heads_dev_ptr):
        """The merge step alone, on S * q device lists; asynchronous on the set's stream until sync()."""
        check(self._lib.sa_hip_token_shards_merge_device(self._h, symbols_dev_ptr, counts_dev_ptr, heads_dev_ptr, q, int(cap),
                                                         out_symbols_dev_ptr, out_counts_dev_ptr, out_heads_dev_ptr))

    def match_batch_device(self, patterns_dev_ptr, offsets_dev_ptr, q, total, max_length, merged_dev_ptr, per_shard_dev_ptr):
        """The longest match over all shards at every one of the `total` = offsets[q] positions of q device documents (max_length 0:
        no cap) into merged_dev_ptr[total] and its span in every shard into per_shard_dev_ptr[S * total]; asynchronous on the set's
        stream until sync()."""
        check(self._lib.sa_hip_token_shards_match_batch_device(self._h, patterns_dev_ptr, offsets_dev_ptr, q, int(total), int(max_length),
                                                               merged_dev_ptr, per_shard_dev_ptr))

    def match_docs_batch_device(self, merged_dev_ptr, offsets_dev_ptr, q, min_length, cap, positions_dev_ptr, out_matches_dev_ptr, heads_dev_ptr):
        """The maximal matches of at least min_length symbols of q device documents from the records match_batch_device wrote (cap 0:
        heads only, positions and out_matches may be None); asynchronous until sync()."""
        check(self._lib.sa_hip_token_shards_match_docs_batch_device(self._h, merged_dev_ptr, offsets_dev_ptr, q, int(min_length), int(cap),
                                                                    positions_dev_ptr, out_matches_dev_ptr, heads_dev_ptr))

    def match_batch(self, docs, max_length=0, per_shard=True):
        """docs as the patterns of query_batch: query documents.  -> (merged structured (length, shards, count)[offsets[Q]], per_shard
        structured (first, count, length, ended)[S, offsets[Q]] or None): for every position of the packed documents the longest
        prefix of what follows in its document (at most max_length symbols, 0: no cap) that some shard holds."""
        buf, off, q = self._contexts(docs)
        total = int(off[q]) if q else 0
        merged = _rows(total, SHARDS_MATCH_DTYPE)
        per = self._shard_rows(total, SPAN_DTYPE) if per_shard else None
        self._call(q, self._lib.sa_hip_token_shards_match_batch, _ptr(buf), _ptr(off), q, int(max_length), _ptr(merged), _ptr(per))
        return merged[:total], (per[:, :total] if per_shard else None)

    def match_docs_batch(self, docs, min_length=1, max_length=0, cap=64, fill=0):
        """Matches as in match_batch, then per document its maximal matches of at least min_length symbols.  -> dict: merged
        [offsets[Q]], positions uint32[Q, cap] (offsets inside the document), out_matches [Q, cap], heads (written, maximal, longest,
        covered)[Q].  Cells beyond heads['written'] keep `fill`."""
        buf, off, q = self._contexts(docs)
        cap = int(cap)
        total = int(off[q]) if q else 0
        merged, heads = _rows(total, SHARDS_MATCH_DTYPE), _rows(q, MATCH_HEAD_DTYPE)
        pos = _rows(q, np.uint32, cap, fill)
        outs = _rows(q, np.uint32, cap * 4, fill).view(SHARDS_MATCH_DTYPE)
        self._call(q, self._lib.sa_hip_token_shards_match_docs_batch, _ptr(buf), _ptr(off), q, int(max_length), int(min_length), cap,
                   _ptr(merged), _ptr(pos), _ptr(outs), _ptr(heads))
        return {"merged": merged[:total], "positions": pos[:q], "out_matches": outs[:q], "heads": heads[:q]}

    def match_info(self):
        return self._info(self._lib.sa_hip_token_shards_match_info, TokenShardsMatchStats)

    def score_batch_device(self, patterns_dev_ptr, offsets_dev_ptr, q, total, max_length, merged_dev_ptr, scores_dev_ptr, per_shard_dev_ptr):
        """The score over all shards of every one of the `total` = offsets[q] positions of q device documents (max_length 0: no cap)
        into scores_dev_ptr[total], and every shard's span of the context with the token into per_shard_dev_ptr[S * total].
        merged_dev_ptr: what match_batch_device wrote for the same batch and max_length, or None (the search over the context
        length instead).  Asynchronous on the set's stream until sync()."""
        check(self._lib.sa_hip_token_shards_score_batch_device(self._h, patterns_dev_ptr, offsets_dev_ptr, q, int(total), int(max_length),
                                                               merged_dev_ptr, scores_dev_ptr, per_shard_dev_ptr))

    def score_docs_batch_device(self, scores_dev_ptr, offsets_dev_ptr, q, heads_dev_ptr):
        """The heads of q device documents from the scores score_batch_device wrote; asynchronous until sync()."""
        check(self._lib.sa_hip_token_shards_score_docs_batch_device(self._h, scores_dev_ptr, offsets_dev_ptr, q, heads_dev_ptr))

    def score_batch(self, docs, max_length=0, scores=True, per_shard=True, heads=True):
        """docs as the patterns of query_batch: query documents.  -> dict: scores (length, shards, context_count, token_count)
        [offsets[Q]], for every position the longest context before it (at most max_length symbols, 0: no cap) that some shard
        holds with a token behind it, how often over all shards, how often followed by the token at the position and in how many
        shards; per_shard (first, count, length, ended)[S, offsets[Q]], every shard's span of that context with the token; heads
        (scored, seen, certain, longest, length_sum)[Q].  An output that is False is not fetched (None)."""
        if not scores and not per_shard and not heads:
            raise ValueError("score_batch: scores, per_shard or heads")
        buf, off, q = self._contexts(docs)
        total = int(off[q]) if q else 0
        sc = _rows(total, SHARDS_SCORE_DTYPE) if scores else None
        per = self._shard_rows(total, SPAN_DTYPE) if per_shard else None
        hd = _rows(q, SCORE_HEAD_DTYPE) if heads else None
        self._call(q, self._lib.sa_hip_token_shards_score_batch, _ptr(buf), _ptr(off), q, int(max_length), _ptr(sc), _ptr(per), _ptr(hd))
        return {"scores": sc[:total] if scores else None, "per_shard": per[:, :total] if per_shard else None,
                "heads": hd[:q] if heads else None}

    def score_info(self):
        return self._info(self._lib.sa_hip_token_shards_score_info, TokenShardsScoreStats)

    def top_batch_device(self, spans_dev_ptr, q, k, budget, symbols_dev_ptr, counts_dev_ptr, heads_dev_ptr):
        """The k most frequent next symbols of q contexts from their S * q device spans, counts summed over the shards (among the
        first `budget` merged continuations of each; 0: all); asynchronous on the set's stream until sync()."""
        check(self._lib.sa_hip_token_shards_top_batch_device(self._h, spans_dev_ptr, q, int(k), int(budget), symbols_dev_ptr, counts_dev_ptr,
                                                             heads_dev_ptr))

    def top_batch(self, patterns, k=8, mode=0, max_length=0, need_next=True, budget=0, fill=0):
        """Spans as in spans_batch, then the k (1 .. 64) most frequent next symbols over all shards.  -> dict: spans [S, Q], symbols
        int32[Q, k] and counts uint64[Q, k] sorted by count descending, then symbol ascending, heads (written, distinct, length,
        shards, covered, total)[Q].  Cells beyond heads['written'] keep `fill`."""
        buf, off, q = self._contexts(patterns)
        k = int(k)
        spans, heads = self._shard_rows(q, SPAN_DTYPE), _rows(q, SHARDS_TOP_DTYPE)
        sym, cnt = _rows(q, np.int32, k, fill), _rows(q, np.uint64, k, fill)
        self._call(q, self._lib.sa_hip_token_shards_top_batch, _ptr(buf), _ptr(off), q, int(mode), int(max_length), int(bool(need_next)), k,
                   int(budget), _ptr(spans), _ptr(sym), _ptr(cnt), _ptr(heads))
        return {"spans": spans[:, :q], "symbols": sym[:q], "counts": cnt[:q], "heads": heads[:q]}

    def sample_batch_device(self, spans_dev_ptr, q, draws_dev_ptr, m, symbols_dev_ptr, shards_dev_ptr=None, ranks_dev_ptr=None):
        """m next symbols per context from its S device spans, one per uint64 draw; asynchronous on the set's stream until sync()."""
        check(self._lib.sa_hip_token_shards_sample_batch_device(self._h, spans_dev_ptr, q, draws_dev_ptr, int(m), symbols_dev_ptr,
                                                                shards_dev_ptr, ranks_dev_ptr))

    def sample_batch(self, patterns, draws, mode=1, max_length=0, need_next=True, shards=True, ranks=True):
        """Spans as in spans_batch, then one next symbol per draw: draws uint64[Q, m] (or [Q]: m = 1) pick continuation
        floor(draw * total / 2^64) of the context's total, the continuations numbered shard by shard.  -> dict: spans [S, Q],
        symbols int32[Q, m] (-1 where nothing follows), shards and ranks uint32[Q, m] (0xFFFFFFFF there; None when not asked for)."""
        buf, off, q = self._contexts(patterns)
        draws = np.ascontiguousarray(draws, dtype=np.uint64)
        if draws.ndim == 1:
            draws = draws.reshape(-1, 1)
        if draws.ndim != 2 or draws.shape[0] != q or (q and draws.shape[1] == 0):
            raise ValueError("draws: uint64[Q, m], m >= 1")
        m = draws.shape[1]
        spans = self._shard_rows(q, SPAN_DTYPE)
        sym = _rows(q, np.int32, m)
        sh = _rows(q, np.uint32, m) if shards else None
        rk = _rows(q, np.uint32, m) if ranks else None
        self._call(q, self._lib.sa_hip_token_shards_sample_batch, _ptr(buf), _ptr(off), q, int(mode), int(max_length), int(bool(need_next)),
                   _ptr(draws), m, _ptr(spans), _ptr(sym), _ptr(sh), _ptr(rk))
        return {"spans": spans[:, :q], "symbols": sym[:q], "shards": sh[:q] if shards else None, "ranks": rk[:q] if ranks else None}

    def top_info(self):
        return self._info(self._lib.sa_hip_token_shards_top_info, TokenShardsTopStats)

    def set_documents(self, starts):
        """starts: one table per shard as TokenIndex.set_documents takes it (every table is checked before a shard is touched);
        None removes the documents from all shards."""
        if starts is None:
            check(self._lib.sa_hip_token_shards_set_documents(self._h, None, None))
            return
        tabs = []
        for t in starts:
            a = np.ascontiguousarray(t)
            if a.ndim != 1 or a.size == 0 or a.size > 0xFFFFFFFF or (a.dtype.kind not in "iu") or int(a.min()) < 0 or int(a.max()) > 2 ** 31 - 1:
                raise ValueError("doc_starts: a non-empty 1-d sequence of text positions per shard")
            tabs.append(a.astype(np.int32))
        if len(tabs) != self.shards:
            raise ValueError("one doc_starts table per shard")
        ptrs = (C.c_void_p * self.shards)(*[a.ctypes.data for a in tabs])
        sizes = (C.c_uint32 * self.shards)(*[a.size for a in tabs])
        check(self._lib.sa_hip_token_shards_set_documents(self._h, ptrs, sizes))

    def adopt_documents(self):
        """Build the set's document table from the documents the shards hold now (set through shard(s), or before create())."""
        check(self._lib.sa_hip_token_shards_adopt_documents(self._h))

    def doc_bases(self):
        """-> uint64[S + 1]: the global id of document d of shard s is bases[s] + d; bases[S] = the documents of the set"""
        out = np.zeros(self.shards + 1, np.uint64)
        check(self._lib.sa_hip_token_shards_doc_bases(self._h, out.ctypes.data))
        return out

    def docs_info(self):
        return self._info(self._lib.sa_hip_token_shards_docs_info, TokenShardsDocsStats)

    def locate_batch_device(self, spans_dev_ptr, q, cap, docs_dev_ptr, offsets_dev_ptr, heads_dev_ptr):
        """(global document uint64, offset int32) of the first cap hits of q contexts from their S * q device spans; asynchronous on
        the set's stream until sync()."""
        check(self._lib.sa_hip_token_shards_locate_batch_device(self._h, spans_dev_ptr, q, int(cap), docs_dev_ptr, offsets_dev_ptr,
                                                                heads_dev_ptr))

    def locate_batch(self, patterns, cap=16, fill=0):
        """The exact spans of every pattern, then its first cap hits over the shards in shard order.  -> dict: spans [S, Q], docs
        uint64[Q, cap], offsets int32[Q, cap], heads (written, reserved, count)[Q].  Cells beyond heads['written'] keep `fill`."""
        buf, off, q = self._contexts(patterns)
        cap = int(cap)
        spans, heads = self._shard_rows(q, SPAN_DTYPE), _rows(q, SHARDS_LOCATE_DTYPE)
        docs, offs = _rows(q, np.uint64, cap, fill), _rows(q, np.int32, cap, fill)
        self._call(q, self._lib.sa_hip_token_shards_locate_batch, _ptr(buf), _ptr(off), q, cap, _ptr(spans), _ptr(docs), _ptr(offs), _ptr(heads))
        return {"spans": spans[:, :q], "docs": docs[:q], "offsets": offs[:q], "heads": heads[:q]}

    def docs_batch_device(self, spans_dev_ptr, q, cap, budget, docs_dev_ptr, offsets_dev_ptr, heads_dev_ptr):
        """Distinct documents of q contexts from their S * q device spans (cap 0: counts only, docs and offsets may be None);
        asynchronous until sync()."""
        check(self._lib.sa_hip_token_shards_docs_batch_device(self._h, spans_dev_ptr, q, int(cap), int(budget), docs_dev_ptr, offsets_dev_ptr,
                                                              heads_dev_ptr))

    def docs_batch(self, patterns, cap=16, budget=0, mode=0, max_length=0, need_next=False, fill=0):
        """Spans as in spans_batch, then the distinct documents among the first `budget` ranks (0: all) of the shards' spans in
        shard order.  -> dict: spans [S, Q], docs uint64[Q, cap], offsets int32[Q, cap], heads (written, reserved, examined,
        distinct, count)[Q].  Cells beyond heads['written'] keep `fill`."""
        buf, off, q = self._contexts(patterns)
        cap = int(cap)
        spans, heads = self._shard_rows(q, SPAN_DTYPE), _rows(q, SHARDS_DOCS_DTYPE)
        docs, offs = _rows(q, np.uint64, cap, fill), _rows(q, np.int32, cap, fill)
        self._call(q, self._lib.sa_hip_token_shards_docs_batch, _ptr(buf), _ptr(off), q, int(mode), int(max_length), int(bool(need_next)), cap,
                   int(budget), _ptr(spans), _ptr(docs), _ptr(offs), _ptr(heads))
        return {"spans": spans[:, :q], "docs": docs[:q], "offsets": offs[:q], "heads": heads[:q]}

    def docs_merge_device(self, docs_dev_ptr, offsets_dev_ptr, heads_dev_ptr, q, cap, out_docs_dev_ptr, out_offsets_dev_ptr, out_heads_dev_ptr,
                          bases_dev_ptr=None):
        """The merge step alone, on S * q device lists with shard-local ids (bases_dev_ptr None: the set's own bases); asynchronous
        on the set's stream until sync()."""
        check(self._lib.sa_hip_token_shards_docs_merge_device(self._h, docs_dev_ptr, offsets_dev_ptr, heads_dev_ptr, bases_dev_ptr, q, int(cap),
                                                              out_docs_dev_ptr, out_offsets_dev_ptr, out_heads_dev_ptr))

    def prepare_doc_ranks(self, on=True):
        """Build the rank-by-document array of every shard, one after another, and the set's table of them (or, with on=False,
        free them all); a no-op per shard where the array is there.  Replacing or removing the documents drops them."""
        check(self._lib.sa_hip_token_shards_prepare_doc_ranks(self._h, int(bool(on))))

    def doc_ranks_info(self):
        return self._info(self._lib.sa_hip_token_shards_doc_ranks_info, TokenShardsRanksStats)

    def doc_counts_batch_device(self, spans_dev_ptr, q, cap, docs_dev_ptr, written_dev_ptr, written_stride, counts_dev_ptr):
        """counts[i, j] = occurrences of context i (its S device spans) inside the document with the global id docs[i, j] (uint64),
        j below the row's length (written_dev_ptr None: cap); asynchronous on the set's stream until sync()."""
        check(self._lib.sa_hip_token_shards_doc_counts_batch_device(self._h, spans_dev_ptr, q, int(cap), docs_dev_ptr, written_dev_ptr,
                                                                    int(written_stride), counts_dev_ptr))

    def doc_counts_batch(self, patterns, docs, written=None, mode=0, max_length=0, need_next=False, fill=0):
        """Spans as in spans_batch, then how often every context occurs in the documents of its row.  docs: uint64[Q, cap] global
        ids; written: uint32[Q] row lengths or None.  -> dict: spans [S, Q], counts uint32[Q, cap].  Cells beyond a row's length
        keep `fill`."""
        buf, off, q = self._contexts(patterns)
        docs = np.ascontiguousarray(docs, dtype=np.uint64)
        if docs.ndim != 2 or docs.shape[0] != q:
            raise ValueError("docs: one row of document ids per pattern")
        cap = docs.shape[1]
        if written is not None:
            written = np.ascontiguousarray(written, dtype=np.uint32)
            if written.shape != (q,):
                raise ValueError("written: one row length per pattern")
        spans, counts = self._shard_rows(q, SPAN_DTYPE), _rows(q, np.uint32, cap, fill)
        self._call(q, self._lib.sa_hip_token_shards_doc_counts_batch, _ptr(buf), _ptr(off), q, int(mode), int(max_length), int(bool(need_next)),
                   cap, docs.ctypes.data, _ptr(written), counts.ctypes.data, _ptr(spans))
        return {"spans": spans[:, :q], "counts": counts[:q]}

    def all_batch_device(self, spans_dev_ptr, p, group_offsets, cap, budget, docs_dev_ptr, offsets_dev_ptr, heads_dev_ptr):
        """Documents of the corpus holding all patterns of every group, from the S * p device spans; group_offsets is a HOST
        uint64[G + 1] (copied by the call), everything else on the device (cap 0: counts only, docs and offsets may be None);
        asynchronous until sync()."""
        go = np.ascontiguousarray(group_offsets, dtype=np.uint64)
        check(self._lib.sa_hip_token_shards_all_batch_device(self._h, spans_dev_ptr, int(p), go.ctypes.data, go.size - 1, int(cap), int(budget),
                                                             docs_dev_ptr, offsets_dev_ptr, heads_dev_ptr))

    def all_batch(self, patterns, group_offsets, cap=16, budget=0, mode=0, max_length=0, need_next=False, fill=0):
        """Spans as in spans_batch, cut into groups by group_offsets (uint64[G + 1]: 0 .. P, 1 .. TOKEN_ALL_MAX patterns each), then
        the documents that hold every pattern of a group.  -> dict: spans [S, P], docs uint64[G, cap], offsets int32[G, cap], heads
        (written, driver, examined, matched, candidates, count)[G].  Cells beyond heads['written'] keep `fill`."""
        buf, off, p = self._contexts(patterns)
        go = np.ascontiguousarray(group_offsets, dtype=np.uint64)
        g = max(go.size - 1, 0)
        cap = int(cap)
        spans, heads = self._shard_rows(p, SPAN_DTYPE), _rows(g, SHARDS_ALL_DTYPE)
        docs, offs = _rows(g, np.uint64, cap, fill), _rows(g, np.int32, cap, fill)
        self._call(g, self._lib.sa_hip_token_shards_all_batch, _ptr(buf), _ptr(off), p, go.ctypes.data, g, int(mode), int(max_length),
                   int(bool(need_next)), cap, int(budget), _ptr(spans), _ptr(docs), _ptr(offs), _ptr(heads))
        return {"spans": spans[:, :p], "docs": docs[:g], "offsets": offs[:g], "heads": heads[:g]}

    def all_merge_device(self, docs_dev_ptr, offsets_dev_ptr, heads_dev_ptr, plan_dev_ptr, g, cap, out_docs_dev_ptr, out_offsets_dev_ptr,
                         out_heads_dev_ptr, bases_dev_ptr=None):
        """The merge step of all_batch alone, on S * g device lists with shard-local ids, their heads (SHARDS_ALL_PAIR_DTYPE) and the
        per-group plan (SHARDS_ALL_PLAN_DTYPE); bases_dev_ptr None: the set's own bases.  Asynchronous until sync()."""
        check(self._lib.sa_hip_token_shards_all_merge_device(self._h, docs_dev_ptr, offsets_dev_ptr, heads_dev_ptr, plan_dev_ptr, bases_dev_ptr,
                                                             g, int(cap), out_docs_dev_ptr, out_offsets_dev_ptr, out_heads_dev_ptr))


def construct_truncated_suffix_array(text, max_suffix_length):
    t = as_u8(text)
    sa = np.zeros(max(t.size, 1), dtype=np.uint32)
    st = SuffixArrayStruct()
    st.suffix_array = sa.ctypes.data
    st.max_suffix_length = max_suffix_length
    st.n = t.size
    st.global_byte_end_idx = t.size
    check(lib().sa_hip_construct_truncated_suffix_array(t.ctypes.data, C.byref(st)))
    return sa[:t.size]


def get_substring_positions(text, sa, max_suffix_length, substring):
    t = as_u8(text)
    s = np.ascontiguousarray(sa, dtype=np.uint32)
    st = SuffixArrayStruct()
    st.suffix_array = s.ctypes.data
    st.max_suffix_length = max_suffix_length
    st.n = t.size
    r = lib().sa_hip_get_substring_positions(t.ctypes.data, C.byref(st), bytes(substring))
    return (r.first, r.second)


class CsvIndex:
    """sa_hip_csv_index through ctypes: the C seam of CSV mode exactly as a C caller sees it (the tests of the record
    retrieval entry points go through this; the Python class binds the same functions from Cython)."""

    def __init__(self, csv_file, search_column, max_suffix_length=32, device=0):
        self._lib = lib()
        self._h = C.c_void_p()
        check(self._lib.sa_hip_csv_index_create(C.byref(self._h), os.fsencode(csv_file), search_column.encode("utf-8"),
                                                int(max_suffix_length), int(device)))

    def close(self):
        if self._h:
            self._lib.sa_hip_csv_index_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def index(self):
        return DeviceIndex.from_handle(self._lib.sa_hip_csv_index_handle(self._h), self)

    @property
    def num_rows(self):
        return int(self._lib.sa_hip_csv_index_num_rows(self._h))

    @property
    def columns(self):
        return [self._lib.sa_hip_csv_index_column_name(self._h, i).decode("utf-8") for i in range(self._lib.sa_hip_csv_index_num_columns(self._h))]

    def get_substring_positions_file(self, substring: bytes):
        r = self._lib.sa_hip_get_substring_positions_file(self._h, substring)
        return (r.first, r.second)

    def get_matching_records_file(self, substring: bytes, k, already=()):
        """-> list of row bytes; `already`: rows that occupy the front of the table (num_matches starts at their count)."""
        table = (C.c_void_p * max(k, 1))()
        num = C.c_uint32(len(already))
        check(self._lib.sa_hip_get_matching_records_file(self._h, substring, k, table, C.byref(num)))
        out = [C.string_at(table[i]) for i in range(len(already), num.value)]
        tail = (C.c_void_p * max(num.value - len(already), 1))(*[table[i] for i in range(len(already), num.value)])
        self._lib.sa_hip_free_records(tail, num.value - len(already))
        return out, num.value


def get_matching_records(text, sa, max_suffix_length, substring: bytes, k):
    """sa_hip_get_matching_records: host text + host SA, engine.c:1168-1215's calling convention."""
    t = as_u8(text)
    s = np.ascontiguousarray(sa, dtype=np.uint32)
    st = SuffixArrayStruct()
    st.suffix_array = s.ctypes.data
    st.max_suffix_length = max_suffix_length
    st.n = t.size
    table = (C.c_void_p * max(k, 1))()
    n = lib().sa_hip_get_matching_records(t.ctypes.data, C.byref(st), substring, k, table)
    out = [C.string_at(table[i]) for i in range(n)]
    lib().sa_hip_free_records(table, n)
    return out


class _CsvOwner:
    """Keeps the malloc'ed arrays of one sa_hip_csv_column alive for the numpy views made of them."""

    def __init__(self, col):
        self.col = col

    def __del__(self):
        try:
            lib().sa_hip_csv_free(C.byref(self.col))
        except Exception:
            pass


def _view(owner, ptr, count, ctype, dtype):
    if not count:
        return np.zeros(0, dtype)
    buf = (ctype * count).from_address(C.cast(ptr, C.c_void_p).value)
    buf._owner = owner   # the view's base is this ctypes array: the owner lives as long as any view does
    return np.frombuffer(buf, dtype=dtype)


def csv_extract_column(path, column, copy=True):
    """Native RFC-4180 column extractor -> (columns, text, row_text_starts, row_file_offsets).
    copy=True: text as bytes, the offsets as numpy arrays of their own.  copy=False: text as a uint8 array and the
    offsets as views of the arrays the extractor allocated (freed when the last view goes): no second copy of the
    ~2 bytes + 16 bytes per row that a 50M-row file yields (0.3 s of the 0.9 s the copying form takes)."""
    col = CsvColumn()
    check(lib().sa_hip_csv_extract_column(os.fsencode(path), column.encode("utf-8"), C.byref(col)))
    owner = _CsvOwner(col)
    names, p = [], col.column_names
    for _ in range(col.num_columns):
        s = C.string_at(p)
        names.append(s.decode("utf-8"))
        p += len(s) + 1
    text = _view(owner, col.text, col.text_len, C.c_uint8, np.uint8)
    starts = _view(owner, col.row_text_starts, col.num_rows, C.c_int64, np.int64)   # offsets are < 2^63: viewed as int64
    offs = _view(owner, col.row_file_offsets, col.num_rows + 1, C.c_int64, np.int64)
    if copy:
        return names, text.tobytes(), starts.copy(), offs.copy()
    return names, text, starts, offs


def synth_csv(path, rows, seed=1):
    check(lib().sa_hip_synth_csv(os.fsencode(path), rows, seed))


def sort_pairs(keys, values=None, begin_bit=0, end_bit=64, device=0):
    """In-place stable device sort of (u64 key, u32 value) records; returns (keys, values)."""
    k = np.ascontiguousarray(keys, dtype=np.uint64).copy()
    v = None if values is None else np.ascontiguousarray(values, dtype=np.uint32).copy()
    check(lib().sa_hip_sort_pairs(k.ctypes.data if k.size else None, None if v is None else v.ctypes.data,
                                  k.size, begin_bit, end_bit, device))
    return k, v


def synth_uniform27(n, seed=88172645463325252):
    out = np.empty(n, dtype=np.uint8)
    lib().sa_hip_synth_uniform27(out.ctypes.data, n, seed)
    return out
