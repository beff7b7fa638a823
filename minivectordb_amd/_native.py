"""ctypes binding of libmvdb.so (include/mvdb.h).

The library is the ONLY compute back end of this package: there is no CPU fallback.  Loading
fails loudly when the in-tree shared object is missing, and every compute entry point raises
``RuntimeError`` when no HIP device is usable.

PyTorch-ROCm bundles its own HIP runtime under the SONAME ``libamdhip64.so.7``; libmvdb.so must bind to
THAT instance, so that device pointers and streams can be exchanged with torch tensors (torch is used
only for device memory, streams and torch.distributed — never for the search arithmetic) and so that a
later ``import torch`` does not bring a second HIP runtime into the process.  If torch is already
imported its runtime is loaded; otherwise torch's ``lib/libamdhip64.so`` is pre-loaded by path WITHOUT
importing torch (a VectorDatabase-only user pays no 1-2 s ``import torch`` on the first query).
"""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libmvdb.so")
LIB_PATH = os.environ.get("MVDB_LIBMVDB", LIB_PATH)  # diagnostics only: e.g. the ablation build (make ABLATE=1)

METRIC_IP = 0
METRIC_L2 = 1

ERR_ARG = 1
ERR_HIP = 2
ERR_NODEVICE = 3
ERR_OOM = 4

_lib = None

c_f32p = ctypes.POINTER(ctypes.c_float)
c_i64p = ctypes.POINTER(ctypes.c_int64)
c_i32p = ctypes.POINTER(ctypes.c_int32)
c_vp = ctypes.c_void_p


class EncoderCfg(ctypes.Structure):
    """mirror of mvdb_encoder_cfg"""
    _fields_ = [
        ("vocab_size", ctypes.c_int),
        ("hidden", ctypes.c_int),
        ("layers", ctypes.c_int),
        ("heads", ctypes.c_int),
        ("intermediate", ctypes.c_int),
        ("max_positions", ctypes.c_int),
        ("type_vocab", ctypes.c_int),
        ("position_offset", ctypes.c_int),
        ("ln_eps", ctypes.c_float),
        ("pooling", ctypes.c_int),
    ]


class M3Heads(ctypes.Structure):
    """mirror of mvdb_m3_heads"""
    _fields_ = [
        ("sparse_w", ctypes.c_void_p),
        ("sparse_b", ctypes.c_void_p),
        ("colbert_w", ctypes.c_void_p),
        ("colbert_b", ctypes.c_void_p),
        ("colbert_dim", ctypes.c_int),
        ("n_unused", ctypes.c_int),
        ("unused_ids", ctypes.c_int * 8),
    ]


class M3Out(ctypes.Structure):
    """mirror of mvdb_m3_out"""
    _fields_ = [
        ("token_weights", ctypes.c_void_p),
        ("lex_count", ctypes.c_void_p),
        ("lex_indices", ctypes.c_void_p),
        ("lex_values", ctypes.c_void_p),
        ("colbert", ctypes.c_void_p),
        ("colbert_count", ctypes.c_void_p),
    ]


# name -> (restype, argtypes); the single source of truth for tests that check the export table
PROTOTYPES = {
    "mvdb_last_error": (ctypes.c_char_p, []),
    "mvdb_abi_version": (ctypes.c_int, []),
    "mvdb_device_count": (ctypes.c_int, [ctypes.POINTER(ctypes.c_int)]),
    "mvdb_index_create": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(c_vp)]),
    "mvdb_index_free": (ctypes.c_int, [c_vp]),
    "mvdb_index_reload_env": (ctypes.c_int, [c_vp]),
    "mvdb_index_set_option": (ctypes.c_int, [c_vp, ctypes.c_char_p, ctypes.c_longlong]),
    "mvdb_index_reset": (ctypes.c_int, [c_vp]),
    "mvdb_index_ntotal": (ctypes.c_int64, [c_vp]),
    "mvdb_index_shadow_rows": (ctypes.c_int64, [c_vp]),
    "mvdb_index_code8_rows": (ctypes.c_int64, [c_vp]),
    "mvdb_index_code8_counters": (ctypes.c_int, [c_vp, c_vp, c_vp, c_vp]),
    "mvdb_code8_margin": (ctypes.c_int, [ctypes.c_int, ctypes.c_float, ctypes.c_float, ctypes.c_float, c_vp, c_vp]),
    "mvdb_code8_pack": (ctypes.c_int, [ctypes.c_int, c_vp, c_vp, c_vp]),
    "mvdb_code8_unpack": (ctypes.c_int, [ctypes.c_int, c_vp, c_vp, c_vp]),
    "mvdb_index_code8_refined": (ctypes.c_int, [c_vp, c_vp]),
    "mvdb_code8_front_pack": (ctypes.c_int, [ctypes.c_int, c_vp, c_vp]),
    "mvdb_code8_front_unpack": (ctypes.c_int, [ctypes.c_int, c_vp, c_vp]),
    "mvdb_code8_front_geometry": (ctypes.c_int, [ctypes.c_int, ctypes.c_int64, ctypes.c_int, c_vp, c_vp]),
    "mvdb_index_code8_front_counters": (ctypes.c_int, [c_vp, c_vp, c_vp, c_vp, c_vp]),
    "mvdb_index_code8_read_row": (ctypes.c_int, [c_vp, ctypes.c_int64, c_vp, c_vp, c_vp]),
    "mvdb_code8_bit2_pack": (ctypes.c_int, [ctypes.c_int, c_vp, c_vp]),
    "mvdb_code8_bit2_unpack": (ctypes.c_int, [ctypes.c_int, c_vp, c_vp]),
    "mvdb_index_code8_read_bit2": (ctypes.c_int, [c_vp, ctypes.c_int64, c_vp, c_vp]),
    "mvdb_code8_front_offset": (ctypes.c_int, [ctypes.c_int, ctypes.c_int64, ctypes.c_int, c_vp, c_vp]),
    "mvdb_code8_scan_geometry": (ctypes.c_int, [ctypes.c_int, ctypes.c_int64, ctypes.c_int, c_vp, c_vp]),
    "mvdb_index_dim": (ctypes.c_int, [c_vp]),
    "mvdb_index_device": (ctypes.c_int, [c_vp]),
    "mvdb_index_reserve": (ctypes.c_int, [c_vp, ctypes.c_int64]),
    "mvdb_index_add": (ctypes.c_int, [c_vp, c_vp, ctypes.c_int64, ctypes.c_int]),
    "mvdb_index_add_device": (ctypes.c_int, [c_vp, c_vp, ctypes.c_int64, ctypes.c_int]),
    "mvdb_index_add_synthetic": (ctypes.c_int, [c_vp, ctypes.c_int64, ctypes.c_uint64, ctypes.c_int64, ctypes.c_int]),
    "mvdb_index_get_rows": (ctypes.c_int, [c_vp, ctypes.c_int64, ctypes.c_int64, c_vp]),
    "mvdb_index_remove_rows": (ctypes.c_int, [c_vp, c_vp, ctypes.c_int64]),
    "mvdb_index_set_rows": (ctypes.c_int, [c_vp, c_vp, c_vp, ctypes.c_int64, ctypes.c_int]),
    "mvdb_index_set_rows_device": (ctypes.c_int, [c_vp, c_vp, c_vp, ctypes.c_int64, ctypes.c_int]),
    "mvdb_index_search": (ctypes.c_int, [c_vp, c_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_vp, c_vp]),
    "mvdb_index_search_device": (ctypes.c_int, [c_vp, c_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                ctypes.c_int64, c_vp, c_vp, c_vp]),
    "mvdb_index_search_subset": (ctypes.c_int, [c_vp, c_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_vp,
                                                ctypes.c_int64, c_vp, c_vp]),
    "mvdb_index_search_subset_device": (ctypes.c_int, [c_vp, c_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_vp,
                                                       ctypes.c_int64, ctypes.c_int, ctypes.c_int64, c_vp, c_vp, c_vp]),
    "mvdb_index_search_masked": (ctypes.c_int, [c_vp, c_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_vp, ctypes.c_int,
                                                c_vp, c_vp]),
    "mvdb_index_search_masked_device": (ctypes.c_int, [c_vp, c_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_vp,
                                                       ctypes.c_int, ctypes.c_int64, c_vp, c_vp, c_vp]),
    "mvdb_rowset_create": (ctypes.c_int, [c_vp, c_vp, ctypes.c_int64, ctypes.c_int, ctypes.POINTER(c_vp)]),
    "mvdb_rowset_size": (ctypes.c_int64, [c_vp]),
    "mvdb_rowset_is_bitmap": (ctypes.c_int, [c_vp]),
    "mvdb_rowset_free": (ctypes.c_int, [c_vp]),
    "mvdb_index_search_rowset": (ctypes.c_int, [c_vp, c_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_vp, c_vp, c_vp]),
    "mvdb_index_search_rowset_device": (ctypes.c_int, [c_vp, c_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_vp,
                                                       ctypes.c_int64, c_vp, c_vp, c_vp]),
    "mvdb_index_search_grouped": (ctypes.c_int, [c_vp, c_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_vp, c_vp, c_vp]),
    "mvdb_index_search_grouped_device": (ctypes.c_int, [c_vp, c_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_vp,
                                                        ctypes.c_int64, c_vp, c_vp, c_vp]),
    "mvdb_index_range_search": (ctypes.c_int, [c_vp, c_vp, ctypes.c_int, ctypes.c_float, ctypes.c_int, c_vp, ctypes.c_int64,
                                               c_vp, c_vp, c_vp]),
    "mvdb_index_range_search_device": (ctypes.c_int, [c_vp, c_vp, ctypes.c_int, ctypes.c_float, ctypes.c_int, c_vp,
                                                      ctypes.c_int64, ctypes.c_int64, c_vp, c_vp, c_vp, c_vp]),
    "mvdb_index_range_search_each": (ctypes.c_int, [c_vp, c_vp, ctypes.c_int, c_vp, ctypes.c_int, c_vp, ctypes.c_int64,
                                                    c_vp, c_vp, c_vp]),
    "mvdb_index_range_search_each_device": (ctypes.c_int, [c_vp, c_vp, ctypes.c_int, c_vp, ctypes.c_int, c_vp,
                                                           ctypes.c_int64, ctypes.c_int64, c_vp, c_vp, c_vp, c_vp]),
    "mvdb_range_band": (ctypes.c_double, [ctypes.c_int, ctypes.c_float, ctypes.c_float]),
    "mvdb_index_range_counters": (ctypes.c_int, [c_vp, c_vp, c_vp, c_vp]),
    "mvdb_index_range_join": (ctypes.c_int, [c_vp, c_vp, ctypes.c_int, ctypes.c_float, c_vp, ctypes.c_int64, c_vp, c_vp, c_vp]),
    "mvdb_index_join_counters": (ctypes.c_int, [c_vp, c_vp, c_vp]),
    "mvdb_index_search_mmr": (ctypes.c_int, [c_vp, c_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_int,
                                             c_vp, c_vp, c_vp]),
    "mvdb_index_search_mmr_device": (ctypes.c_int, [c_vp, c_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_float,
                                                    ctypes.c_int, c_vp, ctypes.c_int64, c_vp, c_vp, c_vp]),
    "mvdb_mmr_form": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "mvdb_grouping_create": (ctypes.c_int, [c_vp, c_vp, ctypes.c_int64, ctypes.c_int64, ctypes.POINTER(c_vp)]),
    "mvdb_grouping_rows": (ctypes.c_int64, [c_vp]),
    "mvdb_grouping_groups": (ctypes.c_int64, [c_vp]),
    "mvdb_grouping_free": (ctypes.c_int, [c_vp]),
    "mvdb_index_search_distinct": (ctypes.c_int, [c_vp, c_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_vp, c_vp,
                                                  c_vp, c_vp, c_vp]),
    "mvdb_index_search_distinct_device": (ctypes.c_int, [c_vp, c_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_vp,
                                                         c_vp, c_vp, c_vp, c_vp, ctypes.c_int64, c_vp]),
    "mvdb_index_distinct_counters": (ctypes.c_int, [c_vp, c_vp, c_vp]),
    "mvdb_index_search_groups": (ctypes.c_int, [c_vp, c_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                c_vp, c_vp, c_vp, c_vp, c_vp]),
    "mvdb_index_search_groups_device": (ctypes.c_int, [c_vp, c_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                       ctypes.c_int, c_vp, c_vp, c_vp, c_vp, c_vp, ctypes.c_int64, c_vp]),
    "mvdb_index_groups_counters": (ctypes.c_int, [c_vp, c_vp, c_vp]),
    "mvdb_index_search_maxsim": (ctypes.c_int, [c_vp, c_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_vp, c_vp, c_vp, c_vp, c_vp,
                                                c_vp]),
    "mvdb_index_search_maxsim_device": (ctypes.c_int, [c_vp, c_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_vp, c_vp, c_vp, c_vp,
                                                       c_vp, c_vp, ctypes.c_int64, c_vp]),
    "mvdb_index_maxsim_counters": (ctypes.c_int, [c_vp, c_vp, c_vp]),
    "mvdb_index_assign": (ctypes.c_int, [c_vp, c_vp, ctypes.c_int, ctypes.c_int, c_vp, c_vp, c_vp]),
    "mvdb_index_assign_device": (ctypes.c_int, [c_vp, c_vp, ctypes.c_int, ctypes.c_int, c_vp, c_vp, c_vp, c_vp]),
    "mvdb_index_assign_counters": (ctypes.c_int, [c_vp, c_vp, c_vp]),
    "mvdb_index_kmeans": (ctypes.c_int, [c_vp, c_vp, ctypes.c_int, ctypes.c_int, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "mvdb_partition_create": (ctypes.c_int, [c_vp, c_vp, ctypes.c_int, ctypes.c_int, c_vp, ctypes.POINTER(c_vp)]),
    "mvdb_partition_update": (ctypes.c_int, [c_vp, c_vp, c_vp, ctypes.c_int64]),
    "mvdb_partition_labels": (ctypes.c_int, [c_vp, ctypes.c_int64, ctypes.c_int64, c_vp]),
    "mvdb_partition_centres": (ctypes.c_int, [c_vp, c_vp]),
    "mvdb_partition_sizes": (ctypes.c_int, [c_vp, c_vp]),
    "mvdb_partition_rows": (ctypes.c_int64, [c_vp]),
    "mvdb_partition_lists": (ctypes.c_int, [c_vp]),
    "mvdb_partition_free": (ctypes.c_int, [c_vp]),
    "mvdb_index_search_probe": (ctypes.c_int, [c_vp, c_vp, c_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_vp, c_vp,
                                               c_vp]),
    "mvdb_index_search_probe_device": (ctypes.c_int, [c_vp, c_vp, c_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_vp,
                                                      ctypes.c_int64, c_vp, c_vp, c_vp]),
    "mvdb_index_probe_counters": (ctypes.c_int, [c_vp, c_vp, c_vp]),
    "mvdb_index_search_examples": (ctypes.c_int, [c_vp, c_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_vp, c_vp,
                                                  ctypes.c_int, c_vp, c_vp]),
    "mvdb_index_search_examples_device": (ctypes.c_int, [c_vp, c_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_vp, c_vp,
                                                         ctypes.c_int, ctypes.c_int64, c_vp, c_vp, c_vp]),
    "mvdb_index_examples_counters": (ctypes.c_int, [c_vp, c_vp, c_vp]),
    "mvdb_rowterm_create": (ctypes.c_int, [c_vp, c_vp, ctypes.c_int64, ctypes.POINTER(c_vp)]),
    "mvdb_rowterm_rows": (ctypes.c_int64, [c_vp]),
    "mvdb_rowterm_free": (ctypes.c_int, [c_vp]),
    "mvdb_index_search_boosted": (ctypes.c_int, [c_vp, c_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_float, c_vp, c_vp, ctypes.c_int,
                                                 c_vp, c_vp, ctypes.c_int64, c_vp, c_vp, c_vp]),
    "mvdb_index_search_boosted_device": (ctypes.c_int, [c_vp, c_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_float, c_vp, c_vp,
                                                        ctypes.c_int, c_vp, c_vp, ctypes.c_int64, c_vp, ctypes.c_int64, c_vp, c_vp, c_vp]),
    "mvdb_index_boost_combine": (ctypes.c_int, [c_vp, c_vp, c_vp, ctypes.c_int, c_vp, c_vp, ctypes.c_int64, c_vp]),
    "mvdb_index_boost_counters": (ctypes.c_int, [c_vp, c_vp, c_vp]),
    "mvdb_sparse_create": (ctypes.c_int, [c_vp, c_vp, c_vp, c_vp, ctypes.c_int64, ctypes.c_int64, ctypes.POINTER(c_vp)]),
    "mvdb_sparse_rows": (ctypes.c_int64, [c_vp]),
    "mvdb_sparse_nnz": (ctypes.c_int64, [c_vp]),
    "mvdb_sparse_dim": (ctypes.c_int64, [c_vp]),
    "mvdb_sparse_free": (ctypes.c_int, [c_vp]),
    "mvdb_sparse_geometry": (ctypes.c_int, [c_vp, c_vp, c_vp]),
    "mvdb_index_sparse_scores": (ctypes.c_int, [c_vp, c_vp, c_vp, c_vp, ctypes.c_int, c_vp, c_vp]),
    "mvdb_index_search_sparse": (ctypes.c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, ctypes.c_int, ctypes.c_int, c_vp, c_vp, c_vp]),
    "mvdb_index_search_sparse_device": (ctypes.c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, ctypes.c_int, ctypes.c_int, c_vp, ctypes.c_int64, c_vp, c_vp,
                                                       c_vp]),
    "mvdb_index_search_hybrid": (ctypes.c_int, [c_vp, c_vp, c_vp, ctypes.c_int, c_vp, c_vp, c_vp, ctypes.c_int, ctypes.c_int, ctypes.c_float,
                                                ctypes.c_float, c_vp, c_vp, c_vp]),
    "mvdb_index_search_hybrid_device": (ctypes.c_int, [c_vp, c_vp, c_vp, ctypes.c_int, c_vp, c_vp, c_vp, ctypes.c_int, ctypes.c_int, ctypes.c_float,
                                                       ctypes.c_float, c_vp, ctypes.c_int64, c_vp, c_vp, c_vp]),
    "mvdb_index_sparse_counters": (ctypes.c_int, [c_vp, c_vp, c_vp]),
    "mvdb_sparse_build_postings": (ctypes.c_int, [c_vp, c_vp]),
    "mvdb_sparse_drop_postings": (ctypes.c_int, [c_vp]),
    "mvdb_sparse_has_postings": (ctypes.c_int, [c_vp]),
    "mvdb_sparse_postings_geometry": (ctypes.c_int, [c_vp, c_vp, c_vp]),
    "mvdb_sparse_postings_read": (ctypes.c_int, [c_vp, c_vp, c_vp, c_vp]),
    "mvdb_index_sparse_postings_counters": (ctypes.c_int, [c_vp, c_vp, c_vp, c_vp]),
    "mvdb_comm_available": (ctypes.c_int, []),
    "mvdb_comm_unique_id": (ctypes.c_int, [c_vp]),
    "mvdb_comm_create": (ctypes.c_int, [c_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(c_vp)]),
    "mvdb_comm_free": (ctypes.c_int, [c_vp]),
    "mvdb_comm_rank": (ctypes.c_int, [c_vp]),
    "mvdb_comm_world": (ctypes.c_int, [c_vp]),
    "mvdb_allgather_topk": (ctypes.c_int, [c_vp, c_vp, c_vp, ctypes.c_int64, c_vp]),
    "mvdb_merge_topk_device": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_vp,
                                              ctypes.c_int64, c_vp, ctypes.c_int64, c_vp, c_vp, ctypes.c_int, c_vp]),
    "mvdb_normalize_l2": (ctypes.c_int, [c_vp, ctypes.c_int64, ctypes.c_int, ctypes.c_int]),
    "mvdb_synth_fill_device": (ctypes.c_int, [c_vp, ctypes.c_int64, ctypes.c_int, ctypes.c_uint64, ctypes.c_int64,
                                              ctypes.c_int, ctypes.c_int, c_vp]),
    "mvdb_split_rerun_count": (ctypes.c_int64, []),
    "mvdb_rescue_tile_stats": (ctypes.c_int, [ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64)]),
    "mvdb_half_eps": (ctypes.c_double, [ctypes.c_int]),
    "mvdb_half_max_queries": (ctypes.c_int, [ctypes.c_int]),
    "mvdb_prof_enable": (ctypes.c_int, [ctypes.c_int]),
    "mvdb_prof_read": (ctypes.c_int, [ctypes.c_char_p, ctypes.POINTER(ctypes.c_int64),
                                      ctypes.POINTER(ctypes.c_double)]),
    "mvdb_prof_symbol": (ctypes.c_int, [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int]),
    "mvdb_prof_live_events": (ctypes.c_int64, []),
    # int8 cosine index (cos8.hip)
    "mvdb_cos8_create": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.POINTER(c_vp)]),
    "mvdb_cos8_free": (ctypes.c_int, [c_vp]),
    "mvdb_cos8_reset": (ctypes.c_int, [c_vp]),
    "mvdb_cos8_reserve": (ctypes.c_int, [c_vp, ctypes.c_int64]),
    "mvdb_cos8_ntotal": (ctypes.c_int64, [c_vp]),
    "mvdb_cos8_dim": (ctypes.c_int, [c_vp]),
    "mvdb_cos8_add": (ctypes.c_int, [c_vp, c_vp, ctypes.c_int64]),
    "mvdb_cos8_add_device": (ctypes.c_int, [c_vp, c_vp, ctypes.c_int64]),
    "mvdb_cos8_get_codes": (ctypes.c_int, [c_vp, ctypes.c_int64, ctypes.c_int64, c_vp, c_vp]),
    "mvdb_cos8_remove_rows": (ctypes.c_int, [c_vp, c_vp, ctypes.c_int64]),
    "mvdb_cos8_set_rows": (ctypes.c_int, [c_vp, c_vp, c_vp, ctypes.c_int64]),
    "mvdb_cos8_set_rows_device": (ctypes.c_int, [c_vp, c_vp, c_vp, ctypes.c_int64]),
    "mvdb_cos8_search": (ctypes.c_int, [c_vp, c_vp, ctypes.c_int, ctypes.c_int, c_vp, c_vp]),
    "mvdb_cos8_search_device": (ctypes.c_int, [c_vp, c_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int64, c_vp, c_vp,
                                               c_vp]),
    "mvdb_cos8_rowset_create": (ctypes.c_int, [c_vp, c_vp, ctypes.c_int64, ctypes.c_int, ctypes.POINTER(c_vp)]),
    "mvdb_cos8_rowset_size": (ctypes.c_int64, [c_vp]),
    "mvdb_cos8_rowset_is_bitmap": (ctypes.c_int, [c_vp]),
    "mvdb_cos8_rowset_free": (ctypes.c_int, [c_vp]),
    "mvdb_cos8_search_rowset": (ctypes.c_int, [c_vp, c_vp, ctypes.c_int, ctypes.c_int, c_vp, c_vp, c_vp]),
    "mvdb_cos8_search_rowset_device": (ctypes.c_int, [c_vp, c_vp, ctypes.c_int, ctypes.c_int, c_vp, ctypes.c_int64,
                                                      c_vp, c_vp, c_vp]),
    # encoder (encoder.hip)
    "mvdb_encoder_weight_count": (ctypes.c_int, [ctypes.POINTER(EncoderCfg)]),
    "mvdb_encoder_weight_name": (ctypes.c_char_p, [ctypes.POINTER(EncoderCfg), ctypes.c_int]),
    "mvdb_encoder_create": (ctypes.c_int, [ctypes.POINTER(EncoderCfg), ctypes.POINTER(c_vp), ctypes.c_int,
                                           ctypes.POINTER(c_vp)]),
    "mvdb_encoder_free": (ctypes.c_int, [c_vp]),
    "mvdb_encoder_gemm_tile_form": (ctypes.c_int, [ctypes.c_int64, ctypes.c_int, ctypes.c_int]),
    "mvdb_encoder_splitk_planes": (ctypes.c_int, [ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "mvdb_index_single_route_suspensions": (ctypes.c_longlong, [c_vp]),
    "mvdb_encoder_walks": (ctypes.c_int, [c_vp, ctypes.c_int, ctypes.c_int]),
    "mvdb_encoder_walk_stats": (ctypes.c_int, [c_vp, c_vp, c_vp, c_vp]),
    "mvdb_encoder_overflow_flag": (c_vp, [c_vp]),
    "mvdb_encoder_forward": (ctypes.c_int, [c_vp, c_vp, c_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_vp]),
    "mvdb_encoder_forward_device": (ctypes.c_int, [c_vp, c_vp, c_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                   c_vp, c_vp, c_vp]),
    "mvdb_encoder_set_heads": (ctypes.c_int, [c_vp, ctypes.POINTER(M3Heads)]),
    "mvdb_encoder_forward_multi_device": (ctypes.c_int, [c_vp, c_vp, c_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_vp,
                                                         ctypes.POINTER(M3Out), c_vp]),
}


def _bind_torch_hip_runtime():
    """One HIP runtime per process (module docstring): torch's own, loaded before libmvdb.so resolves its
    ``libamdhip64.so.7`` dependency."""
    import sys
    if "torch" in sys.modules or os.environ.get("MVDB_IMPORT_TORCH_FIRST") == "1":
        import torch  # noqa: F401
        return
    import importlib.util
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return  # no torch in this environment: the system ROCm runtime serves
    cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if os.path.exists(cand):
        try:
            ctypes.CDLL(cand, mode=ctypes.RTLD_GLOBAL)
            return
        except OSError:
            pass
    import torch  # noqa: F401  (layout not recognised: the slow, certain way)


def lib():
    """Load libmvdb.so (once).  Raises if the in-tree build is missing — never falls back."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: build the HIP library first "
            "(python -c 'import __graft_entry__ as g; g.build()' or make -C minivectordb_amd/csrc). "
            "minivectordb_amd has no CPU fallback.")
    _bind_torch_hip_runtime()
    L = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
    for name, (res, args) in PROTOTYPES.items():
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return _lib


def last_error():
    msg = lib().mvdb_last_error()
    return msg.decode("utf-8", "replace") if msg else ""


def check(rc):
    """Map a non-zero status to the Python exception the drop-in layer promises."""
    if rc == 0:
        return
    msg = last_error()
    if rc == ERR_ARG:
        raise ValueError(msg)
    if rc == ERR_OOM:
        raise MemoryError(msg)
    raise RuntimeError(msg)


def device_count():
    n = ctypes.c_int(0)
    check(lib().mvdb_device_count(ctypes.byref(n)))
    return n.value


def _ptr(a):
    return ctypes.c_void_p(a.ctypes.data)


class FlatIndex:
    """Thin object wrapper over mvdb_index*: the device-resident flat matrix + search."""

    def __init__(self, d, metric=METRIC_IP, device=0):
        self._h = ctypes.c_void_p()
        self.d = int(d)
        self.metric = metric
        self.device = device
        check(lib().mvdb_index_create(self.d, metric, device, ctypes.byref(self._h)))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            lib().mvdb_index_free(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    @property
    def ntotal(self):
        return int(lib().mvdb_index_ntotal(self._h))

    @property
    def shadow_rows(self):
        """Rows in the fp16 shadow the batch passes stream (0: none yet / not applicable)."""
        return int(lib().mvdb_index_shadow_rows(self._h))

    @property
    def code8_rows(self):
        """Rows in the int8 code the single-query prefilter streams (0: none yet / not applicable)."""
        return int(lib().mvdb_index_code8_rows(self._h))

    def code8_counters(self):
        """(fallbacks, candidates of the latest call, calls) of the single-query prefilter route; lags by the calls in flight."""
        v = [ctypes.c_longlong(0) for _ in range(3)]
        check(lib().mvdb_index_code8_counters(self._h, *[ctypes.byref(x) for x in v]))
        return tuple(int(x.value) for x in v)

    def code8_front_counters(self):
        """(rows the front plane could not reject over all calls of the front form, those calls, suspensions of the front
        form, whether the code holds the front plane) — diagnostic; synchronises with the device."""
        v = [ctypes.c_longlong(0) for _ in range(3)]
        held = ctypes.c_int(0)
        check(lib().mvdb_index_code8_front_counters(self._h, *[ctypes.byref(x) for x in v], ctypes.byref(held)))
        return tuple(int(x.value) for x in v) + (bool(held.value),)

    def code8_read_row(self, row, front=True):
        """(high plane, low plane, front-plane image or None) of one stored row of the int8 code, as uint8 arrays (diagnostic)."""
        d = self.d
        high, low = np.empty(d // 4 * 3, np.uint8), np.empty(d // 4, np.uint8)
        image = np.empty(d // 8 * 5, np.uint8) if front else None
        check(lib().mvdb_index_code8_read_row(self._h, int(row), high.ctypes.data, low.ctypes.data, image.ctypes.data if front else None))
        return high, low, image

    def code8_bit_plane_held(self):
        """Whether the int8 code holds the plane of bit 2 (index option code8_bit_plane) — diagnostic."""
        held = ctypes.c_int(0)
        check(lib().mvdb_index_code8_read_bit2(self._h, 0, None, ctypes.byref(held)))
        return bool(held.value)

    def code8_read_bit2(self, row):
        """The d / 8 bytes of one stored row in the bit plane of the int8 code, as a uint8 array (diagnostic)."""
        bits = np.empty(self.d // 8, np.uint8)
        check(lib().mvdb_index_code8_read_bit2(self._h, int(row), bits.ctypes.data, None))
        return bits

    def code8_refined(self):
        """Rows whose low plane the prefilter has fetched, over all calls so far (diagnostic; synchronises with the device)."""
        v = ctypes.c_longlong(0)
        check(lib().mvdb_index_code8_refined(self._h, ctypes.byref(v)))
        return int(v.value)

    def reset(self):
        check(lib().mvdb_index_reset(self._h))

    def reserve(self, n):
        check(lib().mvdb_index_reserve(self._h, int(n)))

    def set_option(self, name, value):
        """Per-index switch set in code (include/mvdb.h: mvdb_index_set_option): "shadow_single_query", "half_shadow",
        "compact_bytes"."""
        check(lib().mvdb_index_set_option(self._h, str(name).encode(), int(value)))

    def reload_env(self):
        """Re-read the MVDB_* hooks (the library reads them once, when the index is created)."""
        check(lib().mvdb_index_reload_env(self._h))

    def add(self, x, normalize=False):
        x = np.ascontiguousarray(x, dtype=np.float32)
        if x.ndim != 2 or x.shape[1] != self.d:
            raise ValueError(f"expected [n,{self.d}] float32, got {x.shape}")
        check(lib().mvdb_index_add(self._h, _ptr(x), x.shape[0], int(bool(normalize))))

    def add_device(self, ptr, n, normalize=False):
        check(lib().mvdb_index_add_device(self._h, ctypes.c_void_p(ptr), int(n), int(bool(normalize))))

    def add_synthetic(self, n, seed, first_row=0, normalize=True):
        check(lib().mvdb_index_add_synthetic(self._h, int(n), int(seed), int(first_row), int(bool(normalize))))

    def get_rows(self, row0, n, out=None):
        """Rows [row0, row0+n) as float32 [n,d]; `out` (C-contiguous float32 [n,d]) is filled in place
        when given (no temporary for multi-GB read-backs)."""
        if out is None:
            out = np.empty((int(n), self.d), dtype=np.float32)
        elif not (isinstance(out, np.ndarray) and out.dtype == np.float32 and out.flags["C_CONTIGUOUS"]
                  and out.shape == (int(n), self.d)):
            raise ValueError("out must be a C-contiguous float32 array of shape [n, d]")
        check(lib().mvdb_index_get_rows(self._h, int(row0), int(n), _ptr(out)))
        return out

    def remove_rows(self, rows):
        rows = np.ascontiguousarray(rows, dtype=np.int64)
        check(lib().mvdb_index_remove_rows(self._h, _ptr(rows), rows.shape[0]))

    def set_rows(self, rows, x, normalize=False):
        """Overwrite the stored rows `rows` (distinct, each in [0, ntotal)) with x[len(rows), d] in place: nothing is
        renumbered, dropped or rebuilt (include/mvdb.h: mvdb_index_set_rows)."""
        rows = np.ascontiguousarray(rows, dtype=np.int64)
        x = np.ascontiguousarray(x, dtype=np.float32)
        if rows.ndim != 1 or x.ndim != 2 or x.shape[1] != self.d or x.shape[0] != rows.shape[0]:
            raise ValueError(f"expected [m] rows and [m,{self.d}] float32, got {rows.shape} and {x.shape}")
        check(lib().mvdb_index_set_rows(self._h, _ptr(rows), _ptr(x), rows.shape[0], int(bool(normalize))))

    def set_rows_device(self, rows, x_ptr, m, normalize=False):
        """Same, the new rows in device memory ([m, d] dense float32 at x_ptr); the row numbers stay a host array."""
        rows = np.ascontiguousarray(rows, dtype=np.int64)
        if rows.ndim != 1 or rows.shape[0] != int(m):
            raise ValueError(f"expected {int(m)} row numbers, got {rows.shape}")
        check(lib().mvdb_index_set_rows_device(self._h, _ptr(rows), ctypes.c_void_p(x_ptr), int(m), int(bool(normalize))))

    def search(self, q, k, normalize_q=False):
        q = np.ascontiguousarray(np.atleast_2d(np.asarray(q, dtype=np.float32)))
        if q.shape[1] != self.d:
            raise ValueError(f"query dimension {q.shape[1]} != index dimension {self.d}")
        nq = q.shape[0]
        D = np.empty((nq, k), dtype=np.float32)
        I = np.empty((nq, k), dtype=np.int64)
        check(lib().mvdb_index_search(self._h, _ptr(q), nq, int(k), int(bool(normalize_q)), _ptr(D), _ptr(I)))
        return D, I

    def search_subset(self, q, k, rows, normalize_q=False):
        q = np.ascontiguousarray(np.atleast_2d(np.asarray(q, dtype=np.float32)))
        if q.shape[1] != self.d:
            raise ValueError(f"query dimension {q.shape[1]} != index dimension {self.d}")
        rows = np.ascontiguousarray(rows, dtype=np.int64)
        nq = q.shape[0]
        D = np.empty((nq, k), dtype=np.float32)
        I = np.empty((nq, k), dtype=np.int64)
        check(lib().mvdb_index_search_subset(self._h, _ptr(q), nq, int(k), int(bool(normalize_q)), _ptr(rows),
                                             rows.shape[0], _ptr(D), _ptr(I)))
        return D, I

    def rowset(self, rows, excluded=False):
        """The listed rows (or, excluded=True, every row BUT them) made resident on the device for repeated searches under
        one filter: see RowSet."""
        return RowSet(self, rows, excluded)

    def search_rowset(self, q, k, rowset, normalize_q=False):
        """Search a resident RowSet; labels are ROW NUMBERS of the index."""
        q = np.ascontiguousarray(np.atleast_2d(np.asarray(q, dtype=np.float32)))
        if q.shape[1] != self.d:
            raise ValueError(f"query dimension {q.shape[1]} != index dimension {self.d}")
        nq = q.shape[0]
        D = np.empty((nq, k), dtype=np.float32)
        I = np.empty((nq, k), dtype=np.int64)
        check(lib().mvdb_index_search_rowset(self._h, _ptr(q), nq, int(k), int(bool(normalize_q)), rowset._h, _ptr(D),
                                             _ptr(I)))
        return D, I

    def search_rowset_device(self, q_ptr, nq, k, rowset, D_ptr, I_ptr, stream=0, normalize_q=False, label_offset=0):
        """Device-pointer variant of search_rowset (labels: row numbers + label_offset); enqueues on `stream` and returns."""
        check(lib().mvdb_index_search_rowset_device(
            self._h, ctypes.c_void_p(q_ptr), int(nq), int(k), int(bool(normalize_q)), rowset._h, int(label_offset),
            ctypes.c_void_p(D_ptr), ctypes.c_void_p(I_ptr), ctypes.c_void_p(stream)))

    @staticmethod
    def _rowset_table(rowsets, nq):
        """The `const mvdb_rowset* const*` argument of the grouped entry points: one handle per query, NULL = every row."""
        rowsets = list(rowsets)
        if len(rowsets) != nq:
            raise ValueError(f"{len(rowsets)} row sets for {nq} queries")
        table = (ctypes.c_void_p * nq)()
        for i, rs in enumerate(rowsets):
            if rs is not None:
                if not rs._h:
                    raise ValueError(f"row set {i} is closed")
                table[i] = rs._h.value
        return table

    def search_grouped(self, q, k, rowsets, normalize_q=False, out=None):
        """Every query under ITS OWN resident RowSet (None = every row): row i is bit for bit what search_rowset(q[i:i+1], k,
        rowsets[i]) / search(q[i:i+1], k) returns.  List-form sets share one gathered launch; labels are row numbers.
        out=(D, I): caller-owned result arrays (float32 / int64, [nq, k], C-contiguous)."""
        q = np.ascontiguousarray(np.atleast_2d(np.asarray(q, dtype=np.float32)))
        if q.shape[1] != self.d:
            raise ValueError(f"query dimension {q.shape[1]} != index dimension {self.d}")
        nq = q.shape[0]
        table = self._rowset_table(rowsets, nq)
        if out is None:
            D = np.empty((nq, k), dtype=np.float32)
            I = np.empty((nq, k), dtype=np.int64)
        else:
            D, I = out
            if (D.dtype != np.float32 or I.dtype != np.int64 or D.shape != (nq, k) or I.shape != (nq, k)
                    or not D.flags.c_contiguous or not I.flags.c_contiguous):
                raise ValueError("out must be C-contiguous (float32[nq, k], int64[nq, k])")
        check(lib().mvdb_index_search_grouped(self._h, _ptr(q), nq, int(k), int(bool(normalize_q)), table, _ptr(D), _ptr(I)))
        return D, I

    def search_grouped_device(self, q_ptr, nq, k, rowsets, D_ptr, I_ptr, stream=0, normalize_q=False, label_offset=0):
        """Device-pointer variant of search_grouped (labels: row numbers + label_offset); enqueues on `stream` and returns."""
        table = self._rowset_table(rowsets, int(nq))
        check(lib().mvdb_index_search_grouped_device(
            self._h, ctypes.c_void_p(q_ptr), int(nq), int(k), int(bool(normalize_q)), table, int(label_offset),
            ctypes.c_void_p(D_ptr), ctypes.c_void_p(I_ptr), ctypes.c_void_p(stream)))

    def search_masked(self, q, k, mask_words, normalize_q=False, labels="rows"):
        """Search the rows whose bit is set in `mask_words` (uint64[(ntotal + 63) // 64], bit r & 63 of word r >> 6 = row r;
        `pack_row_mask` builds it).  labels="rows": row numbers; "positions": positions in the ascending list of the
        selected rows (what search_subset returns for that list)."""
        q = np.ascontiguousarray(np.atleast_2d(np.asarray(q, dtype=np.float32)))
        if q.shape[1] != self.d:
            raise ValueError(f"query dimension {q.shape[1]} != index dimension {self.d}")
        mask_words = np.ascontiguousarray(mask_words, dtype=np.uint64)
        if mask_words.shape[0] < (self.ntotal + 63) // 64:
            raise ValueError("the mask has fewer than (ntotal + 63) // 64 words")
        nq = q.shape[0]
        D = np.empty((nq, k), dtype=np.float32)
        I = np.empty((nq, k), dtype=np.int64)
        check(lib().mvdb_index_search_masked(self._h, _ptr(q), nq, int(k), int(bool(normalize_q)), _ptr(mask_words),
                                             {"positions": 0, "rows": 1}[labels], _ptr(D), _ptr(I)))
        return D, I

    def search_masked_device(self, q_ptr, nq, k, mask_ptr, D_ptr, I_ptr, stream=0, normalize_q=False, labels="rows",
                             label_offset=0):
        """Device-pointer variant of search_masked."""
        check(lib().mvdb_index_search_masked_device(
            self._h, ctypes.c_void_p(q_ptr), int(nq), int(k), int(bool(normalize_q)), ctypes.c_void_p(mask_ptr),
            {"positions": 0, "rows": 1}[labels], int(label_offset), ctypes.c_void_p(D_ptr), ctypes.c_void_p(I_ptr),
            ctypes.c_void_p(stream)))

    def search_device(self, q_ptr, nq, k, D_ptr, I_ptr, stream=0, normalize_q=False, label_offset=0):
        """All buffers are device pointers (ints); enqueues on `stream` and returns."""
        check(lib().mvdb_index_search_device(self._h, ctypes.c_void_p(q_ptr), int(nq), int(k),
                                             int(bool(normalize_q)), int(label_offset), ctypes.c_void_p(D_ptr),
                                             ctypes.c_void_p(I_ptr), ctypes.c_void_p(stream)))


    def search_subset_device(self, q_ptr, nq, k, rows_ptr, m, D_ptr, I_ptr, stream=0, normalize_q=False,
                             map_labels=False, label_offset=0):
        """Device-pointer variant of search_subset (rows already validated and resident on the device)."""
        check(lib().mvdb_index_search_subset_device(
            self._h, ctypes.c_void_p(q_ptr), int(nq), int(k), int(bool(normalize_q)), ctypes.c_void_p(rows_ptr), int(m),
            int(bool(map_labels)), int(label_offset), ctypes.c_void_p(D_ptr), ctypes.c_void_p(I_ptr),
            ctypes.c_void_p(stream)))

    # ---- range search: every selected row at or above a threshold (include/mvdb.h "RANGE SEARCH") -------------------
    RANGE_DEFAULT_CAP = 1024

    def _range_queries(self, q):
        q = np.ascontiguousarray(np.atleast_2d(np.asarray(q, dtype=np.float32)))
        if q.ndim != 2 or q.shape[1] != self.d:
            raise ValueError(f"query dimension {q.shape[-1]} != index dimension {self.d}")
        return q

    @staticmethod
    def _range_thresholds(threshold, nq):
        """None for a scalar threshold; else float32[nq] (one threshold per query; a NaN entry or another length: ValueError)."""
        if np.ndim(threshold) == 0:
            return None
        t = np.ascontiguousarray(threshold, dtype=np.float32)
        if t.ndim != 1 or t.shape[0] != nq:
            raise ValueError(f"{t.shape} thresholds for {nq} queries: pass a scalar or one per query")
        if np.isnan(t).any():
            raise ValueError("a threshold is NaN")
        return t

    def range_counters(self):
        """(calls that took the shared pass, queries its fallback answered, candidates of the latest launch group)."""
        v = [ctypes.c_longlong(0) for _ in range(3)]
        check(lib().mvdb_index_range_counters(self._h, *[ctypes.byref(x) for x in v]))
        return tuple(int(x.value) for x in v)

    def range_search_raw(self, q, threshold, cap, rowset=None, normalize_q=False, out=None):
        """One call of mvdb_index_range_search (scalar `threshold`) or mvdb_index_range_search_each (one per query): (counts
        int64[nq], D float32[nq, cap], I int64[nq, cap]).  A query whose count exceeds `cap` has a row of missing markers (-1);
        its count is still the true count.  out=(counts, D, I): caller-owned arrays (D / I may be None with cap == 0)."""
        q = self._range_queries(q)
        nq, cap = q.shape[0], int(cap)
        each = self._range_thresholds(threshold, nq)
        if out is None:
            counts = np.empty(nq, dtype=np.int64)
            D = np.empty((nq, cap), dtype=np.float32) if cap > 0 else None
            I = np.empty((nq, cap), dtype=np.int64) if cap > 0 else None
        else:
            counts, D, I = out
        if each is not None:
            check(lib().mvdb_index_range_search_each(
                self._h, _ptr(q), nq, _ptr(each), int(bool(normalize_q)), rowset._h if rowset is not None else None, cap,
                _ptr(counts), _ptr(D) if D is not None else None, _ptr(I) if I is not None else None))
            return counts, D, I
        check(lib().mvdb_index_range_search(
            self._h, _ptr(q), nq, float(threshold), int(bool(normalize_q)), rowset._h if rowset is not None else None, cap,
            _ptr(counts), _ptr(D) if D is not None else None, _ptr(I) if I is not None else None))
        return counts, D, I

    def range_count(self, q, threshold, rowset=None, normalize_q=False):
        """int64[nq]: how many selected rows reach the threshold — a scalar, or one per query — (inner product: score >=
        threshold; L2: squared distance <= threshold)."""
        return self.range_search_raw(q, threshold, 0, rowset, normalize_q)[0]

    def range_search(self, q, threshold, rowset=None, normalize_q=False, cap=None):
        """Every selected row that reaches the threshold, in faiss's range_search layout: (lims int64[nq + 1], D, I) with the
        results of query i at [lims[i], lims[i + 1]), best first, ties to the lower row; labels are ROW NUMBERS.  Calls with
        a capacity (`cap`, default 1024 per query) and once more, for the queries that overflowed only, with the largest
        count seen.  `threshold`: a scalar, or one per query."""
        q = self._range_queries(q)
        nq = q.shape[0]
        each = self._range_thresholds(threshold, nq)
        cap = self.RANGE_DEFAULT_CAP if cap is None else int(cap)
        if cap < 0:
            raise ValueError("cap must not be negative")
        for _ in range(3):
            counts, D, I = self.range_search_raw(q, threshold, cap, rowset, normalize_q)
            lims = np.zeros(nq + 1, dtype=np.int64)
            np.cumsum(counts, out=lims[1:])
            Dout = np.empty(int(lims[-1]), dtype=np.float32)
            Iout = np.empty(int(lims[-1]), dtype=np.int64)
            over = np.flatnonzero(counts > cap)
            for i in np.flatnonzero(counts <= cap):
                Dout[lims[i]:lims[i + 1]] = D[i, :counts[i]]
                Iout[lims[i]:lims[i + 1]] = I[i, :counts[i]]
            if over.size:
                c2, D2, I2 = self.range_search_raw(q[over], threshold if each is None else each[over], int(counts[over].max()),
                                                   rowset, normalize_q)
                if not np.array_equal(c2, counts[over]):
                    continue   # rows were added or removed between the two calls: both again, on the index as it is now
                for j, i in enumerate(over):
                    Dout[lims[i]:lims[i + 1]] = D2[j, :c2[j]]
                    Iout[lims[i]:lims[i + 1]] = I2[j, :c2[j]]
            return lims, Dout, Iout
        # the same error class as a row set outdated by a removal: callers that retry after a racing write retry this too
        raise ValueError("the index kept changing between the two calls of a range search")

    def range_search_device(self, q_ptr, nq, threshold, cap, counts_ptr, D_ptr, I_ptr, rowset=None, stream=0,
                            normalize_q=False, label_offset=0, thresholds_ptr=0):
        """Device-pointer variant of range_search_raw (counts int64[nq], D float32[nq, cap], I int64[nq, cap] on the device;
        labels: row numbers + label_offset); enqueues on `stream` and returns.  `threshold`: a Python number, or
        ``thresholds_ptr=`` the device address of float32[nq] (one per query; a NaN there matches nothing)."""
        if thresholds_ptr:
            check(lib().mvdb_index_range_search_each_device(
                self._h, ctypes.c_void_p(q_ptr), int(nq), ctypes.c_void_p(thresholds_ptr), int(bool(normalize_q)),
                rowset._h if rowset is not None else None, int(cap), int(label_offset), ctypes.c_void_p(counts_ptr),
                ctypes.c_void_p(D_ptr) if D_ptr else None, ctypes.c_void_p(I_ptr) if I_ptr else None, ctypes.c_void_p(stream)))
            return
        check(lib().mvdb_index_range_search_device(
            self._h, ctypes.c_void_p(q_ptr), int(nq), float(threshold), int(bool(normalize_q)),
            rowset._h if rowset is not None else None, int(cap), int(label_offset), ctypes.c_void_p(counts_ptr),
            ctypes.c_void_p(D_ptr) if D_ptr else None, ctypes.c_void_p(I_ptr) if I_ptr else None, ctypes.c_void_p(stream)))

    # ---- range join: which stored rows are near each other (include/mvdb.h "RANGE JOIN") ----------------------------
    JOIN_DEFAULT_CAP = 64

    def join_counters(self):
        """(join calls that took the shared pass, query rows its fallback answered): running totals."""
        v = [ctypes.c_longlong(0) for _ in range(2)]
        check(lib().mvdb_index_join_counters(self._h, *[ctypes.byref(x) for x in v]))
        return tuple(int(x.value) for x in v)

    def range_join_raw(self, qrows, threshold, cap, rowset=None):
        """One call of mvdb_index_range_join: query i is STORED row qrows[i], matched against the rows below it (of the row
        set, if one is given).  (counts int64[nq], D float32[nq, cap], I int64[nq, cap]); a row whose count exceeds `cap` has
        missing markers (-1) and its true count; cap == 0: counts only, D and I are None."""
        qrows = np.ascontiguousarray(qrows, dtype=np.int64).reshape(-1)
        nq, cap = qrows.shape[0], int(cap)
        counts = np.empty(nq, dtype=np.int64)
        D = np.empty((nq, cap), dtype=np.float32) if cap > 0 else None
        I = np.empty((nq, cap), dtype=np.int64) if cap > 0 else None
        check(lib().mvdb_index_range_join(self._h, _ptr(qrows), nq, float(threshold), rowset._h if rowset is not None else None, cap,
                                          _ptr(counts), _ptr(D) if D is not None else None, _ptr(I) if I is not None else None))
        return counts, D, I

    def _join_rows(self, first_row, rows):
        if rows is None:
            return np.arange(int(first_row), self.ntotal, dtype=np.int64)
        return np.ascontiguousarray(rows, dtype=np.int64).reshape(-1)

    def range_join(self, threshold, first_row=0, rows=None, rowset=None, cap=None, block=4096):
        """Every pair (earlier row, later row) of stored rows that reaches the threshold, found from its later member:
        (qrows int64[nq], lims int64[nq + 1], D, I) in faiss's range layout — the rows below qrows[i] (of the row set, if one is
        given) that match it are I[lims[i]:lims[i + 1]], best first, ties to the lower row.  The query rows are `rows`, or every
        row from `first_row` on; no row is uploaded.  Works through them `block` at a time with a small per-row `cap`
        (default 64); the rows of a block that overflowed are asked once more with the largest count seen."""
        qrows = self._join_rows(first_row, rows)
        cap = self.JOIN_DEFAULT_CAP if cap is None else int(cap)
        block = int(block)
        if cap < 0 or block <= 0:
            raise ValueError("cap must not be negative and block must be positive")
        lims = np.zeros(qrows.shape[0] + 1, dtype=np.int64)
        Ds, Is = [], []
        for b0 in range(0, qrows.shape[0], block):
            part = qrows[b0:b0 + block]
            for _ in range(3):
                counts, D, I = self.range_join_raw(part, threshold, cap, rowset)
                fits = counts <= cap
                over = np.flatnonzero(~fits)
                if over.size:
                    c2, D2, I2 = self.range_join_raw(part[over], threshold, int(counts[over].max()), rowset)
                    if not np.array_equal(c2, counts[over]):
                        continue   # rows were written between the two calls: both again, on the index as it is now
                keep = np.arange(cap)[None, :] < counts[:, None] if cap > 0 else np.zeros((part.shape[0], 0), dtype=bool)
                if not over.size:
                    Ds.append(D[keep] if cap > 0 else np.empty(0, np.float32))
                    Is.append(I[keep] if cap > 0 else np.empty(0, np.int64))
                else:
                    which = {int(i): j for j, i in enumerate(over)}
                    for i in range(part.shape[0]):
                        if i in which:
                            j = which[i]
                            Ds.append(D2[j, :c2[j]])
                            Is.append(I2[j, :c2[j]])
                        else:
                            Ds.append(D[i, :counts[i]])
                            Is.append(I[i, :counts[i]])
                np.cumsum(counts, out=lims[b0 + 1:b0 + 1 + part.shape[0]])
                lims[b0 + 1:b0 + 1 + part.shape[0]] += lims[b0]
                break
            else:
                raise ValueError("the index kept changing between the two calls of a range join")
        Dout = np.concatenate(Ds) if Ds else np.empty(0, dtype=np.float32)
        Iout = np.concatenate(Is) if Is else np.empty(0, dtype=np.int64)
        return qrows, lims, Dout.astype(np.float32, copy=False), Iout.astype(np.int64, copy=False)

    def range_join_count(self, threshold, first_row=0, rows=None, rowset=None, block=4096):
        """int: how many pairs range_join would list (no pair is fetched)."""
        qrows = self._join_rows(first_row, rows)
        total = 0
        for b0 in range(0, qrows.shape[0], int(block)):
            total += int(self.range_join_raw(qrows[b0:b0 + int(block)], threshold, 0, rowset)[0].sum())
        return total

    # ---- MMR search: k diverse rows picked on the device from the top fetch_k (include/mvdb.h "MMR SEARCH") ----------
    MMR_MAX_FETCH = 1024

    def search_mmr(self, q, k, fetch_k, lambda_mult, rowset=None, normalize_q=False, out=None):
        """(D float32[nq, k], I int64[nq, k]): per query k of the `fetch_k` best rows (of the row set, if one is given), picked
        greedily by lambda_mult * relevance - (1 - lambda_mult) * (largest inner product with a row already picked), in
        selection order; D holds the rows' search scores, labels are ROW NUMBERS, a short row ends in -1 / -FLT_MAX.
        out=(D, I): caller-owned result arrays (float32 / int64, [nq, k], C-contiguous)."""
        q = np.ascontiguousarray(np.atleast_2d(np.asarray(q, dtype=np.float32)))
        if q.ndim != 2 or q.shape[1] != self.d:
            raise ValueError(f"query dimension {q.shape[-1]} != index dimension {self.d}")
        nq, k = q.shape[0], int(k)
        if out is None:
            D = np.empty((nq, max(k, 0)), dtype=np.float32)
            I = np.empty((nq, max(k, 0)), dtype=np.int64)
        else:
            D, I = out
            if (D.dtype != np.float32 or I.dtype != np.int64 or D.shape != (nq, k) or I.shape != (nq, k)
                    or not D.flags.c_contiguous or not I.flags.c_contiguous):
                raise ValueError("out must be C-contiguous (float32[nq, k], int64[nq, k])")
        check(lib().mvdb_index_search_mmr(self._h, _ptr(q), nq, k, int(fetch_k), float(lambda_mult), int(bool(normalize_q)),
                                          rowset._h if rowset is not None else None, _ptr(D), _ptr(I)))
        return D, I

    def search_mmr_device(self, q_ptr, nq, k, fetch_k, lambda_mult, D_ptr, I_ptr, rowset=None, stream=0, normalize_q=False,
                          label_offset=0):
        """Device-pointer variant of search_mmr (labels: row numbers + label_offset); enqueues on `stream` and returns."""
        check(lib().mvdb_index_search_mmr_device(
            self._h, ctypes.c_void_p(q_ptr), int(nq), int(k), int(fetch_k), float(lambda_mult), int(bool(normalize_q)),
            rowset._h if rowset is not None else None, int(label_offset), ctypes.c_void_p(D_ptr), ctypes.c_void_p(I_ptr),
            ctypes.c_void_p(stream)))

    @staticmethod
    def mmr_form(d, fetch_k, device=0):
        """0: the selection holds the fetch_k candidate rows in LDS; 1: it streams them from the matrix at every step."""
        form = int(lib().mvdb_mmr_form(int(d), int(fetch_k), int(device)))
        if form < 0:
            check(-form)
        return form

    # ---- distinct search: the best row of each group, the k best groups (include/mvdb.h "DISTINCT SEARCH") ----------
    def grouping(self, codes, n_groups):
        """A resident Grouping: one int32 group code in [0, n_groups) per stored row."""
        return Grouping(self, codes, n_groups)

    def search_distinct(self, q, k, fetch_k, grouping, rowset=None, normalize_q=False):
        """(D float32[nq, k], I int64[nq, k], G int32[nq, k]): per query the best row of each of the k best groups (of the row
        set, if one is given), best group first; exact whatever fetch_k is (a query whose fetch_k candidates hold fewer than k
        groups is answered by one pass over the selected rows).  Labels are ROW NUMBERS, G their group codes; a short row ends
        in -1 / -FLT_MAX / -1."""
        q = np.ascontiguousarray(np.atleast_2d(np.asarray(q, dtype=np.float32)))
        if q.ndim != 2 or q.shape[1] != self.d:
            raise ValueError(f"query dimension {q.shape[-1]} != index dimension {self.d}")
        nq, k = q.shape[0], int(k)
        D = np.empty((nq, max(k, 0)), dtype=np.float32)
        I = np.empty((nq, max(k, 0)), dtype=np.int64)
        G = np.empty((nq, max(k, 0)), dtype=np.int32)
        check(lib().mvdb_index_search_distinct(self._h, _ptr(q), nq, k, int(fetch_k), int(bool(normalize_q)), grouping._h,
                                               rowset._h if rowset is not None else None, _ptr(D), _ptr(I), _ptr(G)))
        return D, I, G

    def search_distinct_device(self, q_ptr, nq, k, fetch_k, grouping, D_ptr, I_ptr, G_ptr=0, rowset=None, stream=0,
                               normalize_q=False, label_offset=0):
        """Device-pointer variant of search_distinct (labels: row numbers + label_offset; G_ptr 0: no group codes); enqueues on
        `stream` and returns."""
        check(lib().mvdb_index_search_distinct_device(
            self._h, ctypes.c_void_p(q_ptr), int(nq), int(k), int(fetch_k), int(bool(normalize_q)), grouping._h,
            rowset._h if rowset is not None else None, ctypes.c_void_p(D_ptr), ctypes.c_void_p(I_ptr),
            ctypes.c_void_p(G_ptr) if G_ptr else None, int(label_offset), ctypes.c_void_p(stream)))

    def distinct_counters(self):
        """(distinct searches served, queries their one-pass tier answered): running totals, read without synchronising."""
        v = [ctypes.c_longlong(0) for _ in range(2)]
        check(lib().mvdb_index_distinct_counters(self._h, *[ctypes.byref(x) for x in v]))
        return tuple(int(x.value) for x in v)

    # ---- group hits search: the k best groups, each with its group_size best rows (include/mvdb.h "GROUP HITS SEARCH") ----
    def search_groups(self, q, k, group_size, fetch_k, grouping, rowset=None, normalize_q=False):
        """(D float32[nq, k, group_size], I int64[nq, k, group_size], G int32[nq, k]): per query the k best groups (of the row
        set, if one is given) — G, exactly search_distinct's — and of each its group_size best rows, best first.  Labels are
        ROW NUMBERS; a group with fewer rows ends in -FLT_MAX / -1, a missing group (G == -1) is all of that."""
        q = np.ascontiguousarray(np.atleast_2d(np.asarray(q, dtype=np.float32)))
        if q.ndim != 2 or q.shape[1] != self.d:
            raise ValueError(f"query dimension {q.shape[-1]} != index dimension {self.d}")
        nq, k, group_size = q.shape[0], int(k), int(group_size)
        D = np.empty((nq, max(k, 0), max(group_size, 0)), dtype=np.float32)
        I = np.empty((nq, max(k, 0), max(group_size, 0)), dtype=np.int64)
        G = np.empty((nq, max(k, 0)), dtype=np.int32)
        check(lib().mvdb_index_search_groups(self._h, _ptr(q), nq, k, group_size, int(fetch_k), int(bool(normalize_q)), grouping._h,
                                             rowset._h if rowset is not None else None, _ptr(D), _ptr(I), _ptr(G)))
        return D, I, G

    def search_groups_device(self, q_ptr, nq, k, group_size, fetch_k, grouping, D_ptr, I_ptr, G_ptr=0, rowset=None, stream=0,
                             normalize_q=False, label_offset=0):
        """Device-pointer variant of search_groups (labels: row numbers + label_offset; G_ptr 0: no group codes); enqueues on
        `stream` and returns."""
        check(lib().mvdb_index_search_groups_device(
            self._h, ctypes.c_void_p(q_ptr), int(nq), int(k), int(group_size), int(fetch_k), int(bool(normalize_q)), grouping._h,
            rowset._h if rowset is not None else None, ctypes.c_void_p(D_ptr), ctypes.c_void_p(I_ptr),
            ctypes.c_void_p(G_ptr) if G_ptr else None, int(label_offset), ctypes.c_void_p(stream)))

    def groups_counters(self):
        """(group hits searches served, selected rows whose group was one of their query's k): running totals, read without
        synchronising."""
        v = [ctypes.c_longlong(0) for _ in range(2)]
        check(lib().mvdb_index_groups_counters(self._h, *[ctypes.byref(x) for x in v]))
        return tuple(int(x.value) for x in v)

    # ---- MaxSim search: one question of T vectors, a group scores the sum of its per-vector maxima (include/mvdb.h "MAXSIM SEARCH") ----
    def search_maxsim(self, q, k, grouping, rowset=None, normalize_q=False, with_tokens=True):
        """(D float32[k], G int32[k], I_tok int64[k, T], D_tok float32[k, T]) for ONE question q[T, d]: the k groups with the
        largest sum over the T vectors of the group's best row for each vector, best first (equal sums: the lower code);
        I_tok[j, t] is the row of group G[j] that answered vector t and D_tok[j, t] its score (both None without
        with_tokens).  Fewer than k groups end in -FLT_MAX / -1 / -1 / -FLT_MAX."""
        q = np.ascontiguousarray(np.asarray(q, dtype=np.float32))
        if q.ndim != 2 or q.shape[1] != self.d:
            raise ValueError(f"a MaxSim question is a [T, {self.d}] array (got shape {q.shape})")
        T, k = q.shape[0], int(k)
        D = np.empty(max(k, 0), dtype=np.float32)
        G = np.empty(max(k, 0), dtype=np.int32)
        I_tok = np.empty((max(k, 0), T), dtype=np.int64) if with_tokens else None
        D_tok = np.empty((max(k, 0), T), dtype=np.float32) if with_tokens else None
        check(lib().mvdb_index_search_maxsim(self._h, _ptr(q), T, k, int(bool(normalize_q)), grouping._h,
                                             rowset._h if rowset is not None else None, _ptr(D), _ptr(G),
                                             _ptr(I_tok) if with_tokens else None, _ptr(D_tok) if with_tokens else None))
        return D, G, I_tok, D_tok

    def search_maxsim_device(self, q_ptr, T, k, grouping, D_ptr, G_ptr, I_tok_ptr=0, D_tok_ptr=0, rowset=None, stream=0,
                             normalize_q=False, label_offset=0):
        """Device-pointer variant of search_maxsim (I_tok: row numbers + label_offset; a 0 pointer: that output is not
        written); enqueues on `stream` and returns."""
        check(lib().mvdb_index_search_maxsim_device(
            self._h, ctypes.c_void_p(q_ptr), int(T), int(k), int(bool(normalize_q)), grouping._h,
            rowset._h if rowset is not None else None, ctypes.c_void_p(D_ptr), ctypes.c_void_p(G_ptr),
            ctypes.c_void_p(I_tok_ptr) if I_tok_ptr else None, ctypes.c_void_p(D_tok_ptr) if D_tok_ptr else None,
            int(label_offset), ctypes.c_void_p(stream)))

    def maxsim_counters(self):
        """(MaxSim searches served, corpus passes they enqueued): running totals counted on the host."""
        v = [ctypes.c_longlong(0) for _ in range(2)]
        check(lib().mvdb_index_maxsim_counters(self._h, *[ctypes.byref(x) for x in v]))
        return tuple(int(x.value) for x in v)

    # ---- assignment and k-means: every stored row labelled by the nearest of C vectors (include/mvdb.h "ASSIGN AND K-MEANS") ----
    def _centres(self, c):
        c = np.ascontiguousarray(np.asarray(c, dtype=np.float32))
        if c.ndim != 2 or c.shape[1] != self.d:
            raise ValueError(f"the vectors to assign to are a [C, {self.d}] array (got shape {c.shape})")
        return c

    def assign(self, c, rowset=None, normalize_c=False, with_scores=True):
        """(labels int32[ntotal], scores float32[ntotal]) for the vectors c[C, d]: per PHYSICAL row the vector with the largest
        inner product (equal scores: the lower vector) and that score; a row outside `rowset`, or whose every score is NaN,
        gets -1 / -FLT_MAX.  scores is None without with_scores."""
        c = self._centres(c)
        n = self.ntotal
        labels = np.empty(n, dtype=np.int32)
        scores = np.empty(n, dtype=np.float32) if with_scores else None
        check(lib().mvdb_index_assign(self._h, _ptr(c), c.shape[0], int(bool(normalize_c)), rowset._h if rowset is not None else None,
                                      _ptr(labels), _ptr(scores) if with_scores else None))
        return labels, scores

    def assign_device(self, c_ptr, C, labels_ptr, scores_ptr=0, rowset=None, stream=0, normalize_c=False):
        """Device-pointer variant of assign (a 0 scores pointer: not written); enqueues on `stream` and returns."""
        check(lib().mvdb_index_assign_device(
            self._h, ctypes.c_void_p(c_ptr), int(C), int(bool(normalize_c)), rowset._h if rowset is not None else None,
            ctypes.c_void_p(labels_ptr), ctypes.c_void_p(scores_ptr) if scores_ptr else None, ctypes.c_void_p(stream)))

    def kmeans(self, centres, max_iter=25, rowset=None):
        """Spherical k-means from the initial `centres` [C, d]: (centres float32[C, d], labels int32[ntotal], scores
        float32[ntotal], counts int64[C], iterations).  labels / scores are assign(returned centres); counts the members
        under them; iterations the updates performed.  Bit-identical run to run."""
        centres = self._centres(centres).copy()
        n = self.ntotal
        labels = np.empty(n, dtype=np.int32)
        scores = np.empty(n, dtype=np.float32)
        counts = np.zeros(centres.shape[0], dtype=np.int64)
        iterations = ctypes.c_int(0)
        check(lib().mvdb_index_kmeans(self._h, _ptr(centres), centres.shape[0], int(max_iter), rowset._h if rowset is not None else None,
                                      _ptr(labels), _ptr(scores), _ptr(counts), ctypes.byref(iterations)))
        return centres, labels, scores, counts, int(iterations.value)

    def assign_counters(self):
        """(assignments served — those of k-means included —, corpus passes they enqueued): running totals counted on the host."""
        v = [ctypes.c_longlong(0) for _ in range(2)]
        check(lib().mvdb_index_assign_counters(self._h, *[ctypes.byref(x) for x in v]))
        return tuple(int(x.value) for x in v)

    # ---- search by examples: rows like the positives, unlike the negatives (include/mvdb.h "SEARCH BY EXAMPLES") ----
    def search_examples(self, positives, negatives, k, rowset=None, skip_rows=None, normalize=False):
        """(D float32[k], I int64[k]) for the positives [P, d] and the negatives [N, d] (None or empty: none): the k rows with
        the largest S = bp if bp > bn else -(bn * bn), bp / bn the row's best score against a positive / a negative, best first
        (equal S: the lower row).  `skip_rows` are never results.  Fewer than k rows end in -FLT_MAX / -1."""
        p = np.ascontiguousarray(np.asarray(positives, dtype=np.float32))
        if p.ndim != 2 or p.shape[1] != self.d:
            raise ValueError(f"the positives are a [P, {self.d}] array (got shape {p.shape})")
        v, N = p, 0
        if negatives is not None and len(negatives):
            m = np.ascontiguousarray(np.asarray(negatives, dtype=np.float32))
            if m.ndim != 2 or m.shape[1] != self.d:
                raise ValueError(f"the negatives are a [N, {self.d}] array (got shape {m.shape})")
            v, N = np.ascontiguousarray(np.concatenate([p, m])), m.shape[0]
        skip = np.ascontiguousarray(np.asarray(skip_rows if skip_rows is not None else [], dtype=np.int64)).reshape(-1)
        k = int(k)
        D = np.empty(max(k, 0), dtype=np.float32)
        I = np.empty(max(k, 0), dtype=np.int64)
        check(lib().mvdb_index_search_examples(self._h, _ptr(v), p.shape[0], N, k, int(bool(normalize)),
                                               rowset._h if rowset is not None else None, _ptr(skip) if len(skip) else None, len(skip),
                                               _ptr(D), _ptr(I)))
        return D, I

    def search_examples_device(self, v_ptr, P, N, k, D_ptr, I_ptr, rowset=None, skip_rows_ptr=0, n_skip=0, stream=0, normalize=False,
                               label_offset=0):
        """Device-pointer variant of search_examples (v: the positives, then the negatives; I: row numbers + label_offset; skip
        rows outside [0, ntotal) are ignored); enqueues on `stream` and returns."""
        check(lib().mvdb_index_search_examples_device(
            self._h, ctypes.c_void_p(v_ptr), int(P), int(N), int(k), int(bool(normalize)), rowset._h if rowset is not None else None,
            ctypes.c_void_p(skip_rows_ptr) if skip_rows_ptr else None, int(n_skip), int(label_offset), ctypes.c_void_p(D_ptr),
            ctypes.c_void_p(I_ptr), ctypes.c_void_p(stream)))

    def examples_counters(self):
        """(searches by examples served, corpus passes they enqueued): running totals counted on the host."""
        v = [ctypes.c_longlong(0) for _ in range(2)]
        check(lib().mvdb_index_examples_counters(self._h, *[ctypes.byref(x) for x in v]))
        return tuple(int(x.value) for x in v)

    # ---- boosted search: S = w_s * s + T[row], T from resident term columns and sparse entries (include/mvdb.h "BOOSTED SEARCH") ----
    def rowterm(self, values):
        """A resident RowTerm: one float32 value per stored row."""
        return RowTerm(self, values)

    @staticmethod
    def _boost_args(terms, weights, sparse_rows, sparse_values):
        """The term, weight and sparse arguments as ctypes values; the first element keeps the arrays alive."""
        terms = list(terms or ())
        w = np.ascontiguousarray(np.asarray(weights if weights is not None else [], dtype=np.float32)).reshape(-1)
        if len(w) != len(terms):
            raise ValueError(f"{len(terms)} terms, {len(w)} weights")
        handles = (ctypes.c_void_p * max(len(terms), 1))(*[t._h for t in terms])
        rows = np.ascontiguousarray(np.asarray(sparse_rows if sparse_rows is not None else [], dtype=np.int64)).reshape(-1)
        vals = np.ascontiguousarray(np.asarray(sparse_values if sparse_values is not None else [], dtype=np.float32)).reshape(-1)
        if len(rows) != len(vals):
            raise ValueError(f"{len(rows)} sparse rows, {len(vals)} sparse values")
        keep = (terms, w, handles, rows, vals)
        return keep, (handles if terms else None, _ptr(w) if terms else None, len(terms), _ptr(rows) if len(rows) else None,
                      _ptr(vals) if len(rows) else None, len(rows))

    def search_boosted(self, q, k, terms, weights, score_weight=1.0, sparse_rows=None, sparse_values=None, rowset=None, normalize_q=False):
        """(D float32[nq, k], I int64[nq, k]): the k rows with the largest S = score_weight * s + T[row], best first (equal S:
        the lower physical row), T the weighted sum of the `terms` (RowTerm objects, at most four, chained in the order given)
        plus — single query only — `sparse_values` on the distinct `sparse_rows`.  Fewer than k rows end in -FLT_MAX / -1."""
        q = np.ascontiguousarray(np.atleast_2d(np.asarray(q, dtype=np.float32)))
        if q.ndim != 2 or q.shape[1] != self.d:
            raise ValueError(f"query dimension {q.shape[-1]} != index dimension {self.d}")
        nq, k = q.shape[0], int(k)
        keep, args = self._boost_args(terms, weights, sparse_rows, sparse_values)
        D = np.empty((nq, max(k, 0)), dtype=np.float32)
        I = np.empty((nq, max(k, 0)), dtype=np.int64)
        check(lib().mvdb_index_search_boosted(self._h, _ptr(q), nq, k, int(bool(normalize_q)), ctypes.c_float(score_weight), *args,
                                              rowset._h if rowset is not None else None, _ptr(D), _ptr(I)))
        return D, I

    def search_boosted_device(self, q_ptr, nq, k, terms, weights, D_ptr, I_ptr, score_weight=1.0, sparse_rows=None, sparse_values=None,
                              rowset=None, stream=0, normalize_q=False, label_offset=0):
        """Device-pointer variant of search_boosted (I: row numbers + label_offset; the sparse entries stay host arrays);
        enqueues on `stream` and returns — without waiting for anything when there are no sparse entries."""
        keep, args = self._boost_args(terms, weights, sparse_rows, sparse_values)
        check(lib().mvdb_index_search_boosted_device(
            self._h, ctypes.c_void_p(q_ptr), int(nq), int(k), int(bool(normalize_q)), ctypes.c_float(score_weight), *args,
            rowset._h if rowset is not None else None, int(label_offset), ctypes.c_void_p(D_ptr), ctypes.c_void_p(I_ptr),
            ctypes.c_void_p(stream)))

    def boost_combine(self, terms, weights, sparse_rows=None, sparse_values=None):
        """float32[ntotal]: the combined column T of a boosted search with these arguments, computed on the device by the
        combine launches alone."""
        keep, args = self._boost_args(terms, weights, sparse_rows, sparse_values)
        T = np.empty(self.ntotal, dtype=np.float32)
        check(lib().mvdb_index_boost_combine(self._h, *args, _ptr(T)))
        return T

    def boost_counters(self):
        """(boosted searches served, boost_scan_kernel launches enqueued): running totals counted on the host."""
        v = [ctypes.c_longlong(0) for _ in range(2)]
        check(lib().mvdb_index_boost_counters(self._h, *[ctypes.byref(x) for x in v]))
        return tuple(int(x.value) for x in v)

    # ---- sparse vectors and hybrid search (include/mvdb.h "SPARSE VECTORS AND HYBRID SEARCH") ----
    def sparse(self, indptr, indices, values, dim):
        """A resident SparseStore: one sparse vector per stored row, CSR."""
        return SparseStore(self, indptr, indices, values, dim)

    @staticmethod
    def _sparse_queries(queries):
        """[(indices, values), ...] as the CSR arrays of a call: (indptr int64[nq + 1], indices int32, values float32)."""
        indptr, idx, val = [0], [], []
        for qi, qv in queries:
            qi = np.asarray(qi).reshape(-1)
            if qi.size and (qi.min() < -2**31 or qi.max() >= 2**31):
                raise ValueError(f"sparse query: index {int(qi.max() if qi.max() >= 2**31 else qi.min())} does not fit 32 bits")
            qv = np.asarray(qv, dtype=np.float32).reshape(-1)
            if len(qi) != len(qv):
                raise ValueError(f"{len(qi)} sparse query indices, {len(qv)} values")
            idx.append(qi.astype(np.int32))
            val.append(qv)
            indptr.append(indptr[-1] + len(qi))
        return (np.asarray(indptr, dtype=np.int64), np.ascontiguousarray(np.concatenate(idx) if idx else np.empty(0, np.int32), dtype=np.int32),
                np.ascontiguousarray(np.concatenate(val) if val else np.empty(0, np.float32), dtype=np.float32))

    def sparse_scores(self, store, q_indices, q_values, with_matched=True):
        """(T float32[ntotal], matched int32[ntotal]): the sparse score of every stored row against one query and the number
        of its entries the query holds, computed by the scoring launch alone."""
        indptr, qi, qv = self._sparse_queries([(q_indices, q_values)])
        T = np.empty(self.ntotal, dtype=np.float32)
        matched = np.empty(self.ntotal, dtype=np.int32) if with_matched else None
        check(lib().mvdb_index_sparse_scores(self._h, store._h, _ptr(qi), _ptr(qv), len(qi), _ptr(T), _ptr(matched) if with_matched else None))
        return (T, matched) if with_matched else T

    def search_sparse(self, store, queries, k, rowset=None):
        """(D float32[nq, k], I int64[nq, k]): per sparse query (indices, values) the k selected rows with the largest sparse
        score among those that share an index with it, best first (equal scores: the lower row); fewer end in -FLT_MAX / -1."""
        indptr, qi, qv = self._sparse_queries(queries)
        nq, k = len(indptr) - 1, int(k)
        D = np.empty((nq, max(k, 0)), dtype=np.float32)
        I = np.empty((nq, max(k, 0)), dtype=np.int64)
        check(lib().mvdb_index_search_sparse(self._h, store._h, _ptr(indptr), _ptr(qi), _ptr(qv), nq, k, rowset._h if rowset is not None else None,
                                             _ptr(D), _ptr(I)))
        return D, I

    def search_sparse_device(self, store, queries, k, D_ptr, I_ptr, rowset=None, stream=0, label_offset=0):
        """Device-pointer variant of search_sparse (I: row numbers + label_offset; the queries stay host arrays)."""
        indptr, qi, qv = self._sparse_queries(queries)
        check(lib().mvdb_index_search_sparse_device(self._h, store._h, _ptr(indptr), _ptr(qi), _ptr(qv), len(indptr) - 1, int(k),
                                                    rowset._h if rowset is not None else None, int(label_offset), ctypes.c_void_p(D_ptr),
                                                    ctypes.c_void_p(I_ptr), ctypes.c_void_p(stream)))

    def search_hybrid(self, store, q, queries, k, dense_weight=1.0, sparse_weight=1.0, rowset=None, normalize_q=False):
        """(D float32[nq, k], I int64[nq, k]): the k selected rows with the largest S = dense_weight * s + sparse_weight *
        sparse, query i being the dense q[i] with the sparse queries[i]; exact over every selected row."""
        q = np.ascontiguousarray(np.atleast_2d(np.asarray(q, dtype=np.float32)))
        if q.ndim != 2 or q.shape[1] != self.d:
            raise ValueError(f"query dimension {q.shape[-1]} != index dimension {self.d}")
        indptr, qi, qv = self._sparse_queries(queries)
        nq, k = q.shape[0], int(k)
        if len(indptr) - 1 != nq:
            raise ValueError(f"{nq} dense queries, {len(indptr) - 1} sparse queries")
        D = np.empty((nq, max(k, 0)), dtype=np.float32)
        I = np.empty((nq, max(k, 0)), dtype=np.int64)
        check(lib().mvdb_index_search_hybrid(self._h, store._h, _ptr(q), int(bool(normalize_q)), _ptr(indptr), _ptr(qi), _ptr(qv), nq, k,
                                             ctypes.c_float(dense_weight), ctypes.c_float(sparse_weight), rowset._h if rowset is not None else None,
                                             _ptr(D), _ptr(I)))
        return D, I

    def search_hybrid_device(self, store, q_ptr, queries, k, D_ptr, I_ptr, dense_weight=1.0, sparse_weight=1.0, rowset=None, stream=0,
                             normalize_q=False, label_offset=0):
        """Device-pointer variant of search_hybrid (the sparse queries stay host arrays)."""
        indptr, qi, qv = self._sparse_queries(queries)
        check(lib().mvdb_index_search_hybrid_device(
            self._h, store._h, ctypes.c_void_p(q_ptr), int(bool(normalize_q)), _ptr(indptr), _ptr(qi), _ptr(qv), len(indptr) - 1, int(k),
            ctypes.c_float(dense_weight), ctypes.c_float(sparse_weight), rowset._h if rowset is not None else None, int(label_offset),
            ctypes.c_void_p(D_ptr), ctypes.c_void_p(I_ptr), ctypes.c_void_p(stream)))

    def sparse_counters(self):
        """(sparse and hybrid searches served, sparse_scan_kernel launches enqueued): running totals counted on the host."""
        v = [ctypes.c_longlong(0) for _ in range(2)]
        check(lib().mvdb_index_sparse_counters(self._h, *[ctypes.byref(x) for x in v]))
        return tuple(int(x.value) for x in v)

    def sparse_postings_counters(self):
        """(searches served through the postings, sparse_postings_kernel launches enqueued, list entries of the terms of the
        queries staged for them): running totals counted on the host."""
        v = [ctypes.c_longlong(0) for _ in range(3)]
        check(lib().mvdb_index_sparse_postings_counters(self._h, *[ctypes.byref(x) for x in v]))
        return tuple(int(x.value) for x in v)

    # ---- probed search: a k-means partition, a query scans the lists of its nprobe best centres (include/mvdb.h "PROBED SEARCH") ----
    def partition(self, centres, labels=None, normalize_c=False):
        """A resident Partition of the stored rows into len(centres) member lists.  labels None: every row is labelled on the
        device by its nearest centre (what assign(centres, normalize_c=...) returns); else one int32 label in [-1, C) per
        stored row, used as given (-1: the row is in no list)."""
        return Partition(self, centres, labels, normalize_c)

    def search_probe(self, q, k, nprobe, partition, rowset=None, normalize_q=False):
        """(D float32[nq, k], I int64[nq, k]): per query the k best rows of the member lists of its nprobe best centres (of the
        bitmap-form row set, if one is given).  APPROXIMATE in the choice of lists only: given the lists the answer is exact,
        in the single-query scan's bits, ties to the lower row; nprobe = number of lists is the exact search over every
        labelled row.  A short row ends in -1 / -FLT_MAX."""
        q = np.ascontiguousarray(np.atleast_2d(np.asarray(q, dtype=np.float32)))
        if q.ndim != 2 or q.shape[1] != self.d:
            raise ValueError(f"query dimension {q.shape[-1]} != index dimension {self.d}")
        nq, k = q.shape[0], int(k)
        D = np.empty((nq, max(k, 0)), dtype=np.float32)
        I = np.empty((nq, max(k, 0)), dtype=np.int64)
        check(lib().mvdb_index_search_probe(self._h, partition._h, _ptr(q), nq, k, int(nprobe), int(bool(normalize_q)),
                                            rowset._h if rowset is not None else None, _ptr(D), _ptr(I)))
        return D, I

    def search_probe_device(self, q_ptr, nq, k, nprobe, partition, D_ptr, I_ptr, rowset=None, stream=0, normalize_q=False,
                            label_offset=0):
        """Device-pointer variant of search_probe (labels: row numbers + label_offset); enqueues on `stream` and returns."""
        check(lib().mvdb_index_search_probe_device(
            self._h, partition._h, ctypes.c_void_p(q_ptr), int(nq), int(k), int(nprobe), int(bool(normalize_q)),
            rowset._h if rowset is not None else None, int(label_offset), ctypes.c_void_p(D_ptr), ctypes.c_void_p(I_ptr),
            ctypes.c_void_p(stream)))

    def probe_counters(self):
        """(probed searches served, launches they enqueued): running totals counted on the host."""
        v = [ctypes.c_longlong(0) for _ in range(2)]
        check(lib().mvdb_index_probe_counters(self._h, *[ctypes.byref(x) for x in v]))
        return tuple(int(x.value) for x in v)


class Partition:
    """mvdb_partition*: centres, one int32 label per stored row and the member lists, resident on the index's device.  A search
    refuses it once the index has gained or lost a row; update() follows adds and in-place updates, a removal needs a new
    partition (from labels() with the removed rows dropped: no k-means, no re-assign)."""

    def __init__(self, index, centres, labels=None, normalize_c=False):
        centres = index._centres(centres)
        if labels is not None:
            labels = np.ascontiguousarray(labels, dtype=np.int32)
            if labels.ndim != 1 or labels.shape[0] != index.ntotal:
                raise ValueError(f"a partition needs one label per stored row ({labels.shape} labels, {index.ntotal} rows)")
        self._index = index
        self.d = index.d
        self._h = ctypes.c_void_p()
        check(lib().mvdb_partition_create(index._h, _ptr(centres), centres.shape[0], int(bool(normalize_c)),
                                          _ptr(labels) if labels is not None else None, ctypes.byref(self._h)))

    def update(self, changed_rows=None):
        """Label the rows added since, and the listed rows, by their nearest centre and rebuild the lists."""
        rows = np.ascontiguousarray(changed_rows if changed_rows is not None else [], dtype=np.int64).reshape(-1)
        check(lib().mvdb_partition_update(self._h, self._index._h, _ptr(rows) if rows.size else None, rows.shape[0]))

    def __len__(self):
        return int(lib().mvdb_partition_rows(self._h))

    @property
    def n_lists(self):
        return int(lib().mvdb_partition_lists(self._h))

    def labels(self, row0=0, n=None):
        """int32[n]: the labels of rows [row0, row0 + n) (n None: to the last row the partition covers)."""
        n = len(self) - int(row0) if n is None else int(n)
        out = np.empty(max(n, 0), dtype=np.int32)
        check(lib().mvdb_partition_labels(self._h, int(row0), n, _ptr(out)))
        return out

    def centres(self):
        """float32[C, d]: the centres as stored (after their normalisation)."""
        out = np.empty((self.n_lists, self.d), dtype=np.float32)
        check(lib().mvdb_partition_centres(self._h, _ptr(out)))
        return out

    def sizes(self):
        """int64[C]: rows per list."""
        out = np.zeros(self.n_lists, dtype=np.int64)
        check(lib().mvdb_partition_sizes(self._h, _ptr(out)))
        return out

    def free(self):
        if getattr(self, "_h", None) is not None and self._h:
            lib().mvdb_partition_free(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Grouping:
    """mvdb_grouping*: one int32 group code per stored row, resident on the index's device.  Valid until the index it was
    built on gains or loses a row (updating rows in place keeps it valid)."""

    def __init__(self, index, codes, n_groups):
        codes = np.ascontiguousarray(codes, dtype=np.int32)
        if codes.ndim != 1:
            raise ValueError("codes must be one-dimensional")
        self._h = ctypes.c_void_p()
        check(lib().mvdb_grouping_create(index._h, _ptr(codes), codes.shape[0], int(n_groups), ctypes.byref(self._h)))

    def __len__(self):
        return int(lib().mvdb_grouping_rows(self._h))

    @property
    def n_groups(self):
        return int(lib().mvdb_grouping_groups(self._h))

    def free(self):
        if getattr(self, "_h", None) is not None and self._h:
            lib().mvdb_grouping_free(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class RowTerm:
    """mvdb_rowterm*: one float32 value per stored row, resident on the index's device — a term of a boosted search.  Valid
    until the index it was built on gains or loses a row (updating rows in place keeps it valid); its device memory goes with
    the last reference."""

    def __init__(self, index, values):
        values = np.ascontiguousarray(values, dtype=np.float32)
        if values.ndim != 1:
            raise ValueError("values must be one-dimensional")
        self._h = ctypes.c_void_p()
        check(lib().mvdb_rowterm_create(index._h, _ptr(values), values.shape[0], ctypes.byref(self._h)))

    def __len__(self):
        return int(lib().mvdb_rowterm_rows(self._h))

    def free(self):
        if getattr(self, "_h", None) is not None and self._h:
            lib().mvdb_rowterm_free(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def sparse_geometry():
    """(span_entries, tile_rows, table_slots) of the sparse scan of this build (mvdb_sparse_geometry)."""
    v = [ctypes.c_int(0) for _ in range(3)]
    check(lib().mvdb_sparse_geometry(*[ctypes.byref(x) for x in v]))
    return tuple(int(x.value) for x in v)


def sparse_postings_geometry():
    """(block_rows, sort_lds_entries, max_dim) of the sparse postings of this build (mvdb_sparse_postings_geometry)."""
    b, l, m = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_longlong(0)
    check(lib().mvdb_sparse_postings_geometry(ctypes.byref(b), ctypes.byref(l), ctypes.byref(m)))
    return int(b.value), int(l.value), int(m.value)


class SparseStore:
    """mvdb_sparse*: one sparse vector per stored row in CSR form, resident on the index's device.  Valid until the index it
    was built on gains or loses a row (updating rows in place keeps it valid); its device memory goes with the last
    reference."""

    def __init__(self, index, indptr, indices, values, dim):
        indptr = np.ascontiguousarray(indptr, dtype=np.int64).reshape(-1)
        indices = np.ascontiguousarray(indices, dtype=np.int32).reshape(-1)
        values = np.ascontiguousarray(values, dtype=np.float32).reshape(-1)
        if len(indptr) < 1:
            raise ValueError("indptr must hold n + 1 offsets")
        if len(indices) != len(values):
            raise ValueError(f"{len(indices)} indices, {len(values)} values")
        if len(indptr) > 1 and int(indptr[-1]) > len(indices):
            raise ValueError(f"indptr ends at {int(indptr[-1])}, beyond the {len(indices)} entries")
        self._h = ctypes.c_void_p()
        self._index = index
        check(lib().mvdb_sparse_create(index._h, _ptr(indptr), _ptr(indices), _ptr(values), len(indptr) - 1, int(dim), ctypes.byref(self._h)))

    def __len__(self):
        return int(lib().mvdb_sparse_rows(self._h))

    @property
    def nnz(self):
        return int(lib().mvdb_sparse_nnz(self._h))

    @property
    def dim(self):
        return int(lib().mvdb_sparse_dim(self._h))

    # ---- the inverted form (include/mvdb.h "SPARSE POSTINGS") ----
    def build_postings(self):
        """Build the posting lists beside the CSR form, on the device: searches on an index whose option sparse_postings is 1
        (the default) then score this store through them — the same bits, read from the lists of the query's terms only."""
        check(lib().mvdb_sparse_build_postings(self._index._h, self._h))

    def drop_postings(self):
        check(lib().mvdb_sparse_drop_postings(self._h))

    @property
    def has_postings(self):
        return bool(lib().mvdb_sparse_has_postings(self._h))

    def postings(self):
        """(post_ptr int64[dim + 1], rows uint32[nnz], values float32[nnz]): the layout, copied back."""
        post_ptr = np.empty(self.dim + 1, dtype=np.int64)
        rows = np.empty(self.nnz, dtype=np.uint32)
        values = np.empty(self.nnz, dtype=np.float32)
        check(lib().mvdb_sparse_postings_read(self._h, _ptr(post_ptr), _ptr(rows), _ptr(values)))
        return post_ptr, rows, values

    def free(self):
        if getattr(self, "_h", None) is not None and self._h:
            lib().mvdb_sparse_free(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class RowSet:
    """mvdb_rowset*: a filter's rows resident on the device (a bitmap for dense / excluded sets, a row list otherwise).
    Valid until the index it was built on loses a row or is reset; rows appended later are not part of it (include/mvdb.h)."""

    def __init__(self, index, rows, excluded=False):
        rows = np.ascontiguousarray(rows, dtype=np.int64)
        self._h = ctypes.c_void_p()
        check(lib().mvdb_rowset_create(index._h, _ptr(rows), rows.shape[0], int(bool(excluded)), ctypes.byref(self._h)))

    def __len__(self):
        return int(lib().mvdb_rowset_size(self._h))

    @property
    def is_bitmap(self):
        return bool(lib().mvdb_rowset_is_bitmap(self._h))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            lib().mvdb_rowset_free(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Cos8Index:
    """mvdb_cos8*: int8 codes of the rows on the device, exact int8 cosine search (include/mvdb.h "int8 cosine index").
    D holds distances, ascending; missing slots are label -1 / +FLT_MAX.  The method names follow FlatIndex so that the
    database layer drives either; `normalize` / `normalize_q` are accepted and ignored: the quantiser normalises."""

    def __init__(self, d, device=0):
        self._h = ctypes.c_void_p()
        self.d = int(d)
        self.device = device
        check(lib().mvdb_cos8_create(self.d, device, ctypes.byref(self._h)))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            lib().mvdb_cos8_free(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    @property
    def ntotal(self):
        return int(lib().mvdb_cos8_ntotal(self._h))

    def reset(self):
        check(lib().mvdb_cos8_reset(self._h))

    def reserve(self, n):
        check(lib().mvdb_cos8_reserve(self._h, int(n)))

    def _rows2d(self, x):
        x = np.ascontiguousarray(np.atleast_2d(np.asarray(x, dtype=np.float32)))
        if x.ndim != 2 or x.shape[1] != self.d:
            raise ValueError(f"expected [n,{self.d}] float32, got {x.shape}")
        return x

    def add(self, x, normalize=None):
        x = self._rows2d(x)
        check(lib().mvdb_cos8_add(self._h, _ptr(x), x.shape[0]))

    def add_device(self, ptr, n):
        check(lib().mvdb_cos8_add_device(self._h, ctypes.c_void_p(ptr), int(n)))

    def get_codes(self, row0, n):
        """(codes int8 [n, d], a2 int32 [n]) of rows [row0, row0 + n)."""
        codes = np.empty((int(n), self.d), dtype=np.int8)
        a2 = np.empty(int(n), dtype=np.int32)
        check(lib().mvdb_cos8_get_codes(self._h, int(row0), int(n), _ptr(codes), _ptr(a2)))
        return codes, a2

    def remove_rows(self, rows):
        rows = np.ascontiguousarray(rows, dtype=np.int64)
        check(lib().mvdb_cos8_remove_rows(self._h, _ptr(rows), rows.shape[0]))

    def set_rows(self, rows, x, normalize=None):
        """Overwrite the stored rows `rows` (distinct, each in [0, ntotal)) with the codes of x[len(rows), d], in place."""
        rows = np.ascontiguousarray(rows, dtype=np.int64)
        x = self._rows2d(x)
        if rows.ndim != 1 or x.shape[0] != rows.shape[0]:
            raise ValueError(f"expected [m] rows and [m,{self.d}] float32, got {rows.shape} and {x.shape}")
        check(lib().mvdb_cos8_set_rows(self._h, _ptr(rows), _ptr(x), rows.shape[0]))

    def set_rows_device(self, rows, x_ptr, m):
        rows = np.ascontiguousarray(rows, dtype=np.int64)
        if rows.ndim != 1 or rows.shape[0] != int(m):
            raise ValueError(f"expected {int(m)} row numbers, got {rows.shape}")
        check(lib().mvdb_cos8_set_rows_device(self._h, _ptr(rows), ctypes.c_void_p(x_ptr), int(m)))

    def _out(self, nq, k):
        return np.empty((nq, int(k)), dtype=np.float32), np.empty((nq, int(k)), dtype=np.int64)

    def search(self, q, k, normalize_q=None):
        q = self._rows2d(q)
        D, I = self._out(q.shape[0], k)
        check(lib().mvdb_cos8_search(self._h, _ptr(q), q.shape[0], int(k), _ptr(D), _ptr(I)))
        return D, I

    def search_device(self, q_ptr, nq, k, D_ptr, I_ptr, stream=0, label_offset=0):
        """All buffers are device pointers (ints); enqueues on `stream` and returns."""
        check(lib().mvdb_cos8_search_device(self._h, ctypes.c_void_p(q_ptr), int(nq), int(k), int(label_offset),
                                            ctypes.c_void_p(D_ptr), ctypes.c_void_p(I_ptr), ctypes.c_void_p(stream)))

    def rowset(self, rows, excluded=False):
        """The listed rows (or, excluded=True, every row BUT them) resident on the device: see Cos8RowSet."""
        return Cos8RowSet(self, rows, excluded)

    def search_rowset(self, q, k, rowset, normalize_q=None):
        """Search a resident Cos8RowSet; labels are ROW NUMBERS of the index."""
        q = self._rows2d(q)
        D, I = self._out(q.shape[0], k)
        check(lib().mvdb_cos8_search_rowset(self._h, _ptr(q), q.shape[0], int(k), rowset._h, _ptr(D), _ptr(I)))
        return D, I

    def search_rowset_device(self, q_ptr, nq, k, rowset, D_ptr, I_ptr, stream=0, label_offset=0):
        check(lib().mvdb_cos8_search_rowset_device(
            self._h, ctypes.c_void_p(q_ptr), int(nq), int(k), rowset._h, int(label_offset), ctypes.c_void_p(D_ptr),
            ctypes.c_void_p(I_ptr), ctypes.c_void_p(stream)))


class Cos8RowSet:
    """mvdb_cos8_rowset*: a filter's rows resident on the device (an exclusion bitmap or a sorted row list).  Valid until
    rows are removed from the index it was built on; rows appended later are not part of it."""

    def __init__(self, index, rows, excluded=False):
        rows = np.ascontiguousarray(rows, dtype=np.int64)
        self._h = ctypes.c_void_p()
        check(lib().mvdb_cos8_rowset_create(index._h, _ptr(rows), rows.shape[0], int(bool(excluded)),
                                            ctypes.byref(self._h)))

    def __len__(self):
        return int(lib().mvdb_cos8_rowset_size(self._h))

    @property
    def is_bitmap(self):
        return bool(lib().mvdb_cos8_rowset_is_bitmap(self._h))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            lib().mvdb_cos8_rowset_free(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Comm:
    """RCCL communicator owned by libmvdb.so (mvdb_comm*): one all-gather of packed top-k blocks per query batch."""

    def __init__(self, unique_id, rank, world, device=0):
        self._h = ctypes.c_void_p()
        buf = (ctypes.c_ubyte * 128).from_buffer_copy(bytes(unique_id))
        check(lib().mvdb_comm_create(ctypes.cast(buf, ctypes.c_void_p), int(rank), int(world), int(device),
                                     ctypes.byref(self._h)))
        self.rank, self.world = int(rank), int(world)

    @staticmethod
    def unique_id():
        buf = (ctypes.c_ubyte * 128)()
        check(lib().mvdb_comm_unique_id(ctypes.cast(buf, ctypes.c_void_p)))
        return bytes(buf)

    def allgather(self, local_ptr, gathered_ptr, nbytes_per_rank, stream=0):
        check(lib().mvdb_allgather_topk(self._h, ctypes.c_void_p(local_ptr), ctypes.c_void_p(gathered_ptr),
                                        int(nbytes_per_rank), ctypes.c_void_p(stream)))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            lib().mvdb_comm_free(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def normalize_l2(x, device=0):
    """In-place faiss.normalize_L2 equivalent on the GPU for a C-contiguous float32 [n,d] array."""
    if not (isinstance(x, np.ndarray) and x.dtype == np.float32 and x.flags["C_CONTIGUOUS"] and x.ndim == 2):
        raise ValueError("normalize_l2 needs a C-contiguous float32 [n,d] ndarray")
    check(lib().mvdb_normalize_l2(_ptr(x), x.shape[0], x.shape[1], device))
    return x


def prof_enable(on=True):
    """Profiling brackets on / off; off -> on forgets the symbols recorded so far (prof_symbol)."""
    check(lib().mvdb_prof_enable(int(bool(on))))


def pack_row_mask(n, rows=None, excluded=None):
    """uint64 words of the row bitmap search_masked takes: the listed `rows` set, or every row but `excluded`."""
    bits = np.zeros((n + 63) // 64 * 64, dtype=np.uint8)
    if rows is not None:
        bits[np.fromiter(rows, dtype=np.int64, count=len(rows)) if not isinstance(rows, np.ndarray) else rows] = 1
    else:
        bits[:n] = 1
        if excluded is not None and len(excluded):
            bits[np.fromiter(excluded, dtype=np.int64, count=len(excluded)) if not isinstance(excluded, np.ndarray)
                 else excluded] = 0
    return np.packbits(bits, bitorder="little").view(np.uint64)


def split_rerun_count():
    return int(lib().mvdb_split_rerun_count())


def rescue_tile_stats():
    """(tiles the rescue launches were handed, tiles they would have scanned without the tile flags) since the library was loaded."""
    a, b = ctypes.c_int64(0), ctypes.c_int64(0)
    check(lib().mvdb_rescue_tile_stats(ctypes.byref(a), ctypes.byref(b)))
    return int(a.value), int(b.value)


def half_eps(d):
    return float(lib().mvdb_half_eps(int(d)))


def half_max_queries(d):
    return int(lib().mvdb_half_max_queries(int(d)))


def encoder_splitk_planes(tokens, n, k, compute_units=256):
    """Planes a small batch's [tokens, n] = A [tokens, k] W^T GEMM of the encoder is split into over K (0: not split); the
    MVDB_GEMM_X3_SPLITK* switches are read at the call (an encoder reads them when it is created)."""
    return int(lib().mvdb_encoder_splitk_planes(int(tokens), int(n), int(k), int(compute_units)))


def encoder_gemm_tile_form(tokens, n, compute_units=256):
    """256 / 192: the 256-row tile form of the split-precision GEMM applies to `tokens` packed tokens; 0: it does not."""
    return int(lib().mvdb_encoder_gemm_tile_form(int(tokens), int(n), int(compute_units)))


def prof_symbol(name):
    """Kernel instantiation last launched under profiling label `name` ("" if none)."""
    buf = ctypes.create_string_buffer(256)
    check(lib().mvdb_prof_symbol(name.encode(), buf, 256))
    return buf.value.decode()


def prof_read(name):
    n = ctypes.c_int64(0)
    ms = ctypes.c_double(0.0)
    check(lib().mvdb_prof_read(name.encode(), ctypes.byref(n), ctypes.byref(ms)))
    return n.value, ms.value


PROF_LABEL_CAP = 8192   # include/mvdb.h: MVDB_PROF_LABEL_CAP, the unread pairs one label may hold


def prof_live_events():
    """Events the profiler's pool holds, in use or free (include/mvdb.h: the two rules that bound them)."""
    return int(lib().mvdb_prof_live_events())


def range_band(d, qnorm, row_norm_bound):
    """Bound of |fp16 nomination score - fp32 score of the exact scans| in the shared range pass (include/mvdb.h: mvdb_range_band)."""
    return float(lib().mvdb_range_band(int(d), float(qnorm), float(row_norm_bound)))


def code8_margin(d, qnorm, qstep, row_norm_bound):
    """(alpha, beta) of the int8 prefilter's margin alpha * r + beta (include/mvdb.h: mvdb_code8_margin)."""
    a, b = ctypes.c_float(0), ctypes.c_float(0)
    check(lib().mvdb_code8_margin(int(d), float(qnorm), float(qstep), float(row_norm_bound), ctypes.byref(a), ctypes.byref(b)))
    return float(a.value), float(b.value)


def code8_pack(codes):
    """The (high, low) planes of one row of int8 codes, as uint8 arrays of 3 d / 4 and d / 4 bytes (include/mvdb.h: mvdb_code8_pack)."""
    codes = np.ascontiguousarray(codes, dtype=np.int8)
    d = codes.shape[0]
    high = np.empty(d // 4 * 3, np.uint8)
    low = np.empty(d // 4, np.uint8)
    check(lib().mvdb_code8_pack(int(d), codes.ctypes.data, high.ctypes.data, low.ctypes.data))
    return high, low


def code8_unpack(high, low):
    """The int8 codes of one row from its two planes (include/mvdb.h: mvdb_code8_unpack)."""
    high = np.ascontiguousarray(high, dtype=np.uint8)
    low = np.ascontiguousarray(low, dtype=np.uint8)
    d = low.shape[0] * 4
    assert high.shape[0] == d // 4 * 3
    codes = np.empty(d, np.int8)
    check(lib().mvdb_code8_unpack(int(d), high.ctypes.data, low.ctypes.data, codes.ctypes.data))
    return codes


def code8_front_pack(codes):
    """The image of one row of int8 codes in the front plane, 5 d / 8 bytes (include/mvdb.h: mvdb_code8_front_pack)."""
    codes = np.ascontiguousarray(codes, dtype=np.int8)
    d = codes.shape[0]
    image = np.empty(max(d // 8 * 5, 1), np.uint8)
    check(lib().mvdb_code8_front_pack(int(d), codes.ctypes.data, image.ctypes.data))
    return image


def code8_front_unpack(image):
    """c & ~7 of the codes of one row, from its image in the front plane (include/mvdb.h: mvdb_code8_front_unpack)."""
    image = np.ascontiguousarray(image, dtype=np.uint8)
    d = image.shape[0] // 5 * 8
    codes = np.empty(max(d, 1), np.int8)
    check(lib().mvdb_code8_front_unpack(int(d), image.ctypes.data, codes.ctypes.data))
    return codes


def code8_bit2_pack(codes):
    """The d / 8 bytes of one row of int8 codes in the bit plane: bit 2 of every code (include/mvdb.h: mvdb_code8_bit2_pack)."""
    codes = np.ascontiguousarray(codes, dtype=np.int8)
    d = codes.shape[0]
    bits = np.empty(max(d // 8, 1), np.uint8)
    check(lib().mvdb_code8_bit2_pack(int(d), codes.ctypes.data, bits.ctypes.data))
    return bits


def code8_bit2_unpack(bits):
    """(c >> 2) & 1 of the codes of one row, from its bytes of the bit plane (include/mvdb.h: mvdb_code8_bit2_unpack)."""
    bits = np.ascontiguousarray(bits, dtype=np.uint8)
    d = bits.shape[0] * 8
    codes = np.empty(max(d, 1), np.int8)
    check(lib().mvdb_code8_bit2_unpack(int(d), bits.ctypes.data, codes.ctypes.data))
    return codes


def code8_front_geometry(d, n, device=0):
    """code8_scan_geometry for the form of the prefilter's launch that streams the front plane."""
    rb, waves = ctypes.c_int(0), ctypes.c_int(0)
    check(lib().mvdb_code8_front_geometry(int(d), int(n), int(device), ctypes.byref(rb), ctypes.byref(waves)))
    return int(rb.value), int(waves.value)


def code8_front_offset(d, row, chunk):
    """(wide, narrow): the byte offsets of the 16-byte and the 4-byte part of chunk `chunk` of stored row `row` in the front
    plane of an index of width d (include/mvdb.h: mvdb_code8_front_offset)."""
    wide, narrow = ctypes.c_int64(0), ctypes.c_int64(0)
    check(lib().mvdb_code8_front_offset(int(d), int(row), int(chunk), ctypes.byref(wide), ctypes.byref(narrow)))
    return int(wide.value), int(narrow.value)


def code8_scan_geometry(d, n, device=0):
    """(rows per batch, waves) of the prefilter's launch over n rows of width d: wave w takes batches w, w + waves, ...
    (include/mvdb.h: mvdb_code8_scan_geometry)."""
    rb, waves = ctypes.c_int(0), ctypes.c_int(0)
    check(lib().mvdb_code8_scan_geometry(int(d), int(n), int(device), ctypes.byref(rb), ctypes.byref(waves)))
    return int(rb.value), int(waves.value)
