"""ctypes binding of libmse_hip.so (include/mse.h).

This is the only way the Python host layer reaches the device: every compute entry point
below calls the C ABI.  There is NO CPU fallback -- if the shared library is missing or a call
fails, an exception is raised (MseError).
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# MSE_HIP_LIB: developer override (A/B builds of the same library); the default is the in-tree build
LIB_PATH = os.environ.get("MSE_HIP_LIB") or os.path.join(os.path.dirname(_HERE), "lib", "libmse_hip.so")


class MseError(RuntimeError):
    pass


_lib = None


class BuildConfig(C.Structure):
    """mse_build_config == IndexBuildConfig (diskann/src/lib.rs:42-52)."""
    _fields_ = [("r", C.c_uint64), ("l", C.c_uint64), ("maxc", C.c_uint64), ("alpha", C.c_int64), ("query_alpha", C.c_int64),
                ("saturate_graph", C.c_uint32), ("query_breakpoint", C.c_uint32), ("max_add_per_stitch_iter", C.c_uint64)]


u8p, u16p, u32p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint16), C.POINTER(C.c_uint32)
f32p, i64p = C.POINTER(C.c_float), C.POINTER(C.c_int64)
i32p = C.POINTER(C.c_int32)
sz, vp = C.c_size_t, C.c_void_p

# name -> (restype, argtypes); kept in one table so tests can check it against include/mse.h
SIGNATURES = {
    "mse_last_error": (C.c_char_p, []),
    "mse_device_count": (C.c_int, []),
    "mse_set_device": (C.c_int, [C.c_int]),
    "mse_device_synchronize": (C.c_int, []),
    "mse_device_mem_info": (C.c_int, [C.POINTER(sz), C.POINTER(sz)]),
    "mse_version": (C.c_char_p, []),
    "mse_queries_per_pass_max": (sz, [sz]),
    "mse_scale_dot_f32": (C.c_int64, [C.c_float]),
    "mse_scale_dot_f64": (C.c_int64, [C.c_double]),
    "mse_base_from_host": (vp, [u16p, sz, sz]),
    "mse_base_wrap_device": (vp, [vp, sz, sz]),
    "mse_base_generate": (vp, [C.c_uint32, C.c_uint64, sz, sz]),
    "mse_base_free": (None, [vp]),
    "mse_base_len": (sz, [vp]),
    "mse_base_dim": (sz, [vp]),
    "mse_base_device_ptr": (vp, [vp]),
    "mse_base_read_rows": (C.c_int, [vp, sz, sz, u16p]),
    "mse_fast_dot_f16": (C.c_int, [u16p, u16p, sz, i64p]),
    "mse_searcher_new": (vp, [vp]),
    "mse_searcher_free": (None, [vp]),
    "mse_searcher_set_stream": (C.c_int, [vp, vp]),
    "mse_searcher_stream": (vp, [vp]),
    "mse_bruteforce_topk_f16": (C.c_int, [vp, u16p, sz, sz, C.c_int, i64p, u32p]),
    "mse_bruteforce_topk_f16_dev": (C.c_int, [vp, vp, sz, sz, C.c_int, C.c_uint64, vp, vp]),
    "mse_bruteforce_scores_f16": (C.c_int, [vp, u16p, i64p]),
    "mse_filter_from_bits": (vp, [u8p, sz]),
    "mse_filter_from_ids": (vp, [u32p, sz, sz]),
    "mse_filter_free": (None, [vp]),
    "mse_filter_len": (sz, [vp]),
    "mse_filter_count": (sz, [vp]),
    "mse_bruteforce_topk_filtered_f16": (C.c_int, [vp, vp, u16p, sz, sz, C.c_int, i64p, u32p]),
    "mse_bruteforce_topk_filtered_f16_dev": (C.c_int, [vp, vp, vp, sz, sz, C.c_int, C.c_uint64, vp, vp]),
    "mse_groups_from_host": (vp, [u32p, sz]),
    "mse_groups_from_dev": (vp, [vp, sz]),
    "mse_groups_free": (None, [vp]),
    "mse_groups_len": (sz, [vp]),
    "mse_groups_count": (sz, [vp]),
    "mse_bruteforce_topk_grouped_f16": (C.c_int, [vp, vp, vp, u16p, sz, sz, C.c_int, i64p, u32p]),
    "mse_bruteforce_topk_grouped_f16_dev": (C.c_int, [vp, vp, vp, vp, sz, sz, C.c_int, C.c_uint64, vp, vp]),
    "mse_searcher_grouped_stats": (C.c_int, [vp, u32p]),
    "mse_searcher_grouped_timing": (C.c_int, [vp, C.c_int, C.POINTER(C.c_double)]),
    "mse_debug_collapse_topk": (C.c_int, [vp, vp, u32p, sz, sz, sz, u32p, u32p]),
    "mse_bruteforce_ranks_f16": (C.c_int, [vp, u16p, u32p, sz, u32p]),
    "mse_score_rows_f16": (C.c_int, [vp, u32p, sz, u16p, i64p]),
    "mse_merge_topk_dev": (C.c_int, [vp, vp, vp, sz, sz, sz, vp, vp]),
    "mse_topk_block_bytes": (sz, [sz, sz]),
    "mse_merge_topk_packed_dev": (C.c_int, [vp, vp, sz, sz, sz, vp, vp]),
    "mse_base_rows_changed": (C.c_int, [vp]),
    "mse_shard_group_new": (vp, [C.POINTER(C.c_int), sz, sz]),
    "mse_shard_group_free": (None, [vp]),
    "mse_shard_group_n_shards": (sz, [vp]),
    "mse_shard_group_len": (sz, [vp]),
    "mse_shard_group_device": (C.c_int, [vp, sz]),
    "mse_shard_group_peer_mapped": (C.c_int, [vp, sz]),
    "mse_shard_group_searcher": (vp, [vp, sz]),
    "mse_shard_group_generate": (C.c_int, [vp, C.c_uint32, C.c_uint64, sz]),
    "mse_shard_group_load_host": (C.c_int, [vp, u16p, sz]),
    "mse_shard_group_set_shard_device": (C.c_int, [vp, sz, vp, sz, C.c_uint64]),
    "mse_shard_group_search": (C.c_int, [vp, u16p, sz, sz, C.c_int, i64p, u32p]),
    "mse_shard_group_set_exchange": (C.c_int, [vp, C.c_int]),
    "mse_shard_group_exchange": (C.c_int, [vp]),
    "mse_shard_group_rccl_ranks": (C.c_int, [vp]),
    "mse_shard_group_last_timing": (C.c_int, [vp, C.POINTER(C.c_double)]),
    "mse_shard_group_search_dev": (C.c_int, [vp, vp, sz, sz, C.c_int, vp, vp]),
    "mse_comm_unique_id": (C.c_int, [vp]),
    "mse_comm_init": (vp, [vp, C.c_int, C.c_int]),
    "mse_comm_free": (None, [vp]),
    "mse_comm_rank": (C.c_int, [vp]),
    "mse_comm_size": (C.c_int, [vp]),
    "mse_comm_search_dev": (C.c_int, [vp, vp, vp, sz, sz, C.c_int, C.c_uint64, vp, vp]),
    "mse_comm_last_timing": (C.c_int, [vp, C.POINTER(C.c_double)]),
    "mse_debug_mfma_group_max": (C.c_int, [vp, u16p, sz, f32p]),
    "mse_debug_select_topk": (C.c_int, [vp, C.c_int, C.c_int, vp, sz, sz, sz, sz, u32p, vp, C.POINTER(C.c_uint64)]),
    "mse_searcher_scan_timing": (C.c_int, [vp, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]),
    "mse_searcher_last_stats": (C.c_int, [vp, u32p, u32p]),
    "mse_searcher_set_sparse_maxima": (C.c_int, [vp, C.c_int, C.c_uint32, C.c_uint32]),
    "mse_searcher_sparse_stats": (C.c_int, [vp, u32p, u32p, u32p]),
    "mse_index_new": (vp, [C.c_int]),
    "mse_index_free": (None, [vp]),
    "mse_index_add": (C.c_int, [vp, f32p, sz]),
    "mse_index_ntotal": (sz, [vp]),
    "mse_index_search": (C.c_int, [vp, f32p, sz, sz, f32p, i64p]),
    "mse_index_search_filtered": (C.c_int, [vp, vp, f32p, sz, sz, f32p, i64p]),
    "mse_index_search_grouped": (C.c_int, [vp, vp, vp, f32p, sz, sz, f32p, i64p]),
    "mse_index_stats": (C.c_int, [vp, C.POINTER(C.c_uint64)]),
    "mse_dispatcher_new": (vp, [vp, sz, C.c_uint32]),
    "mse_dispatcher_free": (None, [vp]),
    "mse_dispatcher_topk_f16": (C.c_int, [vp, u16p, sz, sz, i64p, u32p]),
    "mse_dispatcher_topk_filtered_f16": (C.c_int, [vp, vp, u16p, sz, sz, i64p, u32p]),
    "mse_dispatcher_stats": (C.c_int, [vp, C.POINTER(C.c_uint64)]),
    "mse_dispatcher_searcher": (vp, [vp]),
    "mse_debug_dispatcher_fail_shared": (C.c_int, [vp, C.c_uint32]),
    "mse_debug_coalescer_selftest": (C.c_int, [C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "mse_pq_load": (vp, [f32p, sz, f32p, sz, sz]),
    "mse_pq_free": (None, [vp]),
    "mse_pq_apply_transform": (C.c_int, [vp, f32p, sz, f32p]),
    "mse_pq_quantize_batch": (C.c_int, [vp, f32p, sz, u8p]),
    "mse_pq_preprocess_query": (C.c_int, [vp, f32p, f32p]),
    "mse_pq_adc": (C.c_int, [vp, f32p, u8p, sz, i64p]),
    "mse_pq_trainer_new": (vp, [sz, sz, sz]),
    "mse_pq_trainer_free": (None, [vp]),
    "mse_pq_trainer_set_sample_f32": (C.c_int, [vp, f32p, sz]),
    "mse_pq_trainer_set_sample_base": (C.c_int, [vp, vp, u32p, sz]),
    "mse_pq_trainer_set_transform": (C.c_int, [vp, f32p]),
    "mse_pq_trainer_set_centroids": (C.c_int, [vp, f32p]),
    "mse_pq_trainer_set_query_moment": (C.c_int, [vp, f32p]),
    "mse_pq_trainer_kmeans": (C.c_int, [vp, sz, C.POINTER(C.c_uint64)]),
    "mse_pq_trainer_refine": (C.c_int, [vp, sz, C.c_float, C.c_float, C.c_float, C.c_float, C.POINTER(C.c_double)]),
    "mse_pq_trainer_loss": (C.c_int, [vp, C.POINTER(C.c_double)]),
    "mse_pq_trainer_cross": (C.c_int, [vp, C.POINTER(C.c_double)]),
    "mse_pq_trainer_read": (C.c_int, [vp, f32p, f32p]),
    "mse_pq_trainer_codes": (C.c_int, [vp, u8p]),
    "mse_pq_trainer_rotated_rows": (C.c_int, [vp, u32p, sz, f32p]),
    "mse_pq_trainer_adam_state": (C.c_int, [vp, f32p, f32p, C.POINTER(C.c_uint64)]),
    "mse_pq_trainer_set_adam_state": (C.c_int, [vp, f32p, f32p, C.c_uint64]),
    "mse_pq_trainer_gradient": (C.c_int, [vp, f32p]),
    "mse_pq_trainer_finish": (vp, [vp]),
    "mse_pq_trainer_timing": (C.c_int, [vp, f32p]),
    "mse_debug_accumulate_by_code": (C.c_int, [f32p, sz, sz, u8p, sz, i64p, C.POINTER(C.c_int)]),
    "mse_debug_residual_gemm": (C.c_int, [f32p, u8p, f32p, f32p, sz, sz, sz, sz, f32p, f32p]),
    "mse_debug_pq_trainer_chunk_rows": (C.c_int, [vp, sz]),
    "mse_partition_config_default": (None, [vp]),
    "mse_partition_new": (vp, [sz, sz, vp]),
    "mse_partition_free": (None, [vp]),
    "mse_partition_set_sample_f16": (C.c_int, [vp, u16p, sz]),
    "mse_partition_set_sample_base": (C.c_int, [vp, vp, u32p, sz]),
    "mse_partition_anneal": (C.c_int, [vp, sz]),
    "mse_partition_state": (C.c_int, [vp, vp]),
    "mse_partition_trace": (C.c_int, [vp, sz, sz, C.POINTER(C.c_uint64), u8p]),
    "mse_partition_centroids": (C.c_int, [vp, f32p, f32p, u16p]),
    "mse_partition_set_centroids": (C.c_int, [vp, f32p]),
    "mse_partition_count": (C.c_int, [vp, f32p, C.POINTER(C.c_uint64), u8p]),
    "mse_partition_scores": (C.c_int, [vp, f32p, C.POINTER(C.c_double)]),
    "mse_partition_assign_f16": (C.c_int, [vp, u16p, sz, C.c_double]),
    "mse_partition_assign_base": (C.c_int, [vp, vp, sz, sz, C.c_double]),
    "mse_partition_assign_reset": (C.c_int, [vp]),
    "mse_partition_assignment": (C.c_int, [vp, sz, sz, u8p]),
    "mse_partition_counts": (C.c_int, [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "mse_partition_shard_filter": (vp, [vp, sz]),
    "mse_partition_timing": (C.c_int, [vp, f32p]),
    "mse_medioid_ids": (C.c_int, [vp, u32p, sz, u32p]),
    "mse_debug_partition_noise": (C.c_int, [C.c_uint32, C.c_uint64, sz, f32p]),
    "mse_debug_partition_normalise": (C.c_int, [f32p, sz, sz, f32p, u16p]),
    "mse_debug_partition_chunk_rows": (C.c_int, [vp, sz]),
    "mse_codes_from_host": (vp, [u8p, sz, sz, u8p, sz]),
    "mse_codes_free": (None, [vp]),
    "mse_codes_quantize_base": (vp, [vp, vp, u8p, sz]),
    "mse_pq_scan_timing": (C.c_int, [vp, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]),
    "mse_pq_scan_sustained": (C.c_int, [vp, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]),
    "mse_codes_len": (sz, [vp]),
    "mse_pq_adc_gather": (C.c_int, [vp, vp, f32p, f32p, u32p, sz, i64p]),
    "mse_pq_scan_topk": (C.c_int, [vp, vp, vp, f32p, f32p, sz, sz, i64p, u32p]),
    "mse_pq_scan_topk_batch": (C.c_int, [vp, vp, vp, f32p, sz, f32p, sz, sz, i64p, u32p]),
    "mse_pq_last_uncertified": (C.c_uint32, [vp]),
    "mse_debug_pq_group_max": (C.c_int, [vp, vp, f32p, f32p, f32p, i64p, i64p]),
    "mse_debug_pq4_group_max": (C.c_int, [vp, vp, f32p, f32p, C.c_int, C.c_int, u32p, C.POINTER(C.c_double)]),
    "mse_pq_scan_topk_filtered": (C.c_int, [vp, vp, vp, vp, f32p, f32p, sz, sz, C.c_int, i64p, u32p]),
    "mse_pq_scan_topk_batch_filtered": (C.c_int, [vp, vp, vp, vp, f32p, sz, f32p, sz, sz, C.c_int, i64p, u32p]),
    "mse_pq_scan_topk_block_filtered": (C.c_int, [vp, vp, vp, vp, f32p, sz, f32p, sz, sz, C.c_int, C.c_uint64, vp]),
    "mse_pq_filtered_plan": (C.c_int, [sz, sz, sz, C.POINTER(C.c_int)]),
    "mse_debug_pq_group_max_filtered": (C.c_int, [vp, vp, vp, f32p, f32p, f32p, i64p, i64p]),
    "mse_debug_pq4_group_max_filtered": (C.c_int, [vp, vp, vp, f32p, f32p, C.c_int, C.c_int, u32p, C.POINTER(C.c_double)]),
    "mse_graph_live_filter": (vp, [vp, C.c_int]),
    "mse_filter_combine": (vp, [vp, vp, C.c_int]),
    "mse_filter_not": (vp, [vp, sz]),
    "mse_filter_from_descriptors": (vp, [vp, u8p, u8p]),
    "mse_filter_from_scores": (vp, [vp, u16p, C.c_int64, vp]),
    "mse_filter_from_bits_dev": (vp, [vp, sz]),
    "mse_filter_to_bits": (C.c_int, [vp, u8p]),
    "mse_filter_read_ids": (C.c_int, [vp, sz, sz, u32p]),
    "mse_filter_kernel_timing": (C.c_int, [C.c_int, C.POINTER(C.c_double)]),
    "mse_filter_slice": (vp, [vp, C.c_uint64, sz, C.c_int]),
    "mse_filter_concat": (vp, [C.POINTER(vp), C.POINTER(C.c_uint64), sz, sz, C.c_int]),
    "mse_join_self": (vp, [vp, C.c_int64, C.c_uint64, vp, C.c_int, C.c_uint64]),
    "mse_pairs_free": (None, [vp]),
    "mse_pairs_rows": (sz, [vp]),
    "mse_pairs_count": (sz, [vp]),
    "mse_pairs_read": (C.c_int, [vp, sz, sz, u32p, u32p, i64p]),
    "mse_join_stats": (C.c_int, [vp, C.POINTER(C.c_uint64)]),
    "mse_join_timing": (C.c_int, [vp, C.c_int, C.POINTER(C.c_double)]),
    "mse_debug_join_candidate_capacity": (C.c_int, [vp, C.c_uint64]),
    "mse_pairs_duplicates": (vp, [vp]),
    "mse_pairs_groups": (vp, [vp]),
    "mse_pairs_representatives": (C.c_int, [vp, u32p]),
    "mse_join_cross": (vp, [vp, vp, C.c_int64, vp, C.c_int, C.c_uint64]),
    "mse_pairs_kind": (C.c_int, [vp]),
    "mse_pairs_base_rows": (sz, [vp]),
    "mse_pairs_admit": (C.c_int, [vp, vp, C.POINTER(vp), u32p, u32p]),
    "mse_base_select": (vp, [vp, vp]),
    "mse_shard_group_filter": (vp, [vp, vp]),
    "mse_shard_group_filter_from_local": (vp, [vp, C.POINTER(vp)]),
    "mse_shard_group_live_filter": (vp, [vp, C.c_int]),
    "mse_shard_filter_free": (None, [vp]),
    "mse_shard_filter_count": (sz, [vp]),
    "mse_shard_filter_n_shards": (sz, [vp]),
    "mse_shard_filter_shard": (vp, [vp, sz]),
    "mse_shard_filter_global": (vp, [vp, C.c_int]),
    "mse_shard_group_search_filtered": (C.c_int, [vp, vp, u16p, sz, sz, C.c_int, i64p, u32p]),
    "mse_shard_group_search_filtered_dev": (C.c_int, [vp, vp, vp, sz, sz, C.c_int, vp, vp]),
    "mse_shard_group_pq_scan_topk_filtered": (C.c_int, [vp, vp, f32p, f32p, sz, sz, sz, C.c_int, i64p, u32p]),
    "mse_shard_group_query_topk_filtered": (C.c_int, [vp, vp, u16p, f32p, f32p, sz, C.c_int, sz, sz, sz, C.c_int, i64p, u32p]),
    "mse_disk_query_topk_block_filtered": (C.c_int, [vp, vp, vp, vp, vp, C.c_int, u32p, u16p, f32p, f32p, sz, C.c_int, sz, sz, sz, C.c_uint64, vp,
                                                     u32p, u32p, u32p]),
    "mse_comm_search_filtered_dev": (C.c_int, [vp, vp, vp, vp, sz, sz, C.c_int, C.c_uint64, vp, vp]),
    "mse_comm_pq_scan_topk_filtered": (C.c_int, [vp, vp, vp, vp, vp, f32p, f32p, sz, sz, sz, C.c_int, C.c_uint64, vp, vp]),
    "mse_comm_query_topk_filtered": (C.c_int, [vp, vp, vp, vp, vp, vp, C.c_int, u16p, f32p, f32p, sz, C.c_int, sz, sz, sz, C.c_uint64, vp, vp]),
    "mse_groups_slice": (vp, [vp, C.c_uint64, sz, C.c_int]),
    "mse_groups_read": (C.c_int, [vp, u32p]),
    "mse_shard_group_groups": (vp, [vp, vp]),
    "mse_shard_groups_part": (vp, [vp, sz]),
    "mse_shard_groups_n_shards": (sz, [vp]),
    "mse_shard_groups_free": (None, [vp]),
    "mse_merge_topk_packed_grouped_dev": (C.c_int, [vp, vp, vp, sz, sz, sz, sz, vp, vp]),
    "mse_shard_group_search_grouped": (C.c_int, [vp, vp, vp, u16p, sz, sz, C.c_int, i64p, u32p]),
    "mse_shard_group_search_grouped_dev": (C.c_int, [vp, vp, vp, vp, sz, sz, C.c_int, vp, vp]),
    "mse_shard_group_pq_scan_topk_grouped": (C.c_int, [vp, vp, vp, f32p, f32p, sz, sz, sz, C.c_int, i64p, u32p]),
    "mse_shard_group_query_topk_grouped": (C.c_int, [vp, vp, vp, u16p, f32p, f32p, sz, C.c_int, sz, sz, sz, C.c_int, i64p, u32p]),
    "mse_disk_query_topk_block_grouped": (C.c_int, [vp, vp, vp, vp, vp, vp, C.c_int, u32p, u16p, f32p, f32p, sz, C.c_int, sz, sz, sz, C.c_uint64, vp,
                                                    u32p, u32p, u32p]),
    "mse_descriptor_product": (C.c_int64, [f32p, sz, u8p, C.c_uint32]),
    "mse_nb_new": (vp, [sz]),
    "mse_nb_free": (None, [vp]),
    "mse_nb_clear": (None, [vp]),
    "mse_nb_len": (sz, [vp]),
    "mse_nb_cap": (sz, [vp]),
    "mse_nb_insert": (None, [vp, C.c_uint32, C.c_int64]),
    "mse_nb_next_unvisited": (C.c_int, [vp, u32p]),
    "mse_nb_ids": (u32p, [vp]),
    "mse_nb_scores": (i64p, [vp]),
    "mse_greedy_search": (C.c_int, [vp, u32p, u32p, sz, C.c_uint32, u16p, C.c_int, C.c_uint32, vp, C.POINTER(sz)]),
    "mse_disk_greedy_search": (C.c_int, [vp, vp, vp, u32p, u32p, sz, u8p, C.c_uint32, u16p, f32p, f32p, C.c_int, sz, vp,
                                         u32p, i64p, sz, C.POINTER(sz), C.POINTER(sz), C.POINTER(sz)]),
    "mse_graph_from_host": (vp, [u32p, u32p, sz, sz, u8p]),
    "mse_graph_free": (None, [vp]),
    "mse_disk_search_batch": (C.c_int, [vp, vp, vp, vp, u32p, u16p, f32p, f32p, sz, C.c_int, sz, sz, u32p, i64p, u32p, u32p, i64p, sz,
                                        u32p, u32p, u32p]),
    "mse_disk_search_batch_f32": (C.c_int, [vp, vp, vp, vp, u32p, f32p, f32p, sz, C.c_int, sz, sz, u32p, i64p, u32p, u32p, i64p, sz,
                                            u32p, u32p, u32p]),
    "mse_graph_set_entries": (C.c_int, [vp, vp, u32p, sz]),
    "mse_disk_query_topk_block": (C.c_int, [vp, vp, vp, vp, u32p, u16p, f32p, f32p, sz, C.c_int, sz, sz, sz, C.c_uint64, vp, u32p, u32p, u32p]),
    "mse_pq_scan_topk_block": (C.c_int, [vp, vp, vp, f32p, sz, f32p, sz, sz, C.c_uint64, vp]),
    "mse_shard_group_base": (vp, [vp, sz]),
    "mse_shard_group_first_row": (C.c_uint64, [vp, sz]),
    "mse_comm_exchange_dev": (C.c_int, [vp, vp, vp, sz, sz, sz, vp, vp]),
    "mse_comm_pq_scan_topk": (C.c_int, [vp, vp, vp, vp, f32p, f32p, sz, sz, sz, C.c_uint64, vp, vp]),
    "mse_comm_query_topk": (C.c_int, [vp, vp, vp, vp, vp, u16p, f32p, f32p, sz, C.c_int, sz, sz, sz, C.c_uint64, vp, vp]),
    "mse_shard_group_attach_pq": (C.c_int, [vp, sz, vp, vp]),
    "mse_shard_group_attach_graph": (C.c_int, [vp, sz, vp]),
    "mse_shard_group_pq_scan_topk": (C.c_int, [vp, f32p, f32p, sz, sz, sz, i64p, u32p]),
    "mse_shard_group_query_topk": (C.c_int, [vp, u16p, f32p, f32p, sz, C.c_int, sz, sz, sz, i64p, u32p]),
    "mse_graph_set_entry_centroids": (C.c_int, [vp, f32p, sz, u32p, sz]),
    "mse_disk_query_topk_f32": (C.c_int, [vp, vp, vp, vp, u32p, f32p, f32p, sz, C.c_int, sz, sz, sz, u32p, i64p, u32p, u32p, u32p]),
    "mse_disk_query_submit_f32": (C.c_int, [vp, vp, vp, vp, f32p, f32p, sz, C.c_int, sz, sz, sz, u32p, i64p, u32p, u32p, u32p, vp, vp, C.POINTER(vp)]),
    "mse_disk_query_submit_f32_nocopy": (C.c_int, [vp, vp, vp, vp, f32p, f32p, sz, C.c_int, sz, sz, sz, u32p, i64p, u32p, u32p, u32p, vp, vp, C.POINTER(vp)]),
    "mse_completion_queue_new": (vp, []),
    "mse_completion_queue_free": (None, [vp]),
    "mse_completion_queue_fd": (C.c_int, [vp]),
    "mse_completion_queue_wait": (C.c_long, [vp, C.POINTER(vp), sz, C.c_long]),
    "mse_graph_completions": (C.c_long, [vp, C.POINTER(vp), sz, C.c_long]),
    "mse_graph_completion_fd": (C.c_int, [vp]),
    "mse_ticket_status": (C.c_int, [vp]),
    "mse_ticket_error": (C.c_char_p, [vp]),
    "mse_ticket_user": (vp, [vp]),
    "mse_ticket_free": (None, [vp]),
    "mse_graph_set_dedup": (C.c_int, [vp, C.c_float]),
    "mse_graph_set_coalescer": (C.c_int, [vp, sz, C.c_uint32, C.c_int]),
    "mse_graph_coalescer_stats": (C.c_int, [vp, C.POINTER(C.c_uint64)]),
    "mse_graph_coalescer_groups": (C.c_int, [vp, C.POINTER(C.c_uint64)]),
    "mse_searcher_wait_stream": (C.c_int, [vp, vp]),
    "mse_searcher_beam_timing": (C.c_int, [vp, C.c_int, C.POINTER(C.c_uint64)]),
    "mse_debug_coalescer_selftest_workers": (C.c_int, [C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "mse_debug_coalescer_selftest_async": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_int, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "mse_disk_query_topk": (C.c_int, [vp, vp, vp, vp, u32p, u16p, f32p, f32p, sz, C.c_int, sz, sz, sz, u32p, i64p, u32p, u32p, u32p]),
    "mse_filtered_plan": (C.c_int, [sz, sz, sz, C.c_int, C.POINTER(C.c_int), C.POINTER(sz)]),
    "mse_disk_search_batch_filtered": (C.c_int, [vp, vp, vp, vp, vp, u32p, u16p, f32p, f32p, sz, C.c_int, sz, sz, u32p, i64p, u32p, u32p, i64p,
                                                 sz, u32p, u32p, u32p]),
    "mse_disk_query_topk_filtered": (C.c_int, [vp, vp, vp, vp, vp, C.c_int, u32p, u16p, f32p, f32p, sz, C.c_int, sz, sz, sz, u32p, i64p, u32p,
                                               u32p, u32p]),
    "mse_disk_query_topk_filtered_f32": (C.c_int, [vp, vp, vp, vp, vp, C.c_int, u32p, f32p, f32p, sz, C.c_int, sz, sz, sz, u32p, i64p, u32p,
                                                   u32p, u32p]),
    "mse_disk_query_submit_filtered_f32": (C.c_int, [vp, vp, vp, vp, vp, C.c_int, f32p, f32p, sz, C.c_int, sz, sz, sz, u32p, i64p, u32p, u32p,
                                                     u32p, vp, vp, C.POINTER(vp)]),
    "mse_disk_query_topk_grouped": (C.c_int, [vp, vp, vp, vp, vp, vp, C.c_int, u32p, u16p, f32p, f32p, sz, C.c_int, sz, sz, sz, u32p, i64p, u32p,
                                              u32p, u32p]),
    "mse_disk_query_topk_grouped_f32": (C.c_int, [vp, vp, vp, vp, vp, vp, C.c_int, u32p, f32p, f32p, sz, C.c_int, sz, sz, sz, u32p, i64p, u32p,
                                                  u32p, u32p]),
    "mse_disk_query_submit_grouped_f32": (C.c_int, [vp, vp, vp, vp, vp, vp, C.c_int, f32p, f32p, sz, C.c_int, sz, sz, sz, u32p, i64p, u32p, u32p,
                                                    u32p, vp, vp, C.POINTER(vp)]),
    # a filter per query: [nq] filter handles (NULL entries: unfiltered) where the single-filter calls take one handle
    "mse_disk_query_topk_filtered_each": (C.c_int, [vp, vp, vp, vp, C.POINTER(vp), C.c_int, vp, u32p, u16p, f32p, f32p, sz, C.c_int, sz, sz, sz,
                                                    u32p, i64p, u32p, u32p, u32p]),
    "mse_disk_query_topk_filtered_each_f32": (C.c_int, [vp, vp, vp, vp, C.POINTER(vp), C.c_int, vp, u32p, f32p, f32p, sz, C.c_int, sz, sz, sz,
                                                        u32p, i64p, u32p, u32p, u32p]),
    "mse_disk_search_batch_filtered_each": (C.c_int, [vp, vp, vp, vp, C.POINTER(vp), u32p, u16p, f32p, f32p, sz, C.c_int, sz, sz, u32p, i64p,
                                                      u32p, u32p, i64p, sz, u32p, u32p, u32p]),
    "mse_debug_visited_collapse": (C.c_int, [vp, vp, u32p, i64p, sz, u32p, sz]),
    "mse_graph_new": (vp, [sz, sz]),
    "mse_graph_to_host": (C.c_int, [vp, u32p, u32p]),
    "mse_graph_len": (sz, [vp]),
    "mse_graph_max_degree": (sz, [vp]),
    "mse_graph_random_fill": (C.c_int, [vp, C.c_uint32, sz]),
    "mse_build_graph": (C.c_int, [vp, vp, u32p, sz, sz, C.c_uint32, vp]),
    "mse_robust_stitch": (C.c_int, [vp, vp, u32p, vp]),
    "mse_robust_prune": (C.c_int, [vp, u32p, i64p, sz, C.c_uint32, vp, u32p, C.POINTER(sz)]),
    "mse_graph_delete_rows": (C.c_int, [vp, vp, vp, vp, sz, C.POINTER(C.c_uint64)]),
    "mse_graph_deleted": (C.c_int, [vp, u8p, C.POINTER(sz)]),
    "mse_graph_restore_rows": (C.c_int, [vp, u32p, sz]),
    "mse_graph_insert_rows": (C.c_int, [vp, vp, vp, vp, u32p, sz, u16p, u8p, u8p, C.c_uint32, vp, sz, C.POINTER(C.c_uint64)]),
    "mse_graph_insert_rows_dev": (C.c_int, [vp, vp, vp, vp, u32p, sz, vp, u8p, u8p, C.c_uint32, vp, sz, C.POINTER(C.c_uint64)]),
    "mse_graph_compact": (C.c_int, [vp, vp, vp, sz, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), u32p, u32p, C.POINTER(C.c_uint64)]),
    "mse_searcher_compact_timing": (C.c_int, [vp, C.c_int, C.POINTER(C.c_double)]),
    "mse_codes_read_rows": (C.c_int, [vp, sz, sz, u8p, u8p]),
    "mse_debug_base_norm_bits": (C.c_int, [vp, u32p]),
    "mse_graph_search_batch": (C.c_int, [vp, vp, u32p, u16p, sz, sz, C.c_int, C.c_uint32, u32p, i64p, u32p, u32p]),
    "mse_dedup_visited": (C.c_int, [vp, u32p, sz, C.c_float, u8p]),
    "mse_select_shard": (C.c_int, [f32p, sz, sz, f32p, C.POINTER(sz)]),
    "mse_medioid": (C.c_int, [vp, u32p]),
    "mse_score_model_load": (vp, [f32p, f32p, f32p, sz, sz, sz]),
    "mse_score_model_free": (None, [vp]),
    "mse_score_model_output_channels": (sz, [vp]),
    "mse_score_model_score_batch": (C.c_int, [vp, f32p, sz, f32p]),
    "mse_descriptor_buckets": (C.c_int, [f32p, sz, sz, f32p, sz, u8p]),
    "mse_scores_from_base": (vp, [vp, vp, u32p, sz, sz, i64p]),
    "mse_scores_from_f16": (vp, [vp, u16p, sz, sz, u32p, sz, sz, i64p]),
    "mse_scores_from_host": (vp, [f32p, sz, sz, i64p]),
    "mse_scores_free": (None, [vp]),
    "mse_scores_len": (sz, [vp]),
    "mse_scores_channels": (sz, [vp]),
    "mse_scores_has_timestamps": (C.c_int, [vp]),
    "mse_scores_read": (C.c_int, [vp, f32p, u32p]),
    "mse_scores_order_statistics": (C.c_int, [vp, sz, C.POINTER(C.c_uint64), sz, C.POINTER(C.c_double)]),
    "mse_scores_fit_cdfs": (C.c_int, [vp, sz, f32p]),
    "mse_codes_describe": (C.c_int, [vp, vp, vp, u32p, sz, f32p, sz]),
    "mse_describe_timing": (C.c_int, [C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    # sparse-autoencoder features (csrc/sae.hip, csrc/sae_api.hip)
    "mse_sae_load": (vp, [f32p, f32p, f32p, f32p, sz, sz, sz]),
    "mse_sae_free": (None, [vp]),
    "mse_sae_d_emb": (sz, [vp]),
    "mse_sae_d_hidden": (sz, [vp]),
    "mse_sae_top_k": (sz, [vp]),
    "mse_sae_encode_base": (vp, [vp, vp, u32p, sz, sz, C.c_int]),
    "mse_sae_encode_f16": (vp, [vp, u16p, sz, sz, C.c_int]),
    "mse_features_free": (None, [vp]),
    "mse_features_len": (sz, [vp]),
    "mse_features_top_k": (sz, [vp]),
    "mse_features_invalid_rows": (C.c_uint64, [vp]),
    "mse_features_read": (C.c_int, [vp, u32p, u32p, f32p]),
    "mse_features_reconstruct": (C.c_int, [vp, vp, f32p, C.POINTER(C.c_double)]),
    "mse_features_filter": (vp, [vp, C.c_uint32, C.c_float, sz]),
    "mse_sae_counters": (C.c_int, [vp, C.POINTER(C.c_uint64), C.c_int]),
    "mse_sae_set_hidden_parts": (C.c_int, [vp, C.c_int]),
    "mse_sae_timing": (C.c_int, [C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "mse_sae_read_weights": (C.c_int, [vp, f32p, f32p, f32p, f32p]),
    # sparse-autoencoder training (csrc/sae_train.hip, csrc/sae_train_api.hip)
    "mse_sae_trainer_create": (vp, [vp, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double]),
    "mse_sae_trainer_free": (None, [vp]),
    "mse_sae_trainer_step_count": (C.c_uint64, [vp]),
    "mse_sae_trainer_steps": (C.c_int, [vp, vp, u32p, sz, sz, C.POINTER(C.c_double), C.POINTER(sz)]),
    "mse_sae_trainer_steps_f16": (C.c_int, [vp, u16p, sz, sz, sz, C.POINTER(C.c_double), C.POINTER(sz)]),
    "mse_sae_trainer_state_read": (C.c_int, [vp, C.POINTER(C.c_uint64), f32p, f32p, f32p, f32p, f32p, f32p, f32p, f32p]),
    "mse_sae_trainer_state_write": (C.c_int, [vp, C.c_uint64, f32p, f32p, f32p, f32p, f32p, f32p, f32p, f32p]),
    "mse_sae_trainer_set_skip": (C.c_int, [vp, C.c_int]),
    "mse_sae_trainer_timing": (C.c_int, [C.c_int, C.POINTER(C.c_double)]),
    # the ensemble rater (csrc/rater.hip, csrc/rater_api.hip)
    "mse_rater_create": (vp, [f32p, f32p, f32p, sz, sz, sz]),
    "mse_rater_free": (None, [vp]),
    "mse_rater_read_weights": (C.c_int, [vp, f32p, f32p, f32p]),
    "mse_rater_trainer_create": (vp, [vp, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double]),
    "mse_rater_trainer_free": (None, [vp]),
    "mse_rater_trainer_step_count": (C.c_uint64, [vp]),
    "mse_rater_trainer_steps": (C.c_int, [vp, vp, u32p, f32p, sz, sz, C.POINTER(C.c_double), C.POINTER(sz)]),
    "mse_rater_trainer_steps_f16": (C.c_int, [vp, u16p, sz, sz, u32p, f32p, sz, sz, C.POINTER(C.c_double), C.POINTER(sz)]),
    "mse_rater_trainer_state_read": (C.c_int, [vp, C.POINTER(C.c_uint64), f32p, f32p, f32p, f32p, f32p, f32p]),
    "mse_rater_trainer_state_write": (C.c_int, [vp, C.c_uint64, f32p, f32p, f32p, f32p, f32p, f32p]),
    "mse_rater_trainer_last_scores": (C.c_int, [vp, f32p, C.POINTER(sz)]),
    "mse_rater_trainer_timing": (C.c_int, [C.c_int, C.POINTER(C.c_double)]),
    "mse_member_scores_from_base": (vp, [vp, vp, u32p, sz, sz]),
    "mse_member_scores_from_f16": (vp, [vp, u16p, sz, sz, u32p, sz, sz]),
    "mse_member_scores_free": (None, [vp]),
    "mse_member_scores_len": (sz, [vp]),
    "mse_member_scores_read": (C.c_int, [vp, f32p]),
    "mse_member_scores_pair_variance": (C.c_int, [vp, u32p, u32p, sz, f32p]),
    "mse_siglip_create": (vp, [vp]),
    "mse_siglip_destroy": (None, [vp]),
    "mse_siglip_n_weights": (C.c_int, [vp]),
    "mse_siglip_weight_name": (C.c_char_p, [vp, C.c_int]),
    "mse_siglip_set_weight": (C.c_int, [vp, C.c_char_p, f32p, C.POINTER(sz), C.c_int]),
    "mse_siglip_finalize": (C.c_int, [vp]),
    "mse_siglip_encode_image": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, f32p, u16p]),
    "mse_siglip_encode_rgb8": (C.c_int, [vp, u8p, C.c_int, C.c_int, f32p, u16p]),
    "mse_bmp24_info": (C.c_int, [C.c_char_p, sz, u32p, u32p, u32p, C.POINTER(C.c_int)]),
    "mse_siglip_encode_bmp": (C.c_int, [vp, C.POINTER(C.c_char_p), C.POINTER(sz), C.c_int, C.c_int, f32p, u16p]),
    "mse_resize_coeffs": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), i32p, i32p]),
    "mse_resize_pick_filter": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "mse_resize_rgb8": (C.c_int, [C.POINTER(vp), u32p, u32p, C.c_int, C.c_int, C.c_int, C.c_int, u8p]),
    "mse_siglip_encode_rgb8_any": (C.c_int, [vp, C.POINTER(vp), u32p, u32p, C.c_int, C.c_int, C.c_int, f32p, u16p]),
    "mse_siglip_encode_bmp_any": (C.c_int, [vp, C.POINTER(C.c_char_p), C.POINTER(sz), C.c_int, C.c_int, C.c_int, f32p, u16p]),
    "mse_debug_siglip_resize_nchw": (C.c_int, [vp, C.c_int, u16p]),
    "mse_resize_timing": (C.c_int, [C.POINTER(C.c_double)]),
    "mse_siglip_output_device": (vp, [vp, C.c_int]),
    "mse_siglip_stream": (vp, [vp]),
    "mse_siglip_debug_residual": (C.c_int, [vp, f32p]),
    "mse_debug_gemm_ms": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, f32p]),
    "mse_debug_gemm_small": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, f32p, C.POINTER(C.c_uint64)]),
    "mse_debug_siglip_attention": (C.c_int, [f32p, f32p, f32p, C.c_int, C.c_int, C.c_int, C.c_int, f32p]),
    "mse_debug_siglip_pool_attention": (C.c_int, [f32p, f32p, f32p, C.c_int, C.c_int, C.c_int, f32p]),
    "mse_debug_siglip_gemm": (C.c_int, [vp]),
    "mse_debug_siglip_gemm_fused": (C.c_int, [vp]),
    "mse_debug_siglip_layernorm": (C.c_int, [vp]),
    "mse_debug_siglip_patchify": (C.c_int, [f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, f32p]),
    "mse_debug_siglip_rgb8": (C.c_int, [u8p, C.c_int, C.c_int, C.c_int, C.c_int, f32p]),
    "mse_debug_siglip_bmp24": (C.c_int, [u8p, sz, C.c_int, u8p, C.c_int, C.c_int, C.c_int, f32p]),
    "mse_debug_siglip_embed_tokens": (C.c_int, [i64p, f32p, f32p, C.c_int, C.c_int, C.c_int, C.c_int, f32p]),
    "mse_debug_siglip_f32_to_bf16_pad": (C.c_int, [f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, f32p]),
    "mse_debug_siglip_small_linear": (C.c_int, [f32p, C.c_int, f32p, C.c_int, f32p, C.c_int, C.c_int, C.c_int, C.c_int, f32p]),
    "mse_debug_siglip_l2norm": (C.c_int, [f32p, C.c_int, C.c_int, C.c_int, C.c_int, f32p, f32p]),
    "mse_debug_siglip_vt_ones_row": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, f32p]),
    "mse_siglip_text_create": (vp, [vp]),
    "mse_siglip_text_destroy": (None, [vp]),
    "mse_siglip_text_n_weights": (C.c_int, [vp]),
    "mse_siglip_text_weight_name": (C.c_char_p, [vp, C.c_int]),
    "mse_siglip_text_set_weight": (C.c_int, [vp, C.c_char_p, f32p, C.POINTER(sz), C.c_int]),
    "mse_siglip_text_finalize": (C.c_int, [vp]),
    "mse_siglip_text_encode": (C.c_int, [vp, i64p, C.c_int, C.c_int, f32p, u16p]),
    "mse_siglip_text_encode_dev": (C.c_int, [vp, i64p, C.c_int, C.c_int]),
    "mse_siglip_text_output_device": (vp, [vp, C.c_int]),
    "mse_siglip_text_stream": (vp, [vp]),
}


class PartitionConfig(C.Structure):
    """mse_partition_config (include/mse.h)"""
    _fields_ = [("temperature0", C.c_float), ("accept_decay", C.c_float), ("reject_decay", C.c_float), ("reroll_heat", C.c_float),
                ("temperature_cap", C.c_float), ("reroll_after", C.c_uint32), ("seed", C.c_uint32), ("stop_fraction", C.c_double)]


class PartitionState(C.Structure):
    """mse_partition_status (include/mse.h)"""
    _fields_ = [("t", C.c_uint64), ("last_fitness", C.c_uint64), ("last_improvement", C.c_uint64), ("temperature", C.c_float),
                ("stopped", C.c_uint32)]


class SiglipTextConfig(C.Structure):
    """mse_siglip_text_config (include/mse.h)"""
    _fields_ = [("width", C.c_int), ("layers", C.c_int), ("heads", C.c_int), ("mlp_dim", C.c_int),
                ("context_length", C.c_int), ("vocab_size", C.c_int), ("eps", C.c_float), ("gelu_tanh", C.c_int),
                ("max_batch", C.c_int)]


class SiglipConfig(C.Structure):
    """mse_siglip_config (include/mse.h)"""
    _fields_ = [("img_size", C.c_int), ("patch_size", C.c_int), ("in_chans", C.c_int), ("emb_dim", C.c_int),
                ("depth", C.c_int), ("num_heads", C.c_int), ("mlp_dim", C.c_int), ("eps", C.c_float),
                ("gelu_tanh", C.c_int), ("max_batch", C.c_int)]


class DebugSiglipGemmArgs(C.Structure):
    """mse_debug_siglip_gemm_args (include/mse.h)"""
    _fields_ = ([(n, C.c_int) for n in ("rows", "N", "K", "epi", "skinny", "gelu_tanh", "flags", "n_valid", "tokens", "heads", "dh", "ksplit")] +
                [(n, f32p) for n in ("x", "w", "bias", "resid", "pos", "out", "q", "k", "vt")] +
                [(n, C.c_int) for n in ("M", "n_pad", "n_seq", "dh_pad", "kdh_pad", "dv_pad", "slab_rows", "cu_count")])


class DebugSiglipGemmFusedArgs(C.Structure):
    """mse_debug_siglip_gemm_fused_args (include/mse.h)"""
    _fields_ = ([(n, C.c_int) for n in ("rows", "N", "K", "epi", "gelu_tanh", "flags", "n_valid", "heads", "dh", "tokens")] +
                [("eps", C.c_float)] +
                [(n, f32p) for n in ("x", "w", "bias", "gamma", "beta", "xres", "out", "q", "k", "vt", "stats")] +
                [(n, C.c_int) for n in ("M", "n_pad", "n_seq", "dh_pad", "kdh_pad", "dv_pad")])


class DebugSiglipLayernormArgs(C.Structure):
    """mse_debug_siglip_layernorm_args (include/mse.h)"""
    _fields_ = ([(n, C.c_int) for n in ("rows", "width", "ldx", "x_is_f16", "ldd", "n_parts", "part_rows", "ldp", "ldo", "wg")] +
                [("eps", C.c_float)] +
                [(n, f32p) for n in ("x", "delta", "parts", "bias", "gamma", "beta", "x_out", "out", "out_f32")])


def lib():
    """Load libmse_hip.so; raises MseError if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise MseError(
                f"{LIB_PATH} is missing: build it with __graft_entry__.build() "
                "(make -C meme-search-engine_amd/csrc).  There is no CPU fallback.")
        try:
            L = C.CDLL(LIB_PATH)
        except OSError as e:  # pragma: no cover - depends on the machine
            raise MseError(f"cannot load {LIB_PATH}: {e}") from e
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def last_error():
    msg = lib().mse_last_error()
    return msg.decode("utf-8", "replace") if msg else ""


def check(rc, what="call"):
    if rc != 0:
        raise MseError(f"{what} failed: {last_error()}")


def check_ptr(p, what="call"):
    if not p:
        raise MseError(f"{what} failed: {last_error()}")
    return p
