"""ctypes binding of include/inferflow_amd.h.  Fails loudly when the HIP
library is missing -- there is no CPU fallback on the product path."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# IFA_LIB: another build of the SAME library (tools/sweep_variants.py: one .so per tuning setting); tuning only
_LIB_PATH = os.environ.get("IFA_LIB") or os.path.join(_HERE, "lib", "libinferflow_amd.so")
_lib = None


class IfaError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("inferflow_amd error %d: %s" % (code, msg))
        self.code = code


def library_path():
    return _LIB_PATH


def lib():
    """Load libinferflow_amd.so (built by inferflow_amd/build.py / __graft_entry__.build())."""
    global _lib
    if _lib is None:
        if not os.path.exists(_LIB_PATH):
            raise ImportError(
                "inferflow_amd: %s is missing -- run `python __graft_entry__.py build` "
                "(hipcc --offload-arch=gfx950); there is no CPU fallback" % _LIB_PATH)
        L = C.CDLL(_LIB_PATH, mode=C.RTLD_GLOBAL)
        _declare(L)
        _lib = L
    return _lib


def check(rc):
    if rc != 0:
        raise IfaError(rc, lib().ifa_last_error().decode(errors="replace"))
    return rc


_vp, _sz, _i, _f = C.c_void_p, C.c_size_t, C.c_int, C.c_float

# name -> (restype, argtypes); mirrors include/inferflow_amd.h one to one
SIGNATURES = {
    "ifa_version": (C.c_char_p, []),
    "ifa_last_error": (C.c_char_p, []),
    "ifa_device_count": (_i, []),
    "ifa_set_device": (_i, [_i]),
    "ifa_malloc": (_i, [C.POINTER(_vp), _sz]),
    "ifa_free": (_i, [_vp]),
    "ifa_memcpy_h2d": (_i, [_vp, _vp, _sz, _vp]),
    "ifa_memcpy_d2h": (_i, [_vp, _vp, _sz, _vp]),
    "ifa_memcpy_d2d": (_i, [_vp, _vp, _sz, _vp]),
    "ifa_memset": (_i, [_vp, _i, _sz, _vp]),
    "ifa_stream_create": (_i, [C.POINTER(_vp)]),
    "ifa_stream_destroy": (_i, [_vp]),
    "ifa_stream_sync": (_i, [_vp]),
    "ifa_block_capacity": (_i, [_i]),
    "ifa_block_bytes": (_i, [_i]),
    "ifa_row_bytes": (_sz, [_i, _sz]),
    "ifa_dtype_from_name": (_i, [C.c_char_p]),
    "ifa_quantize": (_i, [_i, _vp, _sz, _sz, _vp, _vp]),
    "ifa_quantize_f32": (_i, [_i, _vp, _sz, _sz, _vp, _vp]),
    "ifa_dequantize": (_i, [_i, _vp, _sz, _sz, _vp, _vp]),
    "ifa_quantize_act_q8": (_i, [_vp, _sz, _sz, _vp, _vp]),
    "ifa_gemv": (_i, [_i, _vp, _sz, _sz, _i, _vp, _vp, _vp, _vp]),
    "ifa_gemm": (_i, [_i, _vp, _sz, _sz, _vp, _sz, _vp, _vp, _vp]),
    "ifa_attention_two_pass_min": (_i, [_i]),
    "ifa_attention_two_pass_min_keys": (_i, [_i]),
    "ifa_attention_rows": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _f, _i, _i, _i, _vp, _vp]),
    "ifa_attention_plan": (_i, [_vp, _i, _vp, _i]),
    "ifa_gemm_big_tiles": (_i, [_i]),
    "ifa_wait_grid_decision": (_i, [_i, _i, C.c_longlong]),
    "ifa_visible_cus_from_mask": (_i, [C.c_char_p, _i, _i]),
    "ifa_inlaunch_waits_enabled": (_i, []),
    "ifa_gemm_release_stream": (_i, [_vp]),
    "ifa_tiled_row_bytes": (_sz, [_i, _sz]),
    "ifa_repack_weights": (_i, [_i, _vp, _sz, _sz, _vp, _vp]),
    "ifa_gemv_tiled": (_i, [_i, _vp, _sz, _sz, _vp, _vp, _vp, _vp]),
    "ifa_layernorm": (_i, [_i, _vp, _sz, _sz, _vp, _vp, _f, _f, _vp, _vp]),
    "ifa_exact_rmsnorm": (_i, [_vp, _sz, _sz, _vp, _vp, _f, _f, _vp, _vp]),
    "ifa_exact_gemv": (_i, [_i, _vp, _sz, _sz, _i, _vp, _vp, _vp, _vp]),
    "ifa_exact_attention": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _f, _vp, _vp]),
    "ifa_exact_activation_mul": (_i, [_i, _vp, _vp, _sz, _vp, _vp]),
    "ifa_rope": (_i, [_vp, _i, _i, _i, _i, _f, _i, _f, _vp]),
    "ifa_alibi": (_i, [_vp, _i, _i, _i, _i, _i, _vp]),
    "ifa_softmax": (_i, [_vp, _i, _i, _i, _i, _f, _vp]),
    "ifa_activation": (_i, [_i, _i, _vp, _sz, _sz, _vp, _vp]),
    "ifa_mul": (_i, [_vp, _vp, _sz, _vp, _vp]),
    "ifa_add": (_i, [_vp, _vp, _sz, _sz, _vp, _vp]),
    "ifa_scale": (_i, [_vp, _f, _sz, _vp, _vp]),
    "ifa_attention": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _f, _i, _i, _i, _vp, _vp]),
    "ifa_moe_route_topk": (_i, [_vp, _sz, _i, _i, _i, _vp, _vp, _vp]),
    "ifa_moe_build_lists": (_i, [_vp, _vp, _sz, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ifa_moe_gather": (_i, [_vp, _vp, _vp, _sz, _sz, _vp, _vp]),
    "ifa_moe_combine": (_i, [_vp, _vp, _vp, _sz, _i, _sz, _vp, _vp, _vp]),
    "ifa_kv_store": (_i, [_i, _vp, _sz, _sz, _vp, _sz, _vp]),
    "ifa_argmax": (_i, [_vp, _sz, _vp, _vp]),
    "ifa_argmax_masked": (_i, [_vp, _sz, _vp, _vp, _vp]),
    "ifa_topk_pool": (_i, [_vp, _sz, _sz, _i, _vp, _vp, _vp, _vp, _vp]),
    "ifa_sample_pool_rows": (_i, [_vp, _vp, _vp, _sz, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ifa_sample_pool_host": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ifa_sample_verify_rows": (_i, [_vp, _vp, _vp, _sz, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ifa_sample_verify_host": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ifa_logsumexp_workspace": (_sz, [_sz, _sz]),
    "ifa_logsumexp_rows": (_i, [_vp, _sz, _vp, _sz, _sz, _vp, _vp, _vp, _vp, _vp]),
    "ifa_logit_adjust_rows": (_i, [_vp, _sz, _vp, _vp, _sz, _sz, _vp, _vp, _vp, _vp, _vp]),
    "ifa_logit_adjust_draft_rows": (_i, [_vp, _sz, _vp, _sz, _sz, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ifa_logit_state_reset": (_i, [_i, _vp, _sz, _f, _f, _f, _vp, _vp, _sz, _sz, _vp, _vp, _vp, _vp]),
    "ifa_logit_state_add": (_i, [_vp, _vp, _sz, _sz, _sz, _vp, _vp]),
    "ifa_batch_feed_rows": (_i, [_vp, _vp]),
    "ifa_batch_feed_host": (_i, [_vp]),
    "ifa_batch_clamp_counts": (_i, [_vp, _vp, _sz, _vp]),
    "ifa_model_create": (_i, [_vp, C.POINTER(_vp)]),
    "ifa_model_destroy": (_i, [_vp]),
    "ifa_debug_alloc_fail_at": (_i, [C.c_longlong]),
    "ifa_debug_live_allocs": (_i, [C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]),
    "ifa_model_set_tensor": (_i, [_vp, _i, _i, _i, _i, _vp, _sz, _sz]),
    "ifa_model_set_tensor_f16": (_i, [_vp, _i, _i, _i, _i, _vp, _sz, _sz]),
    "ifa_model_finalize": (_i, [_vp]),
    "ifa_model_reset": (_i, [_vp]),
    "ifa_model_set_option": (_i, [_vp, C.c_char_p, _i]),
    "ifa_model_set_excluded_tokens": (_i, [_vp, _vp, _i]),
    "ifa_model_perf_stat": (_i, [_vp, _vp, _vp, _i, _vp, _i]),
    "ifa_model_fused_supported": (_i, [_vp, C.c_char_p, _sz]),
    "ifa_model_forward": (_i, [_vp, _vp, _i, _i, _vp, _vp]),
    "ifa_model_decode": (_i, [_vp, _i, _i, _i, _vp, _vp]),
    "ifa_model_decode_sampled": (_i, [_vp, _i, _i, _i, _vp, _vp, _i, _vp, _vp]),
    "ifa_model_decode_prepare": (_i, [_vp, _i, _i]),
    "ifa_add_by_row_index": (_i, [_vp, _vp, _sz, _sz, _vp, _vp, _vp]),
    "ifa_model_kv_slots": (_i, [_vp, _i]),
    "ifa_model_select_kv": (_i, [_vp, _i]),
    "ifa_model_kv_copy": (_i, [_vp, _i, _i, _i]),
    "ifa_model_kv_shift": (_i, [_vp, _i, _i, _i, _i]),
    "ifa_kv_shift_rows": (_i, [_i, _vp, _vp, _sz, _sz, _i, _i, _vp, _sz, _sz, _sz, _vp]),
    "ifa_model_decode_batch": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _vp]),
    "ifa_model_decode_draft": (_i, [_vp, _i, _vp, _i, _vp, _vp]),
    "ifa_model_decode_draft_sampled": (_i, [_vp, _i, _vp, _i, _vp, _vp, _i, _vp, _vp]),
    "ifa_model_set_pool_excluded": (_i, [_vp, _vp, _i]),
    "ifa_model_decode_pool": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "ifa_model_decode_batch_pool": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _i, _vp, _i, _vp, _vp, _vp]),
    "ifa_model_forward_pool": (_i, [_vp, _vp, _i, _i, _vp, _i, _vp, _vp, _vp, _vp]),
    "ifa_model_pool_lse": (_i, [_vp, _vp, _i, _vp]),
    "ifa_model_logit_state_reset": (_i, [_vp, _i, _vp, _i, _f, _f, _f, _vp, _vp, _i]),
    "ifa_model_logit_state_add": (_i, [_vp, _i, _vp, _vp]),
    "ifa_model_pool_adjust": (_i, [_vp, _i, _vp]),
    "ifa_model_decode_batch_steps": (_i, [_vp, _i, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp]),
    "ifa_model_batch_steps_rows": (_i, [_vp]),
    "ifa_model_forward_score": (_i, [_vp, _vp, _i, _i, _vp, _vp, _vp, _vp]),
    "ifa_model_get_buffer": (_i, [_vp, C.c_char_p, _i, C.POINTER(_vp), C.POINTER(_sz)]),
    "ifa_model_stream": (_vp, [_vp]),
    "ifa_model_time_kernel": (_i, [_vp, _i, _i, _vp]),
    "ifa_decode_route_plan": (_i, [_vp, _i, _vp, _i]),
    "ifa_model_decode_route": (_i, [_vp, _vp, _i]),
    "ifa_decode_gemv_plan": (_i, [_vp, _i, _vp, _i]),
    "ifa_model_gemv_plan": (_i, [_vp, _i, _i, _vp, _i]),
    "ifa_prompt_route_plan": (_i, [_vp, _i, _vp, _i]),
    "ifa_batch_route_plan": (_i, [_vp, _i, _vp, _i]),
    "ifa_model_prompt_route": (_i, [_vp, _vp, _i]),
    "ifa_gemm_mid_plan": (_i, [_vp, _i, _vp, _i]),
    "ifa_gemm_big_plan": (_i, [_vp, _i, _vp, _i]),
    "ifa_gemm_rows_plan": (_i, [_vp, _i, _vp, _i]),
    "ifa_moe_plan": (_i, [_vp, _i, _vp, _i]),
    "ifa_pool_rows_plan": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _i, _vp, _vp]),
    "ifa_model_moe_plan": (_i, [_vp, _i, _i, _i, _vp, _i]),
    "ifa_gemm_rows_launches": (_i, [_vp, _i]),
    "ifa_debug_gemm_rows_record": (_i, [_vp, _i, _i]),
    "ifa_model_set_stream": (_i, [_vp, _vp]),
    "ifa_model_tp_begin": (_i, [_vp, _i, _i]),
    "ifa_model_tp_begin_hidden": (_i, [_vp, _vp, _i]),
    "ifa_model_tp_hidden": (_i, [_vp, _vp]),
    "ifa_model_tp_attn": (_i, [_vp, _i, _vp]),
    "ifa_model_tp_post_attn": (_i, [_vp, _i, _vp]),
    "ifa_model_tp_ffn": (_i, [_vp, _i, _vp]),
    "ifa_model_tp_post_ffn": (_i, [_vp, _i, _vp]),
    "ifa_model_tp_logits": (_i, [_vp, _vp]),
    "ifa_model_tp_set_token": (_i, [_vp, _vp]),
    "ifa_comm_unique_id": (_i, [_vp]),
    "ifa_comm_init_rank": (_i, [_vp, _i, _i, _i, C.POINTER(_vp)]),
    "ifa_comm_init_all": (_i, [_vp, _i, C.POINTER(_vp)]),
    "ifa_comm_destroy": (_i, [_vp]),
    "ifa_comm_capturable": (_i, [_vp]),
    "ifa_comm_serial": (C.c_ulonglong, [_vp]),
    "ifa_comm_abort": (_i, [_vp]),
    "ifa_comm_oneshot": (_i, [_vp]),
    "ifa_comm_oneshot_export": (_i, [_vp, _vp]),
    "ifa_comm_oneshot_import": (_i, [_vp, _vp]),
    "ifa_comm_set_oneshot": (_i, [_vp, _i]),
    "ifa_comm_status": (_i, [_vp]),
    "ifa_comm_rank": (_i, [_vp]),
    "ifa_comm_size": (_i, [_vp]),
    "ifa_comm_group_start": (_i, []),
    "ifa_comm_group_end": (_i, []),
    "ifa_allreduce_sum_f16": (_i, [_vp, _vp, _vp, _sz, _vp]),
    "ifa_allgather": (_i, [_vp, _vp, _vp, _sz, _vp]),
    "ifa_broadcast": (_i, [_vp, _vp, _sz, _i, _vp]),
    "ifa_send": (_i, [_vp, _vp, _sz, _i, _vp]),
    "ifa_recv": (_i, [_vp, _vp, _sz, _i, _vp]),
    "ifa_model_tp_decode": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp]),
    "ifa_model_tp_prefill": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp]),
    "ifa_model_tp_decode_batch": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _vp, _vp]),
    "ifa_model_get_tensor": (_i, [_vp, _i, _i, _vp, C.POINTER(_vp), C.POINTER(_sz), C.POINTER(_sz)]),
    "ifa_model_get_expert_tensor": (_i, [_vp, _i, _i, _i, _vp, C.POINTER(_vp), C.POINTER(_sz), C.POINTER(_sz)]),
}


# include/inferflow_engine.h (the C++ InferenceEngine facade)
_ip = C.POINTER(C.c_int)
ENGINE_SIGNATURES = {
    "ifa_engine_create": (_vp, [C.c_char_p, C.c_char_p, C.c_char_p]),
    "ifa_engine_destroy": (None, [_vp]),
    "ifa_engine_last_error": (C.c_char_p, []),
    "ifa_engine_add_query": (_i, [_vp, _ip, _i]),
    "ifa_engine_add_query_ex": (_i, [_vp, _ip, _i, _i, _i, _f]),
    "ifa_engine_add_query_lp": (_i, [_vp, _ip, _i, _i, _i, _f, _i]),
    "ifa_engine_add_query_opt": (_i, [_vp, _ip, _i, _vp]),
    "ifa_engine_last_logprobs": (_i, [_vp, _i, C.POINTER(_f), _ip, C.POINTER(_f), _i, _ip]),
    "ifa_engine_score": (_i, [_vp, _ip, _i, C.POINTER(_f)]),
    "ifa_engine_strategy_id": (_i, [_vp, C.c_char_p]),
    "ifa_sampling_choose": (_i, [_vp, _i, _i, _i, _f, _i, _f, C.c_longlong, _i, _ip, C.POINTER(_f), _ip, C.POINTER(_f), _i]),
    "ifa_sampling_choose_ex": (_i, [_vp, _i, _i, C.POINTER(_f), _f, C.c_longlong, _i, _ip, C.POINTER(_f), _ip, C.POINTER(_f), _i, C.POINTER(_f), _ip, _i]),
    "ifa_sampling_choose_from_pool": (_i, [_ip, _vp, _i, _i, C.POINTER(_f), _f, C.c_longlong, _i, _ip, C.POINTER(_f), _ip, C.POINTER(_f), _i, C.POINTER(_f), _ip, _i]),
    "ifa_sampling_random_doubles": (_i, [C.c_longlong, _i, C.POINTER(C.c_double)]),
    "ifa_engine_query_count": (_i, [_vp]),
    "ifa_engine_remove_query": (_i, [_vp, _i]),
    "ifa_engine_infer": (_i, [_vp, _ip, _ip, _i]),
    "ifa_engine_commit": (_i, [_vp, _ip, _ip, _ip, _i]),
    "ifa_engine_last_logits": (_i, [_vp, _i, _vp, _sz, _ip, _ip]),
    "ifa_engine_perf_stat": (_i, [_vp, _vp, _vp, _i]),
    "ifa_engine_generate": (_i, [_vp, _i, _i, _ip, C.POINTER(_f)]),
    "ifa_engine_generate_batch": (_i, [_vp, _i, _ip, _ip, _ip, _ip, _ip, _ip, _ip, _ip, C.POINTER(_f)]),
    "ifa_generate_batch_plan": (_i, [_ip, _i, _ip, _i]),
    "ifa_engine_generate_lookup": (_i, [_vp, _i, _i, _ip, _i, _ip, C.POINTER(_f)]),
    "ifa_lookup_draft": (_i, [_ip, _i, _ip, _i, _i, _i, _i, _ip]),
    "ifa_engine_perplexity": (_i, [_vp, _ip, _i, _i, _i, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_longlong)]),
    "ifa_engine_perplexity_device": (_i, [_vp, _ip, _i, _i, _i, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_longlong)]),
    "ifa_perplexity_token_nll": (C.c_double, [_vp, _i, _i]),
    "ifa_engine_model_info": (_i, [_vp, C.c_char_p]),
    "ifa_engine_query_cached_tokens": (_i, [_vp, _i]),
    "ifa_context_shift_plan": (_i, [_i, _i, _i, _i, _ip]),
    "ifa_engine_shift_query": (_i, [_vp, _i, _i, _i]),
    "ifa_engine_query_shifted_tokens": (_i, [_vp, _i]),
    "ifa_engine_query_rng_state": (_i, [_vp, _i, _vp]),
    "ifa_prefix_cache_plan": (_i, [_ip, _ip, _ip, C.POINTER(C.c_longlong), _i, _ip, _i, _i, _ip]),
    "ifa_step_plan_query": (_i, [_i, _i, _i, _i, _i, _ip]),
    "ifa_step_plan_batch": (_i, [_i, _ip, _i, _ip, _ip]),
    "ifa_engine_worker": (_vp, [_vp, _i]),
    "ifa_engine_worker_plan": (_i, [_vp, _i, _ip]),
    "ifa_service_parse_request": (_i, [C.c_char_p, _i, C.c_char_p, _sz]),
    "ifa_service_format_response": (_i, [_ip, _i, _i, _i, _i, _i, C.c_char_p, _sz]),
    "ifa_service_selftest_loop": (_i, [_i, _i, _i, _ip, _i, _i, _i, _i, _i, C.c_char_p, _sz]),
    "ifa_service_selftest_request": (_i, [C.c_char_p, _i, _i, C.c_char_p, _sz]),
    "ifa_partition_slice": (_i, [_i, _i, _i, _i, _i, _i, _i, _i, _sz, _sz, C.POINTER(_sz)]),
    "ifa_partition_split_layers": (_i, [_i, _i, _ip, _i]),
}


class QueryOptions(C.Structure):
    """ifa_query_options (include/inferflow_engine.h); struct_size is filled in by InferenceEngine.add_query"""
    _fields_ = [("struct_size", C.c_size_t), ("strategy_id", C.c_int), ("random_seed", C.c_int), ("temperature", C.c_float),
                ("logprobs", C.c_int), ("repetition_penalty", C.c_float), ("presence_penalty", C.c_float),
                ("frequency_penalty", C.c_float), ("n_logit_bias", C.c_int), ("logit_bias_ids", C.POINTER(C.c_int)),
                ("logit_bias_values", C.POINTER(C.c_float))]


class QueryOptionsShift(C.Structure):
    """ifa_query_options as it has grown: the fields of QueryOptions, then context_shift / context_keep (-1: the engine's keys).
    QueryOptions stays the shorter, earlier struct -- struct_size tells the library which one it was handed."""
    _fields_ = QueryOptions._fields_ + [("context_shift", C.c_int), ("context_keep", C.c_int)]


class SampleParams(C.Structure):
    """ifa_sample_params (include/inferflow_amd.h)"""
    _fields_ = [("strategy_id", C.c_int), ("temperature", C.c_float), ("top_p", C.c_float), ("max_k", C.c_int), ("min_p", C.c_float), ("pool_size", C.c_int)]


class BatchRow(C.Structure):
    """ifa_batch_row (include/inferflow_amd.h): one row of ifa_model_decode_batch_steps"""
    _fields_ = [("struct_size", C.c_int), ("p", SampleParams), ("state_slot", C.c_int), ("rng_state", C.c_ulonglong), ("n_stop", C.c_int),
                ("stop_ids", C.c_int * 8), ("reserved", C.c_int)]


class BatchFeedArgs(C.Structure):
    """ifa_batch_feed_args (include/inferflow_amd.h): the arrays of one feed, all on the device or all on the host"""
    _fields_ = [(n, C.c_int) for n in ("struct_size", "n", "layers", "ring_steps", "k_stride", "reserved")] + [(n, C.c_void_p) for n in (
        "rows", "step", "argmax", "pool_counts", "pool_ids", "drawn", "rng", "tok", "pos", "attn_rows", "ring", "pair_slot", "pair_tok", "err")]


class ModelConfig(C.Structure):
    """ifa_model_config (include/inferflow_amd.h)"""
    _fields_ = [(n, C.c_int) for n in (
        "dim", "layers", "heads", "kv_heads", "head_dim", "ffn", "vocab", "max_ctx",
        "norm_kind", "act_kind", "is_glu", "rope_order", "use_alibi", "parallel_attn",
        "share_input")] + [(n, C.c_float) for n in (
            "rope_theta", "partial_rotary", "kq_scale", "eps")] + [(n, C.c_int) for n in (
                "kv_dtype", "full_quant_gemv", "experts", "moe_top_k", "moe_norm_topk",
                "tp_rank", "tp_size", "device")] + [(n, C.c_float) for n in (
                    "attn_norm_base", "ffn_norm_base", "out_norm_base", "attn_out_scale", "ffn_out_scale", "out_scale", "embd_scale")]


def _declare(L):
    missing = []
    for name, (res, args) in list(SIGNATURES.items()) + list(ENGINE_SIGNATURES.items()):
        try:
            fn = getattr(L, name)
        except AttributeError:
            missing.append(name)
            continue
        fn.restype = res
        fn.argtypes = args
    if missing and os.environ.get("IFA_LIB"):
        return      # a tuning build (tools/sweep_variants.py) may predate the newest entry points; bench.py does not call them
    if missing:
        raise ImportError("libinferflow_amd.so lacks symbols declared in include/*.h: %s" % missing)
