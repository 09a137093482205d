"""Build and loading of the native code: libfa_fwd_gfx950.so (the C-ABI of include/fa_fwd.h, fa_bwd.h, fa_rotary.h, fa_norm.h, fa_xent.h, fa_act.h, fa_gemm_act.h, fa_dropout_norm.h, fa_sample.h, fa_spec_sample.h, fa_tree_sample.h, fa_block_select.h and fa_block_pattern.h) and
the compiled host module flash_attn_2_cuda_C (csrc/torch_binding.cpp), which is the only host path of both operator
surfaces.  Python launches nothing through ctypes: the struct mirrors below serve the ABI tests, `bench.py --variant`
and the developer tools, which call the C-ABI directly.

The shared library is the product: there is no Python/CPU fallback.  If it is
missing or the GPU is absent, every compute entry point raises.
"""
import ctypes
import os
import subprocess
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_NAME = "libfa_fwd_gfx950.so"
LIB_PATH = os.path.join(_HERE, LIB_NAME)
CSRC = os.path.join(_HERE, "csrc")
INCLUDE = os.path.join(os.path.dirname(_HERE), "include")

FA_ABI_VERSION = 13
FA_FLAG_FA3_WINDOW = 1
FA_FLAG_SDMASK_SIGNED = 2
FA_FLAG_PACK_GQA = 4
FA_DTYPE_FP16, FA_DTYPE_BF16, FA_DTYPE_FP8_E4M3, FA_DTYPE_FP32 = 0, 1, 2, 3

# every symbol include/fa_fwd.h declares (tests check the .so exports all of them)
EXPORTED_SYMBOLS = (
    "fa_fwd",
    "fa_fwd_validate",
    "fa_fwd_workspace_size",
    "fa_fwd_plan_name",
    "fa_fwd_last_plan_name",
    "fa_strerror",
    "fa_fwd_params_size",
    "fa_abi_version",
    "fa_fwd_tile_shape",
    "fa_set_default_variant",
    "fa_set_persist_mode",
    "fa_kvcache_append",
    "fa_kvcache_append_params_size",
    "fa_rotary_apply",
    "fa_rotary_params_size",
    "fa_kvcache_append_varlen",
    "fa_kvcache_append_varlen_params_size",
    "fa_rotary_apply_varlen",
    "fa_rotary_varlen_params_size",
    "fa_fwd_combine",
    "fa_combine_params_size",
    "fa_fwd_sink",
    "fa_fwd_sink_validate",
    "fa_sink_params_size",
    "fa_fwd_block_sparse",
    "fa_fwd_block_sparse_validate",
    "fa_block_sparse_params_size",
    "fa_fwd_kv8",
    "fa_fwd_kv8_validate",
    "fa_fwd_kv8_workspace_size",
    "fa_fwd_kv8_plan_name",
    "fa_fwd_qv8",
    "fa_fwd_qv8_validate",
    "fa_fwd_qv8_workspace_size",
    "fa_fwd_qv8_plan_name",
    "fa_kvcache_append_kv8",
    "fa_kvcache_append_kv8_validate",
    "fa_kvcache_append_kv8_params_size",
    "fa_kvcache_append_qv8",
    "fa_kvcache_append_qv8_validate",
    "fa_fwd_sparse_kv",
    "fa_fwd_sparse_kv_validate",
    "fa_fwd_sparse_kv_workspace_size",
    "fa_fwd_sparse_kv_plan_name",
    "fa_sparse_kv_params_size",
    "fa_fwd_tree",
    "fa_fwd_tree_validate",
    "fa_fwd_tree_workspace_size",
    "fa_fwd_tree_plan_name",
    "fa_tree_params_size",
    # include/fa_bwd.h
    "fa_bwd",
    "fa_bwd_validate",
    "fa_bwd_params_size",
    "fa_bwd_plan_name",
    "fa_bwd_last_plan_name",
    "fa_sink_grad",
    "fa_sink_grad_validate",
    "fa_sink_grad_params_size",
    "fa_bwd_block_sparse",
    "fa_bwd_block_sparse_validate",
    "fa_block_sparse_bwd_params_size",
)
# every symbol include/fa_rotary.h declares (csrc/fa_rotary_emb.hip)
ROTARY_EMB_SYMBOLS = ("fa_rotary_emb", "fa_rotary_emb_validate", "fa_rotary_emb_params_size")
# every symbol include/fa_norm.h declares (csrc/fa_norm.hip)
NORM_SYMBOLS = ("fa_norm_fwd", "fa_norm_fwd_validate", "fa_norm_fwd_params_size", "fa_norm_bwd", "fa_norm_bwd_validate",
                "fa_norm_bwd_params_size", "fa_norm_bwd_workspace_bytes", "fa_norm_fwd_plan", "fa_norm_bwd_plan")
FA_NORM_RMS, FA_NORM_ZERO_CENTERED = 1, 2
# every symbol include/fa_xent.h declares (csrc/fa_xent.hip)
XENT_SYMBOLS = ("fa_xent_fwd", "fa_xent_fwd_validate", "fa_xent_fwd_params_size", "fa_xent_bwd", "fa_xent_bwd_validate",
                "fa_xent_bwd_params_size", "fa_xent_fwd_plan", "fa_xent_bwd_plan")
FA_XENT_PRECOMPUTED_LSE, FA_XENT_SPLIT = 1, 2
FA_XENT_LABELS_INT64, FA_XENT_LABELS_INT32 = 0, 1
# every symbol include/fa_act.h declares (csrc/fa_act.hip)
ACT_SYMBOLS = ("fa_act_fwd", "fa_act_fwd_validate", "fa_act_fwd_params_size", "fa_act_bwd", "fa_act_bwd_validate",
               "fa_act_bwd_params_size", "fa_act_bwd_workspace_bytes", "fa_act_fwd_plan", "fa_act_bwd_plan")
FA_ACT_GELU_TANH, FA_ACT_GELU_ERF, FA_ACT_RELU, FA_ACT_SQRELU, FA_ACT_SILU, FA_ACT_SIGMOID, FA_ACT_IDENTITY = range(7)
FA_ACT_GATED = 1
# every symbol include/fa_gemm_act.h declares (csrc/fa_gemm_act.hip)
GEMM_ACT_SYMBOLS = ("fa_gemm_act_fwd", "fa_gemm_act_fwd_validate", "fa_gemm_act_fwd_params_size", "fa_gemm_act_dgrad",
                    "fa_gemm_act_dgrad_validate", "fa_gemm_act_dgrad_params_size", "fa_gemm_act_dgrad_workspace_bytes",
                    "fa_gemm_act_fwd_plan", "fa_gemm_act_dgrad_plan")
# every symbol include/fa_dropout_norm.h declares (csrc/fa_dropout_norm.hip)
DROPOUT_NORM_SYMBOLS = ("fa_dropout_norm_fwd", "fa_dropout_norm_fwd_validate", "fa_dropout_norm_fwd_params_size",
                        "fa_dropout_norm_bwd", "fa_dropout_norm_bwd_validate", "fa_dropout_norm_bwd_params_size",
                        "fa_dropout_norm_bwd_workspace_bytes", "fa_dropout_norm_fwd_plan", "fa_dropout_norm_bwd_plan")
FA_DROPOUT_NORM_RMS = 1
# every symbol include/fa_sample.h declares (csrc/fa_sample.hip)
SAMPLE_SYMBOLS = ("fa_sample", "fa_sample_validate", "fa_sample_params_size", "fa_sample_plan")
FA_SAMPLE_DRAW, FA_SAMPLE_FILTER = 0, 1
# every symbol include/fa_spec_sample.h declares (csrc/fa_spec_sample.hip)
SPEC_SAMPLE_SYMBOLS = ("fa_spec_sample", "fa_spec_sample_validate", "fa_spec_sample_params_size", "fa_spec_sample_workspace_size",
                       "fa_spec_sample_plan")
FA_SPEC_TOKENS_INT32, FA_SPEC_TOKENS_INT64 = 0, 1
FA_SPEC_RECORD_BYTES = 24
# every symbol include/fa_tree_sample.h declares (csrc/fa_tree_sample.hip)
TREE_SAMPLE_SYMBOLS = ("fa_tree_sample", "fa_tree_sample_validate", "fa_tree_sample_params_size", "fa_tree_sample_workspace_size",
                       "fa_tree_sample_plan")
FA_TREE_TOKENS_INT32, FA_TREE_TOKENS_INT64 = 0, 1
FA_TREE_RECORD_BYTES, FA_TREE_SAMPLE_MAX_NODES = 24, 64
# every symbol include/fa_block_select.h declares (csrc/fa_block_select.hip)
BLOCK_SELECT_SYMBOLS = tuple(f"fa_block_{unit}{suffix}" for unit in ("summary_update", "select")
                             for suffix in ("", "_validate", "_workspace_size", "_plan_name")) + (
    "fa_block_summary_params_size", "fa_block_select_params_size")
FA_BLOCK_REDUCE_MAX, FA_BLOCK_REDUCE_SUM = 0, 1
FA_BLOCK_SELECT_MAX_BLOCKS, FA_BLOCK_SELECT_MAX_ROWS = 8192, 128
# every symbol include/fa_block_pattern.h declares (csrc/fa_block_pattern.hip)
BLOCK_PATTERN_SYMBOLS = ("fa_block_pattern", "fa_block_pattern_validate", "fa_block_pattern_workspace_size", "fa_block_pattern_plan_name",
                         "fa_block_pattern_params_size")
FA_BLOCK_PATTERN_BLOCK, FA_BLOCK_PATTERN_MAX_BLOCKS = 128, 8192


class FaFwdParams(ctypes.Structure):
    """Field-for-field mirror of `struct fa_fwd_params` (include/fa_fwd.h)."""

    _fields_ = [
        ("abi_version", ctypes.c_uint32),
        ("struct_size", ctypes.c_uint32),
        ("q", ctypes.c_void_p),
        ("k", ctypes.c_void_p),
        ("v", ctypes.c_void_p),
        ("o", ctypes.c_void_p),
        ("softmax_lse", ctypes.c_void_p),
        ("q_batch_stride", ctypes.c_int64),
        ("q_row_stride", ctypes.c_int64),
        ("q_head_stride", ctypes.c_int64),
        ("k_batch_stride", ctypes.c_int64),
        ("k_row_stride", ctypes.c_int64),
        ("k_head_stride", ctypes.c_int64),
        ("v_batch_stride", ctypes.c_int64),
        ("v_row_stride", ctypes.c_int64),
        ("v_head_stride", ctypes.c_int64),
        ("o_batch_stride", ctypes.c_int64),
        ("o_row_stride", ctypes.c_int64),
        ("o_head_stride", ctypes.c_int64),
        ("b", ctypes.c_int32),
        ("seqlen_q", ctypes.c_int32),
        ("seqlen_k", ctypes.c_int32),
        ("h", ctypes.c_int32),
        ("h_k", ctypes.c_int32),
        ("d", ctypes.c_int32),
        ("total_q", ctypes.c_int32),
        ("dtype", ctypes.c_int32),
        ("cu_seqlens_q", ctypes.c_void_p),
        ("cu_seqlens_k", ctypes.c_void_p),
        ("seqused_q", ctypes.c_void_p),
        ("seqused_k", ctypes.c_void_p),
        ("softmax_scale", ctypes.c_float),
        ("softcap", ctypes.c_float),
        ("is_causal", ctypes.c_int32),
        ("window_size_left", ctypes.c_int32),
        ("window_size_right", ctypes.c_int32),
        ("q_descale", ctypes.c_void_p),
        ("k_descale", ctypes.c_void_p),
        ("v_descale", ctypes.c_void_p),
        ("q_descale_batch_stride", ctypes.c_int64),
        ("q_descale_head_stride", ctypes.c_int64),
        ("k_descale_batch_stride", ctypes.c_int64),
        ("k_descale_head_stride", ctypes.c_int64),
        ("v_descale_batch_stride", ctypes.c_int64),
        ("v_descale_head_stride", ctypes.c_int64),
        ("kernel_variant", ctypes.c_int32),
        ("total_k", ctypes.c_int32),
        ("workspace", ctypes.c_void_p),
        ("workspace_bytes", ctypes.c_uint64),
        ("alibi_slopes", ctypes.c_void_p),
        ("alibi_slopes_batch_stride", ctypes.c_int64),
        ("kv_batch_idx", ctypes.c_void_p),
        ("block_table", ctypes.c_void_p),
        ("block_table_batch_stride", ctypes.c_int64),
        ("page_block_size", ctypes.c_int32),
        ("num_splits", ctypes.c_int32),
        ("leftpad_k", ctypes.c_void_p),
        ("p_dropout", ctypes.c_float),
        ("flags", ctypes.c_int32),
        ("rng_state", ctypes.c_void_p),
        ("s_dmask", ctypes.c_void_p),
        ("s_dmask_rows", ctypes.c_int32),
        ("s_dmask_cols", ctypes.c_int32),
        ("s_dmask_block_n", ctypes.c_int32),
        ("attention_chunk", ctypes.c_int32),
        ("d_v", ctypes.c_int32),
        ("reserved_v12", ctypes.c_int32),
        ("qv", ctypes.c_void_p),
        ("qv_batch_stride", ctypes.c_int64),
        ("qv_row_stride", ctypes.c_int64),
        ("qv_head_stride", ctypes.c_int64),
    ]


class FaCombineParams(ctypes.Structure):
    """Field-for-field mirror of `struct fa_combine_params` (include/fa_fwd.h)."""

    _fields_ = (
        [("abi_version", ctypes.c_uint32), ("struct_size", ctypes.c_uint32)]
        + [(n, ctypes.c_void_p) for n in ("out_partial", "lse_partial", "out", "softmax_lse")]
        + [(f"op_{s}_stride", ctypes.c_int64) for s in ("split", "batch", "row", "head")]
        + [(f"lp_{s}_stride", ctypes.c_int64) for s in ("split", "batch", "row", "head")]
        + [(f"o_{s}_stride", ctypes.c_int64) for s in ("batch", "row", "head")]
        + [(f"lse_{s}_stride", ctypes.c_int64) for s in ("batch", "row", "head")]
        + [(n, ctypes.c_int32) for n in ("num_splits", "b", "seqlen", "h", "d", "out_dtype")]
    )


class FaKvcacheAppendParams(ctypes.Structure):
    """Field-for-field mirror of `struct fa_kvcache_append_params` (include/fa_fwd.h)."""

    _fields_ = (
        [("abi_version", ctypes.c_uint32), ("struct_size", ctypes.c_uint32)]
        + [(n, ctypes.c_void_p) for n in ("k_new", "v_new", "k_cache", "v_cache")]
        + [(f"{t}_{s}_stride", ctypes.c_int64) for t in ("knew", "vnew", "kcache", "vcache")
           for s in ("batch", "row", "head")]
        + [(n, ctypes.c_int32) for n in ("b", "seqlen_new", "seqlen_cache", "h_k", "d", "reserved")]
        + [("cache_seqlens", ctypes.c_void_p), ("cache_batch_idx", ctypes.c_void_p)]
        + [("block_table", ctypes.c_void_p), ("block_table_batch_stride", ctypes.c_int64),
           ("page_block_size", ctypes.c_int32), ("dtype", ctypes.c_int32)]
        + [("rotary_cos", ctypes.c_void_p), ("rotary_sin", ctypes.c_void_p),
           ("rotary_dim", ctypes.c_int32), ("rotary_interleaved", ctypes.c_int32), ("rotary_seqlens", ctypes.c_void_p)]
        + [("d_v", ctypes.c_int32), ("reserved_v13", ctypes.c_int32)]
    )


class FaRotaryParams(ctypes.Structure):
    """Field-for-field mirror of `struct fa_rotary_params` (include/fa_fwd.h)."""

    _fields_ = (
        [("abi_version", ctypes.c_uint32), ("struct_size", ctypes.c_uint32), ("src", ctypes.c_void_p), ("dst", ctypes.c_void_p)]
        + [(f"{t}_{s}_stride", ctypes.c_int64) for t in ("src", "dst") for s in ("batch", "row", "head")]
        + [(n, ctypes.c_int32) for n in ("b", "s", "h", "d", "dtype", "rotary_dim", "rotary_interleaved", "per_row_positions")]
        + [("rotary_cos", ctypes.c_void_p), ("rotary_sin", ctypes.c_void_p), ("seqlen_offsets", ctypes.c_void_p)]
    )


class FaKvcacheAppendVarlenParams(ctypes.Structure):
    """Field-for-field mirror of `struct fa_kvcache_append_varlen_params` (include/fa_fwd.h)."""

    _fields_ = (
        [("abi_version", ctypes.c_uint32), ("struct_size", ctypes.c_uint32)]
        + [(n, ctypes.c_void_p) for n in ("k_new", "v_new", "k_cache", "v_cache")]
        + [(f"{t}_{s}_stride", ctypes.c_int64) for t in ("knew", "vnew") for s in ("row", "head")]
        + [(f"{t}_{s}_stride", ctypes.c_int64) for t in ("kcache", "vcache") for s in ("batch", "row", "head")]
        + [(n, ctypes.c_int32) for n in ("b", "total_k_new", "max_seqlen_k_new", "seqlen_cache", "h_k", "d", "d_v", "dtype")]
        + [(n, ctypes.c_void_p) for n in ("cu_seqlens_k_new", "cache_seqlens", "cache_batch_idx", "seqused_out", "block_table")]
        + [("block_table_batch_stride", ctypes.c_int64), ("page_block_size", ctypes.c_int32), ("rotary_dim", ctypes.c_int32)]
        + [(n, ctypes.c_void_p) for n in ("rotary_cos", "rotary_sin", "rotary_seqlens")]
        + [("rotary_interleaved", ctypes.c_int32), ("reserved", ctypes.c_int32)]
    )


class FaKvcacheAppendKv8Params(ctypes.Structure):
    """Field-for-field mirror of `struct fa_kvcache_append_kv8_params` (include/fa_fwd.h)."""

    _fields_ = (
        [("abi_version", ctypes.c_uint32), ("struct_size", ctypes.c_uint32)]
        + [(n, ctypes.c_void_p) for n in ("k_new", "v_new", "k_cache", "v_cache")]
        + [(f"{t}_{s}_stride", ctypes.c_int64) for t in ("knew", "vnew", "kcache", "vcache")
           for s in ("batch", "row", "head")]
        + [(n, ctypes.c_int32) for n in ("b", "seqlen_new", "total_k_new", "max_seqlen_k_new", "seqlen_cache", "h_k", "d", "d_v",
                                         "dtype", "page_block_size", "rotary_dim", "rotary_interleaved")]
        + [(n, ctypes.c_void_p) for n in ("cu_seqlens_k_new", "cache_seqlens", "cache_batch_idx", "seqused_out", "block_table")]
        + [("block_table_batch_stride", ctypes.c_int64)]
        + [(n, ctypes.c_void_p) for n in ("rotary_cos", "rotary_sin", "rotary_seqlens", "k_descale", "v_descale")]
        + [(f"{t}_descale_{s}_stride", ctypes.c_int64) for t in ("k", "v") for s in ("batch", "head")]
    )


class FaRotaryVarlenParams(ctypes.Structure):
    """Field-for-field mirror of `struct fa_rotary_varlen_params` (include/fa_fwd.h)."""

    _fields_ = (
        [("abi_version", ctypes.c_uint32), ("struct_size", ctypes.c_uint32), ("src", ctypes.c_void_p), ("dst", ctypes.c_void_p)]
        + [(f"{t}_{s}_stride", ctypes.c_int64) for t in ("src", "dst") for s in ("row", "head")]
        + [(n, ctypes.c_int32) for n in ("b", "total_q", "max_seqlen_q", "h", "d", "dtype", "rotary_dim", "rotary_interleaved",
                                         "per_row_positions", "reserved")]
        + [(n, ctypes.c_void_p) for n in ("rotary_cos", "rotary_sin", "cu_seqlens_q", "offsets")]
    )


class FaRotaryEmbParams(ctypes.Structure):
    """Field-for-field mirror of `struct fa_rotary_emb_params` (include/fa_rotary.h)."""

    _fields_ = (
        [("abi_version", ctypes.c_uint32), ("struct_size", ctypes.c_uint32), ("x", ctypes.c_void_p), ("out", ctypes.c_void_p)]
        + [(f"{t}_{s}_stride", ctypes.c_int64) for t in ("x", "out") for s in ("batch", "row", "head", "dim")]
        + [(n, ctypes.c_void_p) for n in ("cos", "sin", "cu_seqlens", "seqlen_offsets")]
        + [("seqlen_offset", ctypes.c_int64)]
        + [(n, ctypes.c_int32) for n in ("b", "seqlen", "total", "max_seqlen", "h", "d", "rotary_dim", "seqlen_ro", "dtype",
                                         "cos_dtype", "sin_dtype", "offsets_int64", "interleaved", "conjugate")]
    )


class FaNormFwdParams(ctypes.Structure):
    """Field-for-field mirror of `struct fa_norm_fwd_params` (include/fa_norm.h)."""

    _fields_ = (
        [("abi_version", ctypes.c_uint32), ("struct_size", ctypes.c_uint32)]
        + [(n, ctypes.c_void_p) for n in ("x", "residual", "weight", "bias", "rowscale", "y", "residual_out", "mean", "rstd")]
        + [(f"{t}_row_stride", ctypes.c_int64) for t in ("x", "residual", "y", "residual_out")]
        + [("M", ctypes.c_int64), ("N", ctypes.c_int32)]
        + [(f"{t}_dtype", ctypes.c_int32) for t in ("x", "residual", "residual_out", "weight", "bias", "y", "rowscale")]
        + [("eps", ctypes.c_float), ("flags", ctypes.c_int32)]
    )


class FaNormBwdParams(ctypes.Structure):
    """Field-for-field mirror of `struct fa_norm_bwd_params` (include/fa_norm.h)."""

    _fields_ = (
        [("abi_version", ctypes.c_uint32), ("struct_size", ctypes.c_uint32)]
        + [(n, ctypes.c_void_p) for n in ("x", "dy", "weight", "bias", "dresidual", "rowscale", "mean", "rstd", "dx", "dresidual_in",
                                          "dw", "db", "y", "workspace")]
        + [("workspace_bytes", ctypes.c_uint64)]
        + [(f"{t}_row_stride", ctypes.c_int64) for t in ("x", "dy", "dresidual", "dx", "dresidual_in", "y")]
        + [("M", ctypes.c_int64), ("N", ctypes.c_int32)]
        + [(f"{t}_dtype", ctypes.c_int32) for t in ("x", "dy", "weight", "bias", "dresidual", "dresidual_in", "dx", "y", "rowscale")]
        + [("eps", ctypes.c_float), ("flags", ctypes.c_int32)]
    )


class FaNormPlan(ctypes.Structure):
    """Field-for-field mirror of `struct fa_norm_plan` (include/fa_norm.h): the form a norm call takes."""

    _fields_ = [(n, ctypes.c_int32) for n in ("cw", "threads", "team_wave", "wide", "rows_per_wg", "grid_x", "grid_y")]


class FaDropoutNormFwdParams(ctypes.Structure):
    """Field-for-field mirror of `struct fa_dropout_norm_fwd_params` (include/fa_dropout_norm.h)."""

    _fields_ = (
        [("abi_version", ctypes.c_uint32), ("struct_size", ctypes.c_uint32)]
        + [(n, ctypes.c_void_p) for n in ("x0", "x1", "residual", "weight0", "bias0", "weight1", "bias1", "rowscale", "colscale",
                                          "rng_state", "z0", "z1", "x", "dmask0", "dmask1", "mu", "rsigma")]
        + [(f"{t}_row_stride", ctypes.c_int64) for t in ("x0", "x1", "residual", "z0", "z1", "x")]
        + [("M", ctypes.c_int64), ("N", ctypes.c_int32)]
        + [(f"{t}_dtype", ctypes.c_int32) for t in ("x0", "residual", "x", "weight", "z", "rowscale", "colscale")]
        + [("eps", ctypes.c_float), ("p_dropout", ctypes.c_float), ("flags", ctypes.c_int32), ("reserved", ctypes.c_int32)]
    )


class FaDropoutNormBwdParams(ctypes.Structure):
    """Field-for-field mirror of `struct fa_dropout_norm_bwd_params` (include/fa_dropout_norm.h)."""

    _fields_ = (
        [("abi_version", ctypes.c_uint32), ("struct_size", ctypes.c_uint32)]
        + [(n, ctypes.c_void_p) for n in ("dz0", "dz1", "dx", "x", "x0", "weight0", "weight1", "rowscale", "colscale", "rng_state",
                                          "mu", "rsigma", "dx0", "dx1", "dresidual", "dw0", "db0", "dw1", "db1", "dcolscale",
                                          "workspace")]
        + [("workspace_bytes", ctypes.c_uint64)]
        + [(f"{t}_row_stride", ctypes.c_int64) for t in ("dz0", "dz1", "dx", "x", "x0", "dx0", "dx1", "dresidual")]
        + [("M", ctypes.c_int64), ("N", ctypes.c_int32)]
        + [(f"{t}_dtype", ctypes.c_int32) for t in ("dz", "x", "x0", "weight", "rowscale", "colscale")]
        + [("p_dropout", ctypes.c_float), ("flags", ctypes.c_int32)]
    )


class FaDropoutNormPlan(ctypes.Structure):
    """Field-for-field mirror of `struct fa_dropout_norm_plan` (include/fa_dropout_norm.h): the form a call takes."""

    _fields_ = [(n, ctypes.c_int32) for n in ("cw", "threads", "wide", "dropout", "two_weights", "sums", "rows_per_wg", "grid_x",
                                              "grid_y")]


class FaXentPlan(ctypes.Structure):
    """Field-for-field mirror of `struct fa_xent_plan` (include/fa_xent.h): the form a cross-entropy call takes."""

    _fields_ = [(n, ctypes.c_int32) for n in ("cw", "grid_x", "grid_y", "lse_given")]


class FaXentFwdParams(ctypes.Structure):
    """Field-for-field mirror of `struct fa_xent_fwd_params` (include/fa_xent.h)."""

    _fields_ = (
        [("abi_version", ctypes.c_uint32), ("struct_size", ctypes.c_uint32)]
        + [(n, ctypes.c_void_p) for n in ("logits", "labels", "losses", "lse", "z_losses")]
        + [(n, ctypes.c_int64) for n in ("logits_row_stride", "M", "ignore_index", "class_start_idx", "total_classes")]
        + [(n, ctypes.c_int32) for n in ("N", "logits_dtype", "labels_dtype", "flags")]
        + [(n, ctypes.c_float) for n in ("smoothing", "logit_scale", "lse_square_scale")]
        + [("reserved", ctypes.c_int32)]
    )


class FaXentBwdParams(ctypes.Structure):
    """Field-for-field mirror of `struct fa_xent_bwd_params` (include/fa_xent.h)."""

    _fields_ = (
        [("abi_version", ctypes.c_uint32), ("struct_size", ctypes.c_uint32)]
        + [(n, ctypes.c_void_p) for n in ("logits", "labels", "lse", "dloss", "dlogits")]
        + [(n, ctypes.c_int64) for n in ("logits_row_stride", "dlogits_row_stride", "dloss_stride", "M", "ignore_index",
                                         "class_start_idx", "total_classes")]
        + [(n, ctypes.c_int32) for n in ("N", "logits_dtype", "labels_dtype", "flags")]
        + [(n, ctypes.c_float) for n in ("smoothing", "logit_scale", "lse_square_scale")]
        + [("reserved", ctypes.c_int32)]
    )


class FaSampleParams(ctypes.Structure):
    """Field-for-field mirror of `struct fa_sample_params` (include/fa_sample.h)."""

    _fields_ = (
        [("abi_version", ctypes.c_uint32), ("struct_size", ctypes.c_uint32)]
        + [(n, ctypes.c_void_p) for n in ("logits", "u", "rng_state", "token", "kept", "mass")]
        + [("logits_row_stride", ctypes.c_int64), ("B", ctypes.c_int64)]
        + [(n, ctypes.c_int32) for n in ("V", "logits_dtype", "mode", "top_k")]
        + [("top_p", ctypes.c_float), ("temperature", ctypes.c_float)]
    )


class FaSampleForm(ctypes.Structure):
    """Field-for-field mirror of `struct fa_sample_form` (include/fa_sample.h): the form a sampling call takes."""

    _fields_ = [(n, ctypes.c_int32) for n in ("cw", "threads", "mode", "greedy", "topk", "topp", "draw", "k", "key_bits",
                                              "key_passes", "index_bits", "index_passes", "frac_bits", "grid_x")]


class FaSpecSampleParams(ctypes.Structure):
    """Field-for-field mirror of `struct fa_spec_sample_params` (include/fa_spec_sample.h)."""

    _fields_ = (
        [("abi_version", ctypes.c_uint32), ("struct_size", ctypes.c_uint32)]
        + [(n, ctypes.c_void_p) for n in ("logits", "logits_draft", "tokens_draft", "u_acc", "u_res", "rng_state", "workspace", "tokens",
                                          "num_generated", "p_tok", "q_tok", "accepted")]
        + [(n, ctypes.c_int64) for n in ("logits_batch_stride", "logits_pos_stride", "draft_batch_stride", "draft_pos_stride",
                                         "tokens_draft_batch_stride", "workspace_bytes", "B")]
        + [(n, ctypes.c_int32) for n in ("S", "V", "logits_dtype", "tokens_dtype", "top_k")]
        + [("top_p", ctypes.c_float), ("temperature", ctypes.c_float), ("reserved", ctypes.c_int32)]
    )


class FaSpecSampleForm(ctypes.Structure):
    """Field-for-field mirror of `struct fa_spec_sample_form` (include/fa_spec_sample.h): the form a verification call takes."""

    _fields_ = [(n, ctypes.c_int32) for n in ("cw", "threads", "topk", "topp", "k", "key_bits", "key_passes", "index_bits",
                                              "index_passes", "frac_bits", "grid_a", "grid_b")]


class FaTreeSampleParams(ctypes.Structure):
    """Field-for-field mirror of `struct fa_tree_sample_params` (include/fa_tree_sample.h)."""

    _fields_ = (
        [("abi_version", ctypes.c_uint32), ("struct_size", ctypes.c_uint32)]
        + [(n, ctypes.c_void_p) for n in ("logits", "logits_draft", "tokens_draft", "parents", "u_acc", "u_res", "rng_state", "workspace",
                                          "path", "path_len", "tokens", "num_generated", "p_tok", "q_tok", "visited", "accepted")]
        + [(n, ctypes.c_int64) for n in ("logits_batch_stride", "logits_node_stride", "draft_batch_stride", "draft_node_stride",
                                         "tokens_draft_batch_stride", "parents_batch_stride", "workspace_bytes", "B")]
        + [(n, ctypes.c_int32) for n in ("T", "V", "logits_dtype", "tokens_dtype", "top_k")]
        + [("top_p", ctypes.c_float), ("temperature", ctypes.c_float), ("reserved", ctypes.c_int32)]
    )


class FaTreeSampleForm(ctypes.Structure):
    """Field-for-field mirror of `struct fa_tree_sample_form` (include/fa_tree_sample.h): the form a tree verification call takes."""

    _fields_ = [(n, ctypes.c_int32) for n in ("cw", "threads", "drafts", "topk", "topp", "k", "key_bits", "key_passes", "index_bits",
                                              "index_passes", "frac_bits", "grid_a", "grid_b")]


class FaBlockSummaryParams(ctypes.Structure):
    """Field-for-field mirror of `struct fa_block_summary_params` (include/fa_block_select.h)."""

    _fields_ = (
        [("abi_version", ctypes.c_uint32), ("struct_size", ctypes.c_uint32)]
        + [(n, ctypes.c_void_p) for n in ("k_summary", "k_cache", "seqlens_old", "seqlens_new", "cache_batch_idx", "page_table",
                                          "cache_leftpad", "cu_seqlens_k_new")]
        + [(f"sum_{s}_stride", ctypes.c_int64) for s in ("slot", "block", "side", "head")]
        + [(f"cache_{s}_stride", ctypes.c_int64) for s in ("batch", "row", "head")]
        + [("page_table_batch_stride", ctypes.c_int64)]
        + [(n, ctypes.c_int32) for n in ("b", "capacity", "h_k", "d", "max_blocks", "block_size", "page_size", "max_seqlen_new",
                                         "summary_dtype", "cache_dtype")]
    )


class FaBlockSelectParams(ctypes.Structure):
    """Field-for-field mirror of `struct fa_block_select_params` (include/fa_block_select.h)."""

    _fields_ = (
        [("abi_version", ctypes.c_uint32), ("struct_size", ctypes.c_uint32)]
        + [(n, ctypes.c_void_p) for n in ("q", "k_summary", "cache_seqlens", "cache_batch_idx", "cu_seqlens_q", "cache_leftpad",
                                          "scores", "block_cnt", "block_idx")]
        + [(f"q_{s}_stride", ctypes.c_int64) for s in ("batch", "row", "head")]
        + [(f"sum_{s}_stride", ctypes.c_int64) for s in ("slot", "block", "side", "head")]
        + [(f"{t}_{s}_stride", ctypes.c_int64) for t in ("scores", "cnt", "idx") for s in ("batch", "head")]
        + [(n, ctypes.c_int32) for n in ("b", "s_q", "h", "h_k", "d", "max_blocks", "list_width", "block_size", "num_blocks",
                                         "sink_blocks", "local_blocks", "group_reduce", "dtype", "reserved")]
    )


class FaBlockPatternParams(ctypes.Structure):
    """Field-for-field mirror of `struct fa_block_pattern_params` (include/fa_block_pattern.h)."""

    _fields_ = (
        [("abi_version", ctypes.c_uint32), ("struct_size", ctypes.c_uint32)]
        + [(n, ctypes.c_void_p) for n in ("q", "k", "full_block_cnt", "full_block_idx", "mask_block_cnt", "mask_block_idx", "q_block_cnt",
                                          "q_block_idx", "scores", "workspace")]
        + [("workspace_bytes", ctypes.c_uint64)]
        + [(f"{t}_{s}_stride", ctypes.c_int64) for t in ("q", "k") for s in ("batch", "row", "head")]
        + [(n, ctypes.c_int32) for n in ("b", "sq", "sk", "h", "h_k", "d", "num_blocks", "sink_blocks", "local_blocks", "is_causal",
                                         "window_size_left", "window_size_right", "dtype", "reserved")]
    )


class FaActPlan(ctypes.Structure):
    """Field-for-field mirror of `struct fa_act_plan` (include/fa_act.h): the form an activation call takes."""

    _fields_ = [(n, ctypes.c_int32) for n in ("cw", "threads", "grid_x", "grid_y", "rows_per_wg")]


class FaActFwdParams(ctypes.Structure):
    """Field-for-field mirror of `struct fa_act_fwd_params` (include/fa_act.h)."""

    _fields_ = (
        [("abi_version", ctypes.c_uint32), ("struct_size", ctypes.c_uint32)]
        + [(n, ctypes.c_void_p) for n in ("pre", "up", "bias", "out")]
        + [(n, ctypes.c_int64) for n in ("pre_row_stride", "out_row_stride", "M")]
        + [(n, ctypes.c_int32) for n in ("H", "activation", "flags", "pre_dtype", "up_dtype", "bias_dtype", "out_dtype", "reserved")]
    )


class FaActBwdParams(ctypes.Structure):
    """Field-for-field mirror of `struct fa_act_bwd_params` (include/fa_act.h)."""

    _fields_ = (
        [("abi_version", ctypes.c_uint32), ("struct_size", ctypes.c_uint32)]
        + [(n, ctypes.c_void_p) for n in ("pre", "up", "bias", "dout", "dpre", "dup", "dbias", "recompute_out", "workspace")]
        + [("workspace_bytes", ctypes.c_uint64)]
        + [(n, ctypes.c_int64) for n in ("pre_row_stride", "dout_row_stride", "dpre_row_stride", "out_row_stride", "M")]
        + [(n, ctypes.c_int32) for n in ("H", "activation", "flags", "pre_dtype", "up_dtype", "bias_dtype", "dout_dtype", "dpre_dtype",
                                         "dup_dtype", "dbias_dtype", "out_dtype", "reserved")]
    )


class FaGemmActPlan(ctypes.Structure):
    """Field-for-field mirror of `struct fa_gemm_act_plan` (include/fa_gemm_act.h): the form a fused GEMM call takes."""

    _fields_ = [(n, ctypes.c_int32) for n in ("tile_m", "tile_n", "tile_k", "threads", "tiles_m", "tiles_n", "grid_x", "k_steps",
                                              "ragged_m", "ragged_n", "ragged_k", "group_m", "partial_rows", "reduce_grid_x",
                                              "dtype", "dgrad")]


class FaGemmActFwdParams(ctypes.Structure):
    """Field-for-field mirror of `struct fa_gemm_act_fwd_params` (include/fa_gemm_act.h)."""

    _fields_ = (
        [("abi_version", ctypes.c_uint32), ("struct_size", ctypes.c_uint32)]
        + [(n, ctypes.c_void_p) for n in ("x", "weight", "bias", "out", "act_input")]
        + [(n, ctypes.c_int64) for n in ("x_row_stride", "weight_row_stride", "out_row_stride", "act_input_row_stride", "M")]
        + [(n, ctypes.c_int32) for n in ("N", "K", "activation", "x_dtype", "weight_dtype", "bias_dtype", "out_dtype",
                                         "act_input_dtype")]
    )


class FaGemmActDgradParams(ctypes.Structure):
    """Field-for-field mirror of `struct fa_gemm_act_dgrad_params` (include/fa_gemm_act.h)."""

    _fields_ = (
        [("abi_version", ctypes.c_uint32), ("struct_size", ctypes.c_uint32)]
        + [(n, ctypes.c_void_p) for n in ("grad_out", "weight", "act_input", "grad_in", "dbias", "workspace")]
        + [("workspace_bytes", ctypes.c_uint64)]
        + [(n, ctypes.c_int64) for n in ("grad_out_row_stride", "weight_row_stride", "act_input_row_stride", "grad_in_row_stride", "M")]
        + [(n, ctypes.c_int32) for n in ("N", "K", "activation", "grad_out_dtype", "weight_dtype", "act_input_dtype", "grad_in_dtype",
                                         "dbias_dtype")]
    )


class FaBwdParams(ctypes.Structure):
    """Field-for-field mirror of `struct fa_bwd_params` (include/fa_bwd.h)."""

    _fields_ = (
        [("abi_version", ctypes.c_uint32), ("struct_size", ctypes.c_uint32)]
        + [(n, ctypes.c_void_p) for n in ("q", "k", "v", "o", "dout", "softmax_lse", "dq", "dk", "dv", "softmax_d")]
        + [(f"{t}_{s}_stride", ctypes.c_int64) for t in ("q", "k", "v", "o", "do", "dq", "dk", "dv")
           for s in ("batch", "row", "head")]
        + [("softmax_d_row_len", ctypes.c_int64)]
        + [(n, ctypes.c_int32) for n in ("b", "seqlen_q", "seqlen_k", "h", "h_k", "d", "total_q", "total_k", "dtype")]
        + [("cu_seqlens_q", ctypes.c_void_p), ("cu_seqlens_k", ctypes.c_void_p)]
        + [("softmax_scale", ctypes.c_float), ("softcap", ctypes.c_float)]
        + [("is_causal", ctypes.c_int32), ("window_size_left", ctypes.c_int32), ("window_size_right", ctypes.c_int32)]
        + [("alibi_slopes", ctypes.c_void_p), ("alibi_slopes_batch_stride", ctypes.c_int64)]
        + [("deterministic", ctypes.c_int32), ("p_dropout", ctypes.c_float), ("rng_state", ctypes.c_void_p)]
        + [("flags", ctypes.c_int32), ("d_v", ctypes.c_int32)]
    )


class FaSinkParams(ctypes.Structure):
    """Field-for-field mirror of `struct fa_sink_params` (include/fa_fwd.h)."""

    _fields_ = (
        [("abi_version", ctypes.c_uint32), ("struct_size", ctypes.c_uint32), ("learnable_sink", ctypes.c_void_p)]
        + [(n, ctypes.c_int32) for n in ("sink_dtype", "sink_head_stride", "sink_row_stride", "reserved")]
    )


class FaBlockSparseParams(ctypes.Structure):
    """Field-for-field mirror of `struct fa_block_sparse_params` (include/fa_fwd.h)."""

    _fields_ = (
        [("abi_version", ctypes.c_uint32), ("struct_size", ctypes.c_uint32)]
        + [(n, ctypes.c_void_p) for n in ("full_block_cnt", "full_block_idx", "mask_block_cnt", "mask_block_idx")]
        + [(n, ctypes.c_int64 * 4) for n in ("full_cnt_stride", "full_idx_stride", "mask_cnt_stride", "mask_idx_stride")]
        + [("block_m", ctypes.c_int32), ("block_n", ctypes.c_int32)]
    )


class FaSparseKvParams(ctypes.Structure):
    """Field-for-field mirror of `struct fa_sparse_kv_params` (include/fa_fwd.h)."""

    _fields_ = (
        [("abi_version", ctypes.c_uint32), ("struct_size", ctypes.c_uint32), ("block_cnt", ctypes.c_void_p), ("block_idx", ctypes.c_void_p)]
        + [(n, ctypes.c_int64) for n in ("cnt_batch_stride", "cnt_head_stride", "idx_batch_stride", "idx_head_stride")]
        + [(n, ctypes.c_int32) for n in ("max_blocks", "block_size", "fp8_cache", "reserved")]
    )


class FaTreeParams(ctypes.Structure):
    """Field-for-field mirror of `struct fa_tree_params` (include/fa_fwd.h)."""

    _fields_ = [("abi_version", ctypes.c_uint32), ("struct_size", ctypes.c_uint32), ("tree_mask", ctypes.c_void_p),
                ("batch_stride", ctypes.c_int64), ("row_stride", ctypes.c_int64), ("fp8_cache", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class FaBlockSparseBwdParams(ctypes.Structure):
    """Field-for-field mirror of `struct fa_block_sparse_bwd_params` (include/fa_bwd.h)."""

    _fields_ = (
        [("abi_version", ctypes.c_uint32), ("struct_size", ctypes.c_uint32)]
        + [(n, ctypes.c_void_p) for n in ("q_block_cnt", "q_block_idx")]
        + [(n, ctypes.c_int64 * 4) for n in ("q_cnt_stride", "q_idx_stride")]
        + [("block_m", ctypes.c_int32), ("block_n", ctypes.c_int32)]
    )


class FaSinkGradParams(ctypes.Structure):
    """Field-for-field mirror of `struct fa_sink_grad_params` (include/fa_bwd.h)."""

    _fields_ = (
        [("abi_version", ctypes.c_uint32), ("struct_size", ctypes.c_uint32)]
        + [(n, ctypes.c_void_p) for n in ("softmax_lse", "softmax_d", "learnable_sink", "dsink", "cu_seqlens_q", "seqused_q")]
        + [("softmax_d_row_len", ctypes.c_int64)]
        + [(n, ctypes.c_int32) for n in ("b", "seqlen_q", "h", "total_q", "sink_dtype", "reserved")]
    )


HASH_PATH = os.path.join(_HERE, "libfa_fwd_gfx950.srchash")


def _deps():
    return sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hip", ".h", ".cpp"))) + sorted(
        os.path.join(INCLUDE, f) for f in os.listdir(INCLUDE) if f.endswith(".h"))


def source_hash():
    """sha256 over the sources the library is built from (what build() records next to the library)."""
    import hashlib
    h = hashlib.sha256()
    for path in _deps():
        h.update(os.path.basename(path).encode())
        h.update(open(path, "rb").read())
    return h.hexdigest()


def is_stale():
    """True when the built library is missing or was not built from the sources in the tree (content hash, not mtimes:
    the tree is copied to the GPU box)."""
    if not os.path.exists(LIB_PATH) or not os.path.exists(HASH_PATH) or not os.path.exists(binding_path()):
        return True
    return open(HASH_PATH).read().strip() != source_hash()


def build(force=False, verbose=False):
    """Compile csrc/ for gfx950 into the in-tree shared library (hipcc cross-compiles without a GPU)."""
    srcs = [os.path.join(CSRC, f) for f in ("fa_fwd_api.hip", "fa_fwd_kv8_api.hip", "fa_fwd_qv8_api.hip", "fa_fwd_sparse_kv_api.hip", "fa_fwd_tree_api.hip", "fa_kvcache_append_kv8.hip",
                                              "fa_kvcache_append_qv8.hip", "fa_bwd_api.hip", "fa_bwd_bs_api.hip", "fa_rotary_emb.hip", "fa_norm.hip", "fa_xent.hip", "fa_act.hip", "fa_gemm_act.hip",
                                              "fa_dropout_norm.hip", "fa_sample.hip", "fa_spec_sample.hip", "fa_tree_sample.hip", "fa_block_select.hip",
                                              "fa_block_pattern.hip")]
    if not force and not is_stale():
        return LIB_PATH
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        hipcc = "hipcc"
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared",
           "-I", INCLUDE, "-I", CSRC, *srcs, "-o", LIB_PATH]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.run(cmd, check=True)
    build_binding(verbose)
    with open(HASH_PATH, "w") as f:
        f.write(source_hash() + "\n")
    return LIB_PATH


def binding_path():
    import sysconfig
    return os.path.join(_HERE, "flash_attn_2_cuda_C" + sysconfig.get_config_var("EXT_SUFFIX"))


def build_binding(verbose=False):
    """The compiled `flash_attn_2_cuda` surface (csrc/torch_binding.cpp): host-only C++ over the C-ABI, plain g++ against
    the torch headers (no hipify: there is no device code in it), linked to the library next to it."""
    import sysconfig
    import torch
    tdir = os.path.dirname(torch.__file__)
    cmd = [os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-fPIC", "-shared", os.path.join(CSRC, "torch_binding.cpp"),
           "-DTORCH_EXTENSION_NAME=flash_attn_2_cuda_C", "-D__HIP_PLATFORM_AMD__=1", "-DUSE_ROCM=1",
           f"-D_GLIBCXX_USE_CXX11_ABI={int(torch._C._GLIBCXX_USE_CXX11_ABI)}",
           "-I", INCLUDE, "-I", os.path.join(tdir, "include"), "-I", os.path.join(tdir, "include", "torch", "csrc", "api", "include"),
           "-I", "/opt/rocm/include", "-I", sysconfig.get_paths()["include"],
           "-L", os.path.join(tdir, "lib"), "-ltorch", "-ltorch_cpu", "-lc10", "-lc10_hip", "-ltorch_hip", "-ltorch_python",
           "-L", _HERE, f"-l:{LIB_NAME}", "-Wl,-rpath,$ORIGIN", f"-Wl,-rpath,{os.path.join(tdir, 'lib')}",
           "-o", binding_path()]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.run(cmd, check=True)
    return binding_path()


_P, _VOID, _INT, _STR = ctypes.POINTER, ctypes.c_void_p, ctypes.c_int, ctypes.c_char_p
_I32, _I64, _U64 = ctypes.c_int32, ctypes.c_int64, ctypes.c_uint64


def _unit(prefix, structs, plan_struct, workspace_struct=None):
    """The prototype rows of one row unit (include/`prefix`.h): per (direction, params struct) the launch with its _params_size,
    _validate and _plan; `workspace_struct`: the struct of the direction that has a _workspace_bytes."""
    for name, struct in structs:
        yield f"{prefix}_{name}", [_P(struct), _VOID], _INT, f"{prefix}_{name}_params_size", struct
        yield f"{prefix}_{name}_validate", [_P(struct)], _INT
        yield f"{prefix}_{name}_plan", [_P(struct), _P(plan_struct)], _INT
        if struct is workspace_struct:
            yield f"{prefix}_{name}_workspace_bytes", [_P(struct)], _U64


_FWD, _BWD, _KV8 = _P(FaFwdParams), _P(FaBwdParams), _P(FaKvcacheAppendKv8Params)
_SINK, _BS, _BS_BWD, _SPARSE_KV = _P(FaSinkParams), _P(FaBlockSparseParams), _P(FaBlockSparseBwdParams), _P(FaSparseKvParams)
_TREE = _P(FaTreeParams)
# every C entry point, by header: (symbol, argtypes, restype); a row whose params struct has a `*_params_size` also names that
# symbol and the mirror it is checked against (the `*_params_size` symbols themselves are all `uint32_t (void)`)
_PROTOTYPES = {
    "fa_fwd.h": (
        ("fa_fwd", [_FWD, _VOID], _INT, "fa_fwd_params_size", FaFwdParams),
        ("fa_fwd_validate", [_FWD], _INT),
        ("fa_fwd_workspace_size", [_FWD], _I64),
        ("fa_fwd_plan_name", [_FWD, _I32], _STR),
        ("fa_fwd_last_plan_name", [], _STR),
        ("fa_strerror", [_INT], _STR),
        ("fa_abi_version", [], ctypes.c_uint32),
        ("fa_fwd_tile_shape", [_I32, _I32, _I32, _P(_I32), _P(_I32)], _INT),
        ("fa_set_default_variant", [_I32], None),
        ("fa_set_persist_mode", [_I32], None),
        ("fa_kvcache_append", [_P(FaKvcacheAppendParams), _VOID], _INT, "fa_kvcache_append_params_size", FaKvcacheAppendParams),
        ("fa_rotary_apply", [_P(FaRotaryParams), _VOID], _INT, "fa_rotary_params_size", FaRotaryParams),
        ("fa_kvcache_append_varlen", [_P(FaKvcacheAppendVarlenParams), _VOID], _INT, "fa_kvcache_append_varlen_params_size",
         FaKvcacheAppendVarlenParams),
        ("fa_rotary_apply_varlen", [_P(FaRotaryVarlenParams), _VOID], _INT, "fa_rotary_varlen_params_size", FaRotaryVarlenParams),
        ("fa_fwd_combine", [_P(FaCombineParams), _VOID], _INT, "fa_combine_params_size", FaCombineParams),
        ("fa_fwd_sink", [_FWD, _SINK, _VOID], _INT, "fa_sink_params_size", FaSinkParams),
        ("fa_fwd_sink_validate", [_FWD, _SINK], _INT),
        ("fa_fwd_block_sparse", [_FWD, _BS, _SINK, _VOID], _INT, "fa_block_sparse_params_size", FaBlockSparseParams),
        ("fa_fwd_block_sparse_validate", [_FWD, _BS, _SINK], _INT),
        ("fa_fwd_kv8", [_FWD, _VOID], _INT),
        ("fa_fwd_kv8_validate", [_FWD], _INT),
        ("fa_fwd_kv8_workspace_size", [_FWD], _I64),
        ("fa_fwd_kv8_plan_name", [_FWD, _I32], _STR),
        ("fa_fwd_qv8", [_FWD, _VOID], _INT),
        ("fa_fwd_qv8_validate", [_FWD], _INT),
        ("fa_fwd_qv8_workspace_size", [_FWD], _I64),
        ("fa_fwd_qv8_plan_name", [_FWD, _I32], _STR),
        ("fa_kvcache_append_kv8", [_KV8, _VOID], _INT, "fa_kvcache_append_kv8_params_size", FaKvcacheAppendKv8Params),
        ("fa_kvcache_append_kv8_validate", [_KV8], _INT),
        ("fa_kvcache_append_qv8", [_KV8, _VOID], _INT),
        ("fa_kvcache_append_qv8_validate", [_KV8], _INT),
        ("fa_fwd_sparse_kv", [_FWD, _SPARSE_KV, _VOID], _INT, "fa_sparse_kv_params_size", FaSparseKvParams),
        ("fa_fwd_sparse_kv_validate", [_FWD, _SPARSE_KV], _INT),
        ("fa_fwd_sparse_kv_workspace_size", [_FWD, _SPARSE_KV], _I64),
        ("fa_fwd_sparse_kv_plan_name", [_FWD, _SPARSE_KV, _I32], _STR),
        ("fa_fwd_tree", [_FWD, _TREE, _VOID], _INT, "fa_tree_params_size", FaTreeParams),
        ("fa_fwd_tree_validate", [_FWD, _TREE], _INT),
        ("fa_fwd_tree_workspace_size", [_FWD, _TREE], _I64),
        ("fa_fwd_tree_plan_name", [_FWD, _TREE, _I32], _STR),
    ),
    "fa_bwd.h": (
        ("fa_bwd", [_BWD, _VOID], _INT, "fa_bwd_params_size", FaBwdParams),
        ("fa_bwd_validate", [_BWD], _INT),
        ("fa_bwd_plan_name", [_BWD], _STR),
        ("fa_bwd_last_plan_name", [], _STR),
        ("fa_sink_grad", [_P(FaSinkGradParams), _VOID], _INT, "fa_sink_grad_params_size", FaSinkGradParams),
        ("fa_sink_grad_validate", [_P(FaSinkGradParams)], _INT),
        ("fa_bwd_block_sparse", [_BWD, _BS, _BS_BWD, _VOID], _INT, "fa_block_sparse_bwd_params_size", FaBlockSparseBwdParams),
        ("fa_bwd_block_sparse_validate", [_BWD, _BS, _BS_BWD], _INT),
    ),
    "fa_rotary.h": (
        ("fa_rotary_emb", [_P(FaRotaryEmbParams), _VOID], _INT, "fa_rotary_emb_params_size", FaRotaryEmbParams),
        ("fa_rotary_emb_validate", [_P(FaRotaryEmbParams)], _INT),
    ),
    "fa_norm.h": tuple(_unit("fa_norm", (("fwd", FaNormFwdParams), ("bwd", FaNormBwdParams)), FaNormPlan, FaNormBwdParams)),
    "fa_xent.h": tuple(_unit("fa_xent", (("fwd", FaXentFwdParams), ("bwd", FaXentBwdParams)), FaXentPlan)),
    "fa_act.h": tuple(_unit("fa_act", (("fwd", FaActFwdParams), ("bwd", FaActBwdParams)), FaActPlan, FaActBwdParams)),
    "fa_gemm_act.h": tuple(_unit("fa_gemm_act", (("fwd", FaGemmActFwdParams), ("dgrad", FaGemmActDgradParams)), FaGemmActPlan,
                                 FaGemmActDgradParams)),
    "fa_dropout_norm.h": tuple(_unit("fa_dropout_norm", (("fwd", FaDropoutNormFwdParams), ("bwd", FaDropoutNormBwdParams)),
                                     FaDropoutNormPlan, FaDropoutNormBwdParams)),
    "fa_sample.h": tuple(_unit("fa", (("sample", FaSampleParams),), FaSampleForm)),
    "fa_spec_sample.h": tuple(_unit("fa_spec", (("sample", FaSpecSampleParams),), FaSpecSampleForm))
    + (("fa_spec_sample_workspace_size", [_I64, _I32], _I64),),
    "fa_tree_sample.h": tuple(_unit("fa_tree", (("sample", FaTreeSampleParams),), FaTreeSampleForm))
    + (("fa_tree_sample_workspace_size", [_I64, _I32], _I64),),
    "fa_block_select.h": tuple(
        row for unit, struct, size in (("fa_block_summary_update", FaBlockSummaryParams, "fa_block_summary_params_size"),
                                       ("fa_block_select", FaBlockSelectParams, "fa_block_select_params_size"))
        for row in ((unit, [_P(struct), _VOID], _INT, size, struct), (f"{unit}_validate", [_P(struct)], _INT),
                    (f"{unit}_workspace_size", [_P(struct)], _I64), (f"{unit}_plan_name", [_P(struct)], _STR))),
    "fa_block_pattern.h": (
        ("fa_block_pattern", [_P(FaBlockPatternParams), _VOID], _INT, "fa_block_pattern_params_size", FaBlockPatternParams),
        ("fa_block_pattern_validate", [_P(FaBlockPatternParams)], _INT),
        ("fa_block_pattern_workspace_size", [_P(FaBlockPatternParams)], _I64),
        ("fa_block_pattern_plan_name", [_P(FaBlockPatternParams)], _STR),
    ),
}

_lib = None


def load():
    """dlopen the library and declare prototypes.  Raises if the library is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_NAME} is not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
            f"(expected at {LIB_PATH}); there is no CPU fallback")
    # FA_FWD_LIB: developer override (ablation / instrumented builds).  RTLD_GLOBAL: the binding, imported after this by
    # binding(), resolves its fa_* references to this instance
    lib = ctypes.CDLL(os.environ.get("FA_FWD_LIB", LIB_PATH), mode=ctypes.RTLD_GLOBAL)
    for header, rows in _PROTOTYPES.items():
        for symbol, argtypes, restype, *sized in rows:
            fn = getattr(lib, symbol)
            fn.argtypes, fn.restype = argtypes, restype
            if sized:
                size, struct = getattr(lib, sized[0]), sized[1]
                size.argtypes, size.restype = [], ctypes.c_uint32
                if size() != ctypes.sizeof(struct):
                    raise RuntimeError(f"{sized[0][:-len('_size')]} layout mismatch between include/{header} and "
                                       f"_lib.{struct.__name__}")
    if lib.fa_abi_version() != FA_ABI_VERSION:
        raise RuntimeError("fa_fwd ABI version mismatch")
    if os.environ.get("FA_FWD_VARIANT"):  # developer override of the kernel shape (never changes results)
        lib.fa_set_default_variant(int(os.environ["FA_FWD_VARIANT"]))
    if os.environ.get("FA_FWD_PERSIST"):  # developer override: -1 never / 1 always the persistent 256-row kernel (never changes results)
        lib.fa_set_persist_mode(int(os.environ["FA_FWD_PERSIST"]))
    _lib = lib
    return lib


_binding = None


def binding():
    """The compiled host module, imported after load(): the ABI / struct-layout checks and the FA_FWD_* overrides apply to
    the library instance every compiled call goes to.  A binding that does not load raises ImportError: there is no other
    host path."""
    global _binding
    if _binding is None:
        try:
            load()
            from . import flash_attn_2_cuda_C
        except (ImportError, RuntimeError) as e:
            raise ImportError(
                f"flash_attn_2_cuda_C is not built or does not load ({e}): run `python -c 'import __graft_entry__ as g; "
                f"g.build()'` (expected at {binding_path()}); there is no CPU fallback") from e
        _binding = flash_attn_2_cuda_C
    return _binding


def strerror(status):
    return load().fa_strerror(status).decode()


def _new(struct, dtypes=(), **defaults):
    """A params struct with its ABI header, the listed `*_dtype` fields bf16 and the given defaults."""
    return struct(abi_version=FA_ABI_VERSION, struct_size=ctypes.sizeof(struct), **{f"{t}_dtype": FA_DTYPE_BF16 for t in dtypes},
                  **defaults)


def new_params():
    return _new(FaFwdParams)


def new_bwd_params():
    return _new(FaBwdParams)


def new_sink_params():
    return _new(FaSinkParams, ("sink",), sink_head_stride=1)


def new_block_sparse_params():
    return _new(FaBlockSparseParams, block_m=128, block_n=128)


def new_block_sparse_bwd_params():
    return _new(FaBlockSparseBwdParams, block_m=128, block_n=128)


def new_sparse_kv_params():
    return _new(FaSparseKvParams, block_size=128)


def new_tree_params():
    return _new(FaTreeParams, row_stride=1)


def new_sink_grad_params():
    return _new(FaSinkGradParams, ("sink",))


def new_kvcache_append_kv8_params():
    return _new(FaKvcacheAppendKv8Params, dtype=FA_DTYPE_BF16)


def new_rotary_emb_params():
    return _new(FaRotaryEmbParams, ("cos", "sin"), dtype=FA_DTYPE_BF16, x_dim_stride=1, out_dim_stride=1)


def new_norm_fwd_params():
    return _new(FaNormFwdParams, ("x", "residual", "residual_out", "weight", "bias", "y", "rowscale"), eps=1e-6)


def new_norm_bwd_params():
    return _new(FaNormBwdParams, ("x", "dy", "weight", "bias", "dresidual", "dresidual_in", "dx", "y", "rowscale"))


def new_dropout_norm_fwd_params():
    return _new(FaDropoutNormFwdParams, ("x0", "residual", "x", "weight", "z", "rowscale", "colscale"), eps=1e-6)


def new_dropout_norm_bwd_params():
    return _new(FaDropoutNormBwdParams, ("dz", "x", "x0", "weight", "rowscale", "colscale"))


def new_xent_fwd_params():
    return _new(FaXentFwdParams, ("logits",), labels_dtype=FA_XENT_LABELS_INT64, ignore_index=-100, logit_scale=1.0)


def new_xent_bwd_params():
    return _new(FaXentBwdParams, ("logits",), labels_dtype=FA_XENT_LABELS_INT64, ignore_index=-100, logit_scale=1.0)


def new_sample_params():
    return _new(FaSampleParams, ("logits",), mode=FA_SAMPLE_DRAW, temperature=1.0)


def new_spec_sample_params():
    return _new(FaSpecSampleParams, ("logits",), tokens_dtype=FA_SPEC_TOKENS_INT64, temperature=1.0)


def new_tree_sample_params():
    return _new(FaTreeSampleParams, ("logits",), tokens_dtype=FA_TREE_TOKENS_INT64, temperature=1.0)


def new_block_summary_params():
    return _new(FaBlockSummaryParams, ("summary", "cache"), block_size=128)


def new_block_select_params():
    return _new(FaBlockSelectParams, dtype=FA_DTYPE_BF16, block_size=128, sink_blocks=1, local_blocks=1)


def new_block_pattern_params():
    return _new(FaBlockPatternParams, dtype=FA_DTYPE_BF16, sink_blocks=1, local_blocks=1, window_size_left=-1, window_size_right=-1)


def new_act_fwd_params():
    return _new(FaActFwdParams, ("pre", "up", "bias", "out"))


def new_act_bwd_params():
    return _new(FaActBwdParams, ("pre", "up", "bias", "dout", "dpre", "dup", "dbias", "out"))


def new_gemm_act_fwd_params():
    return _new(FaGemmActFwdParams, ("x", "weight", "bias", "out", "act_input"))


def new_gemm_act_dgrad_params():
    return _new(FaGemmActDgradParams, ("grad_out", "weight", "act_input", "grad_in", "dbias"))
