"""`torch.ops.flash_attn_3.*`: the FA3 operator library (hopper/flash_api.cpp:1671-1768), defined with the reference's
schema strings so that `hopper/flash_attn_interface.py:66` (`flash_attn_3_gpu.fwd(...)`) and exported graphs bind
unchanged.  hopper/test_flash_attn.py::test_flash3_bw_compatibility (:1163-1201) pins these schemas: arguments may only
be appended with defaults.  Implementations are registered for the GPU dispatch key (HIP devices use `CUDA` in
PyTorch-ROCm) and are one call each into the compiled binding (csrc/torch_binding.cpp: fa3_fwd, fa3_bwd,
fa3_fwd_combine), resolved at call time so that importing this module does not load it.
"""
import torch

from . import _lib, flash_attn_3_cuda

FWD_SCHEMA = (
    "fwd(Tensor q, Tensor k, Tensor v, Tensor(k_new!)? k_new = None, Tensor(v_new!)? v_new = None, Tensor? q_v = None, "
    "Tensor(out!)? out = None, Tensor? cu_seqlens_q = None, Tensor? cu_seqlens_k = None, Tensor? cu_seqlens_k_new = None, "
    "Tensor? seqused_q = None, Tensor? seqused_k = None, int? max_seqlen_q = None, int? max_seqlen_k = None, "
    "Tensor? page_table = None, Tensor? kv_batch_idx = None, Tensor? leftpad_k = None, Tensor? rotary_cos = None, "
    "Tensor? rotary_sin = None, Tensor? seqlens_rotary = None, Tensor? q_descale = None, Tensor? k_descale = None, "
    "Tensor? v_descale = None, float? softmax_scale = None, bool is_causal = False, int window_size_left = -1, "
    "int window_size_right = -1, int attention_chunk = 0, float softcap = 0.0, bool is_rotary_interleaved = False, "
    "Tensor? scheduler_metadata = None, int num_splits = 0, bool? pack_gqa = None, int sm_margin = 0) "
    "-> (Tensor(out!), Tensor, Tensor, Tensor)")
BWD_SCHEMA = (
    "bwd(Tensor dout, Tensor q, Tensor k, Tensor v, Tensor out, Tensor softmax_lse, Tensor(dq!)? dq = None, "
    "Tensor(dk!)? dk = None, Tensor(dv!)? dv = None, Tensor? cu_seqlens_q = None, Tensor? cu_seqlens_k = None, "
    "Tensor? seqused_q = None, Tensor? seqused_k = None, int? max_seqlen_q = None, int? max_seqlen_k = None, "
    "float? softmax_scale = None, bool is_causal = False, int window_size_left = -1, int window_size_right = -1, "
    "float softcap = 0.0, bool deterministic = False, int sm_margin = 0) "
    "-> (Tensor(dq!), Tensor(dk!), Tensor(dv!), Tensor, Tensor, Tensor, Tensor, Tensor)")
COMBINE_SCHEMA = ("fwd_combine(Tensor out_partial, Tensor lse_partial, Tensor(out!)? out = None, ScalarType? out_dtype = None) "
                  "-> (Tensor(out!), Tensor)")
METADATA_SCHEMA = (
    "get_scheduler_metadata(int batch_size, int max_seqlen_q, int max_seqlen_k, int num_heads, int num_heads_k, int headdim, "
    "int headdim_v, ScalarType qkv_dtype, Tensor seqused_k, Tensor? cu_seqlens_q = None, Tensor? cu_seqlens_k = None, "
    "Tensor? cu_seqlens_k_new = None, Tensor? seqused_q = None, Tensor? leftpad_k = None, int? page_size = None, "
    "int max_seqlen_k_new = 0, bool is_causal = False, int window_size_left = -1, int window_size_right = -1, "
    "int attention_chunk = 0, bool has_softcap = False, int num_splits = 0, bool? pack_gqa = None, int sm_margin = 0) -> Tensor")

# not in the reference's library: the write half of an fp8 KV cache as an op of its own (the role of a `reshape_and_cache` op)
APPEND_FP8_SCHEMA = (
    "kvcache_append_fp8(Tensor(a!) k_cache, Tensor(b!) v_cache, Tensor k, Tensor v, Tensor cache_seqlens, Tensor k_descale, "
    "Tensor v_descale, Tensor? cu_seqlens_k_new = None, int? max_seqlen_k_new = None, Tensor? cache_batch_idx = None, "
    "Tensor? page_table = None, Tensor? rotary_cos = None, Tensor? rotary_sin = None, Tensor? rotary_seqlens = None, "
    "bool rotary_interleaved = True) -> Tensor")
# not in the reference's library either: block-sparse attention over a KV cache (key blocks listed per kv head), read-only
KVCACHE_SPARSE_SCHEMA = (
    "fwd_kvcache_sparse(Tensor q, Tensor k_cache, Tensor v_cache, Tensor kv_block_cnt, Tensor kv_block_idx, int kv_block_size = 128, "
    "Tensor? cache_seqlens = None, Tensor? cache_batch_idx = None, Tensor? cache_leftpad = None, Tensor? page_table = None, "
    "Tensor? cu_seqlens_q = None, int? max_seqlen_q = None, Tensor? k_descale = None, Tensor? v_descale = None, "
    "float? softmax_scale = None, bool is_causal = False, int window_size_left = -1, int window_size_right = -1, "
    "float softcap = 0.0, int num_splits = 0) -> (Tensor, Tensor)")
# nor this: tree attention over a KV cache (the verify step of speculative decoding over a token tree), read-only
KVCACHE_TREE_SCHEMA = (
    "fwd_kvcache_tree(Tensor q, Tensor k_cache, Tensor v_cache, Tensor tree_mask, Tensor? cache_seqlens = None, "
    "Tensor? cache_batch_idx = None, Tensor? cache_leftpad = None, Tensor? page_table = None, Tensor? cu_seqlens_q = None, "
    "int? max_seqlen_q = None, Tensor? k_descale = None, Tensor? v_descale = None, float? softmax_scale = None, "
    "float softcap = 0.0, int num_splits = 0) -> (Tensor, Tensor)")
# ... nor what produces the sparse route's lists (include/fa_block_select.h): the block summaries of the keys, updated in place on append, and
# the Quest selection.  Every tensor the launches write is a mutated argument and nothing is returned, so that a traced graph
# holds no alias of an input; hopper_interface allocates what the caller does not give
BLOCK_SUMMARY_SCHEMA = (
    "kvcache_block_summary_update(Tensor(a!) k_summary, Tensor k_cache, Tensor? seqlens_old, Tensor seqlens_new, "
    "int kv_block_size = 128, int? max_seqlen_new = None, Tensor? cache_batch_idx = None, Tensor? page_table = None) -> ()")
SELECT_BLOCKS_SCHEMA = (
    "kvcache_select_blocks(Tensor q, Tensor k_summary, Tensor cache_seqlens, int num_blocks, int kv_block_size, int sink_blocks, "
    "int local_blocks, str group_reduce, Tensor? cache_batch_idx, Tensor(a!) kv_block_cnt, Tensor(b!) kv_block_idx, "
    "Tensor(c!) scores) -> ()")

_ops = torch.library.Library("flash_attn_3", "DEF")
for _schema in (FWD_SCHEMA, BWD_SCHEMA, COMBINE_SCHEMA, METADATA_SCHEMA, APPEND_FP8_SCHEMA, KVCACHE_SPARSE_SCHEMA, KVCACHE_TREE_SCHEMA,
                BLOCK_SUMMARY_SCHEMA, SELECT_BLOCKS_SCHEMA):
    _ops.define(_schema)


def _fwd(q, k, v, k_new=None, v_new=None, q_v=None, out=None, cu_seqlens_q=None, cu_seqlens_k=None, cu_seqlens_k_new=None,
         seqused_q=None, seqused_k=None, max_seqlen_q=None, max_seqlen_k=None, page_table=None, kv_batch_idx=None,
         leftpad_k=None, rotary_cos=None, rotary_sin=None, seqlens_rotary=None, q_descale=None, k_descale=None,
         v_descale=None, softmax_scale=None, is_causal=False, window_size_left=-1, window_size_right=-1,
         attention_chunk=0, softcap=0.0, is_rotary_interleaved=False, scheduler_metadata=None, num_splits=0,
         pack_gqa=None, sm_margin=0):
    o, lse, _, _ = flash_attn_3_cuda.fwd(
        q, k, v, k_new, v_new, q_v, out, cu_seqlens_q, cu_seqlens_k, cu_seqlens_k_new, seqused_q, seqused_k, max_seqlen_q,
        max_seqlen_k, page_table, kv_batch_idx, leftpad_k, rotary_cos, rotary_sin, seqlens_rotary, q_descale, k_descale,
        v_descale, softmax_scale, is_causal, window_size_left, window_size_right, attention_chunk, softcap,
        is_rotary_interleaved, scheduler_metadata, num_splits, pack_gqa, sm_margin)
    # out_accum / softmax_lse_accum: empty when the result was not produced by the split path (hopper/flash_api.cpp:1196)
    return o, lse, torch.empty(0, dtype=torch.float32, device=q.device), torch.empty(0, dtype=torch.float32, device=q.device)


def _bwd(dout, q, k, v, out, softmax_lse, dq=None, dk=None, dv=None, cu_seqlens_q=None, cu_seqlens_k=None, seqused_q=None,
         seqused_k=None, max_seqlen_q=None, max_seqlen_k=None, softmax_scale=None, is_causal=False, window_size_left=-1,
         window_size_right=-1, softcap=0.0, deterministic=False, sm_margin=0):
    """mha_bwd, hopper/flash_api.cpp:1259-1570: the binding's fa3_bwd."""
    return _lib.binding().fa3_bwd(dout, q, k, v, out, softmax_lse, dq, dk, dv, cu_seqlens_q, cu_seqlens_k, seqused_q, seqused_k,
                                  max_seqlen_q, max_seqlen_k, softmax_scale, is_causal, window_size_left, window_size_right,
                                  softcap, deterministic, sm_margin)


def _fwd_combine(out_partial, lse_partial, out=None, out_dtype=None):
    """mha_combine, hopper/flash_api.cpp:1569-1670: the binding's fa3_fwd_combine."""
    return _lib.binding().fa3_fwd_combine(out_partial, lse_partial, out, out_dtype)


def _kvcache_append_fp8(k_cache, v_cache, k, v, cache_seqlens, k_descale, v_descale, cu_seqlens_k_new=None, max_seqlen_k_new=None,
                        cache_batch_idx=None, page_table=None, rotary_cos=None, rotary_sin=None, rotary_seqlens=None,
                        rotary_interleaved=True):
    """The binding's kvcache_append_fp8 (fa_kvcache_append_kv8; the MLA shape: fa_kvcache_append_qv8): one launch, returns the new
    fill levels."""
    return _lib.binding().kvcache_append_fp8(k_cache, v_cache, k, v, cache_seqlens, k_descale, v_descale, cu_seqlens_k_new,
                                             max_seqlen_k_new, cache_batch_idx, page_table, rotary_cos, rotary_sin,
                                             rotary_seqlens, rotary_interleaved)


def _kvcache_append_fp8_meta(k_cache, v_cache, k, v, cache_seqlens, k_descale, v_descale, cu_seqlens_k_new=None,
                             max_seqlen_k_new=None, cache_batch_idx=None, page_table=None, rotary_cos=None, rotary_sin=None,
                             rotary_seqlens=None, rotary_interleaved=True):
    return torch.empty_like(cache_seqlens)


def _fwd_kvcache_sparse(q, k_cache, v_cache, kv_block_cnt, kv_block_idx, kv_block_size=128, cache_seqlens=None, cache_batch_idx=None,
                        cache_leftpad=None, page_table=None, cu_seqlens_q=None, max_seqlen_q=None, k_descale=None, v_descale=None,
                        softmax_scale=None, is_causal=False, window_size_left=-1, window_size_right=-1, softcap=0.0, num_splits=0):
    """The binding's fwd_kvcache_sparse (fa_fwd_sparse_kv): one launch (+ the merge of a split call), no host sync."""
    out, lse = _lib.binding().fwd_kvcache_sparse(q, k_cache, v_cache, kv_block_cnt, kv_block_idx, kv_block_size, cache_seqlens,
                                                 cache_batch_idx, cache_leftpad, page_table, cu_seqlens_q, max_seqlen_q, k_descale,
                                                 v_descale, softmax_scale, is_causal, window_size_left, window_size_right, softcap,
                                                 num_splits)
    return out, lse


def _fwd_kvcache_sparse_meta(q, k_cache, v_cache, kv_block_cnt, kv_block_idx, kv_block_size=128, cache_seqlens=None,
                             cache_batch_idx=None, cache_leftpad=None, page_table=None, cu_seqlens_q=None, max_seqlen_q=None,
                             k_descale=None, v_descale=None, softmax_scale=None, is_causal=False, window_size_left=-1,
                             window_size_right=-1, softcap=0.0, num_splits=0):
    lse_shape = (q.shape[1], q.shape[0]) if q.dim() == 3 else (q.shape[0], q.shape[2], q.shape[1])
    return torch.empty_like(q), q.new_empty(lse_shape, dtype=torch.float32)


def _fwd_kvcache_tree(q, k_cache, v_cache, tree_mask, cache_seqlens=None, cache_batch_idx=None, cache_leftpad=None, page_table=None,
                      cu_seqlens_q=None, max_seqlen_q=None, k_descale=None, v_descale=None, softmax_scale=None, softcap=0.0,
                      num_splits=0):
    """The binding's fwd_kvcache_tree (fa_fwd_tree): one launch (+ the merge of a split call), no host sync."""
    out, lse = _lib.binding().fwd_kvcache_tree(q, k_cache, v_cache, tree_mask, cache_seqlens, cache_batch_idx, cache_leftpad,
                                               page_table, cu_seqlens_q, max_seqlen_q, k_descale, v_descale, softmax_scale, softcap,
                                               num_splits)
    return out, lse


def _fwd_kvcache_tree_meta(q, k_cache, v_cache, tree_mask, cache_seqlens=None, cache_batch_idx=None, cache_leftpad=None,
                           page_table=None, cu_seqlens_q=None, max_seqlen_q=None, k_descale=None, v_descale=None, softmax_scale=None,
                           softcap=0.0, num_splits=0):
    lse_shape = (q.shape[1], q.shape[0]) if q.dim() == 3 else (q.shape[0], q.shape[2], q.shape[1])
    return torch.empty_like(q), q.new_empty(lse_shape, dtype=torch.float32)


def _kvcache_block_summary_update(k_summary, k_cache, seqlens_old, seqlens_new, kv_block_size=128, max_seqlen_new=None,
                                  cache_batch_idx=None, page_table=None):
    """The binding's kvcache_block_summary_update (fa_block_summary_update): one launch, in place."""
    _lib.binding().kvcache_block_summary_update(k_summary, k_cache, seqlens_old, seqlens_new, kv_block_size, max_seqlen_new,
                                                cache_batch_idx, page_table)


def _kvcache_select_blocks(q, k_summary, cache_seqlens, num_blocks, kv_block_size, sink_blocks, local_blocks, group_reduce,
                           cache_batch_idx, kv_block_cnt, kv_block_idx, scores):
    """The binding's kvcache_select_blocks (fa_block_select): the scoring launch and the selection launch, no host sync."""
    _lib.binding().kvcache_select_blocks(q, k_summary, cache_seqlens, num_blocks, kv_block_size, sink_blocks, local_blocks,
                                         group_reduce, cache_batch_idx, kv_block_cnt, kv_block_idx, scores)


def _nothing(*args, **kwargs):
    """The fake of an op that only mutates its arguments."""


def _get_scheduler_metadata(batch_size, max_seqlen_q, max_seqlen_k, num_heads, num_heads_k, headdim, headdim_v, qkv_dtype,
                            seqused_k, cu_seqlens_q=None, cu_seqlens_k=None, cu_seqlens_k_new=None, seqused_q=None,
                            leftpad_k=None, page_size=None, max_seqlen_k_new=0, is_causal=False, window_size_left=-1,
                            window_size_right=-1, attention_chunk=0, has_softcap=False, num_splits=0, pack_gqa=None,
                            sm_margin=0):
    """The tile schedule of this build is computed inside the kernel (decode_tile): the metadata tensor is opaque to
    callers and empty here; `fwd` ignores it (hopper/flash_api.cpp:520-669 builds a semaphore + per-batch split table)."""
    return torch.zeros(1, dtype=torch.int32, device=seqused_k.device)


def _fwd_meta(q, k, v, k_new=None, v_new=None, q_v=None, out=None, cu_seqlens_q=None, cu_seqlens_k=None, cu_seqlens_k_new=None,
              seqused_q=None, seqused_k=None, max_seqlen_q=None, max_seqlen_k=None, page_table=None, kv_batch_idx=None,
              leftpad_k=None, rotary_cos=None, rotary_sin=None, seqlens_rotary=None, q_descale=None, k_descale=None,
              v_descale=None, softmax_scale=None, is_causal=False, window_size_left=-1, window_size_right=-1,
              attention_chunk=0, softcap=0.0, is_rotary_interleaved=False, scheduler_metadata=None, num_splits=0,
              pack_gqa=None, sm_margin=0):
    """Shapes of `fwd` for tracing (meta / fake tensors): out is q's shape with V's head dim (bf16 for fp8 inputs), the LSE
    (b, h, seqlen_q) for dense queries and (h, total_q) for ragged ones -- with cu_seqlens_k (varlen) as well as over a KV
    cache (cu_seqlens_q + seqused_k, k_new dense or ragged with cu_seqlens_k_new)."""
    out_dtype = torch.bfloat16 if q.dtype == torch.float8_e4m3fn else q.dtype
    o = out if out is not None else q.new_empty((*q.shape[:-1], v.shape[-1]), dtype=out_dtype)
    lse_shape = (q.shape[1], q.shape[0]) if q.dim() == 3 else (q.shape[0], q.shape[2], q.shape[1])
    empty = q.new_empty((0,), dtype=torch.float32)
    return o, q.new_empty(lse_shape, dtype=torch.float32), empty, empty


_ops.impl("fwd", _fwd, "CUDA")
_ops.impl("fwd", _fwd_meta, "Meta")
_ops.impl("bwd", _bwd, "CUDA")
_ops.impl("fwd_combine", _fwd_combine, "CUDA")
_ops.impl("get_scheduler_metadata", _get_scheduler_metadata, "CUDA")
_ops.impl("kvcache_append_fp8", _kvcache_append_fp8, "CUDA")
_ops.impl("kvcache_append_fp8", _kvcache_append_fp8_meta, "Meta")
_ops.impl("fwd_kvcache_sparse", _fwd_kvcache_sparse, "CUDA")
_ops.impl("fwd_kvcache_sparse", _fwd_kvcache_sparse_meta, "Meta")
_ops.impl("fwd_kvcache_tree", _fwd_kvcache_tree, "CUDA")
_ops.impl("fwd_kvcache_tree", _fwd_kvcache_tree_meta, "Meta")
_ops.impl("kvcache_block_summary_update", _kvcache_block_summary_update, "CUDA")
_ops.impl("kvcache_block_summary_update", _nothing, "Meta")
_ops.impl("kvcache_select_blocks", _kvcache_select_blocks, "CUDA")
_ops.impl("kvcache_select_blocks", _nothing, "Meta")
