"""FA3-flavoured public API — names, argument order and defaults of `hopper/flash_attn_interface.py`
(`flash_attn_func` :507-585, `flash_attn_varlen_func` :588-633) on top of `torch.ops.flash_attn_3.fwd`
(flash_attn_3_ops.py registers the library with the reference's schema; :10-14 of the reference does the same lookup).
This is the surface that carries fp8 e4m3 inputs with per-(batch, kv head) descales (BASELINE config 5)."""
from typing import NamedTuple

import torch

from . import flash_attn_3_ops  # noqa: F401  (defines torch.ops.flash_attn_3)

flash_attn_3_gpu = torch.ops.flash_attn_3


def maybe_contiguous(x):
    return x.contiguous() if x is not None and x.stride(-1) != 1 else x


def _flash_attn_forward(q, k, v, k_new, v_new, qv, out, cu_seqlens_q, cu_seqlens_k, cu_seqlens_k_new, seqused_q, seqused_k,
                        max_seqlen_q, max_seqlen_k, page_table, kv_batch_idx, leftpad_k, rotary_cos, rotary_sin,
                        seqlens_rotary, q_descale, k_descale, v_descale, softmax_scale, causal, window_size=(-1, -1),
                        attention_chunk=0, softcap=0.0, rotary_interleaved=True, scheduler_metadata=None, num_splits=1,
                        pack_gqa=None, sm_margin=0):
    """hopper/flash_attn_interface.py:20-102"""
    q, k = [maybe_contiguous(x) for x in (q, k)]
    v = v.contiguous() if v.stride(-1) != 1 and v.stride(-3) != 1 else v
    out, softmax_lse, *rest = flash_attn_3_gpu.fwd(
        q, k, v, k_new, v_new, qv, out, cu_seqlens_q, cu_seqlens_k, cu_seqlens_k_new, seqused_q, seqused_k,
        max_seqlen_q, max_seqlen_k, page_table, kv_batch_idx, leftpad_k, rotary_cos, rotary_sin, seqlens_rotary,
        q_descale, k_descale, v_descale, softmax_scale, causal, window_size[0], window_size[1], attention_chunk, softcap,
        rotary_interleaved, scheduler_metadata, num_splits, pack_gqa, sm_margin)
    return out, softmax_lse, *rest


def _flash_attn_backward(dout, q, k, v, out, softmax_lse, cu_seqlens_q, cu_seqlens_k, seqused_q, seqused_k, max_seqlen_q,
                         max_seqlen_k, dq, dk, dv, softmax_scale, causal, window_size=(-1, -1), softcap=0.0,
                         deterministic=False, sm_margin=0):
    """hopper/flash_attn_interface.py:105-154"""
    dout, q, k, v, out = [maybe_contiguous(x) for x in (dout, q, k, v, out)]
    dq, dk, dv, softmax_d, *rest = torch.ops.flash_attn_3.bwd(
        dout, q, k, v, out, softmax_lse, dq, dk, dv, cu_seqlens_q, cu_seqlens_k, seqused_q, seqused_k, max_seqlen_q,
        max_seqlen_k, softmax_scale, causal, window_size[0], window_size[1], softcap, deterministic, sm_margin)
    return dq, dk, dv, softmax_d


class FlashAttnFunc(torch.autograd.Function):
    """hopper/flash_attn_interface.py:254-339"""

    @staticmethod
    def forward(ctx, q, k, v, softmax_scale, causal, qv=None, q_descale=None, k_descale=None, v_descale=None,
                window_size=(-1, -1), attention_chunk=0, softcap=0.0, num_splits=1, pack_gqa=None, deterministic=False,
                sm_margin=0, return_softmax=False):
        if softmax_scale is None:
            softmax_scale = (q.shape[-1] + (qv.shape[-1] if qv is not None else 0)) ** (-0.5)
        out, softmax_lse, *_ = _flash_attn_forward(
            q, k, v, None, None, qv, None, None, None, None, None, None, None, None, None, None, None, None, None, None,
            q_descale, k_descale, v_descale, softmax_scale, causal=causal, window_size=window_size,
            attention_chunk=attention_chunk, softcap=softcap, num_splits=num_splits, pack_gqa=pack_gqa, sm_margin=sm_margin)
        ctx.save_for_backward(q, k, v, out, softmax_lse)
        ctx.softmax_scale, ctx.causal, ctx.window_size = softmax_scale, causal, window_size
        ctx.attention_chunk, ctx.softcap, ctx.deterministic, ctx.sm_margin = attention_chunk, softcap, deterministic, sm_margin
        ctx.has_qv = qv is not None
        if return_softmax:
            ctx.mark_non_differentiable(softmax_lse)
        return (out, softmax_lse) if return_softmax else out

    @staticmethod
    def backward(ctx, dout, *args):
        q, k, v, out, softmax_lse = ctx.saved_tensors
        assert ctx.attention_chunk == 0, "FA3 backward does not support attention_chunk"
        assert not ctx.has_qv, "FA3 backward does not support qv"  # (the reference has no qv backward)
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        _flash_attn_backward(dout, q, k, v, out, softmax_lse, None, None, None, None, None, None, dq, dk, dv,
                             ctx.softmax_scale, ctx.causal, ctx.window_size, ctx.softcap, ctx.deterministic, ctx.sm_margin)
        return (dq, dk, dv) + (None,) * 14


class FlashAttnVarlenFunc(torch.autograd.Function):
    """hopper/flash_attn_interface.py:342-442"""

    @staticmethod
    def forward(ctx, q, k, v, cu_seqlens_q, cu_seqlens_k, seqused_q, seqused_k, max_seqlen_q, max_seqlen_k, softmax_scale,
                causal, qv=None, q_descale=None, k_descale=None, v_descale=None, window_size=(-1, -1), attention_chunk=0,
                softcap=0.0, num_splits=1, pack_gqa=None, deterministic=False, sm_margin=0, return_softmax=False):
        if softmax_scale is None:
            softmax_scale = (q.shape[-1] + (qv.shape[-1] if qv is not None else 0)) ** (-0.5)
        out, softmax_lse, *_ = _flash_attn_forward(
            q, k, v, None, None, qv, None, cu_seqlens_q, cu_seqlens_k, None, seqused_q, seqused_k, max_seqlen_q,
            max_seqlen_k, None, None, None, None, None, None, q_descale, k_descale, v_descale, softmax_scale, causal=causal,
            window_size=window_size, attention_chunk=attention_chunk, softcap=softcap, num_splits=num_splits,
            pack_gqa=pack_gqa, sm_margin=sm_margin)
        ctx.save_for_backward(q, k, v, out, softmax_lse, cu_seqlens_q, cu_seqlens_k, seqused_q, seqused_k)
        ctx.max_seqlen_q, ctx.max_seqlen_k = max_seqlen_q, max_seqlen_k
        ctx.softmax_scale, ctx.causal, ctx.window_size = softmax_scale, causal, window_size
        ctx.attention_chunk, ctx.softcap, ctx.deterministic, ctx.sm_margin = attention_chunk, softcap, deterministic, sm_margin
        ctx.has_qv = qv is not None
        if return_softmax:
            ctx.mark_non_differentiable(softmax_lse)
        return (out, softmax_lse) if return_softmax else out

    @staticmethod
    def backward(ctx, dout, *args):
        q, k, v, out, softmax_lse, cu_seqlens_q, cu_seqlens_k, seqused_q, seqused_k = ctx.saved_tensors
        assert ctx.attention_chunk == 0, "FA3 backward does not support attention_chunk"
        assert not ctx.has_qv, "FA3 backward does not support qv"  # (the reference has no qv backward)
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        _flash_attn_backward(dout, q, k, v, out, softmax_lse, cu_seqlens_q, cu_seqlens_k, seqused_q, seqused_k,
                             ctx.max_seqlen_q, ctx.max_seqlen_k, dq, dk, dv, ctx.softmax_scale, ctx.causal, ctx.window_size,
                             ctx.softcap, ctx.deterministic, ctx.sm_margin)
        return (dq, dk, dv) + (None,) * 20


class FlashAttnQKVPackedFunc(torch.autograd.Function):
    """hopper/flash_attn_interface.py:157-251: qkv (b, s, 3, h, d), or (b, s, h_q + 2 h_k, d) with num_heads_q."""

    @staticmethod
    def forward(ctx, qkv, softmax_scale, causal, q_descale=None, k_descale=None, v_descale=None, window_size=(-1, -1),
                attention_chunk=0, softcap=0.0, deterministic=False, num_heads_q=None, sm_margin=0, return_softmax=False):
        if softmax_scale is None:
            softmax_scale = qkv.shape[-1] ** (-0.5)
        if qkv.dim() == 5:
            assert qkv.shape[-3] == 3
            q, k, v = qkv.unbind(dim=-3)
        else:
            assert qkv.dim() == 4
            assert num_heads_q is not None
            num_heads_k = (qkv.shape[2] - num_heads_q) // 2
            assert num_heads_k * 2 + num_heads_q == qkv.shape[2]
            q, k, v = qkv.split([num_heads_q, num_heads_k, num_heads_k], dim=-2)
        out, softmax_lse, *_ = _flash_attn_forward(
            q, k, v, None, None, None, None, None, None, None, None, None, None, None, None, None, None, None, None, None,
            q_descale, k_descale, v_descale, softmax_scale, causal=causal, window_size=window_size,
            attention_chunk=attention_chunk, softcap=softcap, sm_margin=sm_margin)
        ctx.save_for_backward(q, k, v, out, softmax_lse)
        ctx.softmax_scale, ctx.causal, ctx.window_size = softmax_scale, causal, window_size
        ctx.attention_chunk, ctx.softcap, ctx.deterministic, ctx.sm_margin = attention_chunk, softcap, deterministic, sm_margin
        ctx.ndim = qkv.dim()
        if return_softmax:
            ctx.mark_non_differentiable(softmax_lse)
        return (out, softmax_lse) if return_softmax else out

    @staticmethod
    def backward(ctx, dout, *args):
        q, k, v, out, softmax_lse = ctx.saved_tensors
        assert ctx.attention_chunk == 0, "FA3 backward does not support attention_chunk"
        if ctx.ndim == 5:
            dqkv = torch.empty(q.shape[:-2] + (3, *q.shape[-2:]), dtype=q.dtype, device=q.device)
            dq, dk, dv = dqkv.unbind(dim=-3)
        else:
            hq, hk = q.shape[2], k.shape[2]
            dqkv = torch.empty(q.shape[:-2] + (hq + 2 * hk, q.shape[-1]), dtype=q.dtype, device=q.device)
            dq, dk, dv = dqkv.split([hq, hk, hk], dim=-2)
        _flash_attn_backward(dout, q, k, v, out, softmax_lse, None, None, None, None, None, None, dq, dk, dv,
                             ctx.softmax_scale, ctx.causal, ctx.window_size, ctx.softcap, ctx.deterministic, ctx.sm_margin)
        return (dqkv,) + (None,) * 12


def flash_attn_qkvpacked_func(qkv, softmax_scale=None, causal=False, q_descale=None, k_descale=None, v_descale=None,
                              window_size=(-1, -1), attention_chunk=0, softcap=0.0, deterministic=False, num_heads_q=None,
                              sm_margin=0, return_attn_probs=False):
    """hopper/flash_attn_interface.py:445-504.  qkv: (batch, seqlen, 3, nheads, headdim) -- or (batch, seqlen,
    nheads_q + 2 nheads_k, headdim) with num_heads_q for GQA."""
    return FlashAttnQKVPackedFunc.apply(qkv, softmax_scale, causal, q_descale, k_descale, v_descale, window_size,
                                        attention_chunk, softcap, deterministic, num_heads_q, sm_margin, return_attn_probs)


def flash_attn_func(q, k, v, softmax_scale=None, causal=False, qv=None, q_descale=None, k_descale=None, v_descale=None,
                    window_size=(-1, -1), attention_chunk=0, softcap=0.0, num_splits=1, pack_gqa=None,
                    deterministic=False, sm_margin=0, return_attn_probs=False):
    """hopper/flash_attn_interface.py:507-585.  q: (batch, seqlen, nheads, headdim); k, v: (batch, seqlen_k, nheads_k,
    headdim); fp16 / bf16 (differentiable) / fp8 e4m3 (forward only, bf16 output).
    Returns out, or (out, softmax_lse (batch, nheads, seqlen)) when return_attn_probs.
    pack_gqa: True packs the nheads / nheads_k query heads of a kv head into the rows of a tile, one pass over K / V per kv head
    (pk_fwd_kernel: nheads > nheads_k, 16-bit inputs, headdim <= 128, no attention_chunk, qv or V headdim of its own; a no-op
    on every other call).  False and None run one workgroup per query head, as before: None does not pack by itself yet.  A
    performance hint: results agree to rounding, the backward is unaffected."""
    return FlashAttnFunc.apply(q, k, v, softmax_scale, causal, qv, q_descale, k_descale, v_descale, window_size,
                               attention_chunk, softcap, num_splits, pack_gqa, deterministic, sm_margin, return_attn_probs)


def flash_attn_varlen_func(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, seqused_q=None,
                           seqused_k=None, softmax_scale=None, causal=False, qv=None, q_descale=None, k_descale=None,
                           v_descale=None, window_size=(-1, -1), attention_chunk=0, softcap=0.0, num_splits=1,
                           pack_gqa=None, deterministic=False, sm_margin=0, return_attn_probs=False):
    """hopper/flash_attn_interface.py:588-633.  q: (total_q, nheads, headdim); k, v: (total_k, nheads_k, headdim);
    cu_seqlens_*: (batch+1,) int32; seqused_*: (batch,) int32, the part of each sequence that is actually used.
    pack_gqa: as in flash_attn_func (True = the PackGQA kernel, made for many short sequences; False / None = unpacked)."""
    return FlashAttnVarlenFunc.apply(q, k, v, cu_seqlens_q, cu_seqlens_k, seqused_q, seqused_k, max_seqlen_q, max_seqlen_k,
                                     softmax_scale, causal, qv, q_descale, k_descale, v_descale, window_size,
                                     attention_chunk, softcap, num_splits, pack_gqa, deterministic, sm_margin,
                                     return_attn_probs)


def flash_attn_combine(out_partial, lse_partial, out=None, out_dtype=None):
    """reference hopper/flash_attn_interface.py:636-637"""
    return torch.ops.flash_attn_3.fwd_combine(out_partial, lse_partial, out, out_dtype)


def flash_attn_with_kvcache(q, k_cache, v_cache, k=None, v=None, qv=None, rotary_cos=None, rotary_sin=None,
                            cache_seqlens=None, cache_batch_idx=None, cache_leftpad=None, page_table=None,
                            cu_seqlens_q=None, cu_seqlens_k_new=None, max_seqlen_q=None, rotary_seqlens=None,
                            q_descale=None, k_descale=None, v_descale=None, softmax_scale=None, causal=False,
                            window_size=(-1, -1), attention_chunk=0, softcap=0.0, rotary_interleaved=True,
                            scheduler_metadata=None, num_splits=0, pack_gqa=None, sm_margin=0, return_softmax_lse=False):
    """reference hopper/flash_attn_interface.py:640-800: attention over a KV cache, optionally appending k / v in place
    (rotated by rotary_cos / rotary_sin) first.  Paged caches: any page size.
    An fp8 cache (torch.float8_e4m3fn k_cache / v_cache under fp16 / bf16 q) is read through k_descale / v_descale, fp32
    (batch, nheads_k); with both given, k / v (fp16 / bf16, dense or ragged) are quantised into it in place first and
    rotary_cos / rotary_sin / rotary_seqlens apply as on a 16-bit cache (kvcache_append_fp8 below is that append alone).
    An fp8 cache of the MLA shape (headdim <= 64 beside headdim_v in [256, 512], qv optional) is read only by this call:
    kvcache_append_fp8 writes its rows, and the step is that call followed by this one on the fill levels it returns.
    pack_gqa: True runs the PackGQA kernel on the attention of the step -- dense or ragged (cu_seqlens_q) queries, batched or
    paged cache, split-KV -- so that a verify step of a few tokens or the decode rows of a mixed step share one pass over the
    cache per kv head; a single-token step keeps its own GQA fold and is unaffected.  False / None: unpacked, as before."""
    assert k_cache.stride(-1) == 1, "k_cache must have contiguous last dimension"
    assert v_cache.stride(-1) == 1, "v_cache must have contiguous last dimension"
    if softmax_scale is None:
        softmax_scale = (q.shape[-1] + (qv.shape[-1] if qv is not None else 0)) ** (-0.5)
    if cache_seqlens is not None and isinstance(cache_seqlens, int):
        cache_seqlens = torch.full((q.shape[0],), cache_seqlens, dtype=torch.int32, device=k_cache.device)
    out, softmax_lse, *rest = _flash_attn_forward(
        q, k_cache, v_cache, k, v, qv, None, cu_seqlens_q, None, cu_seqlens_k_new, None, cache_seqlens, max_seqlen_q, None,
        page_table, cache_batch_idx, cache_leftpad, rotary_cos, rotary_sin, rotary_seqlens, q_descale, k_descale, v_descale,
        softmax_scale, causal=causal, window_size=window_size, attention_chunk=attention_chunk, softcap=softcap,
        rotary_interleaved=rotary_interleaved, scheduler_metadata=scheduler_metadata, num_splits=num_splits,
        pack_gqa=pack_gqa, sm_margin=sm_margin)
    return (out, softmax_lse, *rest) if return_softmax_lse else out


def flash_attn_with_kvcache_sparse(q, k_cache, v_cache, kv_block_cnt, kv_block_idx, *, kv_block_size=128, cache_seqlens=None,
                                   cache_batch_idx=None, cache_leftpad=None, page_table=None, cu_seqlens_q=None, max_seqlen_q=None,
                                   k_descale=None, v_descale=None, softmax_scale=None, causal=False, window_size=(-1, -1),
                                   softcap=0.0, num_splits=0, return_softmax_lse=False):
    """Block-sparse attention over a KV cache: a decode, verify or ragged serving step that reads only the key blocks a
    selection step listed (Quest-style page selection, NSA-style selected blocks shared by a GQA group).  Not in the reference.
    q: (batch, seqlen_q, nheads, headdim), or (total_q, nheads, headdim) with cu_seqlens_q + max_seqlen_q; fp16 / bf16,
    headdim <= 128 and a multiple of 16.  k_cache / v_cache: as in flash_attn_with_kvcache (batched with cache_batch_idx /
    cache_leftpad, or pages of any size behind page_table), of q's dtype or torch.float8_e4m3fn; the fp8 case takes both
    k_descale / v_descale, fp32 (batch, nheads_k).
    kv_block_cnt: int32 (batch | 1, nheads_k | 1); kv_block_idx: int32 (batch | 1, nheads_k | 1, max_blocks), on the device; a
    dimension of size 1 is shared.  With B = kv_block_size (a multiple of 64), g = nheads / nheads_k and sk(b) the fill level
    of batch entry b (cache_seqlens, clamped to the capacity, minus cache_leftpad), key j of batch b is visible to query row i of
    head h iff
      * j < sk(b),
      * causal / window_size / softcap allow (i, j) exactly as in flash_attn_with_kvcache (bottom-right aligned on sk(b)), and
      * j // B is among the first min(kv_block_cnt[b, h // g], max_blocks) entries of kv_block_idx[b, h // g, :].
    Lists are per KV head: every query row of the call and every head of the GQA group share them, and with them one pass over
    the listed blocks.  Entries may come in any order (rounding only).  An entry outside [0, ceil(sk(b) / B)) is skipped without
    touching memory, entries at or behind the count are never used as addresses; distinct entries are the caller's duty (a
    duplicate counts twice).  A row with no visible key gives out = 0, lse = +inf.
    The walk: list position t in [0, cnt * B / 64) is entry t // (B / 64), 64-key sub-tile t % (B / 64); the next entry is
    fetched one step ahead.  num_splits: 1 = off, N = N parts of the list POSITIONS (not of the key range), 0 = the count the
    PackGQA shape gets for a key length of max_blocks * B -- from shapes only.  Nothing of the lists is read on the host and
    nothing synchronises: the call can be captured into a HIP graph, and a replay after the lists were overwritten in place
    computes the new selection.
    Read-only: append with flash_attn_with_kvcache(k=, v=) or kvcache_append_fp8 first, then call this on the new fill levels.
    No qv, learnable sink, attention_chunk or V headdim of its own, and no backward.
    Cost, measured on MI355X (tools/sparse_kv_decode_bench.py, profiles/sparse_kv_decode.jsonl; hq32 / hkv8 d128, page 64,
    B = 128, cache 8192 / 32768, batch 1 / 8 / 64): time ~ fixed cost (15 - 27 us) + listed bytes (4.0 - 5.6 TB/s at cache 32768, batch 64).
    Over an fp8 cache, all blocks listed costs 1.01 - 1.09 x flash_attn_with_kvcache on the same cache (the price of the walk)
    and this call wins below a listed fraction of 0.85 - 0.99; over a bf16 cache it is 0.78 - 0.91 x that call (whose decode
    is the GQA-folded kernel, not the packed-row one) even with every block listed.  DESIGN.md section 4.20.
    Returns out, or (out, softmax_lse) when return_softmax_lse: (batch, nheads, seqlen_q), ragged (nheads, total_q)."""
    assert k_cache.stride(-1) == 1, "k_cache must have contiguous last dimension"
    assert v_cache.stride(-1) == 1, "v_cache must have contiguous last dimension"
    if cache_seqlens is not None and isinstance(cache_seqlens, int):
        cache_seqlens = torch.full((q.shape[0],), cache_seqlens, dtype=torch.int32, device=k_cache.device)
    out, softmax_lse = torch.ops.flash_attn_3.fwd_kvcache_sparse(
        q, k_cache, v_cache, kv_block_cnt, kv_block_idx, kv_block_size, cache_seqlens, cache_batch_idx, cache_leftpad, page_table,
        cu_seqlens_q, max_seqlen_q, k_descale, v_descale, softmax_scale, causal, window_size[0], window_size[1], softcap, num_splits)
    return (out, softmax_lse) if return_softmax_lse else out


def flash_attn_with_kvcache_tree(q, k_cache, v_cache, tree_mask, *, cache_seqlens=None, cache_batch_idx=None, cache_leftpad=None,
                                 page_table=None, cu_seqlens_q=None, max_seqlen_q=None, k_descale=None, v_descale=None,
                                 softmax_scale=None, softcap=0.0, num_splits=0, return_softmax_lse=False):
    """Tree attention over a KV cache: the verify step of speculative decoding whose draft is a token TREE (Medusa, EAGLE-2,
    SpecInfer, sequoia) of up to 64 nodes, verified in one pass.  Not in the reference.
    q: (batch, T, nheads, headdim), or (total_q, nheads, headdim) with cu_seqlens_q + max_seqlen_q; fp16 / bf16, headdim <= 128
    and a multiple of 16; T / max_seqlen_q <= 64.  The rows of batch entry b are the sq(b) nodes of its tree (T, or from
    cu_seqlens_q).  k_cache / v_cache: as in flash_attn_with_kvcache (batched with cache_batch_idx / cache_leftpad, or pages of
    any size behind page_table), of q's dtype or torch.float8_e4m3fn; the fp8 case takes both k_descale / v_descale, fp32
    (batch, nheads_k).  sk(b) is the fill level of the cache INCLUDING the sq(b) draft tokens, which the caller appended at
    positions [sk(b) - sq(b), sk(b)): cache_seqlens, clamped to the capacity, minus cache_leftpad.
    tree_mask: int64 (batch, T), or (total_q,) for ragged queries, on the device (any strides).  With shift = sk(b) - sq(b) and
    t = j - shift, key j of batch b is visible to query row i of any head iff
      * j < sk(b), and
      * t < 0, or (t < 64 and bit t of tree_mask[b, i] is set): the committed prefix (t < 0) is seen by every node, a draft key
        by the nodes whose word names it -- their ancestors and themselves (tree_mask_from_parents builds such words).
    softcap applies as elsewhere.  Bits at or above sq(b) are ignored.  A draft key with t >= 64 is invisible: T / max_seqlen_q
    above 64 is refused, and a ragged entry that is longer at run time falls under this rule, without a fault.  No structure is
    assumed of the words: they need not be lower-triangular, and the diagonal bit is the caller's duty.  A chain (row i = bits
    0 .. i) is causal=True of flash_attn_with_kvcache.  A row with no visible key gives out = 0, lse = +inf.
    Positions in a tree are depths, not indices, so there is no rotary here: rotate q and k by the depth of each node yourself
    before the append.  Read-only: append the draft with flash_attn_with_kvcache(k=, v=) or kvcache_append_fp8 first, then call
    this on the new fill levels; kvcache_keep_tree_path_ compacts the cache to the accepted path afterwards.
    The kernel is the PackGQA body (the nheads / nheads_k heads of a group share one pass over the cache, T * g rows fill the
    tiles); only the at most two 64-key tiles that hold draft keys take the mask.  num_splits: 1 = off, N = N parts of the key
    range, 0 = the count the PackGQA shape gets -- from shapes only.  Nothing of tree_mask or cache_seqlens is read on the host
    and nothing synchronises: the call can be captured into a HIP graph, and a replay after both were overwritten in place
    computes the new tree.
    No causal / window_size (the words are the mask), qv, learnable sink, ALiBi, dropout, attention_chunk, rotary or V headdim of
    its own, and no backward.
    Cost, measured on MI355X (tools/tree_verify_bench.py, profiles/tree_verify.jsonl; hq32 / hkv8 d128, page 64, cache 8192 /
    32768, batch 1 / 8 / 64, T = 16 / 64): 0.94 - 1.03 x flash_attn_with_kvcache(causal=True, pack_gqa=True) on a chain over the
    same bf16 cache, 0.97 - 1.00 x over an e4m3 cache, the same for a random forest; a chain's output is bit-equal to that
    call's.  DESIGN.md section 4.31.
    Returns out, or (out, softmax_lse) when return_softmax_lse: (batch, nheads, T), ragged (nheads, total_q)."""
    assert k_cache.stride(-1) == 1, "k_cache must have contiguous last dimension"
    assert v_cache.stride(-1) == 1, "v_cache must have contiguous last dimension"
    if cache_seqlens is not None and isinstance(cache_seqlens, int):
        cache_seqlens = torch.full((q.shape[0],), cache_seqlens, dtype=torch.int32, device=k_cache.device)
    out, softmax_lse = torch.ops.flash_attn_3.fwd_kvcache_tree(
        q, k_cache, v_cache, tree_mask, cache_seqlens, cache_batch_idx, cache_leftpad, page_table, cu_seqlens_q, max_seqlen_q,
        k_descale, v_descale, softmax_scale, softcap, num_splits)
    return (out, softmax_lse) if return_softmax_lse else out


def _bit(i):
    """Bit i of a word as an int64 value (bit 63 is the sign)."""
    return (1 << i) - (1 << 64 if i == 63 else 0)


def tree_mask_from_parents(parents):
    """The words flash_attn_with_kvcache_tree takes, from the parent of every node.  parents: int (batch, T), T <= 64, on any
    device; parents[b, i] < i is the parent of node i, -1 marks a root (a forest is fine).  Returns int64 (batch, T): bit j of
    word i is set iff j is i or an ancestor of i.  A parent precedes its child, so one pass in node order closes the relation:
    T steps of fixed shape, no host sync."""
    assert parents.dim() == 2 and parents.shape[1] <= 64, "parents must be (batch, T) with T <= 64"
    b, T = parents.shape
    parents = parents.long()
    words = torch.zeros((b, T), dtype=torch.int64, device=parents.device)
    for i in range(T):
        par = parents[:, i]
        up = words.gather(1, par.clamp(0, max(i - 1, 0))[:, None])[:, 0]  # (the word of the parent is complete: it precedes i)
        words[:, i] = torch.where((par >= 0) & (par < i), up, torch.zeros_like(up)) | _bit(i)
    return words


def tree_visibility(words, sk, num_keys):
    """The definition of flash_attn_with_kvcache_tree for one batch entry, explicitly: words int64 (sq,), sk the fill level
    including the sq draft keys -> bool (sq, num_keys), [i, j] = key j is visible to row i."""
    sq = words.shape[0]
    t = torch.arange(num_keys, device=words.device) - (sk - sq)
    bits = (words[:, None] >> t.clamp(0, 63)[None, :]) & 1
    tree = (t >= 0) & (t < min(sq, 64))
    return (t + (sk - sq) < sk)[None, :] & ((t < 0)[None, :] | (tree[None, :] & (bits != 0)))


def tree_attention_ref(q, k_cache, v_cache, tree_mask, *, cache_seqlens=None, cache_batch_idx=None, cache_leftpad=None,
                       page_table=None, cu_seqlens_q=None, max_seqlen_q=None, k_descale=None, v_descale=None, softmax_scale=None,
                       softcap=0.0, num_splits=0, return_softmax_lse=False):
    """The oracle of flash_attn_with_kvcache_tree in plain torch, on any device, under the same arguments: a host loop over the
    batch entries that gathers the logical cache (pages, cache_batch_idx, cache_leftpad; an fp8 cache dequantised exactly, value
    times descale), builds the explicit visibility (tree_visibility) and takes the softmax in fp64.  num_splits changes nothing.
    Returns out in fp64 with q's shape, or (out, lse) when return_softmax_lse: lse fp64 (batch, nheads, T), ragged
    (nheads, total_q); a row with no visible key gives out = 0, lse = +inf."""
    ragged = cu_seqlens_q is not None
    batch = cu_seqlens_q.numel() - 1 if ragged else q.shape[0]
    h, d, h_k = q.shape[-2], q.shape[-1], k_cache.shape[2]
    g = h // h_k
    scale = d ** -0.5 if softmax_scale is None else softmax_scale
    out = torch.zeros(q.shape, dtype=torch.float64, device=q.device)
    lse = torch.full((h, q.shape[0]) if ragged else (batch, h, q.shape[1]), float("inf"), dtype=torch.float64, device=q.device)
    for b in range(batch):
        rows = slice(int(cu_seqlens_q[b]), int(cu_seqlens_q[b + 1])) if ragged else slice(None)
        qb = (q[rows] if ragged else q[b]).double()                     # (sq, h, d)
        words = tree_mask[rows] if ragged else tree_mask[b]
        fp8 = k_cache.dtype == torch.float8_e4m3fn
        kc, vc = (c.view(torch.uint8) if fp8 else c for c in (k_cache, v_cache))  # (indexing needs no fp8 kernel)
        if page_table is not None:
            kb, vb = (c[page_table[b].long()].flatten(0, 1) for c in (kc, vc))
        else:
            slot = b if cache_batch_idx is None else int(cache_batch_idx[b])
            kb, vb = kc[slot], vc[slot]
        if fp8:
            kb, vb = kb.view(k_cache.dtype).float(), vb.view(k_cache.dtype).float()
        cap = kb.shape[0]
        sk = cap if cache_seqlens is None else min(int(cache_seqlens[b]), cap)
        lp = 0 if cache_leftpad is None else int(cache_leftpad[b])
        sk = max(sk - lp, 0)
        kb, vb = kb[lp:].double(), vb[lp:].double()                     # (keys, h_k, d): every e4m3 / 16-bit value is an fp64 value
        if k_descale is not None:
            kb, vb = kb * k_descale[b].double()[None, :, None], vb * v_descale[b].double()[None, :, None]
        vis = tree_visibility(words, sk, kb.shape[0])                   # (sq, keys)
        s = torch.einsum("qhd,khd->hqk", qb, kb.repeat_interleave(g, dim=1)) * scale
        if softcap > 0:
            s = softcap * torch.tanh(s / softcap)
        s = s.masked_fill(~vis[None], float("-inf"))
        l = torch.logsumexp(s, dim=-1)                                  # (h, sq); -inf where nothing is visible
        p = torch.exp(s - l.masked_fill(torch.isinf(l), 0.0)[..., None])
        o = torch.einsum("hqk,khd->qhd", p, vb.repeat_interleave(g, dim=1))
        l = l.masked_fill(torch.isinf(l), float("inf"))
        if ragged:
            out[rows], lse[:, rows] = o, l
        else:
            out[b], lse[b] = o, l
    return (out, lse) if return_softmax_lse else out


def kvcache_keep_tree_path_(k_cache, v_cache, cache_seqlens, path, path_len, *, page_table=None, cache_batch_idx=None):
    """After a tree was verified: keeps the accepted root-to-leaf path of the draft and drops the rest, in place.
    cache_seqlens: int32 (batch,), the fill levels of the committed prefix -- the `shift` of flash_attn_with_kvcache_tree, i.e. the
    levels BEFORE the draft was appended (the tree call's cache_seqlens minus its node count); the draft occupies the rows from
    there on.  path: int32 (batch, P), node indices in ascending order, the first path_len[b] (int32 (batch,)) of them valid.
    Moves the K / V rows of the accepted nodes from shift + path[b, j] to shift + j and returns the new fill levels
    shift + path_len (int32 (batch,)); what lies behind them is stale.  Positions count from the start of a cache entry (no
    cache_leftpad).  Torch indexing on any device, the right-hand side gathered before anything is written, so overlapping moves
    are safe; works on 16-bit caches and on the bytes of an fp8 cache alike; no host sync."""
    shift, n = cache_seqlens.long()[:, None], path_len.long()[:, None]
    P = path.shape[1]
    j = torch.arange(P, device=path.device)[None, :]
    paged = page_table is not None
    cap = page_table.shape[1] * k_cache.shape[1] if paged else k_cache.shape[1]
    dst = (shift + j).clamp(0, cap - 1)
    src = torch.where(j < n, (shift + path.long()).clamp(0, cap - 1), dst)  # (behind the path: a row onto itself)
    if paged:
        page = k_cache.shape[1]
        at = lambda pos: (page_table.long().gather(1, pos // page), pos % page)
    else:
        slot = torch.arange(path.shape[0], device=path.device) if cache_batch_idx is None else cache_batch_idx.long()
        at = lambda pos: (slot[:, None].expand_as(pos), pos)
    for cache in (k_cache, v_cache):
        raw = cache.view(torch.uint8) if cache.dtype == torch.float8_e4m3fn else cache  # (indexing needs no fp8 kernel)
        kept = raw[at(src)]
        raw[at(dst)] = kept
    return (cache_seqlens + path_len).to(torch.int32)


def kvcache_append_fp8(k_cache, v_cache, k, v, cache_seqlens, k_descale, v_descale, *, cu_seqlens_k_new=None,
                       max_seqlen_k_new=None, cache_batch_idx=None, page_table=None, rotary_cos=None, rotary_sin=None,
                       rotary_seqlens=None, rotary_interleaved=True):
    """The write half of an fp8 KV cache on its own (the role of a `reshape_and_cache` op): the fp16 / bf16 rows k / v --
    (batch, seqlen_new, nheads_k, headdim), or (total_k_new, nheads_k, headdim) with cu_seqlens_k_new -- are quantised into the
    torch.float8_e4m3fn caches in place at cache_seqlens[b] + i (through cache_batch_idx or page_table, any page size): keys
    rotated like the 16-bit append rotates them, then x / descale[b, head] clamped to +-448 and rounded to nearest even.  Rows
    past the capacity are dropped.  k_descale / v_descale: fp32 (batch, nheads_k), the factors flash_attn_with_kvcache
    dequantises by.  One launch, no host sync (HIP-graph capturable).  Returns the new fill levels
    min(cache_seqlens + new rows, capacity), int32 (batch,) on the device; cache_seqlens itself is not modified.
    flash_attn_with_kvcache(q, k_cache, v_cache, k=, v=, k_descale=, v_descale=, ...) runs the same append in front of the
    attention.
    The MLA shape -- k_cache (..., nheads_k, headdim <= 64) beside v_cache (..., nheads_k, headdim_v in [256, 512]), k the k_pe
    rows and v the latent rows of headdim_v -- is appended by a kernel of its own under the same rules.  There the fused call
    only reads, so a step is two calls, without a host sync in between:
        fill = kvcache_append_fp8(k_cache, v_cache, k_pe, latent, cache_seqlens, k_descale, v_descale, rotary_cos=, ...)
        out = flash_attn_with_kvcache(q, k_cache, v_cache, qv=, cache_seqlens=fill, k_descale=, v_descale=, ...)
    with q rotated by the caller."""
    return torch.ops.flash_attn_3.kvcache_append_fp8(k_cache, v_cache, k, v, cache_seqlens, k_descale, v_descale,
                                                     cu_seqlens_k_new, max_seqlen_k_new, cache_batch_idx, page_table,
                                                     rotary_cos, rotary_sin, rotary_seqlens, rotary_interleaved)


def kvcache_block_summary_update(k_summary, k_cache, seqlens_old, seqlens_new, *, kv_block_size=128, max_seqlen_new=None,
                                 cache_batch_idx=None, page_table=None):
    """Keeps the per-block summaries of the keys of a KV cache up to date: what kvcache_select_blocks ranks blocks by.  Not in the
    reference.  One launch, in place, no host sync (HIP-graph capturable); include/fa_block_select.h pins the rule.
    k_summary: (slots, max_blocks, 2, nheads_k, headdim) fp16 / bf16 (the dtype of the queries), last dimension contiguous;
    [s, j, 0] / [s, j, 1] are the channel-wise minimum / maximum over the filled rows of block j (kv_block_size rows, a multiple of
    64) of slot s.  Dense cache: slots = k_cache.shape[0] and entry b uses slot cache_batch_idx[b] (or b).  Paged cache: slots = the
    batch, blocks are logical (any page size; a block may span pages).  max_blocks * kv_block_size must cover the capacity.
    k_cache: of k_summary's dtype, or torch.float8_e4m3fn, whose stored values count as they are (no descale: a positive factor
    per (batch, head) changes no ranking).  Call it after the append: it reads what attention will read, rotated and quantised.
    seqlens_old / seqlens_new: int32 (batch,) on the device; rows [old, new) were just written.  seqlens_old=None: 0, a rebuild.
    A block that begins inside the range is set from its rows, the block the range begins in is merged (min / max) with what is
    stored, blocks outside the range are not written.  max_seqlen_new: a host bound of new - old that sizes the grid (None: the
    capacity; give 1 in a decode step).  Minimum and maximum are exact: the result equals block_summary_ref bit for bit.
    CPU tensors take block_summary_ref.  Returns k_summary."""
    if not k_summary.is_cuda:
        return block_summary_ref(k_summary, k_cache, seqlens_old, seqlens_new, kv_block_size=kv_block_size,
                                 cache_batch_idx=cache_batch_idx, page_table=page_table)
    torch.ops.flash_attn_3.kvcache_block_summary_update(k_summary, k_cache, seqlens_old, seqlens_new, kv_block_size, max_seqlen_new,
                                                        cache_batch_idx, page_table)
    return k_summary


def kvcache_select_blocks(q, k_summary, cache_seqlens, num_blocks, *, kv_block_size=128, sink_blocks=1, local_blocks=1,
                          group_reduce="max", cache_batch_idx=None, kv_block_cnt=None, kv_block_idx=None, return_scores=False):
    """Quest selection (arXiv 2406.10774) of the key blocks a decode or verify step reads: the lists flash_attn_with_kvcache_sparse
    takes, from the queries and the summaries kvcache_block_summary_update keeps.  Not in the reference.  Two launches (scores split
    over chunks of blocks, so that batch 1 fills the chip; then one workgroup per (batch, kv head) selects), no host sync, no sort;
    HIP-graph capturable with kv_block_cnt / kv_block_idx given.  include/fa_block_select.h pins the rule.
    q: (batch, seqlen_q, nheads, headdim) fp16 / bf16, headdim <= 128 and a multiple of 16, seqlen_q * nheads / nheads_k <= 128.
    With B = kv_block_size, sk(b) = cache_seqlens[b] clamped to max_blocks * B and n = ceil(sk / B): the score of block j for kv
    head hk is U = sum_c max(q_c * min_c, q_c * max_c) (an upper bound of q . k over the block's keys; fp32, unscaled) reduced over
    the seqlen_q * nheads / nheads_k query rows of hk by group_reduce, "max" or "sum".  K = min(num_blocks, n) blocks are chosen:
    the first sink_blocks and the last local_blocks always, the rest by the highest score, equal scores by the lower index.
    Returns (kv_block_cnt, kv_block_idx): int32 (batch, nheads_k) = K and (batch, nheads_k, width >= num_blocks) holding the chosen
    blocks ascending, then -1; fresh tensors (width = num_blocks) or the buffers given.  return_scores: also scores, fp32
    (batch, nheads_k, max_blocks), -inf at and behind n.  max_blocks <= 8192.  CPU tensors take select_blocks_ref.
    Cost, measured on MI355X: tools/block_select_bench.py, profiles/block_select.jsonl, DESIGN.md section 4.29."""
    b, h_k, max_blocks = q.shape[0], k_summary.shape[3], k_summary.shape[1]
    if kv_block_cnt is None:
        kv_block_cnt = torch.empty((b, h_k), dtype=torch.int32, device=q.device)
    if kv_block_idx is None:
        kv_block_idx = torch.empty((b, h_k, num_blocks), dtype=torch.int32, device=q.device)
    if not q.is_cuda:
        ref = select_blocks_ref(q, k_summary, cache_seqlens, num_blocks, kv_block_size=kv_block_size, sink_blocks=sink_blocks,
                                local_blocks=local_blocks, group_reduce=group_reduce, cache_batch_idx=cache_batch_idx,
                                width=kv_block_idx.shape[2])
        kv_block_cnt.copy_(ref.cnt), kv_block_idx.copy_(ref.idx)
        return (kv_block_cnt, kv_block_idx, ref.scores.float()) if return_scores else (kv_block_cnt, kv_block_idx)
    scores = torch.empty((b, h_k, max_blocks), dtype=torch.float32, device=q.device)
    torch.ops.flash_attn_3.kvcache_select_blocks(q, k_summary, cache_seqlens, num_blocks, kv_block_size, sink_blocks, local_blocks,
                                                 group_reduce, cache_batch_idx, kv_block_cnt, kv_block_idx, scores)
    return (kv_block_cnt, kv_block_idx, scores) if return_scores else (kv_block_cnt, kv_block_idx)


def _check_blocks(kv_block_size, num_blocks=0, sink_blocks=0, local_blocks=0, group_reduce="max"):
    assert kv_block_size > 0 and kv_block_size % 64 == 0, "kv_block_size must be a positive multiple of 64"
    assert group_reduce in ("max", "sum"), 'group_reduce must be "max" or "sum"'
    assert sink_blocks >= 0 and local_blocks >= 0 and num_blocks >= sink_blocks + local_blocks, \
        "num_blocks must be at least sink_blocks + local_blocks"


def block_summary_ref(k_summary, k_cache, seqlens_old, seqlens_new, *, kv_block_size=128, cache_batch_idx=None, page_table=None):
    """The oracle of kvcache_block_summary_update in plain torch, on any device, in place: a host loop over batch entries and
    blocks.  Minimum and maximum are exact, so the kernel's result equals this one."""
    _check_blocks(kv_block_size)
    B, paged = kv_block_size, page_table is not None
    capacity = page_table.shape[1] * k_cache.shape[1] if paged else k_cache.shape[1]
    assert k_summary.shape[1] * B >= capacity, "k_summary: max_blocks * kv_block_size must cover the capacity"
    raw = k_cache.view(torch.uint8) if k_cache.dtype == torch.float8_e4m3fn else k_cache  # (indexing needs no fp8 kernel)
    for b in range(seqlens_new.numel()):
        new = min(max(int(seqlens_new[b]), 0), capacity)
        old = 0 if seqlens_old is None else min(max(int(seqlens_old[b]), 0), new)
        slot = b if paged or cache_batch_idx is None else int(cache_batch_idx[b])
        for j in range(old // B, -(-new // B) if old < new else 0):
            lo, hi = max(old, j * B), min(new, (j + 1) * B)
            if paged:
                t = torch.arange(lo, hi, device=k_cache.device)
                rows = raw[page_table[b].long()[t // k_cache.shape[1]], t % k_cache.shape[1]]
            else:
                rows = raw[slot, lo:hi]
            rows = rows.view(k_cache.dtype).float()  # every fp16 / bf16 / e4m3 value is an fp32 value
            mn, mx = rows.amin(0), rows.amax(0)
            if old > j * B:
                mn, mx = torch.minimum(mn, k_summary[slot, j, 0].float()), torch.maximum(mx, k_summary[slot, j, 1].float())
            k_summary[slot, j, 0], k_summary[slot, j, 1] = mn.to(k_summary.dtype), mx.to(k_summary.dtype)
    return k_summary


class SelectedBlocks(NamedTuple):
    """select_blocks_ref's result.  U, A: fp64 (batch, nheads_k, rows, max_blocks), rows = seqlen_q * nheads / nheads_k in the
    order (query row, head of the group): the Quest bound of every row, and A = sum_c max(|q_c min_c|, |q_c max_c|), what an fp32
    sum of the terms of U errs in proportion to; both 0 at and behind n.  scores: fp64 (batch, nheads_k, max_blocks), U reduced
    over the rows, -inf at and behind n."""
    cnt: torch.Tensor
    idx: torch.Tensor
    scores: torch.Tensor
    U: torch.Tensor
    A: torch.Tensor


def select_blocks_ref(q, k_summary, cache_seqlens, num_blocks, *, kv_block_size=128, sink_blocks=1, local_blocks=1,
                      group_reduce="max", cache_batch_idx=None, width=None):
    """The oracle of kvcache_select_blocks in plain torch, on any device: U in fp64, the choice by a stable sort."""
    _check_blocks(kv_block_size, num_blocks, sink_blocks, local_blocks, group_reduce)
    b, s_q, h, d = q.shape
    max_blocks, h_k = k_summary.shape[1], k_summary.shape[3]
    g = h // h_k
    assert h % h_k == 0 and 1 <= s_q * g <= 128 and d == k_summary.shape[4]
    width = num_blocks if width is None else width
    assert width >= num_blocks, "the list must be at least num_blocks wide"
    dev = q.device
    cnt = torch.zeros((b, h_k), dtype=torch.int32, device=dev)
    idx = torch.full((b, h_k, width), -1, dtype=torch.int32, device=dev)
    scores = torch.full((b, h_k, max_blocks), float("-inf"), dtype=torch.float64, device=dev)
    U = torch.zeros((b, h_k, s_q * g, max_blocks), dtype=torch.float64, device=dev)
    A = torch.zeros_like(U)
    for i in range(b):
        sk = min(max(int(cache_seqlens[i]), 0), max_blocks * kv_block_size)
        n = -(-sk // kv_block_size)
        if n == 0:
            continue
        slot = i if cache_batch_idx is None else int(cache_batch_idx[i])
        K = min(num_blocks, n)
        forced = torch.zeros(n, dtype=torch.bool, device=dev)
        forced[:min(sink_blocks, n)] = True
        forced[max(n - local_blocks, 0):] = True
        for hk in range(h_k):
            rows = q[i, :, hk * g:(hk + 1) * g].reshape(s_q * g, 1, d).double()
            lo, hi = k_summary[slot, :n, 0, hk].double(), k_summary[slot, :n, 1, hk].double()  # (n, d)
            U[i, hk, :, :n] = torch.maximum(rows * lo, rows * hi).sum(-1)
            A[i, hk, :, :n] = torch.maximum((rows * lo).abs(), (rows * hi).abs()).sum(-1)
            u = U[i, hk, :, :n].amax(0) if group_reduce == "max" else U[i, hk, :, :n].sum(0)
            scores[i, hk, :n] = u
            free = (~forced).nonzero().flatten()
            order = torch.sort(-u[free], stable=True).indices[:K - int(forced.sum())]  # equal scores: the lower index first
            chosen = forced.clone()
            chosen[free[order]] = True
            cnt[i, hk] = K
            idx[i, hk, :K] = chosen.nonzero().flatten().int()
    return SelectedBlocks(cnt, idx, scores, U, A)


def get_scheduler_metadata(batch_size, max_seqlen_q, max_seqlen_k, num_heads_q, num_heads_kv, headdim, cache_seqlens,
                           qkv_dtype=torch.bfloat16, headdim_v=None, cu_seqlens_q=None, cu_seqlens_k_new=None,
                           cache_leftpad=None, page_size=None, max_seqlen_k_new=0, causal=False, window_size=(-1, -1),
                           attention_chunk=0, has_softcap=False, num_splits=0, pack_gqa=None, sm_margin=0):
    """hopper/flash_attn_interface.py:803-845.  The tile schedule of this build is computed inside the kernel: the
    returned tensor is opaque, and `scheduler_metadata=` is accepted and ignored by the forward."""
    if headdim_v is None:
        headdim_v = headdim
    return torch.ops.flash_attn_3.get_scheduler_metadata(
        batch_size, max_seqlen_q, max_seqlen_k, num_heads_q, num_heads_kv, headdim, headdim_v, qkv_dtype,
        maybe_contiguous(cache_seqlens), cu_seqlens_q, None, cu_seqlens_k_new, None, cache_leftpad, page_size,
        max_seqlen_k_new, causal, window_size[0], window_size[1], attention_chunk, has_softcap, num_splits, pack_gqa,
        sm_margin)
