"""The reference's newest public API -- names, argument order and defaults of `flash_attn/cute/interface.py`
(`flash_attn_func` :1141-1175, `flash_attn_varlen_func` :1177-1210) -- on the gfx950 kernels.  This is the surface that
carries `learnable_sink`: one logit per query head that joins the softmax denominator and contributes no value
(include/fa_fwd.h has the definition, DESIGN.md §4.12 the kernels).  Both functions return `(out, lse)` and are
differentiable; with a sink that requires grad the backward also returns its gradient (the reference's sink is
forward-only).

Routing is the FA3 surface's (csrc/torch_binding.cpp cute_fwd -> fa3_fwd_core): dense and varlen calls, decode steps over
a paged cache with their GQA swap and split-KV, ragged queries over a cache.  The cute signatures carry no max_seqlen:
the grid is made from bounds the shapes give (total_q / total_k), nothing is read from the device.
"""
import math

import torch

from . import _lib


def maybe_contiguous(x):
    return x.contiguous() if x is not None and x.stride(-1) != 1 else x


def _check_block_sparse(mask_mod=None, **tensors):
    given = [n for n, t in dict(mask_mod=mask_mod, **tensors).items() if t is not None]
    if given:
        raise NotImplementedError(
            f"This flash attention build does not support {', '.join(given)} (mask_mod and the block-sparse tensors "
            f"full_block_cnt / full_block_idx / mask_block_cnt / mask_block_idx)")


def _window(window_size):
    left, right = window_size
    return (-1 if left is None else int(left)), (-1 if right is None else int(right))


def _checks(q, k, v, cu_seqlens_q, cu_seqlens_k, seqused_q, seqused_k, page_table, learnable_sink):
    """flash_attn/cute/interface.py:116-194, the checks that do not depend on its kernels."""
    num_head, head_dim = q.shape[-2:]
    if cu_seqlens_q is None:
        assert q.dim() == 4, "q must have shape (batch_size, seqlen_q, num_head, head_dim) without cu_seqlens_q"
        batch_size = q.shape[0]
    else:
        assert q.dim() == 3, "q must have shape (total_q, num_head, head_dim) with cu_seqlens_q"
        batch_size = cu_seqlens_q.shape[0] - 1
    if page_table is not None:
        assert cu_seqlens_k is None, "page_table is not supported with cu_seqlens_k"
        assert page_table.dtype == torch.int32, "page_table must be int32"
        assert page_table.stride(-1) == 1, "page_table must be contiguous in the last dimension"
        assert page_table.dim() == 2 and page_table.shape[0] == batch_size
    if cu_seqlens_k is not None:
        assert cu_seqlens_k.shape == (batch_size + 1,), "cu_seqlens_k must have shape (batch_size + 1,)"
    if cu_seqlens_q is not None:
        assert cu_seqlens_q.shape == (batch_size + 1,), "cu_seqlens_q must have shape (batch_size + 1,)"
    assert seqused_q is None or seqused_q.shape == (batch_size,), "seqused_q must have shape (batch_size,)"
    assert seqused_k is None or seqused_k.shape == (batch_size,), "seqused_k must have shape (batch_size,)"
    assert q.dtype in [torch.float16, torch.bfloat16], "inputs must be float16 or bfloat16"
    assert q.dtype == k.dtype == v.dtype, "inputs must have the same dtype"
    for t in [cu_seqlens_q, cu_seqlens_k, seqused_q, seqused_k]:
        if t is not None:
            assert t.dtype == torch.int32, "cu_seqlens_q, cu_seqlens_k, seqused_q, seqused_k must be int32"
            assert t.stride(0) == 1, "cu_seqlens_q, cu_seqlens_k, seqused_q, seqused_k must be contiguous"
    if learnable_sink is not None:
        assert learnable_sink.shape == (num_head,), "learnable_sink must have shape (num_head,)"
        # (the reference takes bfloat16 only; parameters are often kept in fp32, which is taken as well)
        assert learnable_sink.dtype in (torch.bfloat16, torch.float32), "learnable_sink must be bfloat16 (or float32)"
    assert all(t is None or t.is_cuda for t in (q, k, v, cu_seqlens_q, cu_seqlens_k, seqused_q, seqused_k, page_table,
                                                learnable_sink)), "inputs must be on CUDA device"
    assert all(t is None or t.device == q.device for t in (k, v, cu_seqlens_q, cu_seqlens_k, seqused_q, seqused_k, page_table,
                                                           learnable_sink)), "inputs must be on the same device"
    assert num_head % k.shape[-2] == 0, "num_head must be divisible by num_head_kv"
    assert head_dim <= 256, "head_dim must be less than or equal to 256"
    alignment = 16 // q.element_size()
    assert head_dim % alignment == 0, f"head_dim must be divisible by {alignment}"
    assert v.shape[-1] % alignment == 0, f"head_dim_v must be divisible by {alignment}"


def _flash_attn_fwd(q, k, v, cu_seqlens_q=None, cu_seqlens_k=None, seqused_q=None, seqused_k=None, page_table=None,
                    softmax_scale=None, causal=False, window_size=(None, None), learnable_sink=None, softcap=0.0,
                    num_splits=1):
    q, k, v = [maybe_contiguous(t) for t in (q, k, v)]
    _checks(q, k, v, cu_seqlens_q, cu_seqlens_k, seqused_q, seqused_k, page_table, learnable_sink)
    if softmax_scale is None:
        softmax_scale = 1.0 / math.sqrt(q.shape[-1])
    left, right = _window(window_size)
    # bounds of the lengths from shapes alone (the kernels read the lengths themselves)
    max_seqlen_q = q.shape[0] if cu_seqlens_q is not None else None
    max_seqlen_k = k.shape[0] if cu_seqlens_k is not None else None
    sink = learnable_sink.detach().contiguous() if learnable_sink is not None else None
    return _lib.binding().cute_fwd(q, k, v, cu_seqlens_q, cu_seqlens_k, seqused_q, seqused_k, max_seqlen_q, max_seqlen_k,
                                   page_table, softmax_scale, causal, left, right, sink, softcap or 0.0, num_splits)


def _flash_attn_bwd(dout, q, k, v, out, lse, cu_seqlens_q, cu_seqlens_k, softmax_scale, causal, window_size, softcap,
                    learnable_sink):
    dout, q, k, v, out = [maybe_contiguous(t) for t in (dout, q, k, v, out)]
    left, right = _window(window_size)
    max_seqlen_q = q.shape[0] if cu_seqlens_q is not None else None
    max_seqlen_k = k.shape[0] if cu_seqlens_k is not None else None
    sink = learnable_sink.detach().contiguous() if learnable_sink is not None else None
    return _lib.binding().cute_bwd(dout, q, k, v, out, lse, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k,
                                   softmax_scale, causal, left, right, softcap or 0.0, sink)


class FlashAttnFunc(torch.autograd.Function):
    """flash_attn/cute/interface.py:1004-1070"""

    @staticmethod
    def forward(ctx, q, k, v, softmax_scale=None, causal=False, window_size=(None, None), learnable_sink=None, softcap=0.0,
                num_splits=1, pack_gqa=None, mask_mod=None, full_block_cnt=None, full_block_idx=None, mask_block_cnt=None,
                mask_block_idx=None):
        _check_block_sparse(mask_mod, full_block_cnt=full_block_cnt, full_block_idx=full_block_idx,
                            mask_block_cnt=mask_block_cnt, mask_block_idx=mask_block_idx)
        if softmax_scale is None:
            softmax_scale = 1.0 / math.sqrt(q.shape[-1])
        out, lse = _flash_attn_fwd(q, k, v, softmax_scale=softmax_scale, causal=causal, window_size=window_size,
                                   learnable_sink=learnable_sink, softcap=softcap, num_splits=num_splits)
        ctx.save_for_backward(q, k, v, out, lse, learnable_sink)
        ctx.softmax_scale, ctx.causal, ctx.window_size, ctx.softcap = softmax_scale, causal, window_size, softcap
        ctx.mark_non_differentiable(lse)
        return out, lse

    @staticmethod
    def backward(ctx, dout, *args):
        q, k, v, out, lse, sink = ctx.saved_tensors
        dq, dk, dv, dsink = _flash_attn_bwd(dout, q, k, v, out, lse, None, None, ctx.softmax_scale, ctx.causal,
                                            ctx.window_size, ctx.softcap, sink)
        if sink is None or not ctx.needs_input_grad[6]:
            dsink = None
        return (dq, dk, dv, None, None, None, dsink) + (None,) * 8


class FlashAttnVarlenFunc(torch.autograd.Function):
    """flash_attn/cute/interface.py:1072-1138"""

    @staticmethod
    def forward(ctx, q, k, v, cu_seqlens_q=None, cu_seqlens_k=None, seqused_q=None, seqused_k=None, page_table=None,
                softmax_scale=None, causal=False, window_size=(None, None), learnable_sink=None, softcap=0.0, num_splits=1,
                pack_gqa=None):
        if softmax_scale is None:
            softmax_scale = 1.0 / math.sqrt(q.shape[-1])
        out, lse = _flash_attn_fwd(q, k, v, cu_seqlens_q, cu_seqlens_k, seqused_q, seqused_k, page_table, softmax_scale, causal,
                                   window_size, learnable_sink, softcap, num_splits)
        ctx.save_for_backward(q, k, v, out, lse, cu_seqlens_q, cu_seqlens_k, learnable_sink)
        ctx.softmax_scale, ctx.causal, ctx.window_size, ctx.softcap = softmax_scale, causal, window_size, softcap
        # the backward is the training one: dense, or cu_seqlens_q with cu_seqlens_k
        ctx.trainable = seqused_q is None and seqused_k is None and page_table is None and \
            (cu_seqlens_q is None) == (cu_seqlens_k is None)
        ctx.mark_non_differentiable(lse)
        return out, lse

    @staticmethod
    def backward(ctx, dout, *args):
        q, k, v, out, lse, cu_seqlens_q, cu_seqlens_k, sink = ctx.saved_tensors
        if not ctx.trainable:
            raise NotImplementedError("This flash attention build does not support seqused_q / seqused_k / page_table or "
                                      "cu_seqlens_q without cu_seqlens_k in the backward")
        dq, dk, dv, dsink = _flash_attn_bwd(dout, q, k, v, out, lse, cu_seqlens_q, cu_seqlens_k, ctx.softmax_scale,
                                            ctx.causal, ctx.window_size, ctx.softcap, sink)
        if sink is None or not ctx.needs_input_grad[11]:
            dsink = None
        return (dq, dk, dv) + (None,) * 8 + (dsink,) + (None,) * 3


def flash_attn_func(q, k, v, softmax_scale=None, causal=False, window_size=(None, None), learnable_sink=None, softcap=0.0,
                    num_splits=1, pack_gqa=None, mask_mod=None, full_block_cnt=None, full_block_idx=None, mask_block_cnt=None,
                    mask_block_idx=None):
    """q (b, sq, h, d), k / v (b, sk, h_k, d[_v]) -> (out, lse (b, h, sq)).  learnable_sink: (h,) bf16 or fp32.  num_splits:
    1 = no split-KV, N > 1 = N parts, 0 = the library's heuristic.  pack_gqa is accepted and ignored; mask_mod and the
    block-sparse tensors must be None."""
    return FlashAttnFunc.apply(q, k, v, softmax_scale, causal, window_size, learnable_sink, softcap, num_splits, pack_gqa,
                               mask_mod, full_block_cnt, full_block_idx, mask_block_cnt, mask_block_idx)


def flash_attn_varlen_func(q, k, v, cu_seqlens_q=None, cu_seqlens_k=None, seqused_q=None, seqused_k=None, page_table=None,
                           softmax_scale=None, causal=False, window_size=(None, None), learnable_sink=None, softcap=0.0,
                           num_splits=1, pack_gqa=None):
    """q (total_q, h, d) with cu_seqlens_q, or dense (b, sq, h, d) without -- the decode call: sq = 1, page_table, seqused_k.
    k / v: (total_k, h_k, .) with cu_seqlens_k, a batched cache (b, sk, h_k, .), or pages (num_pages, page_size, h_k, .)
    behind page_table.  Returns (out, lse): lse (h, total_q) with cu_seqlens_q, (b, h, sq) without."""
    return FlashAttnVarlenFunc.apply(q, k, v, cu_seqlens_q, cu_seqlens_k, seqused_q, seqused_k, page_table, softmax_scale, causal,
                                     window_size, learnable_sink, softcap, num_splits, pack_gqa)
