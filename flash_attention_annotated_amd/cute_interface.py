"""The reference's newest public API -- names, argument order and defaults of `flash_attn/cute/interface.py`
(`flash_attn_func` :1141-1175, `flash_attn_varlen_func` :1177-1210) -- on the gfx950 kernels.  This is the surface that
carries `learnable_sink`: one logit per query head that joins the softmax denominator and contributes no value
(include/fa_fwd.h has the definition, DESIGN.md §4.12 the kernels).  Both functions return `(out, lse)` and are
differentiable; with a sink that requires grad the backward also returns its gradient (the reference's sink is
forward-only).

`flash_attn_func` also takes the reference's block-sparse tensors (`full_block_cnt / full_block_idx / mask_block_cnt /
mask_block_idx`, 128 x 128 blocks; include/fa_fwd.h fa_fwd_block_sparse has the definition, DESIGN.md §4.13 the kernel) and
`block_sparse_from_mask` makes them from a block mask.  That route is differentiable when the caller also passes the
key-major lists `q_block_cnt / q_block_idx` the dK / dV sweep walks (`block_sparse_bwd_lists` makes them from the four
forward lists; include/fa_bwd.h fa_bwd_block_sparse; head dims up to 128); without them the backward raises.
`mask_mod`, a CuTe-DSL callable, is not supported.  `block_sparse_select` makes all six lists on the device from q and k: pooled
block scores, a top-k per query block with forced sink and local blocks (include/fa_block_pattern.h);
`block_sparse_select_ref` is its torch oracle.

Routing is the FA3 surface's (csrc/torch_binding.cpp cute_fwd -> fa3_fwd_core): dense and varlen calls, decode steps over
a paged cache with their GQA swap and split-KV, ragged queries over a cache.  The cute signatures carry no max_seqlen:
the grid is made from bounds the shapes give (total_q / total_k), nothing is read from the device.
"""
import collections
import math
from typing import Tuple

import torch
from torch import Tensor

from . import _lib


def maybe_contiguous(x):
    return x.contiguous() if x is not None and x.stride(-1) != 1 else x


def _check_block_sparse(mask_mod=None, **tensors):
    """True when the call is block-sparse.  mask_mod (a CuTe-DSL callable) and full_block_* without mask_block_* are not
    supported; cnt and idx of a pair come together."""
    given = [n for n, t in dict(mask_mod=mask_mod, **tensors).items() if t is not None]
    if not given:
        return False
    if mask_mod is not None or (tensors["mask_block_cnt"] is None and tensors["mask_block_idx"] is None):
        raise NotImplementedError(
            f"This flash attention build does not support {', '.join(given)} (mask_mod, and the block-sparse tensors "
            f"full_block_cnt / full_block_idx without mask_block_cnt / mask_block_idx)")
    for pair in ("mask", "full"):
        if (tensors[f"{pair}_block_cnt"] is None) != (tensors[f"{pair}_block_idx"] is None):
            raise ValueError(f"{pair}_block_cnt and {pair}_block_idx must be specified together")
    return True


def block_sparse_from_mask(block_mask, full=None):
    """Block lists from a block mask -- the role of the reference's compute_block_sparsity for callers who have the mask.
    block_mask: bool (b | 1, h | 1, nm, nk), True = query block m visits key block n (128 x 128 blocks).  full: optional
    bool tensor of the same shape, the visited blocks that go to the full list (those the caller promises need no
    element-wise mask); the others go to the mask list.  Returns (full_block_cnt, full_block_idx, mask_block_cnt,
    mask_block_idx), int32, cnt (b | 1, h | 1, nm), idx (b | 1, h | 1, nm, nk): indices ascending, tails zero.  Pure torch,
    on the device of block_mask."""
    assert block_mask.dim() == 4 and block_mask.dtype == torch.bool, "block_mask must be a bool tensor (b, h, nm, nk)"
    if full is None:
        full = torch.zeros_like(block_mask)
    assert full.shape == block_mask.shape and full.dtype == torch.bool, "full must be a bool tensor of block_mask's shape"
    nk = block_mask.shape[-1]
    col = torch.arange(nk, device=block_mask.device)

    def lists(m):
        cnt = m.sum(-1, dtype=torch.int32)
        # a stable sort on "not visited" brings the visited indices to the front in ascending order
        idx = torch.sort((~m).to(torch.int8), dim=-1, stable=True).indices.to(torch.int32)
        return cnt, torch.where(col < cnt[..., None], idx, torch.zeros_like(idx))

    full_cnt, full_idx = lists(block_mask & full)
    mask_cnt, mask_idx = lists(block_mask & ~full)
    return full_cnt, full_idx, mask_cnt, mask_idx


def block_sparse_bwd_lists(full_block_cnt, full_block_idx, mask_block_cnt, mask_block_idx):
    """The key-major lists of the block-sparse backward from the forward's lists: (q_block_cnt (b | 1, h | 1, nk), q_block_idx
    (b | 1, h | 1, nk, nm)), int32 -- key block n is visited by the first q_block_cnt[.., n] query blocks of q_block_idx[.., n, :].
    One merged list of both forward lists (full_* may be None), counts respected, tails ignored; indices ascending, tails
    zero.  A batch / head dimension of size 1 is kept when both lists broadcast there.  Pure torch on the lists' device,
    nothing is read on the host; a pattern that stays fixed needs this once.  From a block mask,
    block_sparse_from_mask(block_mask.transpose(-1, -2))[2:] gives the same."""
    nm, nk = mask_block_idx.shape[-2:]
    col = torch.arange(nk, device=mask_block_idx.device)
    visited = None
    for cnt, idx in ((full_block_cnt, full_block_idx), (mask_block_cnt, mask_block_idx)):
        if cnt is None:
            continue
        used, at = torch.broadcast_tensors(col < cnt[..., None], idx.long())  # entries in front of the count
        rows = torch.zeros(*at.shape[:-1], nk + 1, dtype=torch.bool, device=idx.device)
        # (column nk swallows the tail and any index outside [0, nk), which names no block)
        rows.scatter_(-1, torch.where(used & (at >= 0) & (at < nk), at, torch.full_like(at, nk)), True)
        rows = rows[..., :nk]
        visited = rows if visited is None else visited | rows
    return block_sparse_from_mask(visited.transpose(-1, -2))[2:]


BlockSparseSelection = collections.namedtuple(
    "BlockSparseSelection", "full_block_cnt full_block_idx mask_block_cnt mask_block_idx q_block_cnt q_block_idx scores")


def _selection_outputs(q, k, with_bwd_lists, return_scores):
    """The seven tensors of a selection, uninitialised; what was not asked for is an empty tensor."""
    b, sq, h = q.shape[:3]
    nm, nk = (sq + 127) // 128, (k.shape[1] + 127) // 128
    new = lambda *shape, dtype=torch.int32: q.new_empty(shape, dtype=dtype)  # noqa: E731
    return (new(b, h, nm), new(b, h, nm, nk), new(b, h, nm), new(b, h, nm, nk),
            new(b, h, nk) if with_bwd_lists else new(0), new(b, h, nk, nm) if with_bwd_lists else new(0),
            new(b, h, nm, nk, dtype=torch.float32) if return_scores else new(0, dtype=torch.float32))


@torch.library.custom_op("flash_attn_amd::_block_sparse_select", mutates_args=(), device_types="cuda")
def _block_sparse_select(q: Tensor, k: Tensor, num_blocks: int, causal: bool, window_left: int, window_right: int, sink_blocks: int,
                         local_blocks: int, with_bwd_lists: bool, return_scores: bool) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor]:
    """The binding's block_pattern (fa_block_pattern): two launches, three with the key-major lists; no host sync.  The outputs
    and the workspace are allocated here, from the caching allocator."""
    outs = _selection_outputs(q, k, with_bwd_lists, return_scores)
    args = (q, k, *outs[:4], *(outs[4:6] if with_bwd_lists else (None, None)), outs[6] if return_scores else None)
    rule = (num_blocks, causal, window_left, window_right, sink_blocks, local_blocks)
    workspace = q.new_empty(_lib.binding().block_pattern_workspace_size(*args, None, *rule), dtype=torch.uint8)
    _lib.binding().block_pattern(*args, workspace, *rule)
    return outs


@torch.library.register_fake("flash_attn_amd::_block_sparse_select")
def _block_sparse_select_fake(q, k, num_blocks, causal, window_left, window_right, sink_blocks, local_blocks, with_bwd_lists,
                              return_scores):
    return _selection_outputs(q, k, with_bwd_lists, return_scores)


def _check_select(q, k, num_blocks, sink_blocks, local_blocks):
    assert q.dim() == 4 and k.dim() == 4, "q must have shape (batch_size, seqlen_q, num_head, head_dim), k (batch_size, seqlen_k, num_head_kv, head_dim)"
    assert q.shape[0] == k.shape[0] and q.shape[3] == k.shape[3], "q and k must have the same batch size and head_dim"
    assert q.shape[2] % k.shape[2] == 0, "num_head must be divisible by num_head_kv"
    assert q.shape[1] >= 1 and k.shape[1] >= 1, "seqlen_q and seqlen_k must be at least 1"
    if sink_blocks < 0 or local_blocks < 0 or num_blocks < sink_blocks + local_blocks:
        raise ValueError(f"num_blocks ({num_blocks}) must be at least sink_blocks + local_blocks ({sink_blocks} + {local_blocks}), "
                         f"both non-negative")


def block_sparse_select(q, k, num_blocks, *, causal=False, window_size=(None, None), sink_blocks=1, local_blocks=1,
                        with_bwd_lists=False, return_scores=False):
    """Block top-k pattern for block-sparse attention, made on the device -- the producer of the lists flash_attn_func takes.
    Not in the reference.  include/fa_block_pattern.h pins the rule; in short, with 128 x 128 blocks: the score of (query block
    m, key block n) is the dot product of the fp32 sum of the rows of m and the fp32 mean of the keys of n (no softmax scale);
    of the key blocks the call's own mask (causal / window_size, bottom-right aligned) lets query block m see, the first
    sink_blocks and the last local_blocks are always chosen, and the other num_blocks - sink_blocks - local_blocks places go to
    the highest scores, ties to the lower index.  A chosen block goes to the full list when the mask hides nothing in it and all
    128 of its keys exist (a ragged last key block never does), else to the mask list.

    q (b, sq, h, d), k (b, sk, h_k, d): fp16 / bf16, any strides with a unit last one, d a multiple of 16, at most 128;
    at most 8192 key blocks.  Returns a BlockSparseSelection: full_block_cnt (b, h, nm), full_block_idx (b, h, nm, nk),
    mask_block_cnt, mask_block_idx of the same shapes; with with_bwd_lists q_block_cnt (b, h, nk), q_block_idx (b, h, nk, nm),
    the key-major lists the backward needs (else None); with return_scores scores (b, h, nm, nk) fp32, -inf at blocks the mask
    hides (else None).  Lists are int32, indices ascending, tails zero: the conventions of block_sparse_from_mask /
    block_sparse_bwd_lists, so `flash_attn_func(q, k, v, causal=..., window_size=..., **sel._asdict())` without `scores` runs.
    Two launches (three with the key-major lists), nothing is read on the host, HIP-graph capturable; given the scores the
    lists equal block_sparse_select_ref(..., scores=scores) bit for bit.  CPU tensors take block_sparse_select_ref.
    Cost, measured on one MI355X at hq32 / hkv8, d128, bf16, causal, num_blocks = nk / 8 (tools/block_pattern_bench.py,
    profiles/block_pattern.jsonl): 0.09 - 0.30 x the torch composition of the same rule, and 0.22 - 0.26 x
    (s 8192), 0.07 - 0.08 x (s 32768), 0.03 x (s 131072) of the sparse forward the lists feed."""
    _check_select(q, k, num_blocks, sink_blocks, local_blocks)
    if not q.is_cuda:
        return block_sparse_select_ref(q, k, num_blocks, causal=causal, window_size=window_size, sink_blocks=sink_blocks,
                                       local_blocks=local_blocks, with_bwd_lists=with_bwd_lists, return_scores=return_scores)
    assert q.dtype in (torch.float16, torch.bfloat16) and k.dtype == q.dtype, "q and k must be float16 or bfloat16, of one dtype"
    q, k = maybe_contiguous(q), maybe_contiguous(k)
    left, right = _window(window_size)
    outs = torch.ops.flash_attn_amd._block_sparse_select(q, k, num_blocks, causal, left, right, sink_blocks, local_blocks,
                                                         with_bwd_lists, return_scores)
    return BlockSparseSelection(*outs[:4], *(outs[4:6] if with_bwd_lists else (None, None)), outs[6] if return_scores else None)


def block_sparse_visibility(sq, sk, causal=False, window_size=(None, None), device=None):
    """(visible, full), bool (nm, nk): whether query block m sees key block n under the call's own mask (some existing pair is
    visible), and whether the block is full (every existing pair is visible and all 128 keys exist).  Pure torch."""
    left, right = _window(window_size)
    if causal:
        right = 0
    nm, nk, off = (sq + 127) // 128, (sk + 127) // 128, sk - sq
    i_lo = torch.arange(nm, device=device)[:, None] * 128
    i_hi = torch.clamp(i_lo + 128, max=sq) - 1
    j_lo = torch.arange(nk, device=device)[None, :] * 128
    j_hi = torch.clamp(j_lo + 128, max=sk) - 1
    visible = torch.ones(nm, nk, dtype=torch.bool, device=device)
    full = (j_lo + 128 <= sk).expand(nm, nk).clone()
    if right >= 0:
        visible &= j_lo <= i_hi + off + right
        full &= j_hi <= i_lo + off + right
    if left >= 0:
        visible &= j_hi >= i_lo + off - left
        full &= j_lo >= i_hi + off - left
    return visible, full & visible


def block_sparse_select_ref(q, k, num_blocks, *, causal=False, window_size=(None, None), sink_blocks=1, local_blocks=1,
                            with_bwd_lists=False, return_scores=False, scores=None):
    """The oracle of block_sparse_select in plain torch, on any device and of any floating dtype: sums and scores in fp64 where
    q is fp64, else in fp32 (in torch's order, not the kernels').  scores: optional (b, h, nm, nk), taken in place of the pooled
    scores (what the mask hides is ignored): given the kernels' scores, the lists are the kernels' bit for bit."""
    _check_select(q, k, num_blocks, sink_blocks, local_blocks)
    b, sq, h, d = q.shape
    sk, h_k = k.shape[1:3]
    nm, nk = (sq + 127) // 128, (sk + 127) // 128
    visible, full = block_sparse_visibility(sq, sk, causal, window_size, q.device)
    if scores is None:
        ct = torch.float64 if q.dtype == torch.float64 else torch.float32

        def pooled(x, n):  # (b, blocks, heads, d): the sums over the rows that exist
            x = torch.nn.functional.pad(x.to(ct), (0, 0, 0, 0, 0, n * 128 - x.shape[1]))
            return x.view(b, n, 128, x.shape[2], d).sum(2)

        count = torch.clamp(sk - torch.arange(nk, device=q.device) * 128, max=128).to(ct)
        qs, km = pooled(q, nm), pooled(k, nk) * (1 / count)[None, :, None, None]
        scores = torch.einsum("bmhc,bnhc->bhmn", qs, km.repeat_interleave(h // h_k, dim=2))
    u = torch.where(visible, scores + 0.0, torch.full_like(scores, float("-inf")))  # (-0 equals +0)
    # the places of a row: forced blocks, then the other visible ones by score (a stable sort: of equal ones the lower index),
    # then what the mask hides
    seen = visible.cumsum(-1)
    cnt = seen[:, -1:]
    forced = visible & ((seen - 1 < sink_blocks) | (cnt - seen < local_blocks))
    by_score = torch.sort(u, dim=-1, descending=True, stable=True).indices
    rank = torch.where(forced, 0, torch.where(visible, 1, 2)).expand(b, h, nm, nk)
    order = by_score.gather(-1, torch.sort(rank.gather(-1, by_score), dim=-1, stable=True).indices)
    place = torch.empty_like(order).scatter_(-1, order, torch.arange(nk, device=q.device).expand(b, h, nm, nk))
    chosen = place < torch.clamp(cnt, max=num_blocks)
    lists = block_sparse_from_mask(chosen, full.expand(b, h, nm, nk))
    key_lists = block_sparse_bwd_lists(*lists) if with_bwd_lists else (None, None)
    return BlockSparseSelection(*lists, *key_lists, u if return_scores else None)


def _check_key_lists(q, k, q_block_cnt, q_block_idx):
    """Both or neither; dtype / device / shape as the forward's lists, with the roles of nm and nk swapped."""
    if (q_block_cnt is None) != (q_block_idx is None):
        raise ValueError("q_block_cnt and q_block_idx must be specified together")
    if q_block_cnt is None:
        return False
    b, sq, h = q.shape[:3]
    nm, nk = (sq + 127) // 128, (k.shape[1] + 127) // 128
    for t, tname, tail in ((q_block_cnt, "q_block_cnt", (nk,)), (q_block_idx, "q_block_idx", (nk, nm))):
        if t.dtype != torch.int32:
            raise ValueError(f"{tname} must be int32")
        if t.device != q.device:
            raise ValueError(f"{tname} must be on the device of q")
        if t.dim() != 2 + len(tail) or t.shape[0] not in (1, b) or t.shape[1] not in (1, h) or tuple(t.shape[2:]) != tail:
            raise ValueError(f"{tname} must have shape ({b} or 1, {h} or 1, {', '.join(map(str, tail))}), got {tuple(t.shape)}")
    return True


def _flash_attn_fwd_block_sparse(q, k, v, softmax_scale, causal, window_size, learnable_sink, softcap, num_splits,
                                 full_block_cnt, full_block_idx, mask_block_cnt, mask_block_idx):
    """The checks of normalize_block_sparse_tensors (flash_attn/cute/block_sparsity.py:33-115) and the launch.  Nothing of
    the lists is read on the host: the call can be captured in a HIP graph."""
    q, k, v = [maybe_contiguous(t) for t in (q, k, v)]
    assert q.dim() == 4, "block sparsity needs q of shape (batch_size, seqlen_q, num_head, head_dim)"
    _checks(q, k, v, None, None, None, None, None, learnable_sink)
    if num_splits not in (0, 1):
        raise NotImplementedError("block sparsity does not support num_splits > 1 (split-KV over block lists)")
    if v.shape[-1] > 256:
        raise NotImplementedError("block sparsity does not support a head dim of V above 256")
    b, sq, h = q.shape[:3]
    nm, nk = (sq + 127) // 128, (k.shape[1] + 127) // 128
    for name, cnt, idx in (("mask", mask_block_cnt, mask_block_idx), ("full", full_block_cnt, full_block_idx)):
        if cnt is None:
            continue
        for t, tname, tail in ((cnt, f"{name}_block_cnt", (nm,)), (idx, f"{name}_block_idx", (nm, nk))):
            if t.dtype != torch.int32:
                raise ValueError(f"{tname} must be int32")
            if t.device != q.device:
                raise ValueError(f"{tname} must be on the device of q")
            if t.dim() != 2 + len(tail) or t.shape[0] not in (1, b) or t.shape[1] not in (1, h) or tuple(t.shape[2:]) != tail:
                raise ValueError(f"{tname} must have shape ({b} or 1, {h} or 1, {', '.join(map(str, tail))}), "
                                 f"got {tuple(t.shape)}")
    left, right = _window(window_size)
    sink = learnable_sink.detach().contiguous() if learnable_sink is not None else None
    return _lib.binding().cute_fwd_block_sparse(q, k, v, softmax_scale, causal, left, right, sink, softcap or 0.0, num_splits,
                                                full_block_cnt, full_block_idx, mask_block_cnt, mask_block_idx)


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
                    num_splits=1, pack_gqa=None):
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
                                   page_table, softmax_scale, causal, left, right, sink, softcap or 0.0, num_splits, pack_gqa)


def _flash_attn_bwd_block_sparse(dout, q, k, v, out, lse, softmax_scale, causal, window_size, softcap, learnable_sink, lists):
    if q.shape[-1] > 128 or v.shape[-1] != q.shape[-1]:
        raise NotImplementedError("block-sparse backward: head dims up to 128 with the same head dim for V "
                                  f"(got {q.shape[-1]} / {v.shape[-1]})")
    dout, q, k, v, out = [maybe_contiguous(t) for t in (dout, q, k, v, out)]
    left, right = _window(window_size)
    sink = learnable_sink.detach().contiguous() if learnable_sink is not None else None
    return _lib.binding().cute_bwd_block_sparse(dout, q, k, v, out, lse, softmax_scale, causal, left, right, softcap or 0.0,
                                                sink, *lists)


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
                mask_block_idx=None, q_block_cnt=None, q_block_idx=None):
        ctx.block_sparse = _check_block_sparse(mask_mod, full_block_cnt=full_block_cnt, full_block_idx=full_block_idx,
                                               mask_block_cnt=mask_block_cnt, mask_block_idx=mask_block_idx)
        if not ctx.block_sparse and (q_block_cnt is not None or q_block_idx is not None):
            raise ValueError("q_block_cnt / q_block_idx are only valid with mask_block_cnt / mask_block_idx")
        ctx.key_lists = ctx.block_sparse and _check_key_lists(q, k, q_block_cnt, q_block_idx)
        if softmax_scale is None:
            softmax_scale = 1.0 / math.sqrt(q.shape[-1])
        if ctx.block_sparse:
            out, lse = _flash_attn_fwd_block_sparse(q, k, v, softmax_scale, causal, window_size, learnable_sink, softcap, num_splits,
                                                    full_block_cnt, full_block_idx, mask_block_cnt, mask_block_idx)
        else:
            out, lse = _flash_attn_fwd(q, k, v, softmax_scale=softmax_scale, causal=causal, window_size=window_size,
                                       learnable_sink=learnable_sink, softcap=softcap, num_splits=num_splits, pack_gqa=pack_gqa)
        lists = (full_block_cnt, full_block_idx, mask_block_cnt, mask_block_idx, q_block_cnt, q_block_idx) if ctx.key_lists else ()
        ctx.save_for_backward(q, k, v, out, lse, learnable_sink, *lists)
        ctx.softmax_scale, ctx.causal, ctx.window_size, ctx.softcap = softmax_scale, causal, window_size, softcap
        ctx.mark_non_differentiable(lse)
        return out, lse

    @staticmethod
    def backward(ctx, dout, *args):
        # (the reference returns the DENSE gradient for a block-sparse forward, flash_attn/cute/interface.py:1055-1069)
        if ctx.block_sparse and not ctx.key_lists:
            raise NotImplementedError("block-sparse backward")  # needs q_block_cnt / q_block_idx (block_sparse_bwd_lists)
        q, k, v, out, lse, sink = ctx.saved_tensors[:6]
        if ctx.block_sparse:
            dq, dk, dv, dsink = _flash_attn_bwd_block_sparse(dout, q, k, v, out, lse, ctx.softmax_scale, ctx.causal, ctx.window_size,
                                                             ctx.softcap, sink, ctx.saved_tensors[6:])
        else:
            dq, dk, dv, dsink = _flash_attn_bwd(dout, q, k, v, out, lse, None, None, ctx.softmax_scale, ctx.causal,
                                                ctx.window_size, ctx.softcap, sink)
        if sink is None or not ctx.needs_input_grad[6]:
            dsink = None
        return (dq, dk, dv, None, None, None, dsink) + (None,) * 10


class FlashAttnVarlenFunc(torch.autograd.Function):
    """flash_attn/cute/interface.py:1072-1138"""

    @staticmethod
    def forward(ctx, q, k, v, cu_seqlens_q=None, cu_seqlens_k=None, seqused_q=None, seqused_k=None, page_table=None,
                softmax_scale=None, causal=False, window_size=(None, None), learnable_sink=None, softcap=0.0, num_splits=1,
                pack_gqa=None):
        if softmax_scale is None:
            softmax_scale = 1.0 / math.sqrt(q.shape[-1])
        out, lse = _flash_attn_fwd(q, k, v, cu_seqlens_q, cu_seqlens_k, seqused_q, seqused_k, page_table, softmax_scale, causal,
                                   window_size, learnable_sink, softcap, num_splits, pack_gqa)
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
                    mask_block_idx=None, q_block_cnt=None, q_block_idx=None):
    """q (b, sq, h, d), k / v (b, sk, h_k, d[_v]) -> (out, lse (b, h, sq)).  learnable_sink: (h,) bf16 or fp32.  num_splits:
    1 = no split-KV, N > 1 = N parts, 0 = the library's heuristic.  mask_mod must be None.
    pack_gqa: True packs the h / h_k query heads of a kv head into the rows of a tile, one pass over K / V per kv head
    (pk_fwd_kernel: h > h_k, head dims <= 128, same head dim for V; a no-op on other calls and on block-sparse ones); False and
    None run one workgroup per query head, as before -- None does not pack by itself yet.  A hint: results agree to rounding.

    Block sparsity: mask_block_cnt (b | 1, h | 1, nm) and mask_block_idx (b | 1, h | 1, nm, nk), int32, on q's device, with
    nm = ceil(sq / 128), nk = ceil(sk / 128), and optionally full_block_cnt / full_block_idx of the same shapes
    (block_sparse_from_mask makes all four from a block mask).  Query block m attends to the first cnt[.., m] key blocks of
    idx[.., m, :] of both lists, and inside them to what causal / window_size allow; distinct in-range indices are the
    caller's duty.  Rows without a visible key give out = 0 and lse = +inf (the sink with learnable_sink).  Not with
    num_splits > 1 or a V head dim above 256.
    The backward of a block-sparse call needs the same pattern key-major: q_block_cnt (b | 1, h | 1, nk) and q_block_idx
    (b | 1, h | 1, nk, nm), int32 -- key block n is visited by the first cnt[.., n] query blocks of idx[.., n, :], indexed by
    the query head, one merged list (block_sparse_bwd_lists makes them from the four forward lists, once per pattern).  That
    they name the same (query block, key block) pairs as the forward lists is the caller's duty.  dq walks the forward
    lists, dk / dv the key-major ones, in list order: no atomics, equal lists give bit-equal gradients; learnable_sink gets
    its gradient.  Without q_block_* the backward raises NotImplementedError("block-sparse backward"), and so it does
    for a head dim above 128 or a V head dim that differs.
    Measured on one MI355X at b4 h16 s8192 d128 bf16 (profiles/block_sparse.jsonl): time is proportional to the listed blocks,
    all of them listed cost 1.46 x the plain dense call, so block sparsity pays below about 0.68 of the blocks (0.40 x the
    dense time at a quarter of them)."""
    return FlashAttnFunc.apply(q, k, v, softmax_scale, causal, window_size, learnable_sink, softcap, num_splits, pack_gqa,
                               mask_mod, full_block_cnt, full_block_idx, mask_block_cnt, mask_block_idx, q_block_cnt, q_block_idx)


def flash_attn_varlen_func(q, k, v, cu_seqlens_q=None, cu_seqlens_k=None, seqused_q=None, seqused_k=None, page_table=None,
                           softmax_scale=None, causal=False, window_size=(None, None), learnable_sink=None, softcap=0.0,
                           num_splits=1, pack_gqa=None):
    """q (total_q, h, d) with cu_seqlens_q, or dense (b, sq, h, d) without -- the decode call: sq = 1, page_table, seqused_k.
    k / v: (total_k, h_k, .) with cu_seqlens_k, a batched cache (b, sk, h_k, .), or pages (num_pages, page_size, h_k, .)
    behind page_table.  Returns (out, lse): lse (h, total_q) with cu_seqlens_q, (b, h, sq) without.  pack_gqa: as in
    flash_attn_func (True = the pk kernel on every one of these forms; the single-token decode step keeps its own GQA swap)."""
    return FlashAttnVarlenFunc.apply(q, k, v, cu_seqlens_q, cu_seqlens_k, seqused_q, seqused_k, page_table, softmax_scale, causal,
                                     window_size, learnable_sink, softcap, num_splits, pack_gqa)
