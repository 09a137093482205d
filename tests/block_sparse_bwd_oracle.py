"""ORACLE of the block-sparse backward -- test infrastructure, a plain module (not collected).

Gradients come by autograd through the oracle of the forward.  tests/block_sparse_oracle.py as it stands cannot be
differentiated where a row has no visible key (a query block with both counts 0, a row the call's own mask empties) and no
sink: its scores are all -inf there, softmax gives NaN, the forward replaces the NaN by zeros, and the backward of the softmax
multiplies by that NaN again -- dq of the row and, through the sums over rows, all of dk.  attention_block_sparse_grad_ref
below is the same computation with those rows guarded:

  * the visited blocks (block_sparse_oracle.block_mask_from_lists / dense_mask) AND the call's own mask
    (oracle.attention_ref.local_mask, bottom-right aligned) make one bool mask `allowed`, which rides as the additive
    bias (0 / -inf) through tests/sink_oracle.py -- the values of the scores are those of attention_block_sparse_ref;
  * a row without an allowed key gets bias 0 on every key (a finite softmax) and its output row is multiplied by 0: O = 0 as
    the definition says, and every gradient through the row is exactly 0;  the other rows are multiplied by 1.
Where no row is keyless the two functions give the same output and the same gradients bit for bit
(tests/test_block_sparse_bwd_oracle.py asserts it)."""
import torch

import block_sparse_oracle as bso
import sink_oracle
from oracle import attention_ref as oracle


def allowed_mask(lists, b, h, sq, sk, causal=False, window_size=(None, None)):
    """bool (b, h, sq, sk): the pairs (i, j) that count -- key block visited and the call's mask allows the pair."""
    visited = bso.block_mask_from_lists(*lists, b, h)
    allowed = bso.dense_mask(visited, sq, sk)
    left, right = (-1 if w is None else w for w in window_size)
    if causal:
        right = 0
    if left >= 0 or right >= 0:
        allowed = allowed & ~oracle.local_mask(sq, sk, (left, right), None, None, None)
    return allowed


def attention_block_sparse_grad_ref(q, k, v, lists, causal=False, window_size=(None, None), softcap=0.0, learnable_sink=None,
                                    upcast=True, reorder_ops=False):
    """attention_block_sparse_ref(q, k, v, *lists, ...) that autograd can differentiate for every list content: -> (out, lse)."""
    b, sq, h = q.shape[:3]
    sk = k.shape[1]
    allowed = allowed_mask(lists, b, h, sq, sk, causal, window_size)
    keyless = ~allowed.any(-1)                                                  # (b, h, sq)
    bias = torch.zeros(b, h, sq, sk).masked_fill(~(allowed | keyless[..., None]), float("-inf"))
    if not upcast:
        bias = bias.to(q.dtype)
    out, lse = sink_oracle.attention_sink_ref(q, k, v, learnable_sink, softcap=softcap, upcast=upcast, reorder_ops=reorder_ops,
                                              attn_bias=bias)
    out = out * (~keyless).transpose(1, 2)[..., None].to(out.dtype)
    empty = torch.full_like(lse, float("inf")) if learnable_sink is None else \
        learnable_sink.detach().float().view(1, h, 1).expand_as(lse)
    return out, torch.where(keyless, empty, lse.detach())


def grads(fn, leaves, g):
    """fn(*leaves, **order) -> out; -> (ref gradients: fp32 math, pt gradients: the same math in the inputs' precision).  A
    1-D leaf is a sink: an fp32 leaf on the ref path (its bf16 values are exact there)."""
    def run(cast, **order):
        ls = [cast(x).clone().requires_grad_(True) for x in leaves]
        return torch.autograd.grad(fn(*ls, **order), ls, g)
    return run(lambda x: x.float() if x.dim() == 1 else x), run(lambda x: x, upcast=False, reorder_ops=True)


def key_major_lists(lists, b, h):
    """The key-major lists straight from the definition: the transpose of block_mask_from_lists, indices ascending, tails 0.
    -> (q_block_cnt (b, h, nk), q_block_idx (b, h, nk, nm)) int32 on the CPU."""
    vt = bso.block_mask_from_lists(*lists, b, h).transpose(-1, -2)             # (b, h, nk, nm)
    nm = vt.shape[-1]
    cnt = vt.sum(-1, dtype=torch.int32)
    idx = torch.zeros(*vt.shape, dtype=torch.int32)
    for pos in torch.nonzero(vt.reshape(-1, nm).any(-1)).flatten().tolist():
        row = torch.nonzero(vt.reshape(-1, nm)[pos]).flatten().to(torch.int32)
        idx.view(-1, nm)[pos, :len(row)] = row
    return cnt, idx
