"""ORACLE of block-sparse attention -- test infrastructure, a plain module (not collected).

The semantics of include/fa_fwd.h (fa_fwd_block_sparse): blocks of 128 query rows x 128 keys; query block m of (batch, head)
visits the first `cnt[.., m]` entries of `idx[.., m, :]` of the mask list and of the full list, entries past the count are
ignored; the pair (i, j) counts iff key block j // 128 is visited for query block i // 128 and the call's own mask (the
seqlen_k bound, causal, window_size, bottom-right aligned) allows it.  The two lists mean the same here: the call's mask
applies inside "full" blocks too.

The lists are expanded into a dense (b, h, sq, sk) bool mask, which rides as an additive bias (0 / -inf) through
tests/sink_oracle.py -- the masks, the softcap, the sink term, the fp32 and the input-precision paths and the LSE are that
file's.  Rows without a visible key: O = 0, LSE = +inf, or the sink.
"""
import torch

import sink_oracle

BLOCK = 128


def block_mask_from_lists(full_block_cnt, full_block_idx, mask_block_cnt, mask_block_idx, b, h):
    """-> bool (b, h, nm, nk), True where a block is visited.  Counts are respected, tails ignored; batch / head dims of
    size 1 broadcast.  full_* may be None."""
    nm, nk = mask_block_idx.shape[-2:]
    visited = torch.zeros(b, h, nm, nk, dtype=torch.bool)
    col = torch.arange(nk)
    for cnt, idx in ((full_block_cnt, full_block_idx), (mask_block_cnt, mask_block_idx)):
        if cnt is None:
            continue
        cnt = cnt.cpu().expand(b, h, nm)
        idx = idx.cpu().expand(b, h, nm, nk).long()
        used = col < cnt[..., None]                             # entries in front of the count
        rows = torch.zeros(b, h, nm, nk + 1, dtype=torch.bool)  # (column nk swallows the ignored tail)
        rows.scatter_(-1, torch.where(used, idx, torch.full_like(idx, nk)), True)
        visited |= rows[..., :nk]
    return visited


def dense_mask(visited, sq, sk):
    """(b, h, nm, nk) -> (b, h, sq, sk): every block blown up to its rows and keys."""
    return visited.repeat_interleave(BLOCK, dim=2)[:, :, :sq].repeat_interleave(BLOCK, dim=3)[..., :sk]


def attention_block_sparse_ref(q, k, v, full_block_cnt, full_block_idx, mask_block_cnt, mask_block_idx, causal=False,
                               window_size=(None, None), softcap=0.0, learnable_sink=None, upcast=True, reorder_ops=False):
    """q (b, sq, h, d), k / v (b, sk, h_k, d[_v]) -> (out (b, sq, h, d_v) in q.dtype, lse (b, h, sq) fp32); upcast /
    reorder_ops as oracle.attention_ref (fp32, or the same math in the input precision)."""
    b, sq, h = q.shape[:3]
    sk = k.shape[1]
    visited = block_mask_from_lists(full_block_cnt, full_block_idx, mask_block_cnt, mask_block_idx, b, h)
    allowed = dense_mask(visited, sq, sk)
    bias = torch.zeros(b, h, sq, sk).masked_fill(~allowed, float("-inf"))
    if not upcast:
        bias = bias.to(q.dtype)
    return sink_oracle.attention_sink_ref(q, k, v, learnable_sink, causal=causal, window_size=window_size, softcap=softcap,
                                          upcast=upcast, reorder_ops=reorder_ops, attn_bias=bias)


def random_lists(seed, b, h, nm, nk, min_visited=0, max_visited=None, to_full=None):
    """Seeded block lists on the CPU, distinct per batch and per query head: every query block visits a random subset of
    min_visited .. max_visited (default nk) key blocks, in shuffled order, split at random between the two lists -- except
    the blocks flagged in to_full (bool (nm, nk)), which go to the full list whenever they are visited.  The tails behind the
    counts hold in-range indices that are NOT visited where one exists (0 otherwise), so ignoring a count changes the numbers
    instead of faulting.  Returns ((full_cnt, full_idx, mask_cnt, mask_idx), visited (b, h, nm, nk) bool)."""
    g = torch.Generator().manual_seed(seed)
    max_visited = nk if max_visited is None else max_visited
    visited = torch.zeros(b, h, nm, nk, dtype=torch.bool)
    cnts = [torch.zeros(b, h, nm, dtype=torch.int32) for _ in range(2)]
    idxs = [torch.zeros(b, h, nm, nk, dtype=torch.int32) for _ in range(2)]
    for bi in range(b):
        for hi in range(h):
            for m in range(nm):
                take = int(torch.randint(min_visited, max_visited + 1, (1,), generator=g))
                vis = torch.randperm(nk, generator=g)[:take].tolist()
                coin = torch.rand(take, generator=g).tolist()
                in_full = [c < 0.5 or (to_full is not None and bool(to_full[m, n])) for n, c in zip(vis, coin)]
                mine = [[n for n, f in zip(vis, in_full) if f], [n for n, f in zip(vis, in_full) if not f]]
                visited[bi, hi, m, vis] = True
                rest = [n for n in range(nk) if n not in vis] or [0]
                for which in range(2):
                    tail = [rest[int(torch.randint(0, len(rest), (1,), generator=g))] for _ in range(nk - len(mine[which]))]
                    cnts[which][bi, hi, m] = len(mine[which])
                    idxs[which][bi, hi, m] = torch.tensor(mine[which] + tail, dtype=torch.int32)
    return (cnts[0], idxs[0], cnts[1], idxs[1]), visited
