"""Oracle of block-sparse attention over a KV cache (a plain helper module; include/fa_fwd.h, fa_fwd_sparse_kv): softmax in fp64
over an explicit visibility built from the definition, nothing else.  With B the block size, g = h / h_k and `fill` the fill
level of a batch entry, key j is visible to query row i of head hd iff
    j < fill   AND   the causal / window rule allows (i, j), bottom-right aligned on `fill`   AND
    j // B is among the first min(cnt[hd // g], max_blocks) entries of idx[hd // g, :].
A duplicate entry counts twice (the visibility is a multiplicity); entries outside [0, ceil(fill / B)) name no key below `fill`
and entries at or behind the count are not looked at.  tests/test_sparse_kv_abi.py checks this module against the project's
dense oracle (oracle/attention_ref.py) and a hand-made case; tests/test_sparse_kv_gpu.py checks the kernel against it."""
import math

import torch


def visibility(sq, cap, fill, cnt, idx, block, h, causal=False, window=(-1, -1)):
    """(h, sq, cap) int64: how often key j counts for row i of head hd.  cnt (h_k,), idx (h_k, max_blocks), one batch entry."""
    hk, max_blocks = idx.shape
    g = h // hk
    left, right = window
    if causal:
        right = 0
    j = torch.arange(cap).view(1, -1)
    i = torch.arange(sq).view(-1, 1)
    ok = (j < fill).expand(sq, cap).clone()
    shift = fill - sq
    if right >= 0:
        ok &= j <= i + shift + right
    if left >= 0:
        ok &= j >= i + shift - left
    vis = torch.zeros(h, sq, cap, dtype=torch.int64)
    for kv in range(hk):
        times = torch.zeros(cap, dtype=torch.int64)
        for e in idx[kv, : max(0, min(int(cnt[kv]), max_blocks))].tolist():
            if e >= 0:
                times[e * block: (e + 1) * block] += 1  # (an empty slice where the block lies past the capacity)
        vis[kv * g: (kv + 1) * g] = (ok.long() * times.view(1, -1)).unsqueeze(0)
    return vis


def attention(q, k, v, vis, softmax_scale=None, softcap=0.0):
    """q (sq, h, d), k / v (cap, h_k, d) of any float dtype, vis (h, sq, cap) multiplicities -> out (sq, h, d) fp32 and
    lse (h, sq) fp32 (+inf and out = 0 where a row sees no key)."""
    sq, h, d = q.shape
    g = h // k.shape[1]
    scale = 1.0 / math.sqrt(d) if softmax_scale is None else softmax_scale
    kk = k.double().repeat_interleave(g, dim=1)
    vv = v.double().repeat_interleave(g, dim=1)
    s = torch.einsum("thd,shd->hts", q.double(), kk) * scale
    if softcap > 0:
        s = torch.tanh(s / softcap) * softcap
    s = s.masked_fill(vis == 0, float("-inf"))
    m = s.amax(-1, keepdim=True)
    m = torch.where(torch.isneginf(m), torch.zeros_like(m), m)
    w = torch.exp(s - m) * vis.double()
    l = w.sum(-1, keepdim=True)
    p = torch.where(l > 0, w / l, torch.zeros_like(w))
    out = torch.einsum("hts,shd->thd", p, vv)
    lse = torch.where(l > 0, m + torch.log(l), torch.full_like(l, float("inf"))).squeeze(-1)
    return out.float(), lse.float()


def sparse_kv_ref(q, k, v, fill, cnt, idx, block, causal=False, window=(-1, -1), softcap=0.0, softmax_scale=None):
    """One batch entry: q (sq, h, d); k / v (cap, h_k, d) its logical cache rows from position 0.  Returns (out, lse, vis)."""
    vis = visibility(q.shape[0], k.shape[0], int(fill), cnt, idx, block, q.shape[1], causal, window)
    out, lse = attention(q, k, v, vis, softmax_scale, softcap)
    return out, lse, vis
