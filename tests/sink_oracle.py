"""ORACLE of the learnable attention sink -- test infrastructure, a plain module (not collected).

Torch restatement of the sink branch of the reference's `attention_ref` (flash_attn/cute/testing.py:300-400, the sink at
:376-387) on top of this project's mask builder (oracle/attention_ref.py local_mask), plus the LSE the reference's oracle
does not return, by the definition of include/fa_fwd.h:

    m' = max(max_j s_ij, z)   l' = sum_j exp(s_ij - m') + exp(z - m')   P_ij = exp(s_ij - m') / l'   LSE_i = m' + log l'

A row without a visible key gives O = 0 and LSE = z (max(z, -inf) = z, l' = 1).  Without a sink (None), or with z = -inf on
such a row, LSE is +inf: the project's convention for rows without keys.

Pinned: tools/make_sink_golden.py asserts this restatement equals the reference's function bit for bit on the cases of
tests/golden/attention_sink_golden.pt; tests/test_sink_oracle.py replays them without the reference.
"""
import math

import torch

from oracle import attention_ref as oracle


def _window(window_size):
    return tuple(-1 if w is None else w for w in window_size)


def attention_sink_ref(q, k, v, learnable_sink=None, causal=False, window_size=(None, None), softcap=0.0, upcast=True,
                       reorder_ops=False, attn_bias=None, softmax_scale=None):
    """q (b, sq, h, d), k / v (b, sk, h_k, d[_v]), learnable_sink (h,) or None -> (out (b, sq, h, d_v) in q.dtype,
    lse (b, h, sq) fp32).  upcast / reorder_ops as oracle.attention_ref: the fp32 reference, or the same math in the input
    precision with k scaled (the yardstick of the tolerance rules).  attn_bias (.., sq, sk) is added to the masked scores (the
    row-sampled comparisons carry their causal mask in it).  Differentiable in q, k, v and learnable_sink."""
    window_size = _window(window_size)
    if causal:
        window_size = (window_size[0], 0)
    dtype_og = q.dtype
    if upcast:
        q, k, v = q.float(), k.float(), v.float()
    sq, sk = q.shape[1], k.shape[1]
    g = q.shape[2] // k.shape[2]
    k = k.repeat_interleave(g, dim=2)
    v = v.repeat_interleave(g, dim=2)
    if softmax_scale is None:
        softmax_scale = 1.0 / math.sqrt(q.shape[-1])
    if not reorder_ops:
        scores = torch.einsum("bthd,bshd->bhts", q * softmax_scale, k)
    else:
        scores = torch.einsum("bthd,bshd->bhts", q, k * softmax_scale)
    if softcap > 0:
        scores = torch.tanh(scores / softcap) * softcap
    masked = None
    if window_size[0] >= 0 or window_size[1] >= 0:
        masked = oracle.local_mask(sq, sk, window_size, None, None, q.device)
        scores = scores.masked_fill(masked, float("-inf"))
    if attn_bias is not None:
        scores = scores + attn_bias
    scores_fp32 = scores.to(torch.float32)
    logits_max = torch.amax(scores_fp32, dim=-1, keepdim=True)
    if learnable_sink is None:
        attention = torch.softmax(scores, dim=-1).to(v.dtype)
        lse = torch.logsumexp(scores_fp32, dim=-1)
    else:
        sink = learnable_sink.view(-1, 1, 1)
        logits_or_sinks_max = torch.maximum(sink, logits_max)
        unnormalized_scores = torch.exp(scores_fp32 - logits_or_sinks_max)
        normalizer = unnormalized_scores.sum(dim=-1, keepdim=True) + torch.exp(sink - logits_or_sinks_max)
        attention = (unnormalized_scores / normalizer).to(v.dtype)
        lse = (logits_or_sinks_max.float() + torch.log(normalizer)).squeeze(-1)
    keyless = torch.isneginf(logits_max)
    attention = attention.masked_fill(keyless, 0.0)  # (rows without a visible key: zeros, also where z = -inf made them NaN)
    out = torch.einsum("bhts,bshd->bthd", attention, v).to(dtype_og)
    lse = torch.where(torch.isneginf(lse) | torch.isnan(lse), torch.full_like(lse, float("inf")), lse)
    return out, lse


def attention_sink_varlen_ref(q, k, v, cu_seqlens_q, cu_seqlens_k, learnable_sink=None, **kw):
    """Packed ragged batch, q (total_q, h, d), k / v (total_k, h_k, .): loops over the sequences.  Returns out (total_q, h, d_v)
    and lse (h, total_q).  A sequence without keys: O = 0, LSE = the sink (+inf without one)."""
    cq, ck = cu_seqlens_q.tolist(), cu_seqlens_k.tolist()
    outs, lses = [], []
    for i in range(len(cq) - 1):
        if ck[i + 1] == ck[i]:  # no key at all
            n, h = cq[i + 1] - cq[i], q.shape[1]
            outs.append(torch.zeros(n, h, v.shape[-1], dtype=q.dtype))
            lses.append(torch.full((h, n), float("inf")) if learnable_sink is None else learnable_sink.float().view(h, 1).expand(h, n))
            continue
        o, l = attention_sink_ref(q[cq[i]:cq[i + 1]][None], k[ck[i]:ck[i + 1]][None], v[ck[i]:ck[i + 1]][None], learnable_sink, **kw)
        outs.append(o[0])
        lses.append(l[0])
    return torch.cat(outs, dim=0), torch.cat(lses, dim=1)
