"""The step between (batch, vocab) logits and the next token, behind the names of the reference's `flash_attn/utils/generation.py`:

    InferenceParams                              reference :23-40
    modify_logits_for_top_k_filtering                      :45-48
    modify_logits_for_top_p_filtering                      :53-66
    sample                                                 :69-95
    sample_speculative                                     :209-265
    sample_ref, filter_ref, uniform_ref          pure torch: the contract of include/fa_sample.h, the CPU oracle
    sample_speculative_ref                       pure torch: the contract of include/fa_spec_sample.h, the CPU oracle
    sample_speculative_tree                      not in the reference: the acceptance walk over a TREE of draft tokens
    sample_speculative_tree_ref                  pure torch: the contract of include/fa_tree_sample.h, the CPU oracle

Same signatures and defaults; `sample` and `sample_speculative` have two keyword-only additions, `generator` and `u`.  Where the reference chains topk,
a full sort, softmax, cumsum, scatter, masked_fill and multinomial, CUDA tensors here take one launch of the HIP kernels of
csrc/fa_sample.hip through `flash_attn_2_cuda_C.sample` / `sample_filter_`, wrapped in torch.library custom ops with fake
implementations, so torch.compile traces them.  There is no eager fall-back on the device: without the built library the ops
raise.  CPU tensors take the oracle.

`sample_speculative` is Algorithm 1 of Leviathan et al. (arXiv 2211.17192): it verifies `seqlen` draft tokens against the target
model's logits, accepts a prefix and resamples the first rejected position from max(p - q, 0).  CUDA tensors take the two
launches of csrc/fa_spec_sample.hip through `flash_attn_2_cuda_C.sample_speculative`; the rule is written out in
include/fa_spec_sample.h.  One thing differs from the reference on purpose: the reference ends with
`tokens[:, first_rejected_idx] = resample`, which for a batch of more than one sequence sets whole columns (every sequence gets
the other sequences' resampled tokens at their rejection columns).  Here the write is per row, `tokens[b, first_rejected_idx[b]]
= resample[b]`, which is what the algorithm means; the tokens up to `num_generated` are the valid ones either way.

`sample_speculative_tree` does the same for a draft that is a token tree (SpecInfer's multi-round rejection, arXiv 2305.09781; a
one-hot rule for deterministic drafters such as Medusa and EAGLE): it follows `flash_attn_with_kvcache_tree`, walks down from the
root accepting at most one child per level, draws one more token, and returns the `path` / `path_len` that
`kvcache_keep_tree_path_` takes.  Two launches of csrc/fa_tree_sample.hip; the rule is written out in include/fa_tree_sample.h.

The rule is written out in include/fa_sample.h.  Unlike the reference's, it leaves no tie open: the token is a function of
(logits, top_k, top_p, temperature, u).  Without `u` the uniforms come from a counter hash of (row, seed, offset), and (seed,
offset) are drawn on the device from torch's generator: `torch.manual_seed` reproduces the tokens, nothing synchronises, and a
HIP graph captures the call.

Not here: the reference's `decode` and `decode_speculative` loops, its CUDA-graph cache (`update_graph_cache`, `capture_graph`), `GenerationMixin` and the
HuggingFace output classes.
"""
from dataclasses import dataclass, field
from typing import Optional, Tuple

import torch
from torch import Tensor

from .._lib import binding as _binding

__all__ = ["InferenceParams", "modify_logits_for_top_k_filtering", "modify_logits_for_top_p_filtering", "sample", "sample_ref",
           "filter_ref", "uniform_ref", "sample_speculative", "sample_speculative_ref", "sample_speculative_tree",
           "sample_speculative_tree_ref"]

_custom_op = torch.library.custom_op
_register_fake = torch.library.register_fake


@dataclass
class InferenceParams:
    """Inference parameters that are passed to the main model in order to calculate and store the context during inference."""

    max_seqlen: int
    max_batch_size: int
    seqlen_offset: int = 0
    batch_size_offset: int = 0
    key_value_memory_dict: dict = field(default_factory=dict)
    lengths_per_sample: Optional[Tensor] = None

    def reset(self, max_seqlen, max_batch_size):
        self.max_seqlen = max_seqlen
        self.max_batch_size = max_batch_size
        self.seqlen_offset = 0
        if self.lengths_per_sample is not None:
            self.lengths_per_sample.zero_()


# ---- the kernel entries ------------------------------------------------------------------------------------------------------
@_custom_op("flash_attn_amd::_sample", mutates_args=(), device_types="cuda")
def _sample(logits: Tensor, top_k: int, top_p: float, temperature: float, u: Optional[Tensor], rng_state: Optional[Tensor],
            stats: bool) -> Tuple[Tensor, Tensor, Tensor]:
    """(token int64, kept int32, mass fp32), each (batch,); kept and mass are empty without `stats` and with top_k == 1.  A
    draw uses `u`, else `rng_state` = (seed, offset) on the device; `sample` always passes one of them, so that the op has no
    hidden state (with neither, the binding would draw a pair from the default generator)."""
    return _binding().sample(logits, top_k, top_p, temperature, u, rng_state, stats)


@_register_fake("flash_attn_amd::_sample")
def _sample_fake(logits, top_k, top_p, temperature, u, rng_state, stats):
    b = logits.shape[0]
    n = b if stats and top_k != 1 else 0
    return (logits.new_empty((b,), dtype=torch.int64), logits.new_empty((n,), dtype=torch.int32),
            logits.new_empty((n,), dtype=torch.float32))


@_custom_op("flash_attn_amd::_sample_filter_", mutates_args=("logits",), device_types="cuda")
def _sample_filter_(logits: Tensor, top_k: int, top_p: float) -> None:
    """-inf over the entries of logits (batch, vocab) that top-k (all ties of the k-th value stay) and then top-p remove."""
    _binding().sample_filter_(logits, top_k, top_p, False)


@_register_fake("flash_attn_amd::_sample_filter_")
def _sample_filter_fake(logits, top_k, top_p):
    return None


@_custom_op("flash_attn_amd::_sample_speculative", mutates_args=(), device_types="cuda")
def _sample_speculative(logits: Tensor, logits_draft: Tensor, tokens_draft: Tensor, top_k: int, top_p: float, temperature: float,
                        u_acc: Optional[Tensor], u_res: Optional[Tensor], rng_state: Optional[Tensor],
                        stats: bool) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor]:
    """(tokens (batch, seqlen + 1) of the dtype of tokens_draft, num_generated (batch,) int64, p_tok, q_tok (batch, seqlen) fp32,
    accepted (batch, seqlen) int32); the last three are empty without `stats`.  The uniforms are (`u_acc`, `u_res`), else
    `rng_state` = (seed, offset) on the device; `sample_speculative` always passes one of them: the op has no hidden state."""
    return _binding().sample_speculative(logits, logits_draft, tokens_draft, top_k, top_p, temperature, u_acc, u_res, rng_state, stats)


@_register_fake("flash_attn_amd::_sample_speculative")
def _sample_speculative_fake(logits, logits_draft, tokens_draft, top_k, top_p, temperature, u_acc, u_res, rng_state, stats):
    b, s = tokens_draft.shape
    shape = (b, s) if stats else (0,)
    return (tokens_draft.new_empty((b, s + 1)), logits.new_empty((b,), dtype=torch.int64), logits.new_empty(shape, dtype=torch.float32),
            logits.new_empty(shape, dtype=torch.float32), logits.new_empty(shape, dtype=torch.int32))


@_custom_op("flash_attn_amd::_sample_speculative_tree", mutates_args=(), device_types="cuda")
def _sample_speculative_tree(logits: Tensor, logits_draft: Optional[Tensor], tokens_draft: Tensor, parents: Tensor, top_k: int,
                             top_p: float, temperature: float, u_acc: Optional[Tensor], u_res: Optional[Tensor],
                             rng_state: Optional[Tensor],
                             stats: bool) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor]:
    """(tokens (batch, nodes) of the dtype of tokens_draft, num_generated (batch,) int64, path (batch, nodes) int32, path_len
    (batch,) int32, p_tok, q_tok (batch, nodes) fp32, visited, accepted (batch, nodes) int32); the last four are empty without
    `stats`.  The uniforms are (`u_acc`, `u_res`), else `rng_state` = (seed, offset) on the device; `sample_speculative_tree`
    always passes one of them: the op has no hidden state."""
    return _binding().sample_speculative_tree(logits, logits_draft, tokens_draft, parents, top_k, top_p, temperature, u_acc, u_res,
                                              rng_state, stats)


@_register_fake("flash_attn_amd::_sample_speculative_tree")
def _sample_speculative_tree_fake(logits, logits_draft, tokens_draft, parents, top_k, top_p, temperature, u_acc, u_res, rng_state, stats):
    b, t = tokens_draft.shape
    shape = (b, t) if stats else (0,)
    return (tokens_draft.new_empty((b, t)), logits.new_empty((b,), dtype=torch.int64), logits.new_empty((b, t), dtype=torch.int32),
            logits.new_empty((b,), dtype=torch.int32), logits.new_empty(shape, dtype=torch.float32),
            logits.new_empty(shape, dtype=torch.float32), logits.new_empty(shape, dtype=torch.int32),
            logits.new_empty(shape, dtype=torch.int32))


def _plan_sample_speculative_tree(logits, logits_draft, tokens_draft, parents, top_k=1, top_p=0.0, temperature=1.0):
    """The form `sample_speculative_tree` takes with these tensors, launching nothing: fa_tree_sample_form
    (include/fa_tree_sample.h) as a dict."""
    return _binding().sample_speculative_tree_plan(logits, logits_draft, tokens_draft, parents, top_k, top_p, temperature, None, None,
                                                   None, False)


def _plan_sample_speculative(logits, logits_draft, tokens_draft, top_k=1, top_p=0.0, temperature=1.0):
    """The form `sample_speculative` takes with these tensors, launching nothing: fa_spec_sample_form (include/fa_spec_sample.h)
    as a dict."""
    return _binding().sample_speculative_plan(logits, logits_draft, tokens_draft, top_k, top_p, temperature, None, None, None, False)


def _plan_sample(logits, top_k=1, top_p=0.0, temperature=1.0, filter=False, stats=False):
    """The form `sample` (filter: the modify_logits_* functions) takes with these logits, launching nothing: fa_sample_form
    (include/fa_sample.h) as a dict."""
    return _binding().sample_plan(logits, top_k, top_p, temperature, filter, stats)


# ---- pure torch: the oracle --------------------------------------------------------------------------------------------------
def _scaled(logits, temperature):
    """s of include/fa_sample.h: one division (by a tensor: no device turns that into a product with the reciprocal) in fp32, or
    in fp64 where given fp64; -0 becomes +0"""
    x = logits if logits.dtype == torch.float64 else logits.float()
    return x / torch.tensor(temperature, dtype=x.dtype, device=x.device) + 0.0


def _top_k_members(s, top_k, ties):
    """(B, V) bool: the min(top_k, V) largest entries of each row, of equal ones the lower indices; with `ties` every entry equal
    to the k-th as well.  top_k == 0: all"""
    v = s.shape[1]
    if top_k <= 0 or top_k >= v:
        return torch.ones_like(s, dtype=torch.bool)
    order = torch.sort(s, dim=1, descending=True, stable=True).indices  # (stable: of equal entries the lower index first)
    if ties:
        return s >= s.gather(1, order[:, top_k - 1:top_k])
    return torch.zeros_like(s, dtype=torch.bool).scatter_(1, order[:, :top_k], True)


def _softmax_over(s, members):
    """softmax of s over `members` (0 elsewhere), written out; rows whose maximum is -inf give zeros"""
    x = s.masked_fill(~members, float("-inf"))
    m = x.max(dim=1, keepdim=True).values
    e = torch.exp(x - torch.where(torch.isinf(m), torch.zeros_like(m), m)).masked_fill(~members, 0.0)
    z = e.sum(dim=1, keepdim=True)
    return e / torch.where(z > 0, z, torch.ones_like(z))


def _top_p_keep(p, members, top_p):
    """-> (keep (B, V) bool, margin (B)).  The members in ascending order of (p, -index); those whose inclusive cumulative
    probability is <= 1 - top_p leave, the largest never.  margin: how close a cumulative sum comes to 1 - top_p"""
    b = p.shape[0]
    if not 0.0 < top_p < 1.0:
        return members, torch.full((b,), float("inf"), dtype=p.dtype, device=p.device)
    # flipped, a stable ascending sort puts the higher index of equal entries first; entries outside come before all (-1)
    srt, idx = torch.sort(p.masked_fill(~members, -1.0).flip(1), dim=1, stable=True)
    inside = srt >= 0
    cum = srt.clamp_min(0.0).cumsum(dim=1)
    threshold = 1.0 - torch.tensor(top_p, dtype=p.dtype, device=p.device)
    leave = (cum <= threshold) & inside
    leave[:, -1] = False
    margin = (cum - threshold).abs().masked_fill(~inside, float("inf")).min(dim=1).values
    keep = members & ~torch.zeros_like(members).scatter_(1, idx, leave).flip(1)
    return keep, margin


def sample_ref(logits, top_k, top_p, temperature, u, stats=False):
    """The contract of include/fa_sample.h in torch, literally and with stable sorts: token (B,) int64 from logits (B, V) and
    uniforms u (B,), in fp64 where logits are fp64 and in fp32 otherwise.  With `stats`: (token, kept, mass, margin), margin (B,)
    being the least distance of a cumulative sum (top-p or draw) from the value it is compared with: rows where it is small are
    those whose result rounding may change."""
    s = _scaled(logits, temperature)
    b, v = s.shape
    u = u.to(s.dtype)
    none = torch.isinf(s.max(dim=1).values) & (s.max(dim=1).values < 0)  # nothing but -inf
    if top_k == 1:
        token = (s == s.max(dim=1, keepdim=True).values).int().argmax(dim=1)
        if not stats:
            return token
        return token, torch.ones(b, dtype=torch.int32, device=s.device), None, torch.full((b,), float("inf"), dtype=s.dtype, device=s.device)
    members = _top_k_members(s, top_k, ties=False)
    p = _softmax_over(s, members)
    keep, margin = _top_p_keep(p, members, top_p)
    left = p.masked_fill(~keep, 0.0)
    mass = left.sum(dim=1)
    cum = (left / torch.where(mass > 0, mass, torch.ones_like(mass))[:, None]).cumsum(dim=1)
    hit = (cum > u[:, None]) & keep
    last = v - 1 - keep.flip(1).int().argmax(dim=1)
    token = torch.where(hit.any(dim=1), hit.int().argmax(dim=1), last)
    token = torch.where(none, torch.zeros_like(token), token)
    if not stats:
        return token
    kept = torch.where(none, torch.zeros_like(token), keep.sum(dim=1)).int()
    margin = torch.minimum(margin, (cum - u[:, None]).abs().masked_fill(~keep, float("inf")).min(dim=1).values)
    return token, kept, torch.where(none, torch.zeros_like(mass), mass), margin


def filter_ref(logits, top_k, top_p, stats=False):
    """What FA_SAMPLE_FILTER leaves of logits (B, V), as a new tensor: -inf over the entries below the min(top_k, V)-th largest
    value (top_k >= 1; all entries equal to it stay), then over those top-p removes of the rest.  With `stats`: (filtered, kept,
    mass, margin)."""
    s = _scaled(logits, 1.0)
    members = _top_k_members(s, top_k, ties=True)
    p = _softmax_over(s, members)
    keep, margin = _top_p_keep(p, members, top_p)
    none = torch.isinf(s.max(dim=1).values) & (s.max(dim=1).values < 0)
    keep = keep | none[:, None]
    out = logits.masked_fill(~keep, float("-inf"))
    if not stats:
        return out
    zero = torch.zeros_like(none, dtype=torch.int64)
    return (out, torch.where(none, zero, keep.sum(dim=1)).int(),
            torch.where(none, torch.zeros_like(p[:, 0]), p.masked_fill(~keep, 0.0).sum(dim=1)), margin)


def _kept_probs(rows, top_k, top_p, temperature):
    """-> (probabilities (N, V) over the kept set of each row of logits (N, V), 0 outside; the top-p margin (N)).  The kept set
    is what FA_SAMPLE_FILTER leaves of s = rows / temperature: all ties of the k-th value stay"""
    s = _scaled(rows, temperature)
    if 0 < top_k < s.shape[1]:  # (what _top_k_members(s, top_k, ties=True) gives: with ties the set needs no order, so no sort)
        members = s >= torch.topk(s, top_k, dim=1).values[:, -1:]
    else:
        members = torch.ones_like(s, dtype=torch.bool)
    keep, margin = _top_p_keep(_softmax_over(s, members), members, top_p)
    # e / Z_kept with e = exp(s - m), as the contract has it: two rows whose kept entries have the same s - m in the same
    # columns get the same probabilities bit for bit, in every precision, and a residual of exactly 0
    m = s.max(dim=1, keepdim=True).values
    e = torch.exp(s - torch.where(torch.isinf(m), torch.zeros_like(m), m)).masked_fill(~keep, 0.0)
    z = e.sum(dim=1, keepdim=True)
    return e / torch.where(z > 0, z, torch.ones_like(z)), margin


def sample_speculative_ref(logits, logits_draft, tokens_draft, top_k, top_p, temperature, u, stats=False):
    """The contract of include/fa_spec_sample.h in torch, literally and with stable sorts: (tokens (B, S + 1) of the dtype of
    tokens_draft, num_generated (B,) int64) from logits (B, S + 1, V), logits_draft (B, S, V), tokens_draft (B, S) and the
    uniforms u = (u_acc (B, S), u_res (B,)); in fp64 where logits are fp64 and in fp32 otherwise.  With `stats`: (tokens,
    num_generated, p_tok, q_tok, accepted, margin).  margin (B,) is the least distance of a comparison made for the sequence
    from the value it compares with: the top-p cumulative sums of the rows up to the first rejected position n_b, the acceptance
    tests up to n_b (|u q - p| relative to max(p, q)), the sum of the residual weights (compared with 0) and the cumulative sums
    of the resample's weights (compared with u_res times their total).  Sequences where it is small are those whose result
    rounding may change.  With stats == "positions" two more follow, both (B, S): the lesser top-p margin of the two rows of a
    position, on which its p_tok and q_tok rest, and the margin of its acceptance test, whatever n_b is."""
    b, s1, v = logits.shape
    s = s1 - 1
    dev = logits.device
    u_acc, u_res = u
    P, mp = _kept_probs(logits.reshape(b * s1, v), top_k, top_p, temperature)
    P, mp = P.view(b, s1, v), mp.view(b, s1)
    dt = P.dtype
    inf = torch.tensor(float("inf"), dtype=dt, device=dev)
    rows = torch.arange(b, device=dev)
    if s > 0:
        Q, mq = _kept_probs(logits_draft.reshape(b * s, v), top_k, top_p, temperature)
        Q, mq = Q.view(b, s, v), mq.view(b, s)
        x = tokens_draft.long()
        inside = (x >= 0) & (x < v)  # a token outside [0, V) is rejected, and nothing is read for it
        xc = x.clamp(0, v - 1)[..., None]
        zero = torch.zeros((), dtype=dt, device=dev)
        p_tok = torch.where(inside, P[:, :s].gather(2, xc)[..., 0], zero)
        q_tok = torch.where(inside, Q.gather(2, xc)[..., 0], zero)
        lhs = u_acc.to(dt) * q_tok
        accepted = (lhs <= p_tok) & inside
        n = torch.where(accepted.all(dim=1), s, (~accepted).int().argmax(dim=1))
        Pn = P[rows, n]
        residual = (Pn - Q[rows, n.clamp(max=s - 1)]).clamp_min(0.0)
        from_p = (n == s) | (residual.sum(dim=1) <= 0)  # no draft row, or no residual weight: p_n itself
        w = torch.where(from_p[:, None], Pn, residual)
    else:
        p_tok = q_tok = torch.zeros(b, 0, dtype=dt, device=dev)
        accepted = torch.zeros(b, 0, dtype=torch.bool, device=dev)
        n = torch.zeros(b, dtype=torch.int64, device=dev)
        w = P[:, 0]
    total = w.sum(dim=1)
    cum, at = w.cumsum(dim=1), (u_res.to(dt) * total)[:, None]  # (the share exceeds u where the sum exceeds u * total)
    positive = w > 0
    hit = (cum > at) & positive
    last = v - 1 - positive.flip(1).int().argmax(dim=1)
    token = torch.where(hit.any(dim=1), hit.int().argmax(dim=1), last)
    token = torch.where(total > 0, token, torch.zeros_like(token))  # (a target row of nothing but -inf)
    tokens = torch.cat([tokens_draft, tokens_draft.new_zeros(b, 1)], dim=1)
    tokens[rows, n] = token.to(tokens.dtype)  # per row; the reference's tokens[:, n] = token writes whole columns
    if not stats:
        return tokens, n + 1
    upto = torch.arange(s1, device=dev)[None, :] <= n[:, None]
    margin = torch.where(upto, mp, inf).min(dim=1).values
    margin = torch.minimum(margin, (cum - at).abs().masked_fill(~positive, float("inf")).min(dim=1).values)
    if s > 0:
        # the residual weights' sum is compared with 0; a sum of exactly 0 is that of two rows equal in the sense of _kept_probs
        margin = torch.minimum(margin, torch.where((n < s) & ~from_p, total, inf))
        margin = torch.minimum(margin, torch.where(upto[:, :s], mq, inf).min(dim=1).values)
        larger = torch.maximum(p_tok, q_tok)
        m_acc = torch.where(inside & (larger > 0), (lhs - p_tok).abs() / torch.where(larger > 0, larger, torch.ones_like(larger)), inf)
        margin = torch.minimum(margin, torch.where(upto[:, :s], m_acc, inf).min(dim=1).values)
    if stats != "positions":
        return tokens, n + 1, p_tok, q_tok, accepted.int(), margin
    if s == 0:
        return tokens, n + 1, p_tok, q_tok, accepted.int(), margin, p_tok, p_tok
    return tokens, n + 1, p_tok, q_tok, accepted.int(), margin, torch.minimum(mp[:, :s], mq), m_acc


def sample_speculative_tree_ref(logits, logits_draft, tokens_draft, parents, top_k, top_p, temperature, u, stats=False):
    """The contract of include/fa_tree_sample.h in torch, literally and with stable sorts: (tokens (B, T) of the dtype of
    tokens_draft, num_generated (B,) int64, path (B, T) int32, path_len (B,) int32) from logits (B, T, V), logits_draft (B, T, V)
    or None (the one-hot rule), tokens_draft (B, T), parents (B, T) and the uniforms u = (u_acc (B, T), u_res (B,)); in fp64 where
    logits are fp64 and in fp32 otherwise.  The nodes are taken in index order, which is the order of the walk: a child follows
    its parent and its earlier siblings.  Probabilities are floating point (P - c Q in two roundings, not the header's fmaf and
    fixed point): what separates the two is what `margin` measures.
    With `stats`: (tokens, num_generated, path, path_len, p_tok, q_tok, visited, accepted, margin).  margin (B,) is the least
    distance of a comparison made along the walk of the sequence from the value it compares with: the top-p cumulative sums of
    the rows of every node on the path (the draft row where a child was tried), the acceptance tests (round 0: |u q - p| relative
    to max(p, q); later rounds |u q - r_x / R| relative to max(q, r_x / R); one-hot: |u Z_r - w_x| relative to max(w_x, Z_r)), the
    sums R(c) and Z_r (compared with 0) and the cumulative sums of the draw's weights (compared with u_res times their total).
    Sequences where it is small are those whose result rounding may change.  With stats == "positions" one more follows, (B, T):
    the lesser top-p margin of the rows of a node's parent, on which its p_tok and q_tok rest."""
    b, t, v = logits.shape
    dev = logits.device
    u_acc, u_res = u
    drafts = logits_draft is not None
    P, mp = _kept_probs(logits.reshape(b * t, v), top_k, top_p, temperature)
    P, mp = P.view(b, t, v), mp.view(b, t)
    dt = P.dtype
    if drafts:
        Q, mq = _kept_probs(logits_draft.reshape(b * t, v), top_k, top_p, temperature)
        Q, mq = Q.view(b, t, v), mq.view(b, t)
    inf = torch.tensor(float("inf"), dtype=dt, device=dev)
    zero, one = torch.zeros((), dtype=dt, device=dev), torch.ones((), dtype=dt, device=dev)
    rows = torch.arange(b, device=dev)
    par_all = parents.long()
    n = torch.zeros(b, dtype=torch.int64, device=dev)    # the node the walk is at
    m = torch.zeros(b, dtype=torch.int64, device=dev)    # the rejections at n
    c = torch.zeros(b, dtype=dt, device=dev)
    R = torch.zeros(b, dtype=dt, device=dev)             # R(c) of the last rejection at n; one-hot: Z_r
    done = torch.zeros(b, dtype=torch.bool, device=dev)  # nothing is left at n: its siblings are not tried
    gone = torch.zeros(b, v, dtype=torch.bool, device=dev)  # one-hot: the tokens rejected at n
    margin = mp[:, 0].clone()
    p_tok, q_tok = torch.zeros(b, t, dtype=dt, device=dev), torch.zeros(b, t, dtype=dt, device=dev)
    m_rows = torch.full((b, t), float("inf"), dtype=dt, device=dev)
    visited, accepted = torch.zeros(b, t, dtype=torch.int32, device=dev), torch.zeros(b, t, dtype=torch.int32, device=dev)
    path = torch.zeros(b, t, dtype=torch.int32, device=dev)
    length = torch.ones(b, dtype=torch.int64, device=dev)
    if not drafts:
        R = P[:, 0].sum(dim=1)
    for i in range(1, t):
        par = par_all[:, i]
        present = (par >= 0) & (par < i)
        pc = par.clamp(0, i - 1)
        x = tokens_draft[:, i].long()
        inside = (x >= 0) & (x < v)  # a token outside [0, V) is rejected, and nothing is read for it
        xc = x.clamp(0, v - 1)
        p0 = torch.where(present & inside, P[rows, pc, xc], zero)
        q0 = torch.where(present & inside, Q[rows, pc, xc] if drafts else one, zero)
        p_tok[:, i], q_tok[:, i] = p0, q0
        m_rows[:, i] = torch.where(present, torch.minimum(mp[rows, pc], mq[rows, pc]) if drafts else mp[rows, pc], inf)
        run = present & (par == n) & ~done
        if not bool(run.any()):
            continue
        ui = u_acc[:, i].to(dt)
        Pn = P[rows, n]
        if drafts:
            Qn = Q[rows, n]
            margin = torch.where(run, torch.minimum(margin, mq[rows, n]), margin)
            first = m == 0
            rx = (p0 - c * q0).clamp_min(0.0)
            lhs = torch.where(first, ui * q0, ui * q0 * R)
            rhs = torch.where(first, p0, rx)
            ok = (lhs <= rhs) & inside
            share = torch.where(first, p0, rx / torch.where(R > 0, R, torch.ones_like(R)))  # (R > 0 where a later round runs)
            larger = torch.maximum(share, q0)
            m_acc = torch.where(inside & (larger > 0), (ui * q0 - share).abs() / torch.where(larger > 0, larger, torch.ones_like(larger)), inf)
        else:
            w = torch.where(inside & ~gone[rows, xc], p0, zero)
            ok = (w > 0) & (ui * R <= w)
            larger = torch.maximum(w, R)
            m_acc = torch.where(w > 0, (ui * R - w).abs() / torch.where(larger > 0, larger, torch.ones_like(larger)), inf)
        margin = torch.where(run, torch.minimum(margin, m_acc), margin)
        visited[:, i] = run.int()
        yes, no = run & ok, run & ~ok
        accepted[:, i] = yes.int()
        # rejected: the next round's c and R
        if drafts:
            c_next = torch.where(first, torch.ones_like(c), c + R)
            R_next = (Pn - c_next[:, None] * Qn).clamp_min(0.0).sum(dim=1)
            c, R = torch.where(no, c_next, c), torch.where(no, R_next, R)
        else:
            gone[rows[no & (w > 0)], xc[no & (w > 0)]] = True
            R = torch.where(no, R - w, R)
        m = torch.where(no, m + 1, m)
        done = done | (no & (R <= 0))
        margin = torch.where(no & (R > 0), torch.minimum(margin, R), margin)  # (a sum of exactly 0: of rows equal entry by entry)
        # accepted: down to i
        path[rows[yes], length[yes]] = i
        length = torch.where(yes, length + 1, length)
        n = torch.where(yes, torch.full_like(n, i), n)
        m, c = torch.where(yes, torch.zeros_like(m), m), torch.where(yes, torch.zeros_like(c), c)
        margin = torch.where(yes, torch.minimum(margin, mp[:, i]), margin)
        if drafts:
            R = torch.where(yes, torch.zeros_like(R), R)
        else:
            R = torch.where(yes, P[:, i].sum(dim=1), R)
            gone[yes] = False
    Pn = P[rows, n]
    if drafts:
        residual = (Pn - c[:, None] * Q[rows, n]).clamp_min(0.0)
        from_p = (m == 0) | (residual.sum(dim=1) <= 0)  # no child, or no residual weight: p_n itself
        w = torch.where(from_p[:, None], Pn, residual)
    else:
        w = Pn.masked_fill(gone, 0.0)
    total = w.sum(dim=1)
    cum, at = w.cumsum(dim=1), (u_res.to(dt) * total)[:, None]  # (the share exceeds u where the sum exceeds u * total)
    positive = w > 0
    hit = (cum > at) & positive
    last = v - 1 - positive.flip(1).int().argmax(dim=1)
    token = torch.where(hit.any(dim=1), hit.int().argmax(dim=1), last)
    token = torch.where(total > 0, token, torch.zeros_like(token))  # (a target row that keeps nothing, or nothing left of it)
    # the tokens of the path without the root's, then the drawn one
    cols = torch.arange(t, device=dev)[None, :]
    nxt = torch.cat([path[:, 1:], path.new_zeros(b, 1)], dim=1).long()
    tokens = torch.where(cols < length[:, None] - 1, tokens_draft.gather(1, nxt), torch.zeros_like(tokens_draft))
    tokens[rows, length - 1] = token.to(tokens.dtype)
    out = (tokens, length.clone(), path, length.int())
    if not stats:
        return out
    margin = torch.minimum(margin, (cum - at).abs().masked_fill(~positive, float("inf")).min(dim=1).values)
    out = out + (p_tok, q_tok, visited, accepted, margin)
    return out + (m_rows,) if stats == "positions" else out


def _lowbias32(x):
    x = x ^ (x >> 16)
    x = (x * 0x7FEB352D) & 0xFFFFFFFF
    x = x ^ (x >> 15)
    x = (x * 0x846CA68B) & 0xFFFFFFFF
    return x ^ (x >> 16)


def uniform_ref(seed, offset, batch, device="cpu"):
    """The uniforms the kernel forms from rng_state = (seed, offset) for rows 0 .. batch - 1 (include/fa_sample.h), fp32."""
    seed, offset = seed & 0xFFFFFFFFFFFFFFFF, offset & 0xFFFFFFFFFFFFFFFF
    x = (seed & 0xFFFFFFFF) ^ ((seed >> 32) * 0x27D4EB2F & 0xFFFFFFFF) ^ ((offset & 0xFFFFFFFF) * 0xC2B2AE3D & 0xFFFFFFFF) ^ (offset >> 32)
    x ^= x >> 15
    x = (x * 0x2C1B3C6D) & 0xFFFFFFFF
    x ^= x >> 12
    r = torch.arange(batch, dtype=torch.int64, device=device)
    h = _lowbias32(((x ^ ((r >> 32) * 0x2545F491 & 0xFFFFFFFF)) ^ ((r & 0xFFFFFFFF) * 0x9E3779B1 & 0xFFFFFFFF)) & 0xFFFFFFFF)
    return (h >> 8).float() * 2.0 ** -24


# ---- the reference's names -----------------------------------------------------------------------------------------------------
def _rows(logits):
    """logits (..., vocab) as (batch, vocab) without a copy"""
    if logits.stride(-1) != 1 and logits.shape[-1] > 1:
        raise ValueError("logits must have a contiguous last dimension")
    return logits if logits.dim() == 2 else logits.view(-1, logits.shape[-1])


def _filter_(logits, top_k, top_p):
    rows = _rows(logits)
    if rows.is_cuda:
        _sample_filter_(rows, top_k, top_p)
    else:
        rows.copy_(filter_ref(rows, top_k, top_p))


def modify_logits_for_top_k_filtering(logits, top_k):
    """Set the logits for none top-k values to -inf. Done in-place."""
    if top_k > logits.shape[-1]:
        raise RuntimeError("selected index k out of range")  # (what the reference's torch.topk raises)
    _filter_(logits, top_k, 0.0)


def modify_logits_for_top_p_filtering(logits, top_p):
    """Set the logits for none top-p values to -inf. Done in-place."""
    if top_p <= 0.0 or top_p >= 1.0:
        return
    _filter_(logits, 0, top_p)


def sample(logits, top_k=1, top_p=0.0, temperature=1.0, *, generator=None, u=None):
    """Sample from top-k logits.
    Arguments:
        logits: Tensor of shape (batch_size, vocab_size), fp16 / bf16 / fp32, any row stride
        generator: the torch.Generator (of the logits' device) that (seed, offset) are drawn from; default: the device's own
        u: (batch_size,) fp32 uniforms in [0, 1) to draw with, instead of a generator
    Returns the tokens, (batch_size,) int64.  logits are not modified.
    """
    if top_k != 1 and top_p > 0.0:
        assert top_p <= 1.0, "top-p should be in (0, 1]."
    top_p = top_p if top_p > 0.0 else 0.0
    if not logits.is_cuda:
        if u is None:
            u = torch.rand(logits.shape[0], generator=generator, device=logits.device)
        return sample_ref(logits, top_k, top_p, temperature, u)
    rng_state = None
    if u is None and top_k != 1:  # drawn here, not inside the op: the op is a function of its arguments
        rng_state = torch.randint(-(1 << 62), 1 << 62, (2,), generator=generator, device=logits.device, dtype=torch.int64)
    return _sample(logits, top_k, top_p, temperature, None if top_k == 1 else u, rng_state, False)[0]


def sample_speculative(logits, logits_draft, tokens_draft, top_k=1, top_p=0.0, temperature=1.0, *, generator=None, u=None):
    """Verify `seqlen` draft tokens per sequence against the target model and emit the accepted prefix plus one more token
    (speculative sampling: Leviathan, Kalman, Matias, arXiv 2211.17192, Algorithm 1).  The rule is in include/fa_spec_sample.h.

    logits        (batch, seqlen + 1, vocab) target logits, fp16 / bf16 / fp32, any batch and position stride
    logits_draft  (batch, seqlen, vocab) draft logits of the same dtype
    tokens_draft  (batch, seqlen) int32 or int64: the tokens the draft model proposed
    top_k, top_p, temperature: as in `sample`, applied to both models' rows with the filter's top-k rule (ties stay)
    generator     the torch.Generator (of the logits' device) that (seed, offset) are drawn from; default: the device's own
    u             (u_acc (batch, seqlen), u_res (batch,)) fp32 uniforms in [0, 1) to accept and to resample with, instead of a
                  generator

    -> (tokens (batch, seqlen + 1) of the dtype of tokens_draft, num_generated (batch,) int64 in [1, seqlen + 1]).  Of row b the
    first num_generated[b] tokens are valid: the accepted drafts and, at column num_generated[b] - 1, the token drawn there.
    That token is written to its own row only (the module docstring says how the reference differs).  Nothing is modified.
    """
    if logits.dim() != 3 or logits.shape[1] < 1:
        raise ValueError("logits must have shape (batch, seqlen + 1, vocab)")
    b, v = logits.shape[0], logits.shape[2]
    s = logits.shape[1] - 1
    if tuple(logits_draft.shape) != (b, s, v) or tuple(tokens_draft.shape) != (b, s):
        raise ValueError(f"logits_draft must have shape {(b, s, v)} and tokens_draft {(b, s)}: got {tuple(logits_draft.shape)} and "
                         f"{tuple(tokens_draft.shape)}")
    if tokens_draft.dtype not in (torch.int32, torch.int64):
        raise TypeError("tokens_draft must be int32 or int64")
    if top_p > 1.0:
        raise ValueError("top_p must be at most 1")
    top_p = max(float(top_p), 0.0)
    if not logits.is_cuda:
        if u is None:
            u = (torch.rand(b, s, generator=generator, device=logits.device), torch.rand(b, generator=generator, device=logits.device))
        return sample_speculative_ref(logits, logits_draft, tokens_draft, top_k, top_p, temperature, u)
    if v > 1 and (logits.stride(-1) != 1 or logits_draft.stride(-1) != 1):
        raise ValueError("logits and logits_draft must have a contiguous last dimension")
    if s > 1 and tokens_draft.stride(-1) != 1:
        tokens_draft = tokens_draft.contiguous()
    rng_state = None
    if u is None:  # drawn here, not inside the op: the op is a function of its arguments
        rng_state = torch.randint(-(1 << 62), 1 << 62, (2,), generator=generator, device=logits.device, dtype=torch.int64)
    u_acc, u_res = u if u is not None else (None, None)
    return _sample_speculative(logits, logits_draft, tokens_draft, top_k, top_p, temperature, u_acc, u_res, rng_state, False)[:2]


def sample_speculative_tree(logits, logits_draft, tokens_draft, parents, top_k=1, top_p=0.0, temperature=1.0, *, generator=None,
                            u=None, stats=False):
    """Verify a TREE of draft tokens per sequence against the target model: walk down from the root, accepting at most one child
    per level by multi-round rejection (SpecInfer, arXiv 2305.09781), and emit the accepted path plus one more token.  What
    follows `flash_attn_with_kvcache_tree` in a tree-shaped verify step; `path` and `path_len` are what
    `kvcache_keep_tree_path_` takes.  Not in the reference.  The rule is in include/fa_tree_sample.h.

    logits        (batch, nodes, vocab) target logits, fp16 / bf16 / fp32, any batch and node stride; row n is the distribution
                  of the token that follows node n.  1 <= nodes <= 64
    logits_draft  (batch, nodes, vocab) of the same dtype: row n is the distribution the children of node n were drawn from,
                  independently (duplicates allowed); or None for a deterministic drafter (Medusa / EAGLE with top-m children):
                  a child is accepted with the target's probability of its token among the tokens not yet rejected at its parent
    tokens_draft  (batch, nodes) int32 or int64: the token of every node; entry 0, the root's (the last committed token), is not
                  read
    parents       (batch, nodes) int32: parents[b, i] in [0, i) is the parent of node i > 0; any other value (-1) marks an absent
                  node, the padding of ragged trees, as in `tree_mask_from_parents`.  The children of a node are tried in
                  ascending index order
    top_k, top_p, temperature: as in `sample_speculative`, applied to both models' rows
    generator     the torch.Generator (of the logits' device) that (seed, offset) are drawn from; default: the device's own
    u             (u_acc (batch, nodes), u_res (batch,)) fp32 uniforms in [0, 1): u_acc[b, i] tests node i (entry 0 unused), u_res
                  draws the last token; instead of a generator

    -> (tokens (batch, nodes) of the dtype of tokens_draft, num_generated (batch,) int64, path (batch, nodes) int32, path_len
    (batch,) int32).  path[b, :path_len[b]] are the accepted nodes in ascending order, the root first; tokens[b, :num_generated[b]]
    are their tokens without the root's and then the token drawn behind the last of them; num_generated = path_len.  Behind
    them both hold 0.  With `stats` four more follow, (batch, nodes) each: p_tok, q_tok fp32 (the target's and the draft's
    probability of a node's token under its parent, before any rejection), visited and accepted int32.  Nothing is modified.
    A chain (parents = -1, 0, 1, ...) is `sample_speculative`, bit for bit.
    """
    if logits.dim() != 3 or not 1 <= logits.shape[1] <= 64:
        raise ValueError("logits must have shape (batch, nodes, vocab) with 1 <= nodes <= 64")
    b, t, v = logits.shape
    if logits_draft is not None and tuple(logits_draft.shape) != (b, t, v):
        raise ValueError(f"logits_draft must have shape {(b, t, v)}: got {tuple(logits_draft.shape)}")
    if tuple(tokens_draft.shape) != (b, t) or tuple(parents.shape) != (b, t):
        raise ValueError(f"tokens_draft and parents must have shape {(b, t)}: got {tuple(tokens_draft.shape)} and {tuple(parents.shape)}")
    if tokens_draft.dtype not in (torch.int32, torch.int64):
        raise TypeError("tokens_draft must be int32 or int64")
    if top_p > 1.0:
        raise ValueError("top_p must be at most 1")
    top_p = max(float(top_p), 0.0)
    if not logits.is_cuda:
        if u is None:
            u = (torch.rand(b, t, generator=generator, device=logits.device), torch.rand(b, generator=generator, device=logits.device))
        out = sample_speculative_tree_ref(logits, logits_draft, tokens_draft, parents, top_k, top_p, temperature, u, stats=bool(stats))
        return out[:8] if stats else out
    if v > 1 and (logits.stride(-1) != 1 or (logits_draft is not None and logits_draft.stride(-1) != 1)):
        raise ValueError("logits and logits_draft must have a contiguous last dimension")
    if t > 1 and tokens_draft.stride(-1) != 1:
        tokens_draft = tokens_draft.contiguous()
    if parents.dtype != torch.int32 or (t > 1 and parents.stride(-1) != 1):
        parents = parents.to(torch.int32).contiguous()
    rng_state = None
    if u is None:  # drawn here, not inside the op: the op is a function of its arguments
        rng_state = torch.randint(-(1 << 62), 1 << 62, (2,), generator=generator, device=logits.device, dtype=torch.int64)
    u_acc, u_res = u if u is not None else (None, None)
    out = _sample_speculative_tree(logits, logits_draft, tokens_draft, parents, top_k, top_p, temperature, u_acc, u_res, rng_state,
                                   bool(stats))
    return out if stats else out[:4]
