"""The step between (batch, vocab) logits and the next token, behind the names of the reference's `flash_attn/utils/generation.py`:

    InferenceParams                              reference :23-40
    modify_logits_for_top_k_filtering                      :45-48
    modify_logits_for_top_p_filtering                      :53-66
    sample                                                 :69-95
    sample_ref, filter_ref, uniform_ref          pure torch: the contract of include/fa_sample.h, the CPU oracle

Same signatures and defaults; `sample` has two keyword-only additions, `generator` and `u`.  Where the reference chains topk,
a full sort, softmax, cumsum, scatter, masked_fill and multinomial, CUDA tensors here take one launch of the HIP kernels of
csrc/fa_sample.hip through `flash_attn_2_cuda_C.sample` / `sample_filter_`, wrapped in torch.library custom ops with fake
implementations, so torch.compile traces them.  There is no eager fall-back on the device: without the built library the ops
raise.  CPU tensors take the oracle.

The rule is written out in include/fa_sample.h.  Unlike the reference's, it leaves no tie open: the token is a function of
(logits, top_k, top_p, temperature, u).  Without `u` the uniforms come from a counter hash of (row, seed, offset), and (seed,
offset) are drawn on the device from torch's generator: `torch.manual_seed` reproduces the tokens, nothing synchronises, and a
HIP graph captures the call.

Not here: the reference's `decode` loop, its CUDA-graph cache (`update_graph_cache`, `capture_graph`), `GenerationMixin` and the
HuggingFace output classes.
"""
from dataclasses import dataclass, field
from typing import Optional, Tuple

import torch
from torch import Tensor

from .._lib import binding as _binding

__all__ = ["InferenceParams", "modify_logits_for_top_k_filtering", "modify_logits_for_top_p_filtering", "sample", "sample_ref",
           "filter_ref", "uniform_ref"]

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
