"""Rotary position embedding behind the names of the reference's `flash_attn/layers/rotary.py`:

    apply_rotary_emb (= apply_rotary_emb_func)    reference :93-127
    apply_rotary_emb_torch                        reference :23-35
    apply_rotary_emb_qkv_                         reference :236-264
    apply_rotary_emb_kv_                          reference :308-328
    RotaryEmbedding                               reference :331-482

Same argument order and defaults.  Where the reference launches a Triton kernel (ops/triton/rotary.py: apply_rotary), this
module launches the HIP kernel of csrc/fa_rotary_emb.hip through `flash_attn_2_cuda_C.rotary_emb`: one launch per call,
forward and -- with conjugate=True -- backward, in place where the forward ran in place.  The kernel entry is a pair of
torch.library custom ops (one returning a new tensor, one mutating x) with fake implementations, so torch.compile traces
the layer.  There is no eager fall-back: without the built library the ops raise.
"""
from typing import Optional, Tuple, Union

import torch

from .._lib import binding as _binding

_custom_op = torch.library.custom_op
_register_fake = torch.library.register_fake


# ---- the kernel entry: an int offset and a tensor offset are two arguments here (an op schema has no unions) -----------------
@_custom_op("flash_attn_amd::_rotary_emb", mutates_args=(), device_types="cuda")
def _rotary_emb(x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, seqlen_offset: int,
                seqlen_offsets: Optional[torch.Tensor], cu_seqlens: Optional[torch.Tensor], max_seqlen: Optional[int],
                interleaved: bool, conjugate: bool) -> torch.Tensor:
    offsets = seqlen_offset if seqlen_offsets is None else seqlen_offsets
    return _binding().rotary_emb(x, cos, sin, offsets, cu_seqlens, max_seqlen, interleaved, False, conjugate)


@_register_fake("flash_attn_amd::_rotary_emb")
def _rotary_emb_fake(x, cos, sin, seqlen_offset, seqlen_offsets, cu_seqlens, max_seqlen, interleaved, conjugate):
    return torch.empty_like(x)


@_custom_op("flash_attn_amd::_rotary_emb_", mutates_args=("x",), device_types="cuda")
def _rotary_emb_(x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, seqlen_offset: int,
                 seqlen_offsets: Optional[torch.Tensor], cu_seqlens: Optional[torch.Tensor], max_seqlen: Optional[int],
                 interleaved: bool, conjugate: bool) -> None:
    offsets = seqlen_offset if seqlen_offsets is None else seqlen_offsets
    _binding().rotary_emb(x, cos, sin, offsets, cu_seqlens, max_seqlen, interleaved, True, conjugate)


@_register_fake("flash_attn_amd::_rotary_emb_")
def _rotary_emb__fake(x, cos, sin, seqlen_offset, seqlen_offsets, cu_seqlens, max_seqlen, interleaved, conjugate):
    return None


def apply_rotary(x, cos, sin, seqlen_offsets: Union[int, torch.Tensor] = 0, cu_seqlens: Optional[torch.Tensor] = None,
                 max_seqlen: Optional[int] = None, interleaved=False, inplace=False, conjugate=False) -> torch.Tensor:
    """The launch itself, under the signature of the reference's ops.triton.rotary.apply_rotary (:102-112)."""
    if not x.is_cuda:
        raise RuntimeError("x must be on CUDA")
    if isinstance(seqlen_offsets, torch.Tensor):
        off, off_t = 0, seqlen_offsets
    else:
        off, off_t = int(seqlen_offsets), None
    if inplace:
        _rotary_emb_(x, cos, sin, off, off_t, cu_seqlens, max_seqlen, interleaved, conjugate)
        return x
    return _rotary_emb(x, cos, sin, off, off_t, cu_seqlens, max_seqlen, interleaved, conjugate)


# ---- pure-torch statement of the rotation ---------------------------------------------------------------------------
def rotate_half(x, interleaved=False):
    if interleaved:
        even, odd = x[..., 0::2], x[..., 1::2]
        return torch.stack((-odd, even), dim=-1).flatten(-2)
    lo, hi = x.chunk(2, dim=-1)
    return torch.cat((-hi, lo), dim=-1)


def apply_rotary_emb_torch(x, cos, sin, interleaved=False):
    """x: (batch, seqlen, nheads, headdim); cos, sin: (seqlen, rotary_dim / 2) or (batch, seqlen, rotary_dim / 2)."""
    rot = 2 * cos.shape[-1]
    assert rot <= x.shape[-1]
    if interleaved:  # every table entry serves the pair (2j, 2j + 1)
        cos, sin = cos.repeat_interleave(2, dim=-1), sin.repeat_interleave(2, dim=-1)
    else:  # ... the pair (j, j + rot / 2)
        cos, sin = torch.cat((cos, cos), dim=-1), torch.cat((sin, sin), dim=-1)
    cos, sin = cos.unsqueeze(-2), sin.unsqueeze(-2)  # one head axis
    head, tail = x[..., :rot], x[..., rot:]
    return torch.cat((head * cos + rotate_half(head, interleaved) * sin, tail), dim=-1)


# ---- autograd ---------------------------------------------------------------------------------------------------------
def _stash_offsets(ctx, seqlen_offsets, *tensors):
    """An int offset lives on ctx, a tensor offset among the saved tensors (last)."""
    if isinstance(seqlen_offsets, torch.Tensor):
        ctx.save_for_backward(*tensors, seqlen_offsets)
        ctx.int_offset = None
    else:
        ctx.save_for_backward(*tensors)
        ctx.int_offset = seqlen_offsets


def _fetch_offsets(ctx):
    saved = ctx.saved_tensors
    if ctx.int_offset is None:
        return saved[:-1], saved[-1]
    return saved, ctx.int_offset


class ApplyRotaryEmb(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, cos, sin, interleaved=False, inplace=False, seqlen_offsets: Union[int, torch.Tensor] = 0,
                cu_seqlens: Optional[torch.Tensor] = None, max_seqlen: Optional[int] = None):
        out = apply_rotary(x, cos, sin, seqlen_offsets=seqlen_offsets, cu_seqlens=cu_seqlens, max_seqlen=max_seqlen,
                           interleaved=interleaved, inplace=inplace)
        _stash_offsets(ctx, seqlen_offsets, cos, sin, cu_seqlens)
        ctx.interleaved, ctx.inplace, ctx.max_seqlen = interleaved, inplace, max_seqlen
        return x if inplace else out

    @staticmethod
    def backward(ctx, do):
        (cos, sin, cu_seqlens), offsets = _fetch_offsets(ctx)
        dx = apply_rotary(do, cos, sin, seqlen_offsets=offsets, cu_seqlens=cu_seqlens, max_seqlen=ctx.max_seqlen,
                          interleaved=ctx.interleaved, inplace=ctx.inplace, conjugate=True)
        return dx, None, None, None, None, None, None, None


def apply_rotary_emb(x, cos, sin, interleaved=False, inplace=False, seqlen_offsets: Union[int, torch.Tensor] = 0,
                     cu_seqlens: Optional[torch.Tensor] = None, max_seqlen: Optional[int] = None):
    """Rotate the first rotary_dim = 2 * cos.shape[-1] columns of every head of x.

    x: (batch, seqlen, nheads, headdim), or (total_seqlen, nheads, headdim) with cu_seqlens (batch + 1) and max_seqlen.
    cos, sin: (seqlen_rotary, rotary_dim / 2), rotary_dim <= headdim.
    interleaved: pairs of neighbouring columns (GPT-J) instead of the first and the second half (GPT-NeoX).
    inplace: write into x.
    seqlen_offsets: an int or a (batch,) tensor: sequence s starts at position seqlen_offsets[s] (decoding with a KV cache).
    Returns a tensor of x's shape.
    """
    return ApplyRotaryEmb.apply(x, cos, sin, interleaved, inplace, seqlen_offsets, cu_seqlens, max_seqlen)


apply_rotary_emb_func = apply_rotary_emb  # (the older name)


def _qkv_heads(qkv, num_heads_q):
    """(q heads, k heads) of a packed (b, s, hq + 2 hk, d) tensor."""
    assert qkv.dim() == 4 and num_heads_q is not None
    num_heads_k = (qkv.shape[2] - num_heads_q) // 2
    assert qkv.shape[2] == num_heads_q + 2 * num_heads_k
    return num_heads_q, num_heads_k


def _rotate_qk_(qkv, cos, sin, cos_k, sin_k, interleaved, seqlen_offsets, num_heads_q, conjugate):
    """Rotate q and k of a packed qkv in place: one launch over the (b, s, hq + hk, d) view where both take the same tables and
    the tensor is contiguous, otherwise one launch each."""
    if qkv.dim() == 5:
        assert qkv.shape[2] == 3
    else:
        hq, hk = _qkv_heads(qkv, num_heads_q)
    if cos_k is None and sin_k is None and qkv.is_contiguous():
        if qkv.dim() == 5:
            b, s, _, h, d = qkv.shape
            qk = qkv[:, :, :2].view(b, s, 2 * h, d)  # (a view: the (3, h) axes of a contiguous tensor merge)
        else:
            qk = qkv[:, :, :hq + hk]
        apply_rotary(qk, cos, sin, seqlen_offsets=seqlen_offsets, interleaved=interleaved, inplace=True, conjugate=conjugate)
        return qkv
    if qkv.dim() == 5:
        q, k = qkv[:, :, 0], qkv[:, :, 1]
    else:
        q, k = qkv[:, :, :hq], qkv[:, :, hq:hq + hk]
    apply_rotary(q, cos, sin, seqlen_offsets=seqlen_offsets, interleaved=interleaved, inplace=True, conjugate=conjugate)
    apply_rotary(k, cos if cos_k is None else cos_k, sin if sin_k is None else sin_k, seqlen_offsets=seqlen_offsets,
                 interleaved=interleaved, inplace=True, conjugate=conjugate)
    return qkv


class ApplyRotaryEmbQKV_(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, cos, sin, cos_k=None, sin_k=None, interleaved=False, seqlen_offsets: Union[int, torch.Tensor] = 0,
                num_heads_q: Optional[int] = None):
        _rotate_qk_(qkv, cos, sin, cos_k, sin_k, interleaved, seqlen_offsets, num_heads_q, conjugate=False)
        _stash_offsets(ctx, seqlen_offsets, cos, sin, cos_k, sin_k)
        ctx.interleaved, ctx.num_heads_q = interleaved, num_heads_q
        return qkv

    @staticmethod
    def backward(ctx, dqkv):
        (cos, sin, cos_k, sin_k), offsets = _fetch_offsets(ctx)
        _rotate_qk_(dqkv, cos, sin, cos_k, sin_k, ctx.interleaved, offsets, ctx.num_heads_q, conjugate=True)
        return dqkv, None, None, None, None, None, None, None


def apply_rotary_emb_qkv_(qkv, cos, sin, cos_k=None, sin_k=None, interleaved=False,
                          seqlen_offsets: Union[int, torch.Tensor] = 0, num_heads_q: Optional[int] = None):
    """Rotate Q and K of a packed tensor *in place*; V is not touched.

    qkv: (batch, seqlen, 3, nheads, headdim), or (batch, seqlen, num_heads_q + 2 * num_heads_k, headdim) for MQA / GQA, which
        needs num_heads_q.
    cos, sin: (seqlen, rotary_dim / 2); cos_k, sin_k: the same shape, tables of K's own (optional).
    interleaved, seqlen_offsets: as in apply_rotary_emb.
    Returns qkv.
    """
    return ApplyRotaryEmbQKV_.apply(qkv, cos, sin, cos_k, sin_k, interleaved, seqlen_offsets, num_heads_q)


class ApplyRotaryEmbKV_(torch.autograd.Function):
    @staticmethod
    def forward(ctx, kv, cos, sin, interleaved=False, seqlen_offsets: Union[int, torch.Tensor] = 0):
        assert kv.dim() == 5 and kv.shape[2] == 2
        apply_rotary(kv[:, :, 0], cos, sin, seqlen_offsets=seqlen_offsets, interleaved=interleaved, inplace=True)
        _stash_offsets(ctx, seqlen_offsets, cos, sin)
        ctx.interleaved = interleaved
        return kv

    @staticmethod
    def backward(ctx, dkv):
        (cos, sin), offsets = _fetch_offsets(ctx)
        apply_rotary(dkv[:, :, 0], cos, sin, seqlen_offsets=offsets, interleaved=ctx.interleaved, inplace=True, conjugate=True)
        return dkv, None, None, None, None


def apply_rotary_emb_kv_(kv, cos, sin, interleaved=False, seqlen_offsets: Union[int, torch.Tensor] = 0):
    """Rotate K of a packed (batch, seqlen, 2, nheads, headdim) tensor *in place*; V is not touched.  Returns kv."""
    return ApplyRotaryEmbKV_.apply(kv, cos, sin, interleaved, seqlen_offsets)


class RotaryEmbedding(torch.nn.Module):
    """Rotary position embedding (RoFormer, Su et al., https://arxiv.org/abs/2104.09864) with a cache of the cos / sin tables.

    With scale_base the tables carry the xPos length scaling (Sun et al., https://arxiv.org/abs/2212.10554): Q's tables are
    multiplied by scale ** ((t - seqlen // 2) / scale_base) and K's divided by it.  512 is the commonly used value.
    """

    def __init__(self, dim: int, base=10000.0, interleaved=False, scale_base=None, device=None):
        super().__init__()
        self.dim = dim
        self.base = float(base)
        self.interleaved = interleaved
        self.scale_base = scale_base
        self.register_buffer("inv_freq", self._compute_inv_freq(device), persistent=False)
        scale = None
        if scale_base is not None:
            scale = (torch.arange(0, dim, 2, device=device, dtype=torch.float32) + 0.4 * dim) / (1.4 * dim)
        self.register_buffer("scale", scale, persistent=False)
        self._seq_len_cached = 0
        self._cos_cached = self._sin_cached = self._cos_k_cached = self._sin_k_cached = None

    def _compute_inv_freq(self, device=None):
        return 1.0 / (self.base ** (torch.arange(0, self.dim, 2, device=device, dtype=torch.float32) / self.dim))

    def _update_cos_sin_cache(self, seqlen, device=None, dtype=None):
        """Rebuild the tables when they are too short, on another device or of another dtype, or were made under inference
        mode and the module now trains."""
        cached = self._cos_cached
        if not (seqlen > self._seq_len_cached or cached is None or cached.device != device or cached.dtype != dtype
                or (self.training and cached.is_inference())):
            return
        self._seq_len_cached = seqlen
        # angles in fp32 whatever the model's dtype: t * inv_freq is large, and inv_freq may have been cast with the module
        inv_freq = self.inv_freq if self.inv_freq.dtype == torch.float32 else self._compute_inv_freq(device=device)
        t = torch.arange(seqlen, device=device, dtype=torch.float32)
        freqs = torch.outer(t, inv_freq)  # (no einsum: autocast would run it in 16 bits)
        if self.scale is None:
            self._cos_cached, self._sin_cached = torch.cos(freqs).to(dtype), torch.sin(freqs).to(dtype)
            return
        power = (torch.arange(seqlen, dtype=self.scale.dtype, device=self.scale.device) - seqlen // 2) / self.scale_base
        scale = self.scale.to(device=power.device) ** power.unsqueeze(-1)
        # (scaled in fp32, rounded once)
        self._cos_cached, self._sin_cached = (torch.cos(freqs) * scale).to(dtype), (torch.sin(freqs) * scale).to(dtype)
        self._cos_k_cached, self._sin_k_cached = (torch.cos(freqs) / scale).to(dtype), (torch.sin(freqs) / scale).to(dtype)

    def forward(self, qkv: torch.Tensor, kv: Optional[torch.Tensor] = None, seqlen_offset: Union[int, torch.Tensor] = 0,
                max_seqlen: Optional[int] = None, num_heads_q: Optional[int] = None
                ) -> Union[torch.Tensor, Tuple[torch.Tensor, torch.Tensor]]:
        """Rotate *in place*.  Without kv, qkv is (batch, seqlen, 3, nheads, headdim) or -- with num_heads_q -- (batch, seqlen,
        num_heads_q + 2 * num_heads_k, headdim), and is returned.  With kv (batch, seqlen, 2, nheads, headdim), qkv is q
        (batch, seqlen, nheads, headdim), and (q, kv) is returned.  seqlen_offset: an int or a (batch,) tensor; with a tensor pass
        max_seqlen, the length up to which the tables are to be kept."""
        seqlen = qkv.shape[1]
        if max_seqlen is not None:
            self._update_cos_sin_cache(max_seqlen, device=qkv.device, dtype=qkv.dtype)
        elif isinstance(seqlen_offset, int):
            self._update_cos_sin_cache(seqlen + seqlen_offset, device=qkv.device, dtype=qkv.dtype)
        xpos = self.scale is not None
        if kv is None:
            return apply_rotary_emb_qkv_(qkv, self._cos_cached, self._sin_cached, self._cos_k_cached if xpos else None,
                                         self._sin_k_cached if xpos else None, interleaved=self.interleaved,
                                         seqlen_offsets=seqlen_offset, num_heads_q=num_heads_q)
        q = apply_rotary_emb_func(qkv, self._cos_cached, self._sin_cached, interleaved=self.interleaved, inplace=True,
                                  seqlen_offsets=seqlen_offset)
        kv = apply_rotary_emb_kv_(kv, self._cos_k_cached if xpos else self._cos_cached,
                                  self._sin_k_cached if xpos else self._sin_cached, interleaved=self.interleaved,
                                  seqlen_offsets=seqlen_offset)
        return q, kv
