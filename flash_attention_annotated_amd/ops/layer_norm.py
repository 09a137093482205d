"""Dropout fused into the residual add and the LayerNorm / RMSNorm, behind the names of the reference's
`flash_attn/ops/layer_norm.py` (:311-800) and, for the RMS forms, of its `flash_attn/ops/rms_norm.py` (:20-174):

    DropoutAddLayerNormFn, DropoutAddLayerNormParallelResidualFn
    layer_norm, dropout_add_layer_norm, dropout_add_layer_norm_parallel_residual, DropoutAddLayerNorm
    dropout_add_rms_norm, dropout_add_rms_norm_parallel_residual, DropoutAddRMSNorm

Same argument orders, defaults and return conventions.  The RMS forms live in this module, not in `ops.rms_norm`: that module's
surface is pinned without them.  Where the reference calls its `dropout_layer_norm` extension, this module launches the HIP
kernels of csrc/fa_dropout_norm.hip through `flash_attn_2_cuda_C.dropout_norm_fwd` / `dropout_norm_bwd`, wrapped in two
torch.library custom ops with fake implementations, so torch.compile traces the layer.  There is no eager fall-back on a GPU:
without the built library the ops raise.  CPU tensors take the pure-torch oracle of `ops.norm` (layer_norm_ref / rms_norm_ref).

    x = drop(x0 * rowscale * layerscale) [+ drop(x1)] [+ residual]      rounded once to the residual stream's dtype
    z0 = norm(x) * weight0 + bias0,  z1 = norm(x) * weight1 + bias1     (z1: the parallel form with weight1)

The decisions come from a counter hash of (row, column group, stream, seed, offset); (seed, offset) are drawn on the device
from torch's generator, so `torch.manual_seed` reproduces a mask, nothing synchronises and a HIP graph captures the call.  The
backward forms the decisions again from the saved pair: no mask is stored unless return_dropout_mask asks for it (uint8,
1 = kept; all ones where nothing is dropped: p == 0, or dmask1 without x1 -- the reference's convention).  Keep probabilities
sit on an 8-bit grid: an element is kept with probability (floor(255 (1 - p)) + 1) / 256 and scaled by 1 / (1 - p).

With p == 0, a 16-bit x0 in the 16-byte form and a stream that is not rounded (fp32, or no add), the forward is bit-equal to
`ops.triton.layer_norm.layer_norm_fn`: same sums in the same order.

Not built: the subset forms (`dropout_add_layer_norm_subset`, `dropout_add_rms_norm_subset`, `DropoutAddLayerNormSubsetFn`);
the names are absent, importing them fails.  `layer_norm_fn(dropout_p > 0)` still raises: it is not routed here.
"""
from typing import Optional, Tuple

import torch
from torch import Tensor
from torch.nn import init

from .._lib import binding as _binding
from .norm import _DTYPE_CODE, _check_width, _flat, layer_norm_ref, rms_norm_ref

_custom_op = torch.library.custom_op
_register_fake = torch.library.register_fake
_Eight = Tuple[Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor]


# ---- the kernel entries ------------------------------------------------------------------------------------------------------
@_custom_op("flash_attn_amd::_dropout_norm_fwd", mutates_args=(), device_types="cuda")
def _dropout_norm_fwd(x0: Tensor, x1: Optional[Tensor], residual: Optional[Tensor], weight0: Tensor, bias0: Optional[Tensor],
                      weight1: Optional[Tensor], bias1: Optional[Tensor], rowscale: Optional[Tensor], colscale: Optional[Tensor],
                      p_dropout: float, eps: float, residual_in_fp32: bool, is_rms_norm: bool, want_x: bool,
                      return_dmask: bool) -> _Eight:
    """(z0, z1, x, dmask0, dmask1, mu, rsigma, rng_state); an output there is none of is an empty tensor."""
    return _binding().dropout_norm_fwd(x0, x1, residual, weight0, bias0, weight1, bias1, rowscale, colscale, p_dropout, eps,
                                       residual_in_fp32, is_rms_norm, want_x, return_dmask)


def _stream_dtype(x0, residual, residual_in_fp32):
    return residual.dtype if residual is not None else torch.float32 if residual_in_fp32 else x0.dtype


def _own_x(x0, x1, residual, rowscale, colscale, p_dropout, residual_in_fp32, want_x):
    """Whether the stream is a tensor of its own (else it is x0): it differs from x0 in value or dtype, or prenorm wants it."""
    return (want_x or p_dropout > 0.0 or any(t is not None for t in (x1, residual, rowscale, colscale))
            or _stream_dtype(x0, residual, residual_in_fp32) != x0.dtype)


@_register_fake("flash_attn_amd::_dropout_norm_fwd")
def _dropout_norm_fwd_fake(x0, x1, residual, weight0, bias0, weight1, bias1, rowscale, colscale, p_dropout, eps, residual_in_fp32,
                           is_rms_norm, want_x, return_dmask):
    m = x0.shape[0]
    stream = _stream_dtype(x0, residual, residual_in_fp32)
    mask = return_dmask and p_dropout > 0.0
    return (torch.empty_like(x0, memory_format=torch.contiguous_format),
            x0.new_empty(x0.shape if weight1 is not None else (0,)),
            x0.new_empty(x0.shape if _own_x(x0, x1, residual, rowscale, colscale, p_dropout, residual_in_fp32, want_x) else (0,),
                         dtype=stream),
            x0.new_empty(x0.shape if mask else (0,), dtype=torch.uint8),
            x0.new_empty(x0.shape if mask and x1 is not None else (0,), dtype=torch.uint8),
            x0.new_empty((0 if is_rms_norm else m,), dtype=torch.float32), x0.new_empty((m,), dtype=torch.float32),
            x0.new_empty((2,), dtype=torch.int64))


@_custom_op("flash_attn_amd::_dropout_norm_bwd", mutates_args=(), device_types="cuda")
def _dropout_norm_bwd(dz0: Tensor, dz1: Optional[Tensor], dx: Optional[Tensor], x: Tensor, x0: Optional[Tensor],
                      mu: Optional[Tensor], rsigma: Tensor, weight0: Tensor, weight1: Optional[Tensor], rowscale: Optional[Tensor],
                      colscale: Optional[Tensor], rng_state: Tensor, p_dropout: float, has_x1: bool, has_residual: bool,
                      has_bias: bool, is_rms_norm: bool, x0_dtype: int) -> _Eight:
    """(dx0, dx1, dresidual, dw0, db0, dw1, db1, dcolscale); an output there is none of is an empty tensor."""
    return _binding().dropout_norm_bwd(dz0, dz1, dx, x, x0, mu, rsigma, weight0, weight1, rowscale, colscale, rng_state, p_dropout,
                                       has_x1, has_residual, has_bias, is_rms_norm, x0_dtype)


def _dtype_of_code(code):
    return next(t for t, c in _DTYPE_CODE.items() if c == code)


def _own_dresidual(has_residual, x, x0_dtype, rowscale, colscale, p_dropout):
    """Whether the gradient of the residual is a tensor of its own (else dx0 serves): the reference's rule."""
    return has_residual and (p_dropout > 0.0 or rowscale is not None or colscale is not None or x.dtype != _dtype_of_code(x0_dtype))


@_register_fake("flash_attn_amd::_dropout_norm_bwd")
def _dropout_norm_bwd_fake(dz0, dz1, dx, x, x0, mu, rsigma, weight0, weight1, rowscale, colscale, rng_state, p_dropout, has_x1,
                           has_residual, has_bias, is_rms_norm, x0_dtype):
    in_dtype = _dtype_of_code(x0_dtype)
    none = lambda like: like.new_empty((0,))  # noqa: E731
    two = weight1 is not None
    return (x.new_empty(x.shape, dtype=in_dtype), x.new_empty(x.shape if has_x1 else (0,), dtype=in_dtype),
            x.new_empty(x.shape if _own_dresidual(has_residual, x, x0_dtype, rowscale, colscale, p_dropout) else (0,)),
            torch.empty_like(weight0), torch.empty_like(weight0) if has_bias else none(weight0),
            torch.empty_like(weight0) if two else none(weight0), torch.empty_like(weight0) if two and has_bias else none(weight0),
            torch.empty_like(colscale) if colscale is not None else none(weight0))


# ---- host side of a launch ---------------------------------------------------------------------------------------------------
def _grad_rows(t):
    """An incoming gradient as (M, N) rows.  One of no rows can arrive expanded, with strides of zero that nothing reads."""
    t = _flat(t)
    return t if t is None or t.numel() else t.new_empty(t.shape)


def _vector(t):
    return t.contiguous() if t is not None else None


def _check_call(x0, x1, residual, p_dropout):
    for name, t in (("x1", x1), ("residual", residual)):
        if t is not None and t.shape != x0.shape:
            raise ValueError(f"{name} must have the shape of x0")
    if not 0.0 <= p_dropout < 1.0:
        raise ValueError("dropout_p must be in [0, 1)")


def _forward_args(x0, x1, residual, weight0, bias0, weight1, bias1, rowscale, colscale, p_dropout, eps, residual_in_fp32, rms,
                  want_x, return_dmask):
    """The arguments of the forward op (and of its plan) for tensors in the caller's shapes."""
    _check_call(x0, x1, residual, p_dropout)
    _check_width(x0)
    return (_flat(x0), _flat(x1), _flat(residual), _vector(weight0), _vector(bias0), _vector(weight1), _vector(bias1),
            rowscale.reshape(-1).contiguous() if rowscale is not None else None, _vector(colscale), float(p_dropout), float(eps),
            bool(residual_in_fp32), bool(rms), bool(want_x), bool(return_dmask))


def _plan_forward(*args):
    """The form the forward takes with the arguments of _forward_args, launching nothing: fa_dropout_norm_plan as a dict."""
    return _binding().dropout_norm_fwd_plan(*_forward_args(*args))


def _plan_backward(dz0, dz1, dx, x, x0, mu, rsigma, weight0, weight1, rowscale, colscale, rng_state, p_dropout, has_x1,
                   has_residual, has_bias, rms, in_dtype):
    """The form the backward takes with these (M, N) tensors, launching nothing."""
    return _binding().dropout_norm_bwd_plan(dz0, dz1, dx, x, x0, mu, rsigma, weight0, weight1, rowscale, colscale, rng_state,
                                            float(p_dropout), has_x1, has_residual, has_bias, rms, _DTYPE_CODE[in_dtype])


def _ones_mask(x0):
    return torch.ones(x0.shape, dtype=torch.uint8, device=x0.device)


def _cpu_forward(rms, x0, x1, residual, weight0, bias0, weight1, bias1, rowscale, colscale, p_dropout, eps, residual_in_fp32,
                 prenorm):
    """The oracle on CPU tensors, differentiable by torch itself: (z0, z1, x, dmask0, dmask1), x None without prenorm, masks
    None where nothing is dropped.  colscale enters by pre-multiplying x0."""
    _check_call(x0, x1, residual, p_dropout)
    ref = rms_norm_ref if rms else layer_norm_ref
    mask0 = mask1 = None
    if p_dropout > 0.0:
        mask0 = torch.rand(x0.shape, device=x0.device) >= p_dropout
        mask1 = torch.rand(x0.shape, device=x0.device) >= p_dropout if x1 is not None else None
    h0 = (x0 * colscale).to(x0.dtype) if colscale is not None else x0
    out = ref(h0, weight0, bias0, residual=residual, x1=x1, weight1=weight1, bias1=bias1, eps=eps, dropout_p=p_dropout,
              rowscale=rowscale, prenorm=prenorm, dropout_mask=mask0, dropout_mask1=mask1)
    out = out if isinstance(out, tuple) else (out,)
    x = out[-1].to(_stream_dtype(x0, residual, residual_in_fp32)) if prenorm else None
    zs = out[:-1] if prenorm else out
    to_u8 = lambda m: m.to(torch.uint8) if m is not None else None  # noqa: E731
    return zs[0], zs[1] if len(zs) > 1 else None, x, to_u8(mask0), to_u8(mask1)


def _returns(zs, x, prenorm, return_dmask, masks):
    ret = tuple(zs) + ((x,) if prenorm else ()) + (tuple(masks) if return_dmask else ())
    return ret if len(ret) > 1 else ret[0]


# ---- autograd ------------------------------------------------------------------------------------------------------------------
class DropoutAddLayerNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x0, residual, gamma, beta, rowscale, colscale, dropout_p, epsilon, residual_in_fp32=False, prenorm=False,
                is_rms_norm=False, return_dmask=False):
        args = _forward_args(x0, None, residual, gamma, beta, None, None, rowscale, colscale, dropout_p, epsilon, residual_in_fp32,
                             is_rms_norm, prenorm, return_dmask)
        z, _, x, dmask, _, mu, rsigma, rng_state = _dropout_norm_fwd(*args)
        x0mat, _, _, gamma, _, _, _, rowscale, colscale = args[:9]
        stream = x if _own_x(x0mat, None, args[2], rowscale, colscale, dropout_p, residual_in_fp32, prenorm) else x0mat
        ctx.save_for_backward(stream, x0mat if colscale is not None else None, gamma, None if is_rms_norm else mu, rsigma, rowscale,
                              colscale, rng_state)
        ctx.call = (x0.shape, x0.dtype, float(dropout_p), prenorm, residual is not None, beta is not None, is_rms_norm)
        masks = ()
        if return_dmask:
            masks = (dmask.view(x0.shape) if dropout_p > 0.0 else _ones_mask(x0),)
            ctx.mark_non_differentiable(*masks)
        return _returns((z.view(x0.shape),), stream.view(x0.shape), prenorm, return_dmask, masks)

    @staticmethod
    def backward(ctx, dz, *args):
        shape, in_dtype, p, prenorm, has_residual, has_beta, rms = ctx.call
        x, x0, gamma, mu, rsigma, rowscale, colscale, rng_state = ctx.saved_tensors
        dx0, _, dres, dgamma, dbeta, _, _, dcolscale = _dropout_norm_bwd(
            _grad_rows(dz), None, _grad_rows(args[0]) if prenorm else None, x, x0, mu, rsigma, gamma, None, rowscale, colscale, rng_state, p,
            False, has_residual, has_beta, rms, _DTYPE_CODE[in_dtype])
        dx0 = dx0.view(shape)
        if not has_residual:
            dres = None
        elif not _own_dresidual(True, x, _DTYPE_CODE[in_dtype], rowscale, colscale, p):
            dres = dx0
        else:
            dres = dres.view(shape)
        return (dx0, dres, dgamma, dbeta if has_beta else None, None, dcolscale if colscale is not None else None, None, None, None,
                None, None, None)


class DropoutAddLayerNormParallelResidualFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x0, x1, residual, gamma0, beta0, gamma1, beta1, dropout_p, epsilon, residual_in_fp32=False, prenorm=False,
                is_rms_norm=False, return_dmask=False):
        args = _forward_args(x0, x1, residual, gamma0, beta0, gamma1, beta1, None, None, dropout_p, epsilon, residual_in_fp32,
                             is_rms_norm, prenorm, return_dmask)
        z0, z1, x, dmask0, dmask1, mu, rsigma, rng_state = _dropout_norm_fwd(*args)
        x0mat, gamma0, gamma1 = args[0], args[3], args[5]
        stream = x if _own_x(x0mat, args[1], args[2], None, None, dropout_p, residual_in_fp32, prenorm) else x0mat
        ctx.save_for_backward(stream, gamma0, gamma1, None if is_rms_norm else mu, rsigma, rng_state)
        ctx.call = (x0.shape, x0.dtype, float(dropout_p), prenorm, x1 is not None, residual is not None, beta0 is not None, is_rms_norm)
        masks = ()
        if return_dmask:
            masks = (dmask0.view(x0.shape) if dropout_p > 0.0 else _ones_mask(x0),
                     dmask1.view(x0.shape) if dropout_p > 0.0 and x1 is not None else _ones_mask(x0))
            ctx.mark_non_differentiable(*masks)
        return _returns((z0.view(x0.shape), z1.view(x0.shape) if gamma1 is not None else None), stream.view(x0.shape), prenorm,
                        return_dmask, masks)

    @staticmethod
    def backward(ctx, dz0, dz1, *args):
        shape, in_dtype, p, prenorm, has_x1, has_residual, has_beta, rms = ctx.call
        x, gamma0, gamma1, mu, rsigma, rng_state = ctx.saved_tensors
        two = gamma1 is not None
        dx0, dx1, dres, dgamma0, dbeta0, dgamma1, dbeta1, _ = _dropout_norm_bwd(
            _grad_rows(dz0), _grad_rows(dz1) if two else None, _grad_rows(args[0]) if prenorm else None, x, None, mu, rsigma, gamma0, gamma1, None,
            None, rng_state, p, has_x1, has_residual, has_beta, rms, _DTYPE_CODE[in_dtype])
        dx0 = dx0.view(shape)
        if not has_residual:
            dres = None
        elif not _own_dresidual(True, x, _DTYPE_CODE[in_dtype], None, None, p):
            dres = dx0
        else:
            dres = dres.view(shape)
        return (dx0, dx1.view(shape) if has_x1 else None, dres, dgamma0, dbeta0 if has_beta else None, dgamma1 if two else None,
                dbeta1 if two and has_beta else None, None, None, None, None, None, None)


def _apply(rms, x0, residual, weight, bias, rowscale, layerscale, dropout_p, epsilon, residual_in_fp32, prenorm, return_dropout_mask):
    if x0.is_cuda:
        return DropoutAddLayerNormFn.apply(x0, residual, weight, bias, rowscale, layerscale, dropout_p, epsilon, residual_in_fp32,
                                           prenorm, rms, return_dropout_mask)
    z, _, x, dmask, _ = _cpu_forward(rms, x0, None, residual, weight, bias, None, None, rowscale, layerscale, dropout_p, epsilon,
                                     residual_in_fp32, prenorm)
    return _returns((z,), x, prenorm, return_dropout_mask, (dmask if dmask is not None else _ones_mask(x0),))


def _apply_parallel(rms, x0, x1, residual, weight0, bias0, weight1, bias1, dropout_p, epsilon, prenorm, residual_in_fp32,
                    return_dropout_mask):
    if x0.is_cuda:
        return DropoutAddLayerNormParallelResidualFn.apply(x0, x1, residual, weight0, bias0, weight1, bias1, dropout_p, epsilon,
                                                           residual_in_fp32, prenorm, rms, return_dropout_mask)
    z0, z1, x, dmask0, dmask1 = _cpu_forward(rms, x0, x1, residual, weight0, bias0, weight1, bias1, None, None, dropout_p, epsilon,
                                             residual_in_fp32, prenorm)
    masks = tuple(m if m is not None else _ones_mask(x0) for m in (dmask0, dmask1))
    return _returns((z0, z1), x, prenorm, return_dropout_mask, masks)


# ---- the reference's functions -----------------------------------------------------------------------------------------------
def layer_norm(x, weight, bias, epsilon):
    return _apply(False, x, None, weight, bias, None, None, 0.0, epsilon, False, False, False)


def dropout_add_layer_norm(x0, residual, weight, bias, dropout_p, epsilon, rowscale=None, layerscale=None, prenorm=False,
                           residual_in_fp32=False, return_dropout_mask=False):
    """LayerNorm(drop(x0 * rowscale * layerscale) + residual) * weight + bias.  Returns z, (z, x) with prenorm, and the uint8
    mask last with return_dropout_mask.  residual_in_fp32 only has an effect if residual is None; otherwise the stream is in
    residual.dtype."""
    return _apply(False, x0, residual, weight, bias, rowscale, layerscale, dropout_p, epsilon, residual_in_fp32, prenorm,
                  return_dropout_mask)


def dropout_add_layer_norm_parallel_residual(x0, x1, residual, weight0, bias0, weight1, bias1, dropout_p, epsilon, prenorm=False,
                                             residual_in_fp32=False, return_dropout_mask=False):
    """x = drop(x0) + drop(x1) + residual; (z0, z1) = the two norms of x (z1 None without weight1).  Returns (z0, z1), then x
    with prenorm, then (dmask0, dmask1) with return_dropout_mask."""
    return _apply_parallel(False, x0, x1, residual, weight0, bias0, weight1, bias1, dropout_p, epsilon, prenorm, residual_in_fp32,
                           return_dropout_mask)


def dropout_add_rms_norm(x0, residual, weight, bias, dropout_p, epsilon, rowscale=None, layerscale=None, prenorm=False,
                         residual_in_fp32=False, return_dropout_mask=False):
    """dropout_add_layer_norm with RMSNorm."""
    return _apply(True, x0, residual, weight, bias, rowscale, layerscale, dropout_p, epsilon, residual_in_fp32, prenorm,
                  return_dropout_mask)


def dropout_add_rms_norm_parallel_residual(x0, x1, residual, weight0, bias0, weight1, bias1, dropout_p, epsilon, prenorm=False,
                                           residual_in_fp32=False, return_dropout_mask=False):
    """dropout_add_layer_norm_parallel_residual with RMSNorm."""
    return _apply_parallel(True, x0, x1, residual, weight0, bias0, weight1, bias1, dropout_p, epsilon, prenorm, residual_in_fp32,
                           return_dropout_mask)


class DropoutAddLayerNorm(torch.nn.Module):
    def __init__(self, hidden_size, prenorm=False, p=0.0, eps=1e-5, residual_in_fp32=False, device=None, dtype=None):
        factory_kwargs = {"device": device, "dtype": dtype}
        super().__init__()
        self.prenorm = prenorm
        self.p = p
        self.eps = eps
        self.residual_in_fp32 = residual_in_fp32
        self.weight = torch.nn.Parameter(torch.empty(hidden_size, **factory_kwargs))
        self.bias = torch.nn.Parameter(torch.empty(hidden_size, **factory_kwargs))
        self.reset_parameters()

    def reset_parameters(self):
        init.ones_(self.weight)
        init.zeros_(self.bias)

    def forward(self, x0, residual=None):
        return dropout_add_layer_norm(x0, residual, self.weight, self.bias, self.p if self.training else 0.0, self.eps,
                                      prenorm=self.prenorm, residual_in_fp32=self.residual_in_fp32)


class DropoutAddRMSNorm(torch.nn.Module):
    def __init__(self, hidden_size, prenorm=False, p=0.0, eps=1e-5, residual_in_fp32=False, device=None, dtype=None):
        factory_kwargs = {"device": device, "dtype": dtype}
        super().__init__()
        self.prenorm = prenorm
        self.p = p
        self.eps = eps
        self.residual_in_fp32 = residual_in_fp32
        self.weight = torch.nn.Parameter(torch.empty(hidden_size, **factory_kwargs))
        self.register_parameter("bias", None)
        self.reset_parameters()

    def reset_parameters(self):
        init.ones_(self.weight)

    def forward(self, x0, residual=None):
        return dropout_add_rms_norm(x0, residual, self.weight, None, self.p if self.training else 0.0, self.eps,
                                    prenorm=self.prenorm, residual_in_fp32=self.residual_in_fp32)
