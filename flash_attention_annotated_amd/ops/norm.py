"""Fused residual-add + LayerNorm / RMSNorm behind the names of the reference's `flash_attn/ops/triton/layer_norm.py`:

    layer_norm_ref, rms_norm_ref          reference :44-160   (pure torch: the CPU oracle)
    LayerNormFn, layer_norm_fn, rms_norm_fn          :846-1090
    RMSNorm                                          :1093-1126
    LayerNormLinearFn, layer_norm_linear_fn          :1129-1252

Same argument orders and defaults.  Where the reference launches its Triton kernels, this module launches the HIP kernels of
csrc/fa_norm.hip through `flash_attn_2_cuda_C.norm_fwd` / `norm_bwd`, wrapped in two torch.library custom ops with fake
implementations, so torch.compile traces the layer.  There is no eager fall-back: without the built library the ops raise.

Not built: dropout (dropout_p > 0) and the parallel form (x1 / weight1 / bias1); they raise NotImplementedError.
"""
import collections
from typing import Optional, Tuple

import torch
import torch.nn.functional as F
from torch import Tensor

from .._lib import FA_DTYPE_BF16, FA_DTYPE_FP16, FA_DTYPE_FP32
from .._lib import binding as _binding

_custom_op = torch.library.custom_op
_register_fake = torch.library.register_fake
_DTYPE_CODE = {torch.float16: FA_DTYPE_FP16, torch.bfloat16: FA_DTYPE_BF16, torch.float32: FA_DTYPE_FP32}
MAX_ROW_BYTES = 65536


# ---- the kernel entries ------------------------------------------------------------------------------------------------------
@_custom_op("flash_attn_amd::_norm_fwd", mutates_args=("out", "residual_out"), device_types="cuda")
def _norm_fwd(x: Tensor, weight: Tensor, bias: Optional[Tensor], residual: Optional[Tensor], rowscale: Optional[Tensor],
              out: Tensor, residual_out: Optional[Tensor], eps: float, zero_centered_weight: bool,
              is_rms_norm: bool) -> Tuple[Tensor, Tensor]:
    """Writes out and residual_out; returns (mean, rstd), mean empty with is_rms_norm."""
    return _binding().norm_fwd(x, weight, bias, residual, rowscale, out, residual_out, eps, zero_centered_weight, is_rms_norm)


@_register_fake("flash_attn_amd::_norm_fwd")
def _norm_fwd_fake(x, weight, bias, residual, rowscale, out, residual_out, eps, zero_centered_weight, is_rms_norm):
    m = x.shape[0]
    return x.new_empty((0 if is_rms_norm else m,), dtype=torch.float32), x.new_empty((m,), dtype=torch.float32)


@_custom_op("flash_attn_amd::_norm_bwd", mutates_args=(), device_types="cuda")
def _norm_bwd(dy: Tensor, x: Tensor, weight: Tensor, bias: Optional[Tensor], mean: Optional[Tensor], rstd: Tensor,
              dresidual: Optional[Tensor], rowscale: Optional[Tensor], has_residual: bool, zero_centered_weight: bool,
              is_rms_norm: bool, dx_dtype: int, recompute_output: bool) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor]:
    """(dx, dw, db, dresidual_in, y); an output there is none of is an empty tensor."""
    return _binding().norm_bwd(dy, x, weight, bias, mean, rstd, dresidual, rowscale, has_residual, zero_centered_weight,
                               is_rms_norm, dx_dtype, recompute_output)


def _dtype_of_code(code):
    return next(t for t, c in _DTYPE_CODE.items() if c == code)


def _own_dresidual(has_residual, x, dx_dtype, rowscale):
    """Whether the gradient of the residual is a tensor of its own (else dx serves): the reference's rule, :761-766."""
    return has_residual and (_dtype_of_code(dx_dtype) != x.dtype or rowscale is not None)


@_register_fake("flash_attn_amd::_norm_bwd")
def _norm_bwd_fake(dy, x, weight, bias, mean, rstd, dresidual, rowscale, has_residual, zero_centered_weight, is_rms_norm,
                   dx_dtype, recompute_output):
    none = lambda: x.new_empty((0,))  # noqa: E731
    return (x.new_empty(x.shape, dtype=_dtype_of_code(dx_dtype)), torch.empty_like(weight),
            torch.empty_like(bias) if bias is not None else none(),
            x.new_empty(x.shape) if _own_dresidual(has_residual, x, dx_dtype, rowscale) else none(),
            dy.new_empty(x.shape) if recompute_output else none())


# ---- host side of a launch ---------------------------------------------------------------------------------------------------
def _refuse(dropout_p, x1, weight1, bias1):
    """The forms that are not built, named; before anything touches a device."""
    if dropout_p > 0.0:
        raise NotImplementedError("dropout_p > 0 is not built: the fused norm has no dropout")
    for name, value in (("x1", x1), ("weight1", weight1), ("bias1", bias1)):
        if value is not None:
            raise NotImplementedError(f"{name} is not built: the fused norm has no parallel (x1 / weight1 / bias1) form")


def _check_width(x):
    if x.shape[-1] * x.element_size() > MAX_ROW_BYTES:
        raise RuntimeError("This layer norm doesn't support feature dim >= 64KB.")


def _flat(t, written=False):
    """(..., N) as the (M, N) rows the kernels take, unit last stride.  What is read may be copied to get there; a tensor the
    caller gave to be written must collapse as a view (view raises where it does not), or the launch would fill a temporary."""
    if t is None:
        return None
    if written:
        return t.view(-1, t.shape[-1])
    t = t.reshape(-1, t.shape[-1])
    return t if t.stride(-1) == 1 else t.contiguous()


def _forward_operands(x, residual, rowscale, out_dtype, stream_dtype, out, residual_out):
    """(out, residual_out) of a forward launch: y and the stream are allocated here, not in the custom op, which neither returns
    an argument nor sees an output that aliases an input.  residual_out stays None where the stream is x itself."""
    _check_width(x)
    if residual is not None:
        stream_dtype = residual.dtype
    elif stream_dtype is None:
        stream_dtype = x.dtype
    if out is None:
        out = torch.empty_like(x, dtype=out_dtype or x.dtype)
    if residual_out is not None:
        if residual_out.dtype != stream_dtype:
            raise ValueError(f"residual_out must be of the residual stream's dtype, {stream_dtype}")
    elif residual is not None or stream_dtype != x.dtype or rowscale is not None:
        residual_out = torch.empty_like(x, dtype=stream_dtype)
    return out, residual_out


def _launch_forward(x, weight, bias, eps, residual=None, rowscale=None, out_dtype=None, stream_dtype=None,
                    zero_centered_weight=False, is_rms_norm=False, out=None, residual_out=None):
    """x (M, N) -> (y, stream, mean, rstd); mean is None for RMS.  `stream` is the new residual stream, x * rowscale + residual
    in stream_dtype (the residual's dtype where there is one): a tensor of its own when that differs from x in value or dtype,
    or when the caller gave residual_out; otherwise x itself."""
    out, residual_out = _forward_operands(x, residual, rowscale, out_dtype, stream_dtype, out, residual_out)
    mean, rstd = _norm_fwd(x, weight, bias, residual, rowscale, out, residual_out, eps, zero_centered_weight, is_rms_norm)
    return out, x if residual_out is None else residual_out, None if is_rms_norm else mean, rstd


def _plan_forward(x, weight, bias, eps, residual=None, rowscale=None, out_dtype=None, stream_dtype=None,
                  zero_centered_weight=False, is_rms_norm=False, out=None, residual_out=None):
    """The form _launch_forward takes with these tensors, launching nothing: fa_norm_plan (include/fa_norm.h) as a dict.  Outputs
    not given are allocated as the launch allocates them: the plan depends on the alignment of every operand."""
    out, residual_out = _forward_operands(x, residual, rowscale, out_dtype, stream_dtype, out, residual_out)
    return _binding().norm_fwd_plan(x, weight, bias, residual, rowscale, out, residual_out, eps, zero_centered_weight, is_rms_norm)


def _launch_backward(dy, stream, weight, bias, mean, rstd, dresidual=None, rowscale=None, has_residual=False,
                     zero_centered_weight=False, is_rms_norm=False, dx_dtype=None, recompute_output=False):
    """stream: what _launch_forward returned as such.  -> (dx, dw, db, dresidual_in, y): dx in dx_dtype (the forward's x), db
    None without a bias, dresidual_in None without a residual and dx itself where the two would be equal, y None unless asked."""
    _check_width(stream)
    code = _DTYPE_CODE[dx_dtype or stream.dtype]
    dx, dw, db, dresidual_in, y = _norm_bwd(_flat(dy), stream, weight, bias, mean, rstd, _flat(dresidual), rowscale, has_residual,
                                            zero_centered_weight, is_rms_norm, code, recompute_output)
    if not has_residual:
        dresidual_in = None
    elif not _own_dresidual(has_residual, stream, code, rowscale):
        dresidual_in = dx
    return dx, dw, db if bias is not None else None, dresidual_in, y if recompute_output else None


def _plan_backward(dy, stream, weight, bias, mean, rstd, dresidual=None, rowscale=None, has_residual=False,
                   zero_centered_weight=False, is_rms_norm=False, dx_dtype=None, recompute_output=False):
    """The form _launch_backward takes with these tensors, launching nothing: fa_norm_plan as a dict (grid_y: the column slabs)."""
    _check_width(stream)
    return _binding().norm_bwd_plan(_flat(dy), stream, weight, bias, mean, rstd, _flat(dresidual), rowscale, has_residual,
                                    zero_centered_weight, is_rms_norm, _DTYPE_CODE[dx_dtype or stream.dtype], recompute_output)


# ---- pure torch: the oracle ---------------------------------------------------------------------------------------------------
def _dropped(x, dropout_p, mask):
    if mask is not None:
        return x.masked_fill(~mask, 0.0) / (1.0 - dropout_p)
    return F.dropout(x, p=dropout_p)


def _norm_ref(rms, x, weight, bias, residual, x1, weight1, bias1, eps, dropout_p, rowscale, prenorm, zero_centered_weight,
              dropout_mask, dropout_mask1, upcast):
    dtype = x.dtype
    if upcast:
        x, weight = x.float(), weight.float()
        bias, residual, x1, weight1, bias1 = (t.float() if t is not None else None for t in (bias, residual, x1, weight1, bias1))
    if zero_centered_weight:
        weight = weight + 1.0
        weight1 = weight1 + 1.0 if weight1 is not None else None
    if x1 is not None:
        assert rowscale is None, "rowscale is not supported with parallel LayerNorm"
    if rowscale is not None:
        x = x * rowscale[..., None]
    if dropout_p > 0.0:
        x = _dropped(x, dropout_p, dropout_mask)
        if x1 is not None:
            x1 = _dropped(x1, dropout_p, dropout_mask1)
    if x1 is not None:
        x = x + x1
    if residual is not None:
        x = (x + residual).to(x.dtype)
    if rms:
        rstd = 1 / torch.sqrt((x.square()).mean(dim=-1, keepdim=True) + eps)

        def norm(w, b):
            return ((x * rstd * w) + b if b is not None else (x * rstd * w)).to(dtype)
    else:
        def norm(w, b):
            return F.layer_norm(x.to(w.dtype), x.shape[-1:], weight=w, bias=b, eps=eps).to(dtype)
    outs = (norm(weight, bias),) if weight1 is None else (norm(weight, bias), norm(weight1, bias1))
    if prenorm:
        return (*outs, x)
    return outs[0] if len(outs) == 1 else outs


def layer_norm_ref(x, weight, bias, residual=None, x1=None, weight1=None, bias1=None, eps=1e-6, dropout_p=0.0, rowscale=None,
                   prenorm=False, zero_centered_weight=False, dropout_mask=None, dropout_mask1=None, upcast=False):
    """LayerNorm((x * rowscale, dropped) + x1 + residual) in torch, in x's and the weight's dtypes, or in fp32 with upcast."""
    return _norm_ref(False, x, weight, bias, residual, x1, weight1, bias1, eps, dropout_p, rowscale, prenorm, zero_centered_weight,
                     dropout_mask, dropout_mask1, upcast)


def rms_norm_ref(x, weight, bias, residual=None, x1=None, weight1=None, bias1=None, eps=1e-6, dropout_p=0.0, rowscale=None,
                 prenorm=False, zero_centered_weight=False, dropout_mask=None, dropout_mask1=None, upcast=False):
    """RMSNorm of the same sum."""
    return _norm_ref(True, x, weight, bias, residual, x1, weight1, bias1, eps, dropout_p, rowscale, prenorm, zero_centered_weight,
                     dropout_mask, dropout_mask1, upcast)


# ---- autograd ------------------------------------------------------------------------------------------------------------------
# what a backward needs to know of its forward, beside the saved tensors (stream, weight, bias, rowscale, mean, rstd)
_Call = collections.namedtuple("_Call", "shape in_dtype rms zero_centered has_residual prenorm")


def _forward(x, weight, bias, residual, rowscale, eps, residual_in_fp32, zero_centered, rms, prenorm, out_dtype=None, out=None,
             residual_out=None):
    """The forward of both autograd functions: flatten, launch.  -> (y, stream) in x's shape, the tensors to save, the _Call."""
    if residual is not None and residual.shape != x.shape:
        raise ValueError("residual must have the shape of x")
    call = _Call(x.shape, x.dtype, rms, zero_centered, residual is not None, prenorm)
    weight = weight.contiguous()
    bias = bias.contiguous() if bias is not None else None
    rowscale = rowscale.reshape(-1).contiguous() if rowscale is not None else None
    y, stream, mean, rstd = _launch_forward(
        _flat(x), weight, bias, eps, _flat(residual), rowscale, out_dtype, torch.float32 if residual_in_fp32 else None, zero_centered,
        rms, _flat(out, written=True), _flat(residual_out, written=True))
    return y.view(call.shape), stream.view(call.shape), (stream, weight, bias, rowscale, mean, rstd), call


def _backward(call, saved, dy, dstream, recompute_output=False):
    """-> (dx, dweight, dbias, dresidual) in the forward's shapes, and y (M, N) where asked for."""
    stream, weight, bias, rowscale, mean, rstd = saved
    dx, dw, db, dres, y = _launch_backward(dy, stream, weight, bias, mean, rstd, dstream if call.prenorm else None, rowscale,
                                           call.has_residual, call.zero_centered, call.rms, call.in_dtype, recompute_output)
    return dx.view(call.shape), dw, db, dres.view(call.shape) if dres is not None else None, y


class LayerNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, residual=None, x1=None, weight1=None, bias1=None, eps=1e-6, dropout_p=0.0, rowscale=None,
                prenorm=False, residual_in_fp32=False, zero_centered_weight=False, is_rms_norm=False, return_dropout_mask=False,
                out_dtype=None, out=None, residual_out=None):
        _refuse(dropout_p, x1, weight1, bias1)
        y, stream, saved, ctx.call = _forward(x, weight, bias, residual, rowscale, eps, residual_in_fp32, zero_centered_weight,
                                              is_rms_norm, prenorm, out_dtype, out, residual_out)
        ctx.save_for_backward(*saved)
        ret = (y, stream) if prenorm else (y,)
        if return_dropout_mask:  # (no dropout: two None where the masks would be)
            ret += (None, None)
        return ret if len(ret) > 1 else y

    @staticmethod
    def backward(ctx, dy, *more):
        grads = _backward(ctx.call, ctx.saved_tensors, dy, more[0] if ctx.call.prenorm else None)[:4]
        return grads + (None,) * 14  # x, weight, bias, residual; nothing for the other fourteen arguments


def layer_norm_fn(x, weight, bias, residual=None, x1=None, weight1=None, bias1=None, eps=1e-6, dropout_p=0.0, rowscale=None,
                  prenorm=False, residual_in_fp32=False, zero_centered_weight=False, is_rms_norm=False, return_dropout_mask=False,
                  out_dtype=None, out=None, residual_out=None):
    """y = norm(x * rowscale + residual) * weight + bias over the last dim, in one pass over the hidden state.

    x: (..., N) in bf16 / fp16 / fp32, any row stride; weight, bias: (N) in any of the three; residual: of x's shape, in x's
    dtype or fp32.  prenorm: also return the sum (the new residual stream), in the residual's dtype -- fp32 with
    residual_in_fp32 where no residual is given.  out / residual_out: tensors to write into (residual_out may be residual).
    Returns y, or (y, residual_out) with prenorm; with return_dropout_mask two None follow.  dropout_p > 0 and x1 / weight1 /
    bias1 raise NotImplementedError.
    """
    return LayerNormFn.apply(x, weight, bias, residual, x1, weight1, bias1, eps, dropout_p, rowscale, prenorm, residual_in_fp32,
                             zero_centered_weight, is_rms_norm, return_dropout_mask, out_dtype, out, residual_out)


def rms_norm_fn(x, weight, bias, residual=None, x1=None, weight1=None, bias1=None, eps=1e-6, dropout_p=0.0, rowscale=None,
                prenorm=False, residual_in_fp32=False, zero_centered_weight=False, return_dropout_mask=False, out_dtype=None,
                out=None, residual_out=None):
    """layer_norm_fn with is_rms_norm=True."""
    return LayerNormFn.apply(x, weight, bias, residual, x1, weight1, bias1, eps, dropout_p, rowscale, prenorm, residual_in_fp32,
                             zero_centered_weight, True, return_dropout_mask, out_dtype, out, residual_out)


class RMSNorm(torch.nn.Module):
    """weight * x / rms(x) as a module: one parameter, `weight` (ones; zeros where it is stored minus one), and a `bias` that is
    always None.  dropout_p is kept for the signature; training with it set raises, as rms_norm_fn does."""

    def __init__(self, hidden_size, eps=1e-5, dropout_p=0.0, zero_centered_weight=False, device=None, dtype=None):
        super().__init__()
        self.eps, self.dropout_p, self.zero_centered_weight = eps, float(dropout_p), zero_centered_weight
        fill = torch.zeros if zero_centered_weight else torch.ones
        self.weight = torch.nn.Parameter(fill(hidden_size, device=device, dtype=dtype))
        self.register_parameter("bias", None)

    def reset_parameters(self):
        with torch.no_grad():
            self.weight.fill_(0.0 if self.zero_centered_weight else 1.0)

    def forward(self, x, residual=None, prenorm=False, residual_in_fp32=False):
        return rms_norm_fn(x, self.weight, None, residual=residual, eps=self.eps, dropout_p=self.dropout_p if self.training else 0.0,
                           prenorm=prenorm, residual_in_fp32=residual_in_fp32, zero_centered_weight=self.zero_centered_weight)


class LayerNormLinearFn(torch.autograd.Function):
    """linear(norm(x + residual)).  The normalised rows are not saved: the backward launch writes them again beside dx.  Under
    autocast the norm writes the autocast dtype and the product runs in it; otherwise in x's dtype."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda")
    def forward(ctx, x, norm_weight, norm_bias, linear_weight, linear_bias, residual=None, eps=1e-6, prenorm=False,
                residual_in_fp32=False, is_rms_norm=False):
        amp = torch.get_autocast_dtype("cuda") if torch.is_autocast_enabled() else None
        y, stream, saved, ctx.call = _forward(x, norm_weight, norm_bias, residual, None, eps, residual_in_fp32, False, is_rms_norm,
                                              prenorm, out_dtype=amp)
        proj = linear_weight.to(y.dtype)
        ctx.has_linear_bias = linear_bias is not None
        ctx.save_for_backward(proj, *saved)
        out = F.linear(y, proj, linear_bias.to(y.dtype) if ctx.has_linear_bias else None)
        return (out, stream) if prenorm else out

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, dout, *more):
        proj, *saved = ctx.saved_tensors
        g = dout.reshape(-1, dout.shape[-1])
        dx, dw, db, dres, y = _backward(ctx.call, saved, g @ proj, more[0] if ctx.call.prenorm else None, recompute_output=True)
        return dx, dw, db, g.t() @ y, g.sum(0) if ctx.has_linear_bias else None, dres, None, None, None, None


def layer_norm_linear_fn(x, norm_weight, norm_bias, linear_weight, linear_bias, residual=None, eps=1e-6, prenorm=False,
                         residual_in_fp32=False, is_rms_norm=False):
    """F.linear(norm(x + residual), linear_weight, linear_bias), or (that, the new residual) with prenorm."""
    return LayerNormLinearFn.apply(x, norm_weight, norm_bias, linear_weight, linear_bias, residual, eps, prenorm, residual_in_fp32,
                                   is_rms_norm)
