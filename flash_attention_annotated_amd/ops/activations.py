"""The fused MLP activations behind the names of the reference's `flash_attn/ops/activations.py`:

    bias_gelu, bias_gelu_back, bias_gelu_impl      reference :15-51
    gelu_fwd, gelu_bwd, fast_gelu_impl                       :56-88
    relu_bwd, sqrelu_fwd, sqrelu_bwd                         :91-104
    swiglu_fwd, swiglu_bwd, swiglu                           :107-135
    act, gated_act                                 every activation of include/fa_act.h, plain (+ bias) and gated
    act_ref, gated_act_ref, act_grad_ref, gated_act_grad_ref   pure torch: the contract of include/fa_act.h, the CPU oracle

Same argument order and defaults.  Where the reference has TorchScript and jiterator functions, this module launches the HIP
kernels of csrc/fa_act.hip through `flash_attn_2_cuda_C.act_fwd` / `act_bwd`, wrapped in torch.library custom ops with fake
implementations, so torch.compile traces forward and backward.  For tensors on the GPU there is no eager fall-back: without the
built library the ops raise.  CPU tensors, which no kernel can take, go to the oracle.

`gated_act(x12, activation)` takes the (..., 2H) output of an fc1 as it is, first half the value and second half the gate (the
order of F.glu and of the reference's GatedMlp): out = x12[..., :H] * act(x12[..., H:]).  Its backward returns one (..., 2H)
gradient whose halves the kernel writes in place: no chunk backward, no cat.

One departure from the reference: relu_bwd passes no gradient at x == 0 (the reference's `x >= 0` does), as autograd of F.relu
has it.
"""
import math
from typing import Optional, Tuple

import torch
import torch.nn.functional as F
from torch import Tensor

from .._lib import binding as _binding

__all__ = ["bias_gelu", "bias_gelu_back", "bias_gelu_impl", "gelu_fwd", "gelu_bwd", "fast_gelu_impl", "relu_bwd", "sqrelu_fwd",
           "sqrelu_bwd", "swiglu_fwd", "swiglu_bwd", "swiglu", "act", "gated_act", "act_ref", "gated_act_ref", "act_grad_ref",
           "gated_act_grad_ref", "ACTIVATIONS"]

_custom_op = torch.library.custom_op
_register_fake = torch.library.register_fake

# the codes of include/fa_act.h by name ("gelu_approx": the reference's name of the tanh form)
GELU_TANH, GELU_ERF, RELU, SQRELU, SILU, SIGMOID, IDENTITY = range(7)
ACTIVATIONS = {"gelu_approx": GELU_TANH, "gelu_tanh": GELU_TANH, "gelu": GELU_ERF, "gelu_erf": GELU_ERF, "relu": RELU,
               "sqrelu": SQRELU, "silu": SILU, "swish": SILU, "sigmoid": SIGMOID, "identity": IDENTITY}


def _code(activation):
    if isinstance(activation, str):
        if activation not in ACTIVATIONS:
            raise ValueError(f"unknown activation {activation!r}: one of {sorted(ACTIVATIONS)}")
        return ACTIVATIONS[activation]
    if not (isinstance(activation, int) and GELU_TANH <= activation <= IDENTITY):
        raise ValueError(f"unknown activation code {activation!r}")
    return activation


# ---- the kernel entries ------------------------------------------------------------------------------------------------------
@_custom_op("flash_attn_amd::_act_fwd", mutates_args=(), device_types="cuda")
def _act_fwd(pre: Tensor, up: Optional[Tensor], bias: Optional[Tensor], activation: int) -> Tensor:
    """out (M, H) = act(pre + bias), or act(pre) * up with `up` (pre is then the gate).  pre / up: (M, H) of any row stride."""
    return _binding().act_fwd(pre, up, bias, activation)


@_register_fake("flash_attn_amd::_act_fwd")
def _act_fwd_fake(pre, up, bias, activation):
    return pre.new_empty(pre.shape)


@_custom_op("flash_attn_amd::_act_bwd", mutates_args=(), device_types="cuda")
def _act_bwd(dout: Tensor, pre: Tensor, up: Optional[Tensor], bias: Optional[Tensor], activation: int, want_dbias: bool,
             recompute_out: bool, packed: bool) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """(dpre, dup, dbias, out) of one pass.  Gated with `packed`: dpre is one (M, 2H) tensor, dup its first half and dgate its
    second, and the dup returned is empty.  dbias / out are empty unless asked for."""
    return _binding().act_bwd(dout, pre, up, bias, activation, want_dbias, recompute_out, packed)


@_register_fake("flash_attn_amd::_act_bwd")
def _act_bwd_fake(dout, pre, up, bias, activation, want_dbias, recompute_out, packed):
    m, h = pre.shape
    none = lambda: pre.new_empty((0,))  # noqa: E731
    return (pre.new_empty((m, 2 * h if packed else h)), pre.new_empty((m, h)) if up is not None and not packed else none(),
            (bias if bias is not None else pre).new_empty((h,)) if want_dbias else none(),
            pre.new_empty((m, h)) if recompute_out else none())


def _plan_forward(pre, up=None, bias=None, activation=GELU_TANH):
    """The form _act_fwd takes with these tensors, launching nothing: fa_act_plan (include/fa_act.h) as a dict."""
    return _binding().act_fwd_plan(pre, up, bias, _code(activation))


def _plan_backward(dout, pre, up=None, bias=None, activation=GELU_TANH, want_dbias=False, recompute_out=False, packed=False):
    """The form _act_bwd takes with these tensors, launching nothing: fa_act_plan as a dict."""
    return _binding().act_bwd_plan(dout, pre, up, bias, _code(activation), want_dbias, recompute_out, packed)


def _rows(x):
    """x as (M, last) with a unit column stride: a view wherever x allows one"""
    if x.stride(-1) != 1:
        x = x.contiguous()
    return x.reshape(-1, x.shape[-1])


# ---- pure torch: the oracle --------------------------------------------------------------------------------------------------
_K = math.sqrt(2.0 / math.pi)  # 0.79788456 in the reference's digits
_C = 0.044715


def _apply(x, code):
    if code == GELU_TANH:
        return F.gelu(x, approximate="tanh")
    if code == GELU_ERF:
        return F.gelu(x)
    if code == RELU:
        return F.relu(x)
    if code == SQRELU:
        return F.relu(x).square()
    if code == SILU:
        return F.silu(x)
    if code == SIGMOID:
        return torch.sigmoid(x)
    return x


def _derivative(x, code):
    """act'(x) in closed form, written as the kernels write it: 1 - sigmoid(z) is sigmoid(-z), and a product with a factor that
    saturated to 0 is 0"""
    if code == GELU_TANH:
        x2 = x * x
        z = 2 * _K * x * (1 + _C * x2)
        s, w = torch.sigmoid(z), torch.sigmoid(z) * torch.sigmoid(-z)
        return s + torch.where(w > 0, x * w * (2 * _K * (1 + 3 * _C * x2)), torch.zeros_like(x))
    if code == GELU_ERF:
        return 0.5 * torch.erfc(-x / math.sqrt(2.0)) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)
    if code == RELU:
        return (x > 0).to(x.dtype)
    if code == SQRELU:
        return 2 * F.relu(x)
    if code == SILU:
        s = torch.sigmoid(x)
        return s + x * (s * torch.sigmoid(-x))
    if code == SIGMOID:
        return torch.sigmoid(x) * torch.sigmoid(-x)
    return torch.ones_like(x)


def act_ref(x, activation, bias=None):
    """The plain forward contract of include/fa_act.h in torch: act(x + bias), evaluated in the dtype of x (fp64 where given
    fp64); differentiable in x and bias."""
    return _apply(x if bias is None else x + bias.to(x.dtype), _code(activation))


def gated_act_ref(x12, activation):
    """The gated forward contract on a packed (..., 2H) tensor: x12[..., :H] * act(x12[..., H:]), in the dtype of x12."""
    up, gate = x12.chunk(2, dim=-1)
    return up * _apply(gate, _code(activation))


def act_grad_ref(dout, x, activation, bias=None):
    """The plain backward contract in closed form: (dpre, dbias), dbias (the sum of dpre over all rows) None without a bias."""
    dpre = _derivative(x if bias is None else x + bias.to(x.dtype), _code(activation)) * dout
    return dpre, None if bias is None else dpre.reshape(-1, dpre.shape[-1]).sum(dim=0)


def gated_act_grad_ref(dout, x12, activation):
    """The gated backward contract in closed form: the (..., 2H) gradient of gated_act_ref, [dup | dgate]."""
    up, gate = x12.chunk(2, dim=-1)
    code = _code(activation)
    return torch.cat([_apply(gate, code) * dout, _derivative(gate, code) * (up * dout)], dim=-1)


# ---- autograd ------------------------------------------------------------------------------------------------------------------
class _Act(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, bias, code):
        rows = _rows(x)
        bias = None if bias is None else bias.contiguous()
        ctx.save_for_backward(rows, bias)
        ctx.code = code
        return _act_fwd(rows, None, bias, code).view(x.shape)

    @staticmethod
    def backward(ctx, dout):
        rows, bias = ctx.saved_tensors
        want_dbias = bias is not None and ctx.needs_input_grad[1]
        dpre, _, dbias, _ = _act_bwd(_rows(dout), rows, None, bias, ctx.code, want_dbias, False, False)
        return dpre.view(dout.shape), dbias if want_dbias else None, None


class _Gated(torch.autograd.Function):
    """act(gate) * up of two tensors"""

    @staticmethod
    def forward(ctx, gate, up, code):
        if gate.shape != up.shape or gate.dtype != up.dtype:
            raise ValueError("gate and up must have the same shape and dtype")
        g, u = _rows(gate), _rows(up)
        if g.shape[0] > 1 and g.stride(0) != u.stride(0):  # (the kernel takes one pitch for both)
            g, u = g.contiguous(), u.contiguous()
        ctx.save_for_backward(g, u)
        ctx.code = code
        return _act_fwd(g, u, None, code).view(gate.shape)

    @staticmethod
    def backward(ctx, dout):
        g, u = ctx.saved_tensors
        dgate, dup, _, _ = _act_bwd(_rows(dout), g, u, None, ctx.code, False, False, False)
        return dgate.view(dout.shape), dup.view(dout.shape), None


class _GatedPacked(torch.autograd.Function):
    """x12[..., :H] * act(x12[..., H:]) of one tensor, with one gradient tensor"""

    @staticmethod
    def forward(ctx, x12, code):
        if x12.shape[-1] % 2:
            raise ValueError("the last dimension of x12 must be even")
        rows, h = _rows(x12), x12.shape[-1] // 2
        ctx.save_for_backward(rows)
        ctx.code = code
        return _act_fwd(rows[:, h:], rows[:, :h], None, code).view(*x12.shape[:-1], h)

    @staticmethod
    def backward(ctx, dout):
        (rows,) = ctx.saved_tensors
        h = rows.shape[1] // 2
        dx12, _, _, _ = _act_bwd(_rows(dout), rows[:, h:], rows[:, :h], None, ctx.code, False, False, True)
        return dx12.view(*dout.shape[:-1], 2 * h), None


def act(x, activation, bias=None):
    """act(x + bias) for x (..., H) in fp16 / bf16 / fp32 and an optional bias (H) of that dtype or fp32; differentiable in
    both.  activation: a name of ACTIVATIONS."""
    code = _code(activation)
    if not x.is_cuda:
        return act_ref(x, code, bias)
    return _Act.apply(x, bias, code)


def gated_act(x12, activation):
    """x12[..., :H] * act(x12[..., H:]) for the (..., 2H) output of an fc1, read in place through its two halves; the gradient
    is one (..., 2H) tensor."""
    code = _code(activation)
    if not x12.is_cuda:
        return gated_act_ref(x12, code)
    return _GatedPacked.apply(x12, code)


def _gated(gate, up, code):
    if not gate.is_cuda:
        return _apply(gate, code) * up
    return _Gated.apply(gate, up, code)


# ---- the reference's names -----------------------------------------------------------------------------------------------------
def _forward_only(x, up, bias, code):
    if not x.is_cuda:
        y = _apply(x if bias is None else x + bias.to(x.dtype), code)
        return y if up is None else y * up
    rows = _rows(x)
    urows = None if up is None else _rows(up)
    if urows is not None and rows.shape[0] > 1 and rows.stride(0) != urows.stride(0):
        rows, urows = rows.contiguous(), urows.contiguous()
    return _act_fwd(rows, urows, None if bias is None else bias.contiguous(), code).view(x.shape)


def _backward_only(g, x, up, bias, code, want_dbias=False):
    """(dpre or dgate, dup, dbias)"""
    if not x.is_cuda:
        xb = x if bias is None else x + bias.to(x.dtype)
        if up is None:
            dpre = (_derivative(xb, code) * g).to(x.dtype)
            return dpre, None, dpre.reshape(-1, x.shape[-1]).sum(dim=0, dtype=bias.dtype) if want_dbias else None
        return (_derivative(x, code) * (up * g)).to(x.dtype), (_apply(x, code) * g).to(x.dtype), None
    rows = _rows(x)
    urows = None if up is None else _rows(up)
    if urows is not None and rows.shape[0] > 1 and rows.stride(0) != urows.stride(0):
        rows, urows = rows.contiguous(), urows.contiguous()
    dpre, dup, dbias, _ = _act_bwd(_rows(g), rows, urows, None if bias is None else bias.contiguous(), code, want_dbias, False, False)
    return dpre.view(x.shape), dup.view(x.shape) if up is not None else None, dbias if want_dbias else None


def bias_gelu(y, bias):
    """gelu (tanh form) of bias + y, in the dtype of y"""
    return _forward_only(y, None, bias, GELU_TANH)


def bias_gelu_back(g, y, bias):
    """-> (grad_y, grad_bias) for y (..., D) and bias (D): grad_bias is the sum of grad_y over the rows, in the dtype of bias"""
    dpre, _, dbias = _backward_only(g, y, None, bias, GELU_TANH, want_dbias=True)
    return dpre, dbias


def bias_gelu_impl(input, bias):
    return act(input, GELU_TANH, bias)


def gelu_fwd(x):
    return _forward_only(x, None, None, GELU_TANH)


def gelu_bwd(g, x):
    return _backward_only(g, x, None, None, GELU_TANH)[0]


def fast_gelu_impl(input):
    return act(input, GELU_TANH)


def relu_bwd(g, x):
    return _backward_only(g, x, None, None, RELU)[0]


def sqrelu_fwd(x):
    return _forward_only(x, None, None, SQRELU)


def sqrelu_bwd(g, x):
    return _backward_only(g, x, None, None, SQRELU)[0]


def swiglu_fwd(x, y):
    """silu(x) * y"""
    return _forward_only(x, y, None, SILU)


def swiglu_bwd(x, y, g):
    """-> (dx, dy)"""
    dgate, dup, _ = _backward_only(g, x, y, None, SILU)
    return dgate, dup


def swiglu(x, y):
    """silu(x) * y, differentiable in both: x is the gate"""
    return _gated(x, y, SILU)
