"""The GEMM with a fused bias + activation epilogue behind the names of the reference's `flash_attn/ops/triton/linear.py`:

    triton_linear_act      reference :258-347   act(x @ weight.T + bias), optionally also the activation's input
    triton_dgrad_act                 :529-594   (grad_output @ weight) * act'(act_input)
    gemm_act_dgrad         the same with the column sums of the result (the bias gradient) from the same call
    linear_act_ref, dgrad_act_ref    pure torch, in the dtype they are given (fp64 where given fp64): the oracle

Same names, argument order, defaults, asserts and return conventions.  Where the reference launches Triton kernels, this module
launches the HIP kernels of csrc/fa_gemm_act.hip (include/fa_gemm_act.h) through `flash_attn_2_cuda_C.gemm_act_fwd` /
`gemm_act_dgrad`, wrapped in torch.library custom ops with fake implementations, so torch.compile traces them.  The activation
is applied to the unrounded fp32 sum; `act_input` is that sum rounded once.

The kernels take fp16 and bf16 with N and K multiples of 8; an operand whose base or row pitch is not 16-byte aligned is copied
first.  A call they do not take (N or K not a multiple of 8, fp32) runs `torch.mm` followed by the activation kernels of
ops.activations: `_plan_linear_act` / `_plan_dgrad_act` name the form a call takes ("fused" or "mm_act") without launching.
CPU tensors take the eager composition.  As in the reference, these functions are not differentiable: ops.triton.mlp holds the
autograd function built on them.
"""
from typing import Optional, Tuple

import torch
import torch.nn.functional as F
from torch import Tensor

from ..._lib import binding as _binding
from ..activations import GELU_ERF, GELU_TANH, IDENTITY, RELU, SQRELU, _act_bwd, _act_fwd, _apply, _derivative

__all__ = ["triton_linear_act", "triton_dgrad_act", "gemm_act_dgrad", "linear_act_ref", "dgrad_act_ref"]

_custom_op = torch.library.custom_op
_register_fake = torch.library.register_fake

# the reference's activation names (and relu, which ops.fused_dense has) as codes of include/fa_act.h
_ACTIVATIONS = {"id": IDENTITY, "gelu": GELU_ERF, "gelu_approx": GELU_TANH, "squared_relu": SQRELU, "relu": RELU}


def _aligned(t: Optional[Tensor]) -> Optional[Tensor]:
    """t (rows, cols) or (cols) as the kernels read it: unit last stride, 16-byte base and row pitch; a copy where it is not"""
    if t is None:
        return None
    if t.stride(-1) != 1 or (t.dim() == 2 and t.shape[0] > 1 and t.stride(0) % 8):
        t = t.contiguous()
    if t.data_ptr() % 16:  # (contiguous already, at an odd base: a fresh allocation is aligned)
        t = t.clone(memory_format=torch.contiguous_format)
    return t


# ---- the kernel entries ------------------------------------------------------------------------------------------------------
@_custom_op("flash_attn_amd::_gemm_act_fwd", mutates_args=(), device_types="cuda")
def _gemm_act_fwd(x: Tensor, weight: Tensor, bias: Optional[Tensor], activation: int, save_act_input: bool) -> Tuple[Tensor, Tensor]:
    """(out, act_input) (M, N) of act(x @ weight.T + bias) for x (M, K), weight (N, K); act_input is empty unless asked for."""
    return _binding().gemm_act_fwd(_aligned(x), _aligned(weight), _aligned(bias), activation, save_act_input)


@_register_fake("flash_attn_amd::_gemm_act_fwd")
def _gemm_act_fwd_fake(x, weight, bias, activation, save_act_input):
    m, n = x.shape[0], weight.shape[0]
    return x.new_empty((m, n)), x.new_empty((m, n)) if save_act_input else x.new_empty((0,))


@_custom_op("flash_attn_amd::_gemm_act_dgrad", mutates_args=(), device_types="cuda")
def _gemm_act_dgrad(grad_out: Tensor, weight: Tensor, act_input: Optional[Tensor], activation: int,
                    want_dbias: bool) -> Tuple[Tensor, Tensor]:
    """(grad_in (M, N), dbias (N)) of (grad_out @ weight) * act'(act_input) for grad_out (M, K), weight (K, N); dbias is empty
    unless asked for."""
    return _binding().gemm_act_dgrad(_aligned(grad_out), _aligned(weight), _aligned(act_input), activation, want_dbias)


@_register_fake("flash_attn_amd::_gemm_act_dgrad")
def _gemm_act_dgrad_fake(grad_out, weight, act_input, activation, want_dbias):
    m, n = grad_out.shape[0], weight.shape[1]
    return grad_out.new_empty((m, n)), grad_out.new_empty((n,)) if want_dbias else grad_out.new_empty((0,))


def _fused(a: Tensor, n: int, k: int) -> bool:
    """whether the kernels take a GEMM of 16-bit `a` with these N and K"""
    return a.dtype in (torch.float16, torch.bfloat16) and n >= 8 and k >= 8 and n % 8 == 0 and k % 8 == 0


def _rows(x: Tensor) -> Tensor:
    """x as (M, last); copied, as in the reference, when neither stride is 1"""
    x = x.reshape(-1, x.shape[-1])
    if x.stride(0) > 1 and x.stride(1) > 1:
        x = x.contiguous()
    return x


def _plan_linear_act(x, weight, bias=None, activation="id", save_act_input=False):
    """The form triton_linear_act takes with these tensors, launching nothing: {"form": "fused", + fa_gemm_act_plan} or
    {"form": "mm_act"}."""
    rows = _rows(x)
    if not _fused(rows, weight.shape[0], weight.shape[1]):
        return {"form": "mm_act"}
    plan = _binding().gemm_act_fwd_plan(_aligned(rows), _aligned(weight), _aligned(bias),
                                        _ACTIVATIONS[activation], save_act_input)
    return {"form": "fused", **plan}


def _plan_dgrad_act(grad_output, weight, activation="id", act_input=None, want_dbias=False):
    """The form triton_dgrad_act / gemm_act_dgrad takes with these tensors, launching nothing."""
    rows = _rows(grad_output)
    if not _fused(rows, weight.shape[1], weight.shape[0]):
        return {"form": "mm_act"}
    act_rows = None if act_input is None else _aligned(act_input.reshape(-1, act_input.shape[-1]))
    plan = _binding().gemm_act_dgrad_plan(_aligned(rows), _aligned(weight), act_rows, _ACTIVATIONS[activation], want_dbias)
    return {"form": "fused", **plan}


# ---- pure torch: the oracle --------------------------------------------------------------------------------------------------
def linear_act_ref(x, weight, bias=None, activation="id", save_act_input=False):
    """The forward contract of include/fa_gemm_act.h in torch, in the dtype of x: act(x @ weight.T + bias), with save_act_input
    the tuple (out, act_input)."""
    act_input = F.linear(x, weight, bias)
    out = _apply(act_input, _ACTIVATIONS[activation])
    return out if not save_act_input else (out, act_input)


def dgrad_act_ref(grad_output, weight, activation="id", act_input=None):
    """The dgrad contract in closed form, in the dtype of grad_output: (grad_output @ weight) * act'(act_input)."""
    grad = grad_output @ weight
    if activation != "id":
        assert act_input is not None, f"act_input is required for activation {activation}"
        grad = grad * _derivative(act_input.to(grad.dtype), _ACTIVATIONS[activation])
    return grad


# ---- the reference's names -----------------------------------------------------------------------------------------------------
def triton_linear_act(x: Tensor, weight: Tensor, bias: Optional[Tensor] = None, activation: str = "id",
                      save_act_input: bool = False) -> Tensor:
    """Compute e = activation(x @ weight.T + bias) for x (..., K), weight (N, K) and an optional bias (N), all of one dtype.
    With save_act_input returns (e, act_input), act_input being x @ weight.T + bias."""
    assert activation in ["id", "gelu", "gelu_approx", "squared_relu", "relu"]
    code = _ACTIVATIONS[activation]
    batch_shape = x.shape[:-1]
    x_reshaped = _rows(x)
    if weight.stride(0) > 1 and weight.stride(1) > 1:
        weight = weight.contiguous()
    bias = bias.contiguous() if bias is not None else None
    assert x.dtype == weight.dtype, f"Input and weight must have the same dtype, got {x.dtype} and {weight.dtype}"
    if bias is not None:
        assert x.dtype == bias.dtype, f"Input and bias must have the same dtype, got {x.dtype} and {bias.dtype}"
    assert x_reshaped.shape[1] == weight.shape[1], f"Incompatible dimensions: {x_reshaped.shape} - {weight.shape}"
    assert bias is None or bias.shape[0] == weight.shape[0], "Incompatible dimensions in between weight and bias"
    n, k = weight.shape
    if not x.is_cuda:
        result = linear_act_ref(x_reshaped, weight, bias, activation, True)
    elif _fused(x_reshaped, n, k):
        result = _gemm_act_fwd(x_reshaped, weight, bias, code, save_act_input)
    elif save_act_input:  # (act_input carries the bias: the activation pass adds none)
        act_input = torch.mm(x_reshaped, weight.t()) if bias is None else torch.addmm(bias, x_reshaped, weight.t())
        result = _act_fwd(act_input, None, None, code), act_input
    else:
        result = _act_fwd(torch.mm(x_reshaped, weight.t()), None, bias, code), None
    output, act_input = result
    if not save_act_input:
        return output.reshape(*batch_shape, n)
    return output.reshape(*batch_shape, n), act_input.reshape(*batch_shape, n)


def gemm_act_dgrad(grad_output: Tensor, weight: Tensor, activation: str = "id", act_input: Optional[Tensor] = None,
                   want_dbias: bool = False) -> Tuple[Tensor, Optional[Tensor]]:
    """(grad_input, dbias) for grad_output (..., K), weight (K, N) and act_input (..., N): grad_input = (grad_output @ weight) *
    act'(act_input) and, with want_dbias, its sum over all rows, taken in fp32 from the unrounded products (None otherwise)."""
    assert activation in ["id", "gelu", "gelu_approx", "squared_relu", "relu"]
    code = _ACTIVATIONS[activation]
    batch_shape = grad_output.shape[:-1]
    grad_output_reshaped = _rows(grad_output)
    if weight.stride(0) > 1 and weight.stride(1) > 1:
        weight = weight.contiguous()
    assert grad_output.dtype == weight.dtype, f"grad_output and weight must have the same dtype, got {grad_output.dtype} and {weight.dtype}"
    assert grad_output_reshaped.shape[1] == weight.shape[0], f"Incompatible dimensions: {grad_output_reshaped.shape} - {weight.shape}"
    if activation != "id":
        assert act_input is not None, f"act_input is required for activation {activation}"
    k, n = weight.shape
    act_rows = None if act_input is None or code == IDENTITY else act_input.reshape(-1, n)
    if not grad_output.is_cuda:
        grad_input = dgrad_act_ref(grad_output_reshaped, weight, activation, act_rows)
        dbias = grad_input.sum(dim=0) if want_dbias else None
    elif _fused(grad_output_reshaped, n, k):
        grad_input, dbias = _gemm_act_dgrad(grad_output_reshaped, weight, act_rows, code, want_dbias)
    else:
        grad = torch.mm(grad_output_reshaped, weight)
        if act_rows is None:
            grad_input, dbias = grad, grad.sum(dim=0, dtype=torch.float32).to(grad.dtype) if want_dbias else None
        else:
            grad_input, _, dbias, _ = _act_bwd(grad, act_rows if act_rows.stride(-1) == 1 else act_rows.contiguous(), None, None, code,
                                               want_dbias, False, False)
    return grad_input.reshape(*batch_shape, n), dbias if want_dbias else None


def triton_dgrad_act(grad_output: Tensor, weight: Tensor, activation: str = "id", act_input: Optional[Tensor] = None) -> Tensor:
    """Compute e = (grad_output @ weight) * activation'(act_input) for grad_output (..., K) and weight (K, N)."""
    return gemm_act_dgrad(grad_output, weight, activation, act_input, False)[0]
