"""The single-GPU part of the reference's `flash_attn/ops/fused_dense.py` by name:

    fused_dense_func, FusedDense      reference :118-163   F.linear plus return_residual: there is nothing to fuse
    fused_mlp_func, FusedMLP                    :249-610   fc1 -> bias + activation -> fc2

The two GEMMs stay on torch (hipBLASLt); what the reference reaches through cuBLASLt epilogues is one pass of the HIP kernels
of csrc/fa_act.hip after the GEMM: the forward adds bias1 and applies the activation in one read of the fc1 output, and the
backward takes dpre, dbias1 and -- at checkpoint_lvl 1 and 2 -- the recomputed activation output from one fa_act_bwd call.

checkpoint_lvl has the reference's meaning: 0 saves the fc1 output and the activation output; 1 saves the fc1 output and
recomputes the activation output in the backward (for relu the reference saves both, and so does this); 2 saves neither and
recomputes both.  `heuristic` chose cuBLASLt algorithms: it is accepted and ignored.

Not built: tensor and sequence parallelism.  `process_group is not None` raises NotImplementedError, and ColumnParallelLinear,
RowParallelLinear and ParallelFusedMLP do not exist here: importing them fails.
"""
from functools import partial
from typing import Optional

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch import Tensor

from .activations import ACTIVATIONS, RELU, _act_bwd, _act_fwd

__all__ = ["fused_dense_func", "FusedDense", "fused_mlp_func", "FusedMLP"]

_MLP_ACTIVATIONS = ("gelu_approx", "relu", "sqrelu")


def _refuse_process_group(process_group):
    if process_group is not None:
        raise NotImplementedError("process_group is not supported: tensor and sequence parallelism are not built")


def fused_dense_func(x: Tensor, weight: Tensor, bias: Optional[Tensor] = None, return_residual: bool = False,
                     process_group=None, sequence_parallel: bool = True):
    """F.linear(x, weight, bias); with return_residual also x itself."""
    _refuse_process_group(process_group)
    out = F.linear(x, weight, bias)
    return out if not return_residual else (out, x)


class FusedDense(nn.Linear):
    def __init__(self, in_features: int, out_features: int, bias: bool = True, return_residual: bool = False, device=None,
                 dtype=None) -> None:
        super().__init__(in_features, out_features, bias=bias, device=device, dtype=dtype)
        self.return_residual = return_residual

    def forward(self, x, process_group=None):
        return fused_dense_func(x, self.weight, self.bias, return_residual=self.return_residual, process_group=process_group)


class FusedMLPFunc(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight1, bias1, weight2, bias2, activation="gelu_approx", save_pre_act=True, checkpoint_lvl=0):
        if not save_pre_act:
            checkpoint_lvl = 2
        code = ACTIVATIONS[activation]
        if torch.is_autocast_enabled():
            dtype = torch.get_autocast_gpu_dtype()
            x, weight1, weight2 = (a.to(dtype=dtype) for a in (x, weight1, weight2))
            bias1 = bias1.to(dtype=dtype) if bias1 is not None else None
            bias2 = bias2.to(dtype=dtype) if bias2 is not None else None
        x = x.contiguous()
        weight1, weight2 = weight1.contiguous(), weight2.contiguous()
        bias1 = bias1.contiguous() if bias1 is not None else None
        batch_shape, n = x.shape[:-1], x.shape[-1]
        pre_act = torch.mm(x.reshape(-1, n), weight1.t())  # (bias1 is added by the activation kernel)
        output1 = _act_fwd(pre_act, None, bias1, code)
        output2 = F.linear(output1, weight2, bias2)
        ctx.checkpoint_lvl, ctx.code = checkpoint_lvl, code
        ctx.has_bias1 = bias1 is not None
        if checkpoint_lvl == 0 or (checkpoint_lvl == 1 and code == RELU):
            ctx.save_for_backward(x, weight1, weight2, bias1, pre_act, output1)
        elif checkpoint_lvl == 1:
            ctx.save_for_backward(x, weight1, weight2, bias1, pre_act)
        else:
            ctx.save_for_backward(x, weight1, weight2, bias1)
        return output2.reshape(*batch_shape, output2.shape[-1])

    @staticmethod
    def backward(ctx, grad_output):
        x, weight1, weight2, bias1, *rest = ctx.saved_tensors
        batch_shape, n = x.shape[:-1], x.shape[-1]
        x2d = x.reshape(-1, n)
        grad_output = grad_output.reshape(-1, grad_output.shape[-1]).to(weight2.dtype)
        output1 = None
        if len(rest) == 2:
            pre_act, output1 = rest
        elif len(rest) == 1:
            (pre_act,) = rest
        else:
            pre_act = torch.mm(x2d, weight1.t())
        grad_output1 = torch.mm(grad_output, weight2)
        # one pass: dpre, dbias1 and, unless it was saved, the activation output fc2's weight gradient needs
        want_dbias1 = ctx.has_bias1 and ctx.needs_input_grad[2]
        need_output1 = output1 is None and ctx.needs_input_grad[3]
        grad_pre_act, _, grad_bias1, recomputed = _act_bwd(grad_output1, pre_act, None, bias1, ctx.code, want_dbias1, need_output1, False)
        if need_output1:
            output1 = recomputed
        grad_weight2 = torch.mm(grad_output.t(), output1) if ctx.needs_input_grad[3] else None
        grad_bias2 = grad_output.sum(dim=0) if ctx.needs_input_grad[4] else None
        grad_input = torch.mm(grad_pre_act, weight1).reshape(*batch_shape, n) if ctx.needs_input_grad[0] else None
        grad_weight1 = torch.mm(grad_pre_act.t(), x2d) if ctx.needs_input_grad[1] else None
        return (grad_input, grad_weight1, grad_bias1 if want_dbias1 else None, grad_weight2, grad_bias2, None, None, None)


def fused_mlp_func(x: Tensor, weight1: Tensor, weight2: Tensor, bias1: Optional[Tensor] = None, bias2: Optional[Tensor] = None,
                   activation: str = "gelu_approx", save_pre_act: bool = True, return_residual: bool = False,
                   checkpoint_lvl: int = 0, heuristic: int = 0, process_group=None, sequence_parallel: bool = True):
    """fc2(act(fc1(x))) for x (..., in) with the activation pass on the HIP kernels; fp16, bf16 or fp32 on the GPU.  CPU tensors
    take the eager composition."""
    _refuse_process_group(process_group)
    assert activation in _MLP_ACTIVATIONS
    assert checkpoint_lvl in (0, 1, 2)
    if x.is_cuda:  # (the residual is x itself: autograd adds its gradient to that of the MLP)
        out = FusedMLPFunc.apply(x, weight1, bias1, weight2, bias2, activation, save_pre_act, checkpoint_lvl)
        return out if not return_residual else (out, x)
    pre_act = F.linear(x, weight1, bias1)
    activation_fn = (partial(F.gelu, approximate="tanh") if activation == "gelu_approx"
                     else (lambda t: F.relu(t).square()) if activation == "sqrelu" else F.relu)
    output2 = F.linear(activation_fn(pre_act), weight2, bias2)
    return output2 if not return_residual else (output2, x)


class FusedMLP(nn.Module):
    def __init__(self, in_features, hidden_features=None, out_features=None, bias1=True, bias2=True, activation="gelu_approx",
                 return_residual=False, checkpoint_lvl=0, heuristic="auto", device=None, dtype=None):
        """checkpoint_lvl (increasing lvl means slower but more memory saving):
            0: no recomputation in the bwd
            1: recompute the activation output in the bwd
            2: recompute the fc1 output and the activation output in the bwd
        heuristic: accepted and ignored (it chose cuBLASLt algorithms).
        return_residual: whether to return the input x along with the output."""
        assert checkpoint_lvl in [0, 1, 2]
        assert activation in _MLP_ACTIVATIONS
        factory_kwargs = {"device": device, "dtype": dtype}
        super().__init__()
        out_features = out_features or in_features
        hidden_features = hidden_features or in_features * 4
        self.activation = activation
        self.return_residual = return_residual
        self.checkpoint_lvl = checkpoint_lvl
        self.heuristic = heuristic if activation != "sqrelu" else -1
        self.fc1 = nn.Linear(in_features, hidden_features, bias=bias1, **factory_kwargs)
        self.fc2 = nn.Linear(hidden_features, out_features, bias=bias2, **factory_kwargs)

    def forward(self, x, process_group=None):
        _refuse_process_group(process_group)
        heuristic = 0 if self.heuristic == "auto" else self.heuristic
        return fused_mlp_func(x, self.fc1.weight, self.fc2.weight, self.fc1.bias, self.fc2.bias, activation=self.activation,
                              save_pre_act=self.training, return_residual=self.return_residual,
                              checkpoint_lvl=self.checkpoint_lvl, heuristic=heuristic, process_group=process_group)
