"""`flash_attn.modules.mlp` by name: Mlp and GatedMlp with the reference's constructor arguments and defaults (reference
flash_attn/modules/mlp.py:25-51, 99-136), the activation between the two linears on the HIP kernels of csrc/fa_act.hip.

Mlp fuses the activation where it is one the kernel knows -- F.gelu (erf), partial(F.gelu, approximate="tanh"), F.relu,
F.silu -- and calls any other as given.  GatedMlp routes F.sigmoid (GLU), F.silu (SwiGLU), F.gelu (GEGLU, erf) and F.relu
(ReGLU) through `gated_act` on the fc1 output: its two halves are read in place and its gradient is written as one tensor.
The reference's half order is kept: first half the value, second half the gate.  Any other callable goes the eager way, and so
do CPU tensors.  ParallelMLP and ParallelGatedMlp are not built.
"""
from functools import partial

import torch
import torch.nn as nn
import torch.nn.functional as F

from ..ops.activations import act, gated_act

__all__ = ["Mlp", "GatedMlp"]


def _kernel_activation(activation, gated):
    """the name in ops.activations.ACTIVATIONS of a callable the kernels know, or None"""
    if activation is F.gelu:
        return "gelu_erf"
    if activation is F.relu:
        return "relu"
    if activation is F.silu:
        return "silu"
    if gated and (activation is F.sigmoid or activation is torch.sigmoid):
        return "sigmoid"
    if (not gated and isinstance(activation, partial) and activation.func is F.gelu and not activation.args
            and activation.keywords == {"approximate": "tanh"}):
        return "gelu_tanh"
    return None


class Mlp(nn.Module):
    def __init__(self, in_features, hidden_features=None, out_features=None, activation=F.gelu, bias1=True, bias2=True,
                 return_residual=False, device=None, dtype=None):
        factory_kwargs = {"device": device, "dtype": dtype}
        super().__init__()
        out_features = out_features if out_features is not None else in_features
        hidden_features = hidden_features if hidden_features is not None else in_features * 4
        self.return_residual = return_residual
        self.fc1 = nn.Linear(in_features, hidden_features, bias=bias1, **factory_kwargs)
        self.activation = activation
        self.fc2 = nn.Linear(hidden_features, out_features, bias=bias2, **factory_kwargs)

    def forward(self, x):
        y = self.fc1(x)
        name = _kernel_activation(self.activation, gated=False) if y.is_cuda else None
        y = act(y, name) if name is not None else self.activation(y)
        y = self.fc2(y)
        return y if not self.return_residual else (y, x)


class GatedMlp(nn.Module):
    def __init__(self, in_features, hidden_features=None, out_features=None, activation=F.sigmoid, bias1=True, bias2=True,
                 multiple_of=128, return_residual=False, device=None, dtype=None):
        factory_kwargs = {"device": device, "dtype": dtype}
        super().__init__()
        out_features = out_features if out_features is not None else in_features
        hidden_features = hidden_features if hidden_features is not None else int(8 * in_features / 3)
        hidden_features = (hidden_features + multiple_of - 1) // multiple_of * multiple_of
        self.return_residual = return_residual
        self.fc1 = nn.Linear(in_features, 2 * hidden_features, bias=bias1, **factory_kwargs)
        self.activation = activation
        self.fc2 = nn.Linear(hidden_features, out_features, bias=bias2, **factory_kwargs)

    def forward(self, x):
        y = self.fc1(x)
        name = _kernel_activation(self.activation, gated=True) if y.is_cuda else None
        if name is not None:
            y = gated_act(y, name)
        elif self.activation == F.sigmoid:  # GLU
            y = F.glu(y, dim=-1)
        else:
            y, gate = y.chunk(2, dim=-1)
            y = y * self.activation(gate)
        y = self.fc2(y)
        return y if not self.return_residual else (y, x)
