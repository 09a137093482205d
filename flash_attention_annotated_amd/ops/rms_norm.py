"""`flash_attn.ops.rms_norm` by name (reference :14-17, :124-138): rms_norm and the RMSNorm module over the fused kernel of
ops/norm.py.  The dropout_add_* names of the reference's file are not built."""
import torch

from .norm import rms_norm_fn


def rms_norm(x, weight, epsilon):
    """x / sqrt(mean(x^2) + epsilon) * weight over the last dim, in x's dtype."""
    return rms_norm_fn(x, weight, None, eps=epsilon)


class RMSNorm(torch.nn.Module):
    def __init__(self, hidden_size, eps=1e-5, device=None, dtype=None):
        super().__init__()
        self.eps = eps
        self.weight = torch.nn.Parameter(torch.empty(hidden_size, device=device, dtype=dtype))
        self.register_parameter("bias", None)
        self.reset_parameters()

    def reset_parameters(self):
        torch.nn.init.ones_(self.weight)

    def forward(self, x):
        return rms_norm(x, self.weight, self.eps)
