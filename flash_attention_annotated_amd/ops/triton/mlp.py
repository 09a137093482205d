"""The reference's `flash_attn/ops/triton/mlp.py` by name: fc1 -> squared ReLU -> fc2 with the activation inside fc1's GEMM.

    FusedDenseSqreluDenseFunc, fused_dense_sqrelu_dense_function      reference :13-113
    FusedDenseSqreluDense                                                       :116-149

fc1 with bias1 and the squared ReLU is one `triton_linear_act` call (ops.triton.linear: the HIP GEMM of csrc/fa_gemm_act.hip) for
fp16 and bf16 alike (the reference sends bf16 to cuBLASLt and an activation pass); in the backward, the gradient of the
activation's input and grad_bias1 come from one `gemm_act_dgrad` call.  fc2, both weight gradients and grad_input stay on torch.

checkpoint_lvl has the reference's meaning: 0 saves act_input and the activation output; 1 saves act_input and recomputes the
output; 2 saves neither and recomputes both with the forward's call.  The three levels give the same bits, which costs level 1
its shortcut: the output is the activation of the unrounded fp32 sum, so level 1 recomputes it with the forward's call too.
CPU tensors take the eager composition through the same functions.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .linear import gemm_act_dgrad, triton_linear_act

__all__ = ["FusedDenseSqreluDenseFunc", "fused_dense_sqrelu_dense_function", "FusedDenseSqreluDense"]


class FusedDenseSqreluDenseFunc(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight1, bias1, weight2, bias2, checkpoint_lvl=0):
        """checkpoint_lvl:
        0: no recomputation in the bwd
        1: recompute gelu_out in the bwd
        2: recompute act_input and gelu_out in the bwd
        """
        if torch.is_autocast_enabled():
            dtype = torch.get_autocast_gpu_dtype()
            x, weight1, bias1, weight2, bias2 = [a.to(dtype=dtype) for a in [x, weight1, bias1, weight2, bias2]]
        assert checkpoint_lvl in [0, 1, 2]
        x = x.contiguous()
        weight1 = weight1.contiguous()
        bias1 = bias1.contiguous()
        weight2 = weight2.contiguous()
        bias2 = bias2.contiguous()
        batch_shape, n = x.shape[:-1], x.shape[-1]
        # (act_input is written at every level, so that the output has the same bits at every level; level 2 drops it)
        output1, act_input = triton_linear_act(x.reshape(-1, n), weight1, bias1, activation="squared_relu", save_act_input=True)
        output2 = F.linear(output1, weight2, bias2)
        ctx.checkpoint_lvl = checkpoint_lvl
        if checkpoint_lvl == 0:
            ctx.save_for_backward(x, weight1, bias1, weight2, act_input, output1)
        elif checkpoint_lvl == 1:
            ctx.save_for_backward(x, weight1, bias1, weight2, act_input)
        elif checkpoint_lvl == 2:
            ctx.save_for_backward(x, weight1, bias1, weight2)
        return output2.reshape(*batch_shape, output2.shape[-1])

    @staticmethod
    def backward(ctx, grad_output):
        grad_output = grad_output.contiguous()
        checkpoint_lvl = ctx.checkpoint_lvl
        x, weight1, bias1, weight2, *rest = ctx.saved_tensors
        batch_shape, n = x.shape[:-1], x.shape[-1]
        x2d = x.reshape(-1, n)
        if checkpoint_lvl == 0:
            act_input, output1 = rest
        elif checkpoint_lvl == 1:
            (act_input,) = rest
            output1 = None
        elif checkpoint_lvl == 2:
            output1, act_input = triton_linear_act(x2d, weight1, bias1, activation="squared_relu", save_act_input=True)
        grad_output = grad_output.reshape(-1, grad_output.shape[-1]).to(weight2.dtype)
        grad_weight2 = grad_bias2 = None
        if ctx.needs_input_grad[3]:
            if output1 is None:  # (level 1: one rounding of the fp32 square of the stored act_input; see _recompute_output1)
                output1 = _recompute_output1(x2d, weight1, bias1)
            grad_weight2 = torch.mm(grad_output.t(), output1)
        if ctx.needs_input_grad[4]:
            grad_bias2 = grad_output.sum(dim=0)
        # one call: the gradient of the activation's input and, from the unrounded products, grad_bias1
        grad_act_input, grad_bias1 = gemm_act_dgrad(grad_output, weight2, "squared_relu", act_input, want_dbias=ctx.needs_input_grad[2])
        grad_input = torch.mm(grad_act_input, weight1).reshape(*batch_shape, n) if ctx.needs_input_grad[0] else None
        grad_weight1 = torch.mm(grad_act_input.t(), x2d) if ctx.needs_input_grad[1] else None
        return grad_input, grad_weight1, grad_bias1, grad_weight2, grad_bias2, None


def _recompute_output1(x2d, weight1, bias1):
    """The activation output at checkpoint level 1.  The forward's output is the activation of the unrounded fp32 sum, which the
    stored (rounded) act_input cannot reproduce bit for bit, so level 1 runs the forward's call again, as level 2 does."""
    return triton_linear_act(x2d, weight1, bias1, activation="squared_relu", save_act_input=False)


fused_dense_sqrelu_dense_function = FusedDenseSqreluDenseFunc.apply


class FusedDenseSqreluDense(nn.Module):
    def __init__(self, in_features, hidden_features=None, out_features=None, bias1=True, bias2=True, checkpoint_lvl=0, device=None,
                 dtype=None):
        """
        checkpoint_lvl (increasing lvl means slower but more memory saving):
            0: no recomputation in the bwd
            1: recompute gelu_out in the bwd
            2: recompute gelu_in and gelu_out in the bwd
        """
        assert checkpoint_lvl in [0, 1, 2]
        factory_kwargs = {"device": device, "dtype": dtype}
        super().__init__()
        out_features = out_features or in_features
        hidden_features = hidden_features or in_features * 4
        assert bias1 == True, "DenseSqreluDense module without bias is currently not supported"  # noqa: E712
        assert bias2 == True, "DenseSqreluDense module without bias is currently not supported"  # noqa: E712
        self.checkpoint_lvl = checkpoint_lvl
        self.fc1 = nn.Linear(in_features, hidden_features, bias=bias1, **factory_kwargs)
        self.fc2 = nn.Linear(hidden_features, out_features, bias=bias2, **factory_kwargs)

    def forward(self, x):
        return fused_dense_sqrelu_dense_function(x, self.fc1.weight, self.fc1.bias, self.fc2.weight, self.fc2.bias,
                                                 self.checkpoint_lvl)
