"""`flash_attn.losses.cross_entropy` by name: the CrossEntropyLoss module over the fused loss of ops/triton/cross_entropy.py
(HIP kernels, csrc/fa_xent.hip)."""
import torch.nn as nn

from ..ops.triton.cross_entropy import cross_entropy_loss

__all__ = ["CrossEntropyLoss"]


class CrossEntropyLoss(nn.Module):
    """torch.nn.CrossEntropyLoss for (batch, vocab_size) logits on the GPU, with the reference's further arguments.

    ignore_index: rows with this label lose nothing and get a zero gradient.  reduction: "mean" (the sum over the count of
    rows that are not ignored), "sum" or "none".  logit_scale multiplies the logits first.  lse_square_scale > 0 adds the z-loss
    lse_square_scale * lse^2.  inplace_backward writes the gradient over the logits.  process_group: every rank holds its
    columns of the vocabulary.  return_z_loss: also return the z-loss part, reduced the same way; it is for logging and is not
    differentiable."""

    def __init__(self, ignore_index=-100, reduction="mean", label_smoothing=0.0, logit_scale=1.0, lse_square_scale=0.0,
                 inplace_backward=False, process_group=None, return_z_loss=False):
        super().__init__()
        if reduction not in ("mean", "none", "sum"):
            raise NotImplementedError("Only support reduction = 'mean' or 'none' or 'sum'")
        self.ignore_index = ignore_index
        self.reduction = reduction
        self.label_smoothing = label_smoothing
        self.logit_scale = logit_scale
        self.lse_square_scale = lse_square_scale
        self.inplace_backward = inplace_backward
        self.process_group = process_group
        self.return_z_loss = return_z_loss

    def _reduce(self, per_row, target):
        if self.reduction == "mean":
            return per_row.sum() / (target != self.ignore_index).sum()
        return per_row.sum() if self.reduction == "sum" else per_row

    def forward(self, input, target, precomputed_lse=None):
        """input (batch, vocab_size), target (batch,) -> the loss, fp32: (batch,) with reduction "none", else a scalar; with
        return_z_loss a pair (loss, z_loss)."""
        if not (input.is_cuda and target.is_cuda):
            raise ValueError("Only support CUDA tensors")
        loss, z_loss = cross_entropy_loss(input, target, precomputed_lse=precomputed_lse, label_smoothing=self.label_smoothing,
                                          logit_scale=self.logit_scale, lse_square_scale=self.lse_square_scale,
                                          ignore_index=self.ignore_index, inplace_backward=self.inplace_backward,
                                          process_group=self.process_group)
        loss = self._reduce(loss, target)
        return (loss, self._reduce(z_loss, target)) if self.return_z_loss else loss
