"""The fused cross-entropy loss behind the names of the reference's `flash_attn/ops/triton/cross_entropy.py`:

    CrossEntropyLoss (the autograd function)   reference :149-289
    cross_entropy_loss                                   :292-330
    cross_entropy_ref, cross_entropy_grad_ref            pure torch: the contract of include/fa_xent.h, the CPU oracle

Same argument order and defaults.  Where the reference launches its Triton kernels, this module launches the HIP kernels of
csrc/fa_xent.hip through `flash_attn_2_cuda_C.xent_fwd` / `xent_bwd`, wrapped in torch.library custom ops with fake
implementations, so torch.compile traces the loss.  There is no eager fall-back: without the built library the ops raise.

One departure from the reference: a row whose label is ignore_index gets a gradient of exact zeros without its logits being
read (the reference multiplies by zero, so a NaN in a padding row reaches the gradient).
"""
from typing import Optional, Tuple

import torch
from torch import Tensor

from ..._lib import binding as _binding

_custom_op = torch.library.custom_op
_register_fake = torch.library.register_fake


# ---- the kernel entries ------------------------------------------------------------------------------------------------------
@_custom_op("flash_attn_amd::_xent_fwd", mutates_args=(), device_types="cuda")
def _xent_fwd(logits: Tensor, labels: Tensor, precomputed_lse: Optional[Tensor], smoothing: float, logit_scale: float,
              lse_square_scale: float, ignore_index: int, class_start_idx: int, total_classes: int,
              split: bool) -> Tuple[Tensor, Tensor, Tensor]:
    """(losses, lse, z_losses), fp32 (M).  lse is empty with precomputed_lse (that tensor is read instead); with split the
    losses lack the lse and the z-loss (_finish_split adds the global ones) and z_losses is empty."""
    return _binding().xent_fwd(logits, labels, precomputed_lse, smoothing, logit_scale, lse_square_scale, ignore_index,
                               class_start_idx, total_classes, split)


@_register_fake("flash_attn_amd::_xent_fwd")
def _xent_fwd_fake(logits, labels, precomputed_lse, smoothing, logit_scale, lse_square_scale, ignore_index, class_start_idx,
                   total_classes, split):
    m = logits.shape[0]
    vec = lambda n: logits.new_empty((n,), dtype=torch.float32)  # noqa: E731
    return vec(m), vec(0 if precomputed_lse is not None else m), vec(0 if split else m)


@_custom_op("flash_attn_amd::_xent_bwd", mutates_args=(), device_types="cuda")
def _xent_bwd(dloss: Tensor, logits: Tensor, labels: Tensor, lse: Tensor, smoothing: float, logit_scale: float,
              lse_square_scale: float, ignore_index: int, class_start_idx: int, total_classes: int) -> Tensor:
    """dlogits, a tensor allocated like logits."""
    dlogits = torch.empty_like(logits)
    _binding().xent_bwd(dloss, logits, labels, lse, dlogits, smoothing, logit_scale, lse_square_scale, ignore_index,
                        class_start_idx, total_classes)
    return dlogits


@_register_fake("flash_attn_amd::_xent_bwd")
def _xent_bwd_fake(dloss, logits, labels, lse, smoothing, logit_scale, lse_square_scale, ignore_index, class_start_idx,
                   total_classes):
    return torch.empty_like(logits)


@_custom_op("flash_attn_amd::_xent_bwd_inplace", mutates_args=("logits",), device_types="cuda")
def _xent_bwd_inplace(dloss: Tensor, logits: Tensor, labels: Tensor, lse: Tensor, smoothing: float, logit_scale: float,
                      lse_square_scale: float, ignore_index: int, class_start_idx: int, total_classes: int) -> None:
    """The gradient overwrites logits.  An op of its own: an output of an op may not alias an input, so this one declares
    logits mutated and returns nothing."""
    _binding().xent_bwd(dloss, logits, labels, lse, logits, smoothing, logit_scale, lse_square_scale, ignore_index,
                        class_start_idx, total_classes)


@_register_fake("flash_attn_amd::_xent_bwd_inplace")
def _xent_bwd_inplace_fake(dloss, logits, labels, lse, smoothing, logit_scale, lse_square_scale, ignore_index, class_start_idx,
                           total_classes):
    return None


def _plan_forward(logits, labels, precomputed_lse=None, smoothing=0.0, logit_scale=1.0, lse_square_scale=0.0, ignore_index=-100,
                  class_start_idx=0, total_classes=None, split=False):
    """The form _xent_fwd takes with these tensors, launching nothing: fa_xent_plan (include/fa_xent.h) as a dict."""
    total_classes = logits.shape[1] if total_classes is None else total_classes
    return _binding().xent_fwd_plan(logits, labels, precomputed_lse, smoothing, logit_scale, lse_square_scale, ignore_index,
                                    class_start_idx, total_classes, split)


def _plan_backward(dloss, logits, labels, lse, dlogits, smoothing=0.0, logit_scale=1.0, lse_square_scale=0.0, ignore_index=-100,
                   class_start_idx=0, total_classes=None):
    """The form the backward takes writing into `dlogits` (logits itself: in place), launching nothing: fa_xent_plan as a dict."""
    total_classes = logits.shape[1] if total_classes is None else total_classes
    return _binding().xent_bwd_plan(dloss, logits, labels, lse, dlogits, smoothing, logit_scale, lse_square_scale, ignore_index,
                                    class_start_idx, total_classes)


# ---- pure torch: the oracle --------------------------------------------------------------------------------------------------
def _working(logits):
    return logits if logits.dtype == torch.float64 else logits.float()


def cross_entropy_ref(logits, labels, precomputed_lse=None, label_smoothing=0.0, logit_scale=1.0, lse_square_scale=0.0,
                      ignore_index=-100, class_start_idx=0, total_classes=None, split=False):
    """The forward contract of include/fa_xent.h in torch: (losses, z_losses, lse), in fp64 where given fp64 and in fp32
    otherwise; differentiable in logits.  logits (M, N) are the columns class_start_idx ... class_start_idx + N of total_classes
    (default N).  With split the losses lack the lse and the z-loss, z_losses are zeros, and lse is that of these columns."""
    x = _working(logits) * logit_scale
    n = x.shape[1]
    total_classes = n if total_classes is None else total_classes
    lse = torch.logsumexp(x, dim=1) if precomputed_lse is None else precomputed_lse.to(x.dtype)
    lab = labels.long() - class_start_idx
    inside = (lab >= 0) & (lab < n)
    x_lab = x.gather(1, lab.clamp(0, n - 1)[:, None])[:, 0]
    base = torch.zeros_like(lse) if split else lse
    mean_x = x.sum(dim=1) / total_classes if label_smoothing > 0 else torch.zeros_like(lse)
    losses = torch.where(inside, base - label_smoothing * mean_x - (1 - label_smoothing) * x_lab,
                         label_smoothing * (base - mean_x) if label_smoothing > 0 else torch.zeros_like(lse))
    z_losses = torch.zeros_like(lse) if split else lse_square_scale * lse.square()
    keep = labels != ignore_index
    zero = torch.zeros_like(lse)
    return torch.where(keep, losses + z_losses, zero), torch.where(keep, z_losses, zero).detach(), lse


def cross_entropy_grad_ref(logits, labels, lse, dloss, label_smoothing=0.0, logit_scale=1.0, lse_square_scale=0.0,
                           ignore_index=-100, class_start_idx=0, total_classes=None):
    """The backward contract of include/fa_xent.h in torch: dlogits (unrounded: fp64 where logits are, else fp32) from the saved
    lse (under a split: the global one).  Rows with the ignore label are zeros whatever their logits hold."""
    x = _working(logits) * logit_scale
    n = x.shape[1]
    total_classes = n if total_classes is None else total_classes
    lse = lse.to(x.dtype)
    p = torch.exp(x - lse[:, None]) * (1 + 2 * lse_square_scale * lse)[:, None]
    lab = labels.long() - class_start_idx
    cols = torch.arange(n, device=x.device)
    p = p - (1 - label_smoothing) * (cols[None, :] == lab[:, None]).to(x.dtype) - label_smoothing / total_classes
    keep = labels != ignore_index
    d = torch.where(keep, dloss.to(x.dtype).expand(x.shape[0]), torch.zeros((), dtype=x.dtype, device=x.device))
    return torch.where(keep[:, None], d[:, None] * logit_scale * p, torch.zeros((), dtype=x.dtype, device=x.device))


# ---- a vocabulary split over ranks --------------------------------------------------------------------------------------------
def _finish_split(losses, lse, labels, lse_square_scale, ignore_index, process_group):
    """What follows the kernel where every rank holds N columns of the vocabulary (reference :217-244): -> (losses, z_losses,
    lse), all global.  `losses` and `lse` (M) are this rank's partials from _xent_fwd with split set; the lse of all ranks are
    gathered and the losses summed over `process_group`.  With process_group None nothing is communicated: `losses` and `lse`
    are then (parts, M), the partials of all parts stacked, and the sum over dim 0 stands in for the collectives.  Works on CPU
    tensors as on device ones."""
    if process_group is not None:
        parts = [torch.empty_like(lse) for _ in range(torch.distributed.get_world_size(process_group))]
        torch.distributed.all_gather(parts, lse.contiguous(), group=process_group)
        lse = torch.stack(parts)
        losses = losses.clone()
        torch.distributed.all_reduce(losses, op=torch.distributed.ReduceOp.SUM, group=process_group)
    else:
        losses = losses.sum(dim=0)
    lse = torch.logsumexp(lse, dim=0)
    keep = labels != ignore_index
    z_losses = (lse_square_scale * lse.square()).masked_fill(~keep, 0.0)
    return (losses + lse).masked_fill(~keep, 0.0) + z_losses, z_losses, lse


# ---- autograd ------------------------------------------------------------------------------------------------------------------
class CrossEntropyLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, labels, precomputed_lse=None, smoothing=0.0, logit_scale=1.0, lse_square_scale=0.0, ignore_index=-100,
                inplace_backward=False, process_group=None):
        if not logit_scale > 0.0:
            raise ValueError("logit_scale must be positive")
        if logits.dim() != 2 or labels.shape != (logits.shape[0],):
            raise ValueError("logits must have shape (batch, vocab_size) and labels (batch,)")
        n_cols = logits.shape[1]
        world_size = 1 if process_group is None else torch.distributed.get_world_size(process_group)
        rank = 0 if process_group is None else torch.distributed.get_rank(process_group)
        ctx.total_classes, ctx.class_start_idx = world_size * n_cols, rank * n_cols
        # (the reference's rule: a precomputed lse is that of the unscaled logits and says nothing of their sum)
        given = precomputed_lse is not None and logit_scale == 1.0 and smoothing == 0.0
        if logits.stride(-1) != 1:
            logits = logits.contiguous()
        labels = labels.contiguous()
        if given:
            if precomputed_lse.shape != labels.shape:
                raise ValueError("precomputed_lse must have shape (batch,)")
            precomputed_lse = precomputed_lse.contiguous().float()
        losses, lse, z_losses = _xent_fwd(logits, labels, precomputed_lse if given else None, smoothing, logit_scale,
                                          lse_square_scale, ignore_index, ctx.class_start_idx, ctx.total_classes, world_size > 1)
        if given:
            lse = precomputed_lse
        if world_size > 1:
            losses, z_losses, lse = _finish_split(losses, lse, labels, lse_square_scale, ignore_index, process_group)
        ctx.save_for_backward(logits, lse, labels)
        ctx.mark_non_differentiable(z_losses)
        ctx.args = (smoothing, logit_scale, lse_square_scale, ignore_index, ctx.class_start_idx, ctx.total_classes)
        ctx.inplace_backward = inplace_backward
        return losses, z_losses

    @staticmethod
    def backward(ctx, grad_losses, grad_z_losses):
        del grad_z_losses  # (z_losses are for logging)
        logits, lse, labels = ctx.saved_tensors
        grad_losses = grad_losses.float()  # (as it comes: the gradient of losses.sum() is an expanded scalar of stride 0)
        if ctx.inplace_backward:
            _xent_bwd_inplace(grad_losses, logits, labels, lse, *ctx.args)
            dlogits = logits
        else:
            dlogits = _xent_bwd(grad_losses, logits, labels, lse, *ctx.args)
        return dlogits, None, None, None, None, None, None, None, None


def cross_entropy_loss(logits: Tensor, labels: Tensor, precomputed_lse: Optional[Tensor] = None, label_smoothing: float = 0.0,
                       logit_scale: float = 1.0, lse_square_scale: float = 0.0, ignore_index=-100, inplace_backward: bool = False,
                       process_group=None) -> Tuple[Tensor, Tensor]:
    """Per-row cross-entropy of logits (batch, vocab_size) in fp16 / bf16 / fp32, any row stride, against labels (batch,) in
    int64 / int32: the logits are read once forward and read and written once backward.

    logit_scale multiplies the logits first; lse_square_scale > 0 adds the z-loss lse_square_scale * lse^2; rows whose label is
    ignore_index lose nothing and get a zero gradient; precomputed_lse (batch,), used where logit_scale == 1 and
    label_smoothing == 0, spares the forward its read of the logits; inplace_backward writes the gradient over the logits;
    process_group: every rank holds vocab_size columns of the vocabulary, and the losses are those over all of it.
    Returns (losses, z_losses), fp32 (batch,); z_losses is the z-loss part of losses and is not differentiable."""
    return CrossEntropyLoss.apply(logits, labels, precomputed_lse, label_smoothing, logit_scale, lse_square_scale, ignore_index,
                                  inplace_backward, process_group)
