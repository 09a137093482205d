"""`flash_attn.ops.triton.layer_norm` by name: the fused residual-add + LayerNorm / RMSNorm of ops/norm.py (HIP kernels, not
Triton; the path is the one model code imports from)."""
from ..norm import (LayerNormFn, LayerNormLinearFn, RMSNorm, layer_norm_fn, layer_norm_linear_fn, layer_norm_ref, rms_norm_fn,
                    rms_norm_ref)

__all__ = ["layer_norm_fn", "rms_norm_fn", "LayerNormFn", "RMSNorm", "layer_norm_ref", "rms_norm_ref", "LayerNormLinearFn",
           "layer_norm_linear_fn"]
