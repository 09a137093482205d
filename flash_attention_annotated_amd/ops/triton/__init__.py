"""The reference's import paths of the fused norm (flash_attn.ops.triton.layer_norm) and of the fused cross-entropy loss
(flash_attn.ops.triton.cross_entropy); the kernels behind them are HIP."""
