"""The reference's import paths of the fused norm (flash_attn.ops.triton.layer_norm), of the fused cross-entropy loss
(flash_attn.ops.triton.cross_entropy) and of the GEMM with a fused bias + activation epilogue (flash_attn.ops.triton.linear,
flash_attn.ops.triton.mlp); the kernels behind them are HIP."""
