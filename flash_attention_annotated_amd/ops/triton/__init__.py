"""The reference's import path of the fused norm (flash_attn.ops.triton.layer_norm); the kernels behind it are HIP."""
