"""`flash_attn.utils` by name: generation.py holds the step from logits to the next token (HIP kernels, csrc/fa_sample.hip)."""
