"""`flash_attn.utils` by name: generation.py holds the step from logits to the next token and the verification of draft tokens (HIP kernels, csrc/fa_sample.hip and csrc/fa_spec_sample.hip)."""
