"""Fused operators beside the attention functions, under the reference's import paths (flash_attn.ops.*)."""
