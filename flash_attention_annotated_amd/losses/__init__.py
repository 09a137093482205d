"""Losses of the reference's `flash_attn.losses` that this package provides: `cross_entropy`."""
