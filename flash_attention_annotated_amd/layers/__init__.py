"""Layers of the reference's `flash_attn.layers` that this package provides: `rotary`."""
