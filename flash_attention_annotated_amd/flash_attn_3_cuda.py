"""FA3 operator surface: `flash_attn_3::fwd` (hopper/flash_api.cpp:672-1198; schema :1672-1707), as the Python
callable `hopper/flash_attn_interface.py:66` invokes — 34 positional arguments, returns
(out, softmax_lse, out_accum, softmax_lse_accum).

`fwd` is the compiled binding's `fa3_fwd` itself (csrc/torch_binding.cpp: the checks, the KV-cache / decode / dense /
varlen routes, fp8 descales, the FA3 window rule), resolved on first access through `_lib.binding()` like the names of
flash_attn_2_cuda.py.  `bwd`, `fwd_combine` and `get_scheduler_metadata` go through the `torch.ops.flash_attn_3` library
that flash_attn_3_ops.py registers.
"""
import torch

from . import _lib

__all__ = ["fwd", "bwd", "fwd_combine", "get_scheduler_metadata"]


def __getattr__(name):
    if name != "fwd":
        raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
    globals()["fwd"] = _lib.binding().fa3_fwd  # a plain module attribute from here on: no wrapper in the call path
    return globals()["fwd"]


def bwd(*args, **kwargs):
    """flash_attn_3::bwd (hopper/flash_api.cpp:1259-1570): see flash_attn_3_ops._bwd."""
    from . import flash_attn_3_ops  # noqa: F401
    return torch.ops.flash_attn_3.bwd(*args, **kwargs)


def fwd_combine(out_partial, lse_partial, out=None, out_dtype=None):
    """flash_attn_3::fwd_combine (hopper/flash_api.cpp:1569-1670): see flash_attn_3_ops._fwd_combine."""
    from . import flash_attn_3_ops  # noqa: F401
    return torch.ops.flash_attn_3.fwd_combine(out_partial, lse_partial, out, out_dtype)


def get_scheduler_metadata(*args, **kwargs):
    """flash_attn_3::get_scheduler_metadata: opaque and empty in this build (tiles are scheduled inside the kernel)."""
    from . import flash_attn_3_ops  # noqa: F401
    return torch.ops.flash_attn_3.get_scheduler_metadata(*args, **kwargs)
