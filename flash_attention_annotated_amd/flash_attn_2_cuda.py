"""Extension-module surface the reference's Python API binds to: `flash_attn_2_cuda`.

`flash_attn/flash_attn_interface.py:15` does `import flash_attn_2_cuda as flash_attn_gpu`
and calls `.fwd` (:91), `.varlen_fwd` (:168), `.bwd` (:269), `.varlen_bwd` (:369) and
`.fwd_kvcache` (:1594).  These five names, and `_fwd_kvcache_impl` with the page-size rule of the calling surface, are
the functions of the compiled pybind module `flash_attn_2_cuda_C` (the pybind module of
`csrc/flash_attn/flash_api.cpp:1478-1485`, built by `_lib.build()`).  The FA2 host logic -- checks with the reference's
`TORCH_CHECK` texts, output allocation, params, the kernel launches through the C-ABI on torch's current stream -- lives
only in `csrc/torch_binding.cpp`.

The binding is resolved on first access to one of those names (`_lib.binding()`), so that the package imports before
anything is built.  A binding that does not load raises ImportError: there is no other host path.
"""
from . import _lib

__all__ = ["fwd", "varlen_fwd", "bwd", "varlen_bwd", "fwd_kvcache"]

_NAMES = ("fwd", "varlen_fwd", "bwd", "varlen_bwd", "fwd_kvcache", "_fwd_kvcache_impl")


def __getattr__(name):
    if name not in _NAMES:
        raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
    binding = _lib.binding()
    # bound as plain module attributes: later lookups never come back here, and no wrapper sits in the call path
    globals().update((n, getattr(binding, n)) for n in _NAMES)
    return globals()[name]
