"""Extension-module surface the reference's Python API binds to: `flash_attn_2_cuda`.

`flash_attn/flash_attn_interface.py:15` does `import flash_attn_2_cuda as flash_attn_gpu`
and calls `.fwd` (:91), `.varlen_fwd` (:168), `.bwd` (:269), `.varlen_bwd` (:369) and
`.fwd_kvcache` (:1594).  These five names, and `_fwd_kvcache_impl` that the FA3 surface calls, are the functions of the
compiled pybind module `flash_attn_2_cuda_C` (the pybind module of `csrc/flash_attn/flash_api.cpp:1478-1485`, built by
`_lib.build()`).  The FA2 host logic -- checks with the reference's `TORCH_CHECK` texts, output allocation, params, the
kernel launches through the C-ABI on torch's current stream -- lives only in `csrc/torch_binding.cpp`.

The binding is resolved on first access to one of those names, so that the package imports before anything is built.
A binding that does not load raises ImportError: there is no other host path.
"""
import contextlib

from . import _lib

__all__ = ["fwd", "varlen_fwd", "bwd", "varlen_bwd", "fwd_kvcache"]

_NAMES = ("fwd", "varlen_fwd", "bwd", "varlen_bwd", "fwd_kvcache", "_fwd_kvcache_impl")


def _binding():
    try:
        from . import flash_attn_2_cuda_C
    except ImportError as e:
        raise ImportError(
            f"flash_attn_2_cuda_C is not built or does not load ({e}): run `python -c 'import __graft_entry__ as g; "
            f"g.build()'` (expected at {_lib.binding_path()}); there is no CPU fallback") from e
    # ABI / struct-layout checks and the FA_FWD_* developer overrides, applied to the library instance the binding links
    # (the dynamic loader maps libfa_fwd_gfx950.so once); after the import, so that an unbuilt tree raises ImportError
    _lib.load()
    return flash_attn_2_cuda_C


def __getattr__(name):
    if name not in _NAMES:
        raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
    binding = _binding()
    # bound as plain module attributes: later lookups never come back here, and no wrapper sits in the call path
    globals().update((n, getattr(binding, n)) for n in _NAMES)
    return globals()[name]


@contextlib.contextmanager
def fa3_window_rule():
    """The FA3 operator surface (flash_attn_3_ops._bwd) runs its backward through bwd / varlen_bwd with ITS window rule
    (a missing side is unbounded, include/fa_fwd.h FA_FLAG_FA3_WINDOW); the reference signatures have no room for that
    switch.  The flag is thread-local in the binding; nested use keeps the outer rule."""
    binding = _binding()
    prev = binding._set_fa3_window_rule(True)
    try:
        yield
    finally:
        binding._set_fa3_window_rule(prev)
