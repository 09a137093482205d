"""The kernels of tree attention over a KV cache (a plain module, not collected): every instantiation of tr_fwd_kernel
(csrc/fa_fwd_kernel_tr.h) as the plan text of fa_fwd_tree names it, and as parity_helpers.plan_key keys it.  tests/test_tree_abi.py
holds the translation unit to this set, tests/test_tree_gpu.py the set of keys its parity cases launched."""
from parity_helpers import plan_key

DTYPES = ("bf16", "fp16")
TILES = (64, 128)


def plan_text(tile, softcap, fp8, splits=1):
    return f"tr_fwd_kernel D={tile} waves=4{' SOFTCAP' if softcap else ''} KV={'e4m3' if fp8 else '16'} block_m=128 splits={splits}"


# (element type, head-dim tile, SOFTCAP, e4m3 cache): the 16 instantiations
INSTANTIATIONS = [(dt, tile, softcap, fp8) for dt in DTYPES for tile in TILES for softcap in (False, True) for fp8 in (False, True)]


def instantiation_key(dt, tile, softcap, fp8):
    """plan_key without its epilogue: the split and the unsplit launch of an instantiation are the same kernel."""
    return plan_key(plan_text(tile, softcap, fp8), dt)[:2]


UNIVERSE = {instantiation_key(*i) for i in INSTANTIATIONS}
