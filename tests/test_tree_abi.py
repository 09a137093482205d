"""CPU tests of tree attention over a KV cache (include/fa_fwd.h: fa_fwd_tree_validate, fa_fwd_tree_plan_name,
fa_fwd_tree_workspace_size) and of the device code of its translation unit, csrc/fa_fwd_tree_api.hip.  Nothing here touches a
device; tests/test_tree_gpu.py checks what the kernel computes, tests/test_tree_ref.py the torch helpers beside it."""
import re

import pytest

from flash_attention_annotated_amd import _lib
import tree_plan_universe as universe

ADDR = 0x10000  # an aligned dummy address: nothing is dereferenced
OK, NULLP, BAD_DTYPE, BAD_HEAD_DIM, BAD_HEADS, BAD_SHAPE, BAD_STRIDE, UNSUPPORTED, BAD_ABI, WORKSPACE = 0, -1, -2, -3, -4, -5, -6, -7, -9, -11
FP8 = _lib.FA_DTYPE_FP8_E4M3


def _params(b=2, h=8, h_k=2, sq=16, sk=640, d=128, dtype=_lib.FA_DTYPE_BF16, fp8_cache=False, **fields):
    """Dense q (b, sq, h, d) over a dense cache (b, sk, h_k, d), 16-bit elements or e4m3 bytes + descales; a dummy workspace."""
    p = _lib.new_params()
    for f in ("q", "k", "v", "o", "softmax_lse", "workspace"):
        setattr(p, f, ADDR)
    if fp8_cache:
        p.k_descale = p.v_descale = ADDR
        p.k_descale_batch_stride = p.v_descale_batch_stride = h_k
        p.k_descale_head_stride = p.v_descale_head_stride = 1
    p.workspace_bytes = 1 << 40
    p.b, p.seqlen_q, p.seqlen_k, p.h, p.h_k, p.d, p.dtype = b, sq, sk, h, h_k, d, dtype
    for t, rows, heads in (("q", sq, h), ("k", sk, h_k), ("v", sk, h_k), ("o", sq, h)):
        setattr(p, f"{t}_head_stride", d)
        setattr(p, f"{t}_row_stride", heads * d)
        setattr(p, f"{t}_batch_stride", rows * heads * d)
    p.softmax_scale = d ** -0.5
    p.window_size_left = p.window_size_right = -1
    p.num_splits = 1
    for k, v in fields.items():
        setattr(p, k, v)
    return p


def _tree(sq=16, fp8_cache=False, **fields):
    t = _lib.new_tree_params()
    t.tree_mask, t.batch_stride, t.row_stride, t.fp8_cache = ADDR, sq, 1, int(fp8_cache)
    for k, v in fields.items():
        setattr(t, k, v)
    return t


def _pair(params=None, tree=None, fp8_cache=False):
    params = params or {}
    return _params(fp8_cache=fp8_cache, **params), _tree(sq=params.get("sq", 16), fp8_cache=fp8_cache, **(tree or {}))


VALIDATE = [
    # accepted forms
    ("bf16", _pair(), OK),
    ("fp16", _pair(dict(dtype=_lib.FA_DTYPE_FP16)), OK),
    ("fp8_cache", _pair(fp8_cache=True), OK),
    ("fp8_cache_fp16", _pair(dict(dtype=_lib.FA_DTYPE_FP16), fp8_cache=True), OK),
    ("T64", _pair(dict(sq=64)), OK),
    ("T1", _pair(dict(sq=1)), OK),
    ("d64", _pair(dict(d=64)), OK),
    ("d96", _pair(dict(d=96)), OK),
    ("d_v_same", _pair(dict(d_v=128)), OK),
    ("softcap", _pair(dict(softcap=30.0)), OK),
    ("strided_words", _pair(tree=dict(batch_stride=200, row_stride=3)), OK),
    ("ragged", _pair(dict(cu_seqlens_q=ADDR, seqused_k=ADDR, total_q=14, sq=13, b=2)), OK),
    ("paged_64", _pair(dict(block_table=ADDR, page_block_size=64, block_table_batch_stride=16)), OK),
    ("paged_16_fp8", _pair(dict(block_table=ADDR, page_block_size=16, block_table_batch_stride=16), fp8_cache=True), OK),
    ("batch_idx_leftpad", _pair(dict(kv_batch_idx=ADDR, leftpad_k=ADDR, seqused_k=ADDR)), OK),
    ("empty_cache", _pair(dict(sk=0)), OK),
    # the refusals of the route, one row each
    ("T65", _pair(dict(sq=65)), UNSUPPORTED),
    ("ragged_bound_65", _pair(dict(cu_seqlens_q=ADDR, seqused_k=ADDR, total_q=70, sq=65, b=2)), UNSUPPORTED),
    ("causal", _pair(dict(is_causal=1)), UNSUPPORTED),
    ("window_left", _pair(dict(window_size_left=100)), UNSUPPORTED),
    ("window_right", _pair(dict(window_size_right=0)), UNSUPPORTED),
    ("chunk", _pair(dict(attention_chunk=64)), UNSUPPORTED),
    ("qv", _pair(dict(qv=ADDR)), UNSUPPORTED),
    ("alibi", _pair(dict(alibi_slopes=ADDR)), UNSUPPORTED),
    ("dropout", _pair(dict(p_dropout=0.1, rng_state=ADDR)), UNSUPPORTED),
    ("cu_seqlens_k", _pair(dict(cu_seqlens_q=ADDR, cu_seqlens_k=ADDR, seqused_k=ADDR, total_q=2)), UNSUPPORTED),
    ("d192", _pair(dict(d=192)), UNSUPPORTED),
    ("d72", _pair(dict(d=72)), UNSUPPORTED),
    ("d_v_own", _pair(dict(d_v=64)), UNSUPPORTED),
    ("all_fp8", _pair(dict(dtype=FP8), fp8_cache=True), UNSUPPORTED),
    # (a learnable sink and a rotary table have no way in: test_tree_has_no_sink_or_rotary_argument)
    # what is unsupported is said before what the params lack
    ("unsupported_first", _pair(dict(is_causal=1, q=0, h=7)), UNSUPPORTED),
    # the rest
    ("null_words", _pair(tree=dict(tree_mask=0)), NULLP),
    ("words_pointer", _pair(tree=dict(tree_mask=ADDR + 4)), BAD_STRIDE),
    ("words_stride_negative", _pair(tree=dict(row_stride=-1)), BAD_STRIDE),
    ("fp32_q", _pair(dict(dtype=_lib.FA_DTYPE_FP32)), BAD_DTYPE),
    ("fp8_cache_without_descales", _pair(dict(v_descale=0), fp8_cache=True), NULLP),
    ("fp8_cache_k_stride_8", _pair(dict(k_head_stride=136), fp8_cache=True), BAD_STRIDE),  # bytes there
    ("k_stride_8_16bit", _pair(dict(k_head_stride=136)), OK),  # 16 bytes = 8 16-bit elements
    ("heads", _pair(dict(h=7)), BAD_HEADS),
    ("null_q", _pair(dict(q=0)), NULLP),
    ("ragged_without_fill_levels", _pair(dict(cu_seqlens_q=ADDR, total_q=14, sq=13, b=2)), BAD_SHAPE),
    ("paged_batch_idx", _pair(dict(block_table=ADDR, page_block_size=64, block_table_batch_stride=16, kv_batch_idx=ADDR)), UNSUPPORTED),
    ("k_row_stride_2_24", _pair(dict(k_row_stride=1 << 24)), BAD_STRIDE),
    ("splits_negative", _pair(dict(num_splits=-1)), BAD_SHAPE),
    ("splits_without_workspace", _pair(dict(num_splits=3, workspace=0)), WORKSPACE),
    ("splits_small_workspace", _pair(dict(num_splits=3, workspace_bytes=1024), fp8_cache=True), WORKSPACE),
    ("unsplit_without_workspace", _pair(dict(num_splits=1, workspace=0)), OK),
]


@pytest.mark.parametrize("name,pair,status", VALIDATE, ids=[r[0] for r in VALIDATE])
def test_tree_validate(name, pair, status):
    """fa_fwd_tree_plan_name is NULL exactly when the validation rejects."""
    p, t = pair
    lib = _lib.load()
    assert lib.fa_fwd_tree_validate(p, t) == status
    assert (lib.fa_fwd_tree_plan_name(p, t, 256) is None) == (status != OK)


def test_tree_validate_null_and_abi():
    lib = _lib.load()
    p, t = _pair()
    assert lib.fa_fwd_tree_validate(None, t) == NULLP
    assert lib.fa_fwd_tree_validate(p, None) == NULLP
    t.struct_size -= 8
    assert lib.fa_fwd_tree_validate(p, t) == BAD_ABI
    assert lib.fa_fwd_tree_workspace_size(p, t) == BAD_ABI
    assert lib.fa_fwd_tree_plan_name(p, t, 256) is None
    p, t = _pair()
    p.abi_version = 12
    assert lib.fa_fwd_tree_validate(p, t) == BAD_ABI
    p, t = _pair()
    t.abi_version = 12
    assert lib.fa_fwd_tree_validate(p, t) == BAD_ABI


def test_tree_struct_and_symbols():
    lib = _lib.load()
    for name in ("fa_fwd_tree", "fa_fwd_tree_validate", "fa_fwd_tree_workspace_size", "fa_fwd_tree_plan_name", "fa_tree_params_size"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert lib.fa_tree_params_size() == 40
    assert [n for n, _ in _lib.FaTreeParams._fields_] == ["abi_version", "struct_size", "tree_mask", "batch_stride", "row_stride",
                                                         "fp8_cache", "reserved"]
    assert lib.fa_abi_version() == 13 == _lib.FA_ABI_VERSION


def test_tree_has_no_sink_or_rotary_argument():
    """A learnable sink and a rotary table cannot reach this route: its entry points take fa_fwd_params (which has neither) and
    the words."""
    lib = _lib.load()
    assert len(lib.fa_fwd_tree.argtypes) == 3 and len(lib.fa_fwd_tree_validate.argtypes) == 2
    assert _lib.FaSinkParams not in [getattr(a, "_type_", None) for a in lib.fa_fwd_tree.argtypes]
    assert not any("sink" in n or "rotary" in n for n, _ in _lib.FaTreeParams._fields_ + _lib.FaFwdParams._fields_)


def _inst_pair(dt, tile, softcap, fp8, **params):
    dtype = _lib.FA_DTYPE_BF16 if dt == "bf16" else _lib.FA_DTYPE_FP16
    return _pair(dict(dtype=dtype, d=tile, softcap=30.0 if softcap else 0.0, **params), fp8_cache=fp8)


@pytest.mark.parametrize("inst", universe.INSTANTIATIONS, ids=["-".join(map(str, i)) for i in universe.INSTANTIATIONS])
def test_tree_plan_name_of_every_instantiation(inst):
    dt, tile, softcap, fp8 = inst
    lib = _lib.load()
    p, t = _inst_pair(*inst)
    assert lib.fa_fwd_tree_plan_name(p, t, 256).decode() == universe.plan_text(tile, softcap, fp8)
    assert lib.fa_fwd_tree_plan_name(p, t, 64).decode() == universe.plan_text(tile, softcap, fp8)  # the CU count decides nothing
    p, t = _inst_pair(*inst, num_splits=3)
    assert lib.fa_fwd_tree_plan_name(p, t, 256).decode() == universe.plan_text(tile, softcap, fp8, splits=3)


PLANS = [
    ("d96_is_tile_128", _pair(dict(d=96)), universe.plan_text(128, False, False)),
    ("d48_is_tile_64", _pair(dict(d=48)), universe.plan_text(64, False, False)),
    # N parts never exceed the 64-key tiles of the capacity: 640 keys = 10 tiles
    ("splits_clamped", _pair(dict(num_splits=99)), universe.plan_text(128, False, False, splits=10)),
    ("empty_cache_still_runs", _pair(dict(sk=0, num_splits=4)), universe.plan_text(128, False, False)),
    # the heuristic splits from 8 key tiles on: 4 tiles stay whole (test_tree_heuristic_equals_the_pk_plan has the long ones)
    ("heuristic_short_cache", _pair(dict(sk=256, num_splits=0)), universe.plan_text(128, False, False)),
]


@pytest.mark.parametrize("name,pair,plan", PLANS, ids=[r[0] for r in PLANS])
def test_tree_plan_name(name, pair, plan):
    p, t = pair
    assert _lib.load().fa_fwd_tree_plan_name(p, t, 256).decode() == plan


def test_tree_heuristic_equals_the_pk_plan():
    """num_splits = 0 is fwd_pk_split_count: the 16-bit causal fa_fwd call with FA_FLAG_PACK_GQA on the same shapes plans the
    same parts, for both cache types -- from shapes only."""
    lib = _lib.load()
    for b, sq, sk in ((1, 16, 8192), (1, 64, 32768), (8, 16, 8192), (64, 64, 32768), (2, 13, 512)):
        for fp8_cache in (False, True):
            p, t = _pair(dict(b=b, h=32, h_k=8, sq=sq, sk=sk, num_splits=0), fp8_cache=fp8_cache)
            n = re.search(r"splits=(\d+)", lib.fa_fwd_tree_plan_name(p, t, 256).decode()).group(1)
            p16 = _params(b=b, h=32, h_k=8, sq=sq, sk=sk, num_splits=0, is_causal=1, flags=_lib.FA_FLAG_PACK_GQA)
            name16 = lib.fa_fwd_plan_name(p16, 256).decode()
            assert name16.startswith("pk_fwd_kernel") and re.search(r"splits=(\d+)", name16).group(1) == n, (b, sq, sk, name16, n)


def _align256(x):
    return (x + 255) & ~255


def test_tree_workspace_size():
    """0 unsplit; split: the fp32 partials fa_fwd_combine merges -- O (splits, b, sq, h, d) and LSE (splits, b, h, sq), each
    rounded up to 256 bytes; ragged queries count total_q rows.  The same for both cache types."""
    lib = _lib.load()
    for fp8_cache in (False, True):
        assert lib.fa_fwd_tree_workspace_size(*_pair(fp8_cache=fp8_cache)) == 0
        assert lib.fa_fwd_tree_workspace_size(*_pair(dict(sq=0, num_splits=3), fp8_cache=fp8_cache)) == 0
        pair = _pair(dict(b=2, h=8, h_k=2, sq=13, d=80, num_splits=3), fp8_cache=fp8_cache)
        assert lib.fa_fwd_tree_workspace_size(*pair) == _align256(3 * 2 * 13 * 8 * 80 * 4) + _align256(3 * 2 * 13 * 8 * 4)
        pair = _pair(dict(cu_seqlens_q=ADDR, seqused_k=ADDR, total_q=14, sq=13, b=2, num_splits=2), fp8_cache=fp8_cache)
        assert lib.fa_fwd_tree_workspace_size(*pair) == _align256(2 * 14 * 8 * 128 * 4) + _align256(2 * 14 * 8 * 4)
    assert lib.fa_fwd_tree_workspace_size(*_pair(dict(dtype=FP8))) == UNSUPPORTED
    assert lib.fa_fwd_tree_workspace_size(*_pair(dict(sq=65))) == UNSUPPORTED
    assert lib.fa_fwd_tree_workspace_size(*_pair(dict(is_causal=1))) == UNSUPPORTED
    assert lib.fa_fwd_tree_workspace_size(None, None) == NULLP


def test_tree_instantiations_and_no_scratch():
    """The translation unit holds exactly {bf16, fp16} x {64, 128} x {plain, SOFTCAP} x {Kv16, Kv8} of tr_fwd_kernel and nothing
    else (the merge is fa_fwd_combine's kernel, in fa_fwd_api.hip), and none of them has a private segment: nothing spills."""
    from device_asm import TYPES, kernel_bodies
    kernels = {}
    for sym, body in kernel_bodies("fa_fwd_tree_api.hip"):
        k = re.match(r"_ZN2fa13tr_fwd_kernelI(DF16b|DF16_)Li(\d+)ELb([01])ENS_(?:4Kv16|3Kv8)I(DF16b|DF16_)Li(\d+)EEEEEvNS_8TrParamsE$", sym)
        assert k, f"a kernel in fa_fwd_tree_api.hip that is no tr_fwd_kernel: {sym}"
        assert k.group(1) == k.group(4) and k.group(2) == k.group(5), sym  # the tile policy of the kernel's own T and D
        key = (TYPES[k.group(1)], int(k.group(2)), bool(int(k.group(3))), "3Kv8" in sym)
        assert key not in kernels
        kernels[key] = int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body).group(1))
    assert set(kernels) == set(universe.INSTANTIATIONS) and len(kernels) == 16
    assert all(v == 0 for v in kernels.values()), kernels
