"""CPU tests of the block-sparse forward over a KV cache (include/fa_fwd.h: fa_fwd_sparse_kv_validate,
fa_fwd_sparse_kv_plan_name, fa_fwd_sparse_kv_workspace_size), of the device code of its translation unit,
csrc/fa_fwd_sparse_kv_api.hip, and of the oracle the GPU tests use (tests/sparse_kv_oracle.py).  Nothing here touches a device;
tests/test_sparse_kv_gpu.py checks what the kernel computes."""
import re

import pytest
import torch

from flash_attention_annotated_amd import _lib
from oracle import attention_ref as oracle
import sparse_kv_oracle

ADDR = 0x10000  # an aligned dummy address: nothing is dereferenced
OK, NULLP, BAD_DTYPE, BAD_HEAD_DIM, BAD_HEADS, BAD_SHAPE, BAD_STRIDE, UNSUPPORTED, BAD_ABI, WORKSPACE = 0, -1, -2, -3, -4, -5, -6, -7, -9, -11
FP8 = _lib.FA_DTYPE_FP8_E4M3


def _params(b=2, h=8, h_k=2, sq=1, sk=640, d=128, dtype=_lib.FA_DTYPE_BF16, fp8_cache=False, **fields):
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


def _lists(b=2, h_k=2, max_blocks=5, block=128, fp8_cache=False, **fields):
    s = _lib.new_sparse_kv_params()
    s.block_cnt = s.block_idx = ADDR
    s.cnt_batch_stride, s.cnt_head_stride = h_k, 1
    s.idx_batch_stride, s.idx_head_stride = h_k * max_blocks, max_blocks
    s.max_blocks, s.block_size, s.fp8_cache = max_blocks, block, int(fp8_cache)
    for k, v in fields.items():
        setattr(s, k, v)
    return s


def _pair(params=None, lists=None, fp8_cache=False):
    return _params(fp8_cache=fp8_cache, **(params or {})), _lists(fp8_cache=fp8_cache, **(lists or {}))


VALIDATE = [
    # accepted forms
    ("bf16", _pair(), OK),
    ("fp16", _pair(dict(dtype=_lib.FA_DTYPE_FP16)), OK),
    ("fp8_cache", _pair(fp8_cache=True), OK),
    ("fp8_cache_fp16", _pair(dict(dtype=_lib.FA_DTYPE_FP16), fp8_cache=True), OK),
    ("B64", _pair(lists=dict(block=64)), OK),
    ("B256", _pair(lists=dict(block=256)), OK),
    ("B192", _pair(lists=dict(block=192)), OK),
    ("broadcast_lists", _pair(lists=dict(cnt_batch_stride=0, cnt_head_stride=0, idx_batch_stride=0, idx_head_stride=0)), OK),
    ("max_blocks_0", _pair(lists=dict(max_blocks=0)), OK),
    ("d64", _pair(dict(d=64)), OK),
    ("d80", _pair(dict(d=80)), OK),
    ("ragged", _pair(dict(cu_seqlens_q=ADDR, seqused_k=ADDR, total_q=6, sq=4, b=3)), OK),
    ("paged_64", _pair(dict(block_table=ADDR, page_block_size=64, block_table_batch_stride=16)), OK),
    ("paged_16_fp8", _pair(dict(block_table=ADDR, page_block_size=16, block_table_batch_stride=16), fp8_cache=True), OK),
    ("batch_idx_leftpad", _pair(dict(kv_batch_idx=ADDR, leftpad_k=ADDR, seqused_k=ADDR)), OK),
    ("causal_window_softcap", _pair(dict(is_causal=1, window_size_left=100, softcap=30.0)), OK),
    ("k_stride_8_16bit", _pair(dict(k_head_stride=136)), OK),  # 16 bytes = 8 16-bit elements
    # the refusals of the issue, one row each
    ("B_not_multiple", _pair(lists=dict(block=96)), BAD_SHAPE),
    ("B_zero", _pair(lists=dict(block=0)), BAD_SHAPE),
    ("B_negative", _pair(lists=dict(block=-128)), BAD_SHAPE),
    ("max_blocks_negative", _pair(lists=dict(max_blocks=-1)), BAD_SHAPE),
    ("max_blocks_times_B_overflows", _pair(lists=dict(max_blocks=1 << 24, block=128)), BAD_SHAPE),
    ("null_cnt", _pair(lists=dict(block_cnt=0)), NULLP),
    ("null_idx", _pair(lists=dict(block_idx=0)), NULLP),
    ("d192", _pair(dict(d=192)), UNSUPPORTED),
    ("d72", _pair(dict(d=72)), UNSUPPORTED),
    ("all_fp8", _pair(dict(dtype=FP8), fp8_cache=True), UNSUPPORTED),
    ("qv", _pair(dict(qv=ADDR)), UNSUPPORTED),
    ("d_v_own", _pair(dict(d_v=64)), UNSUPPORTED),
    ("d_v_same", _pair(dict(d_v=128)), OK),
    ("alibi", _pair(dict(alibi_slopes=ADDR)), UNSUPPORTED),
    ("dropout", _pair(dict(p_dropout=0.1, rng_state=ADDR)), UNSUPPORTED),
    ("chunk", _pair(dict(attention_chunk=64)), UNSUPPORTED),
    ("cu_seqlens_k", _pair(dict(cu_seqlens_q=ADDR, cu_seqlens_k=ADDR, seqused_k=ADDR, total_q=2)), UNSUPPORTED),
    # (a learnable sink has no way in: the entry point takes no fa_sink_params, test_sparse_kv_has_no_sink_argument)
    # what is unsupported is said before what the params lack
    ("unsupported_first", _pair(dict(d=192, q=0, h=7)), UNSUPPORTED),
    # the rest
    ("fp32_q", _pair(dict(dtype=_lib.FA_DTYPE_FP32)), BAD_DTYPE),
    ("fp8_cache_without_descales", _pair(dict(k_descale=0), fp8_cache=True), NULLP),
    ("fp8_cache_k_stride_8", _pair(dict(k_head_stride=136), fp8_cache=True), BAD_STRIDE),  # bytes there
    ("list_stride_negative", _pair(lists=dict(idx_head_stride=-1)), BAD_STRIDE),
    ("list_pointer", _pair(lists=dict(block_idx=ADDR + 2)), BAD_STRIDE),
    ("heads", _pair(dict(h=7)), BAD_HEADS),
    ("null_q", _pair(dict(q=0)), NULLP),
    ("ragged_without_fill_levels", _pair(dict(cu_seqlens_q=ADDR, total_q=6, sq=4, b=3)), BAD_SHAPE),
    ("paged_batch_idx", _pair(dict(block_table=ADDR, page_block_size=64, block_table_batch_stride=16, kv_batch_idx=ADDR)), UNSUPPORTED),
    ("k_row_stride_2_24", _pair(dict(k_row_stride=1 << 24)), BAD_STRIDE),
    ("splits_negative", _pair(dict(num_splits=-1)), BAD_SHAPE),
    ("splits_without_workspace", _pair(dict(num_splits=3, workspace=0)), WORKSPACE),
    ("splits_small_workspace", _pair(dict(num_splits=3, workspace_bytes=1024), fp8_cache=True), WORKSPACE),
]


@pytest.mark.parametrize("name,pair,status", VALIDATE, ids=[r[0] for r in VALIDATE])
def test_sparse_kv_validate(name, pair, status):
    p, s = pair
    lib = _lib.load()
    assert lib.fa_fwd_sparse_kv_validate(p, s) == status
    if status != OK:
        assert lib.fa_fwd_sparse_kv_plan_name(p, s, 256) is None


def test_sparse_kv_validate_null_and_abi():
    lib = _lib.load()
    p, s = _pair()
    assert lib.fa_fwd_sparse_kv_validate(None, s) == NULLP
    assert lib.fa_fwd_sparse_kv_validate(p, None) == NULLP
    s.struct_size -= 8
    assert lib.fa_fwd_sparse_kv_validate(p, s) == BAD_ABI
    assert lib.fa_fwd_sparse_kv_workspace_size(p, s) == BAD_ABI
    p, s = _pair()
    p.abi_version = 12
    assert lib.fa_fwd_sparse_kv_validate(p, s) == BAD_ABI


def test_sparse_kv_has_no_sink_argument():
    """A learnable sink cannot reach this route: its entry points take fa_fwd_params (which has no sink field) and the lists."""
    lib = _lib.load()
    assert len(lib.fa_fwd_sparse_kv.argtypes) == 3 and len(lib.fa_fwd_sparse_kv_validate.argtypes) == 2
    assert _lib.FaSinkParams not in [getattr(a, "_type_", None) for a in lib.fa_fwd_sparse_kv.argtypes]
    assert not any("sink" in n for n, _ in _lib.FaSparseKvParams._fields_)


PLANS = [
    ("decode", _pair(), "sp_fwd_kernel D=128 waves=4 KV=16 B=128 block_m=128 splits=1"),
    ("fp8", _pair(fp8_cache=True), "sp_fwd_kernel D=128 waves=4 KV=e4m3 B=128 block_m=128 splits=1"),
    ("fp16_B64", _pair(dict(dtype=_lib.FA_DTYPE_FP16), dict(block=64)), "sp_fwd_kernel D=128 waves=4 KV=16 B=64 block_m=128 splits=1"),
    ("d64_B256", _pair(dict(d=64), dict(block=256)), "sp_fwd_kernel D=64 waves=4 KV=16 B=256 block_m=128 splits=1"),
    ("d80", _pair(dict(d=80)), "sp_fwd_kernel D=128 waves=4 KV=16 B=128 block_m=128 splits=1"),
    ("softcap_fp8", _pair(dict(softcap=30.0), fp8_cache=True), "sp_fwd_kernel D=128 waves=4 SOFTCAP KV=e4m3 B=128 block_m=128 splits=1"),
    ("splits_3", _pair(dict(num_splits=3)), "sp_fwd_kernel D=128 waves=4 KV=16 B=128 block_m=128 splits=3"),
    # N parts never exceed the 64-key tiles of max_blocks blocks: 5 blocks of 128 keys = 10 positions
    ("splits_clamped", _pair(dict(num_splits=99)), "sp_fwd_kernel D=128 waves=4 KV=16 B=128 block_m=128 splits=10"),
    ("splits_clamped_B64", _pair(dict(num_splits=99), dict(block=64)), "sp_fwd_kernel D=128 waves=4 KV=16 B=64 block_m=128 splits=5"),
    # the heuristic reads max_blocks * B, never the cache: 1 group, 16 blocks of 128 = 32 tiles -> 8 parts; a short list: none
    ("heuristic_long_list", _pair(dict(b=1, h_k=1, sk=65536, num_splits=0), dict(b=1, h_k=1, max_blocks=16)),
     "sp_fwd_kernel D=128 waves=4 KV=16 B=128 block_m=128 splits=8"),
    ("heuristic_short_list", _pair(dict(b=1, h_k=1, sk=65536, num_splits=0), dict(b=1, h_k=1, max_blocks=2)),
     "sp_fwd_kernel D=128 waves=4 KV=16 B=128 block_m=128 splits=1"),
    ("empty_list_still_runs", _pair(dict(num_splits=0), dict(max_blocks=0)), "sp_fwd_kernel D=128 waves=4 KV=16 B=128 block_m=128 splits=1"),
]


@pytest.mark.parametrize("name,pair,plan", PLANS, ids=[r[0] for r in PLANS])
def test_sparse_kv_plan_name(name, pair, plan):
    p, s = pair
    got = _lib.load().fa_fwd_sparse_kv_plan_name(p, s, 256)
    assert got is not None and got.decode() == plan
    assert _lib.load().fa_fwd_sparse_kv_plan_name(p, s, 64).decode() == plan  # the CU count decides nothing


def test_sparse_kv_heuristic_equals_the_pk_plan_for_the_listed_length():
    """num_splits = 0 is split_plan's count for the pk shape at a key length of max_blocks * B: the 16-bit fa_fwd call with
    FA_FLAG_PACK_GQA over a cache of that length plans the same parts -- whatever the capacity of the sparse call's cache."""
    lib = _lib.load()
    for b, max_blocks, block in ((1, 16, 128), (4, 64, 128), (64, 64, 128), (2, 5, 64), (1, 8, 256), (8, 256, 64)):
        for fp8_cache in (False, True):
            p, s = _pair(dict(b=b, h=32, h_k=8, sk=1 << 17, num_splits=0), dict(b=b, h_k=8, max_blocks=max_blocks, block=block), fp8_cache)
            n = re.search(r"splits=(\d+)", lib.fa_fwd_sparse_kv_plan_name(p, s, 256).decode()).group(1)
            p16 = _params(b=b, h=32, h_k=8, sk=max_blocks * block, num_splits=0, flags=_lib.FA_FLAG_PACK_GQA)
            name16 = lib.fa_fwd_plan_name(p16, 256).decode()
            assert name16.startswith("pk_fwd_kernel") and re.search(r"splits=(\d+)", name16).group(1) == n, (b, max_blocks, block, name16, n)


def _align256(x):
    return (x + 255) & ~255


def test_sparse_kv_workspace_size():
    """0 unsplit; split: the fp32 partials fa_fwd_combine merges -- O (splits, b, sq, h, d) and LSE (splits, b, h, sq), each
    rounded up to 256 bytes; ragged queries count total_q rows.  The same for both cache types."""
    lib = _lib.load()
    for fp8_cache in (False, True):
        assert lib.fa_fwd_sparse_kv_workspace_size(*_pair(fp8_cache=fp8_cache)) == 0
        assert lib.fa_fwd_sparse_kv_workspace_size(*_pair(dict(sq=0, num_splits=3), fp8_cache=fp8_cache)) == 0
        pair = _pair(dict(b=2, h=8, h_k=2, sq=3, d=80, num_splits=3), fp8_cache=fp8_cache)
        assert lib.fa_fwd_sparse_kv_workspace_size(*pair) == _align256(3 * 2 * 3 * 8 * 80 * 4) + _align256(3 * 2 * 3 * 8 * 4)
        pair = _pair(dict(cu_seqlens_q=ADDR, seqused_k=ADDR, total_q=6, sq=4, b=3, num_splits=2), dict(b=3), fp8_cache)
        assert lib.fa_fwd_sparse_kv_workspace_size(*pair) == _align256(2 * 6 * 8 * 128 * 4) + _align256(2 * 6 * 8 * 4)
    pair = _pair(dict(b=1, h_k=1, num_splits=0), dict(b=1, h_k=1, max_blocks=16))  # the heuristic's 8 parts
    assert lib.fa_fwd_sparse_kv_workspace_size(*pair) == _align256(8 * 8 * 128 * 4) + _align256(8 * 8 * 4)
    assert lib.fa_fwd_sparse_kv_workspace_size(*_pair(dict(dtype=FP8))) == UNSUPPORTED
    assert lib.fa_fwd_sparse_kv_workspace_size(*_pair(lists=dict(block=100))) == BAD_SHAPE
    assert lib.fa_fwd_sparse_kv_workspace_size(None, None) == NULLP


def test_sparse_kv_symbols_are_exported():
    lib = _lib.load()
    for name in ("fa_fwd_sparse_kv", "fa_fwd_sparse_kv_validate", "fa_fwd_sparse_kv_workspace_size", "fa_fwd_sparse_kv_plan_name"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert lib.fa_sparse_kv_params_size() == 72


def test_sparse_kv_instantiations_and_no_scratch():
    """The translation unit holds exactly {bf16, fp16} x {64, 128} x {plain, SOFTCAP} x {Kv16, Kv8} of sp_fwd_kernel and nothing
    else (the merge is fa_fwd_combine's kernel, in fa_fwd_api.hip), and none of them has a private segment: nothing spills."""
    from device_asm import TYPES, kernel_bodies
    kernels = {}
    for sym, body in kernel_bodies("fa_fwd_sparse_kv_api.hip"):
        k = re.match(r"_ZN2fa13sp_fwd_kernelI(DF16b|DF16_)Li(\d+)ELb([01])ENS_(?:4Kv16|3Kv8)I(DF16b|DF16_)Li(\d+)EEEEEvNS_8SpParamsE$", sym)
        assert k, f"a kernel in fa_fwd_sparse_kv_api.hip that is no sp_fwd_kernel: {sym}"
        assert k.group(1) == k.group(4) and k.group(2) == k.group(5), sym  # the tile policy of the kernel's own T and D
        key = (TYPES[k.group(1)], int(k.group(2)), bool(int(k.group(3))), "Kv8" if "3Kv8" in sym else "Kv16")
        assert key not in kernels
        kernels[key] = int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body).group(1))
    assert set(kernels) == {(t, d, s, kv) for t in ("bf16", "fp16") for d in (64, 128) for s in (False, True) for kv in ("Kv16", "Kv8")}
    assert len(kernels) == 16
    assert all(v == 0 for v in kernels.values()), kernels


# ---- the oracle helper --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("causal,window,softcap", [(False, (-1, -1), 0.0), (True, (-1, -1), 0.0), (False, (70, 0), 0.0), (False, (-1, -1), 15.0)],
                         ids=["plain", "causal", "window", "softcap"])
@pytest.mark.parametrize("block", [64, 128])
def test_oracle_with_every_block_listed_equals_the_dense_oracle(block, causal, window, softcap):
    torch.manual_seed(3)
    sq, cap, fill, h, hk, d = 3, 320, 200, 4, 2, 32
    q, k, v = torch.randn(sq, h, d), torch.randn(cap, hk, d), torch.randn(cap, hk, d)
    nblk = -(-fill // block)
    idx = torch.stack([torch.arange(nblk), torch.arange(nblk).flip(0)]).to(torch.int32)  # ascending and descending
    out, lse, _ = sparse_kv_oracle.sparse_kv_ref(q, k, v, fill, torch.tensor([nblk, nblk]), idx, block, causal, window, softcap)
    kmask = (torch.arange(cap) < fill).view(1, -1)
    ref, _, ref_lse = oracle.attention_ref(q[None], k[None], v[None], None, kmask, causal=causal, window_size=window, softcap=softcap,
                                           return_lse=True)
    assert torch.allclose(out, ref[0], atol=2e-6, rtol=1e-5)
    assert torch.allclose(lse, ref_lse[0], atol=1e-5, rtol=0)


def test_oracle_on_a_hand_made_two_block_case():
    """One head, d = 1, q = 1, keys all 0 (every visible key weighs the same), v[j] = j, B = 64, fill = 100: listing blocks {0, 1}
    averages keys 0..99; listing {1} averages 64..99; a stale entry behind the count, an entry past the fill level and a count
    above max_blocks change nothing; cnt = 0 gives out = 0, lse = +inf; a duplicate counts twice."""
    q, k = torch.ones(1, 1, 1), torch.zeros(192, 1, 1)
    v = torch.arange(192.0).view(192, 1, 1)
    run = lambda cnt, idx: sparse_kv_oracle.sparse_kv_ref(q, k, v, 100, torch.tensor([cnt]), torch.tensor([idx], dtype=torch.int32), 64)
    out, lse, vis = run(2, [1, 0])
    assert vis.sum() == 100 and out.item() == pytest.approx(49.5) and lse.item() == pytest.approx(torch.log(torch.tensor(100.0)).item())
    out, lse, _ = run(1, [1, 0])  # 0 is stale: behind the count
    assert out.item() == pytest.approx((64 + 99) / 2) and lse.item() == pytest.approx(torch.log(torch.tensor(36.0)).item())
    out, lse, _ = run(7, [1, 2])  # block 2 starts at 128 >= fill; the count is clamped to max_blocks
    assert out.item() == pytest.approx((64 + 99) / 2)
    out, lse, _ = run(0, [1, 0])
    assert out.item() == 0 and lse.item() == float("inf")
    out, lse, vis = run(3, [0, 1, 1])  # keys 64..99 twice
    assert vis.sum() == 136 and out.item() == pytest.approx((sum(range(64)) + 2 * sum(range(64, 100))) / 136)
    # causal, two rows: row 0 ends at key 98, row 1 at 99
    out, _, vis = sparse_kv_oracle.sparse_kv_ref(torch.ones(2, 1, 1), k, v, 100, torch.tensor([1]), torch.tensor([[1]], dtype=torch.int32), 64,
                                                 causal=True)
    assert vis[0, 0].sum() == 35 and vis[0, 1].sum() == 36 and out[0].item() == pytest.approx((64 + 98) / 2)
