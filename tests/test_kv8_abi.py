"""CPU tests of the fp8-KV-cache entry points (include/fa_fwd.h: fa_fwd_kv8_validate, fa_fwd_kv8_plan_name,
fa_fwd_kv8_workspace_size) and of the device code of their translation unit, csrc/fa_fwd_kv8_api.hip.  Nothing here touches a
device; tests/test_kv8_kvcache_gpu.py checks what the kernel computes."""
import re

import pytest

from flash_attention_annotated_amd import _lib

ADDR = 0x10000  # an aligned dummy address: nothing is dereferenced
OK, NULLP, BAD_DTYPE, BAD_HEAD_DIM, BAD_HEADS, BAD_SHAPE, BAD_STRIDE, UNSUPPORTED, WORKSPACE = 0, -1, -2, -3, -4, -5, -6, -7, -11
FP8 = _lib.FA_DTYPE_FP8_E4M3


def _params(b=2, h=8, h_k=2, sq=1, sk=320, d=128, dtype=_lib.FA_DTYPE_BF16, **fields):
    """Dense q (b, sq, h, d) of 16-bit elements over a dense e4m3 cache (b, sk, h_k, d) of bytes; a dummy workspace."""
    p = _lib.new_params()
    for f in ("q", "k", "v", "o", "softmax_lse", "workspace"):
        setattr(p, f, ADDR)
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


def _ragged(**kw):
    return _params(**{**dict(cu_seqlens_q=ADDR, seqused_k=ADDR, total_q=6, sq=4, b=3), **kw})


def _paged(page, **kw):
    return _params(block_table=ADDR, page_block_size=page, block_table_batch_stride=16, **kw)


VALIDATE = [
    ("bf16", _params(), OK),
    ("fp16", _params(dtype=_lib.FA_DTYPE_FP16), OK),
    ("fp8_q", _params(dtype=FP8), UNSUPPORTED),
    ("fp32_q", _params(dtype=_lib.FA_DTYPE_FP32), BAD_DTYPE),
    ("d16", _params(d=16), OK),
    ("d80", _params(d=80), OK),
    ("d192", _params(d=192), UNSUPPORTED),
    ("d72", _params(d=72), UNSUPPORTED),
    ("d_v_same", _params(d_v=128), OK),
    ("d_v_own", _params(d_v=64), UNSUPPORTED),
    ("qv", _params(qv=ADDR), UNSUPPORTED),
    ("alibi", _params(alibi_slopes=ADDR), UNSUPPORTED),
    ("dropout", _params(p_dropout=0.1, rng_state=ADDR), UNSUPPORTED),
    ("chunk", _params(attention_chunk=64), UNSUPPORTED),
    ("s_dmask", _params(s_dmask=ADDR), UNSUPPORTED),
    ("cu_seqlens_k", _params(cu_seqlens_q=ADDR, cu_seqlens_k=ADDR, seqused_k=ADDR, total_q=2), UNSUPPORTED),
    # what is unsupported is said before what the params lack
    ("unsupported_first", _params(d=192, q=0, h=7), UNSUPPORTED),
    ("ragged", _ragged(), OK),
    ("ragged_without_fill_levels", _ragged(seqused_k=0), BAD_SHAPE),
    ("paged_64", _paged(64), OK),
    ("paged_1", _paged(1), OK),
    ("paged_0", _paged(0), BAD_SHAPE),
    ("paged_batch_idx", _paged(64, kv_batch_idx=ADDR), UNSUPPORTED),
    ("paged_leftpad", _paged(64, leftpad_k=ADDR, seqused_k=ADDR), UNSUPPORTED),
    ("batch_idx_leftpad", _params(kv_batch_idx=ADDR, leftpad_k=ADDR, seqused_k=ADDR), OK),
    ("heads", _params(h=7), BAD_HEADS),
    ("null_q", _params(q=0), NULLP),
    ("k_stride_8", _params(k_head_stride=136), BAD_STRIDE),  # 16 bytes = 16 e4m3 elements
    ("k_stride_16", _params(k_head_stride=144), OK),
    ("q_stride_8", _params(q_head_stride=136), OK),          # q is 16-bit: 8 elements
    ("k_pointer", _params(k=ADDR + 8), BAD_STRIDE),
    ("splits_negative", _params(num_splits=-1), BAD_SHAPE),
    ("splits_without_workspace", _params(num_splits=3, workspace=0), WORKSPACE),
    ("splits_small_workspace", _params(num_splits=3, workspace_bytes=1024), WORKSPACE),
    ("softcap", _params(softcap=30.0), OK),
    ("softcap_negative", _params(softcap=-1.0), BAD_SHAPE),
]


@pytest.mark.parametrize("name,p,status", VALIDATE, ids=[r[0] for r in VALIDATE])
def test_kv8_validate(name, p, status):
    assert _lib.load().fa_fwd_kv8_validate(p) == status
    if status != OK:
        assert _lib.load().fa_fwd_kv8_plan_name(p, 256) is None


def test_kv8_validate_null_and_abi():
    lib = _lib.load()
    assert lib.fa_fwd_kv8_validate(None) == NULLP
    p = _params()
    p.abi_version = 12
    assert lib.fa_fwd_kv8_validate(p) == -9
    assert lib.fa_fwd_kv8_workspace_size(p) == -9


def test_fa_fwd_still_refuses_the_all_fp8_cache_call():
    """fa_fwd / fa_fwd_validate are untouched: fp8 q beside a paged cache stays FA_ERR_UNSUPPORTED there."""
    p = _params(dtype=FP8, block_table=ADDR, page_block_size=256, block_table_batch_stride=16)
    assert _lib.load().fa_fwd_validate(p) == UNSUPPORTED


PLANS = [
    ("decode", _params(), "kv8_fwd_kernel D=128 waves=4 block_m=128 splits=1"),
    ("fp16", _params(dtype=_lib.FA_DTYPE_FP16), "kv8_fwd_kernel D=128 waves=4 block_m=128 splits=1"),
    ("d64", _params(d=64), "kv8_fwd_kernel D=64 waves=4 block_m=128 splits=1"),
    ("d16", _params(d=16), "kv8_fwd_kernel D=64 waves=4 block_m=128 splits=1"),
    ("d80", _params(d=80), "kv8_fwd_kernel D=128 waves=4 block_m=128 splits=1"),
    ("d96", _params(d=96), "kv8_fwd_kernel D=128 waves=4 block_m=128 splits=1"),
    ("softcap", _params(softcap=30.0), "kv8_fwd_kernel D=128 waves=4 SOFTCAP block_m=128 splits=1"),
    ("d64_softcap", _params(d=64, softcap=30.0), "kv8_fwd_kernel D=64 waves=4 SOFTCAP block_m=128 splits=1"),
    ("splits_3", _params(num_splits=3), "kv8_fwd_kernel D=128 waves=4 block_m=128 splits=3"),
    # N parts never exceed the 64-key blocks of the capacity
    ("splits_clamped", _params(num_splits=9), "kv8_fwd_kernel D=128 waves=4 block_m=128 splits=5"),
    # the heuristic of the pk shape (fa_fwd's split_plan): 1 (batch, kv head) group, 32 key blocks -> 8 parts of 4 blocks
    ("heuristic_b1", _params(b=1, h=8, h_k=1, sk=2048, num_splits=0), "kv8_fwd_kernel D=128 waves=4 block_m=128 splits=8"),
    # ... and none when the groups fill the chip, or the cache is short
    ("heuristic_full", _params(b=128, h=32, h_k=8, sk=8192, num_splits=0), "kv8_fwd_kernel D=128 waves=4 block_m=128 splits=1"),
    ("heuristic_short", _params(b=1, sk=320, num_splits=0), "kv8_fwd_kernel D=128 waves=4 block_m=128 splits=1"),
    ("ragged_split", _ragged(num_splits=2), "kv8_fwd_kernel D=128 waves=4 block_m=128 splits=2"),
    ("paged_16", _paged(16), "kv8_fwd_kernel D=128 waves=4 block_m=128 splits=1"),
    ("mha_prefill", _params(h=2, h_k=2, sq=130, is_causal=1), "kv8_fwd_kernel D=128 waves=4 block_m=128 splits=1"),
]


@pytest.mark.parametrize("name,p,plan", PLANS, ids=[r[0] for r in PLANS])
def test_kv8_plan_name(name, p, plan):
    got = _lib.load().fa_fwd_kv8_plan_name(p, 256)
    assert got is not None and got.decode() == plan
    assert _lib.load().fa_fwd_kv8_plan_name(p, 64).decode() == plan  # the CU count decides nothing


def test_kv8_heuristic_equals_the_pk_plan_of_fa_fwd():
    """num_splits = 0 is split_plan's count for the pk shape: the 16-bit call with FA_FLAG_PACK_GQA plans the same parts."""
    lib = _lib.load()
    for b, sk in ((1, 2048), (4, 8192), (64, 8192), (2, 320)):
        p8 = _params(b=b, h=32, h_k=8, sk=sk, num_splits=0)
        p16 = _params(b=b, h=32, h_k=8, sk=sk, num_splits=0, flags=_lib.FA_FLAG_PACK_GQA)
        for t in ("k", "v"):  # 16-bit strides of the same shape
            setattr(p16, f"{t}_batch_stride", sk * 8 * 128)
        n8 = re.search(r"splits=(\d+)", lib.fa_fwd_kv8_plan_name(p8, 256).decode()).group(1)
        name16 = lib.fa_fwd_plan_name(p16, 256).decode()
        assert name16.startswith("pk_fwd_kernel") and re.search(r"splits=(\d+)", name16).group(1) == n8, (b, sk, name16)


def _align256(x):
    return (x + 255) & ~255


def test_kv8_workspace_size():
    """0 unsplit; split: the fp32 partials fa_fwd_combine merges -- O (splits, b, sq, h, d) and LSE (splits, b, h, sq), each
    rounded up to 256 bytes; ragged queries count total_q rows."""
    lib = _lib.load()
    assert lib.fa_fwd_kv8_workspace_size(_params()) == 0
    assert lib.fa_fwd_kv8_workspace_size(_params(sq=0)) == 0
    assert lib.fa_fwd_kv8_workspace_size(_params(sq=0, num_splits=3)) == 0
    p = _params(b=2, h=8, h_k=2, sq=3, sk=320, d=80, num_splits=3)
    assert lib.fa_fwd_kv8_workspace_size(p) == _align256(3 * 2 * 3 * 8 * 80 * 4) + _align256(3 * 2 * 3 * 8 * 4)
    p = _ragged(num_splits=2)  # total_q = 6
    assert lib.fa_fwd_kv8_workspace_size(p) == _align256(2 * 6 * 8 * 128 * 4) + _align256(2 * 6 * 8 * 4)
    p = _params(b=1, h=8, h_k=1, sk=2048, num_splits=0)  # the heuristic's 8 parts
    assert lib.fa_fwd_kv8_workspace_size(p) == _align256(8 * 8 * 128 * 4) + _align256(8 * 8 * 4)
    assert lib.fa_fwd_kv8_workspace_size(_params(dtype=FP8)) == UNSUPPORTED
    assert lib.fa_fwd_kv8_workspace_size(None) == NULLP


def test_kv8_large_cache_entries_are_served_not_refused():
    """The extent rule (csrc/fa_fwd_kernel_kv8.h): the kernel rebuilds a 64-bit base per 64-key tile, so a K or V of 2^31 bytes or
    more per cache entry -- and a cache far beyond 2^32 bytes in all -- validates; what is bounded is the row stride, which the
    32-bit lane offset inside a tile multiplies by up to 63."""
    lib = _lib.load()
    sk, h_k, d = 1 << 20, 32, 128                      # 4 GiB of K per cache entry
    p = _params(b=4, h=32, h_k=h_k, sk=sk, d=d)
    assert p.k_batch_stride == 1 << 32
    assert lib.fa_fwd_kv8_validate(p) == OK
    assert lib.fa_fwd_kv8_plan_name(p, 256).decode() == "kv8_fwd_kernel D=128 waves=4 block_m=128 splits=1"
    paged = _paged(64, b=4, h=32, h_k=h_k, d=d, sk=sk, k_batch_stride=64 * h_k * d, v_batch_stride=64 * h_k * d)
    assert lib.fa_fwd_kv8_validate(paged) == OK        # 2^14 pages per sequence, 64 GiB pool: the page offset is 64-bit
    assert lib.fa_fwd_kv8_validate(_params(k_row_stride=(1 << 24) - 16)) == OK
    assert lib.fa_fwd_kv8_validate(_params(k_row_stride=1 << 24)) == BAD_STRIDE
    assert lib.fa_fwd_kv8_validate(_params(v_row_stride=1 << 24)) == BAD_STRIDE
    assert lib.fa_fwd_kv8_validate(_params(v_row_stride=-16)) == BAD_STRIDE


def test_kv8_symbols_are_exported():
    lib = _lib.load()
    for name in ("fa_fwd_kv8", "fa_fwd_kv8_validate", "fa_fwd_kv8_workspace_size", "fa_fwd_kv8_plan_name"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)


def _kv8_kernels():
    """{(type, D, SOFTCAP): private segment bytes} of the device code of fa_fwd_kv8_api.hip (any other kernel in it is an error)."""
    from device_asm import fp8_cache_kernels
    return fp8_cache_kernels("fa_fwd_kv8_api.hip", "kv8_fwd_kernel", "PkParams")


def test_kv8_instantiations_and_no_scratch():
    """The translation unit holds exactly {bf16, fp16} x {64, 128} x {plain, SOFTCAP} of kv8_fwd_kernel and nothing else (the
    merge is fa_fwd_combine's kernel, in fa_fwd_api.hip), and none of them has a private segment: nothing spills."""
    kernels = _kv8_kernels()
    assert set(kernels) == {(t, d, s) for t in ("bf16", "fp16") for d in (64, 128) for s in (False, True)}
    assert len(kernels) == 8
    assert all(v == 0 for v in kernels.values()), kernels
