"""CPU tests of the MLA-shape entry points over an fp8 KV cache (include/fa_fwd.h: fa_fwd_qv8_validate, fa_fwd_qv8_plan_name,
fa_fwd_qv8_workspace_size) and of the device code of their translation unit, csrc/fa_fwd_qv8_api.hip.  Nothing here touches a
device; tests/test_qv8_kvcache_gpu.py checks what the kernel computes."""
import re

import pytest

from flash_attention_annotated_amd import _lib

ADDR = 0x10000  # an aligned dummy address: nothing is dereferenced
OK, NULLP, BAD_DTYPE, BAD_HEAD_DIM, BAD_HEADS, BAD_SHAPE, BAD_STRIDE, UNSUPPORTED, BAD_ABI, WORKSPACE = 0, -1, -2, -3, -4, -5, -6, -7, -9, -11
FP8 = _lib.FA_DTYPE_FP8_E4M3


def _params(b=2, h=16, h_k=1, sq=1, sk=320, d=64, dv=512, dtype=_lib.FA_DTYPE_BF16, **fields):
    """Dense q (b, sq, h, d) and qv (b, sq, h, dv) of 16-bit elements over a dense e4m3 cache K (b, sk, h_k, d), V (b, sk, h_k, dv)
    of bytes; a dummy workspace."""
    p = _lib.new_params()
    for f in ("q", "k", "v", "o", "softmax_lse", "workspace", "qv"):
        setattr(p, f, ADDR)
    p.workspace_bytes = 1 << 40
    p.b, p.seqlen_q, p.seqlen_k, p.h, p.h_k, p.d, p.d_v, p.dtype = b, sq, sk, h, h_k, d, dv, dtype
    for t, rows, heads, w in (("q", sq, h, d), ("k", sk, h_k, d), ("v", sk, h_k, dv), ("o", sq, h, dv), ("qv", sq, h, dv)):
        setattr(p, f"{t}_head_stride", w)
        setattr(p, f"{t}_row_stride", heads * w)
        setattr(p, f"{t}_batch_stride", rows * heads * w)
    p.softmax_scale = (d + dv) ** -0.5
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
    ("without_qv", _params(qv=0), OK),
    ("fp8_q", _params(dtype=FP8), UNSUPPORTED),
    ("fp32_q", _params(dtype=_lib.FA_DTYPE_FP32), BAD_DTYPE),
    ("d16", _params(d=16), OK),
    ("d48", _params(d=48), OK),
    ("d128", _params(d=128), UNSUPPORTED),
    ("d40", _params(d=40), UNSUPPORTED),
    ("d_v_missing", _params(d_v=0), BAD_HEAD_DIM),
    ("d_v_256", _params(dv=256), OK),
    ("d_v_320", _params(dv=320), OK),
    ("d_v_128", _params(dv=128), UNSUPPORTED),
    ("d_v_528", _params(dv=528), UNSUPPORTED),
    ("d_v_264", _params(dv=264), UNSUPPORTED),
    ("alibi", _params(alibi_slopes=ADDR), UNSUPPORTED),
    ("dropout", _params(p_dropout=0.1, rng_state=ADDR), UNSUPPORTED),
    ("chunk", _params(attention_chunk=64), UNSUPPORTED),
    ("s_dmask", _params(s_dmask=ADDR), UNSUPPORTED),
    ("cu_seqlens_k", _params(cu_seqlens_q=ADDR, cu_seqlens_k=ADDR, seqused_k=ADDR, total_q=2), UNSUPPORTED),
    # what is unsupported is said before what the params lack
    ("unsupported_first", _params(d=128, q=0, h=7), UNSUPPORTED),
    ("ragged", _ragged(), OK),
    ("ragged_without_fill_levels", _ragged(seqused_k=0), BAD_SHAPE),
    ("paged_64", _paged(64), OK),
    ("paged_16", _paged(16), OK),
    ("paged_0", _paged(0), BAD_SHAPE),
    ("paged_batch_idx", _paged(64, kv_batch_idx=ADDR), UNSUPPORTED),
    ("paged_leftpad", _paged(64, leftpad_k=ADDR, seqused_k=ADDR), UNSUPPORTED),
    ("batch_idx_leftpad", _params(kv_batch_idx=ADDR, leftpad_k=ADDR, seqused_k=ADDR), OK),
    ("heads", _params(h=7, h_k=2), BAD_HEADS),
    ("null_q", _params(q=0), NULLP),
    ("q_stride_8", _params(q_head_stride=72), OK),           # q / o / qv are 16-bit: 8 elements
    ("q_stride_4", _params(q_head_stride=68), BAD_STRIDE),
    ("o_stride_4", _params(o_row_stride=16 * 512 + 4), BAD_STRIDE),
    ("qv_stride_4", _params(qv_row_stride=16 * 512 + 4), BAD_STRIDE),
    ("qv_stride_ignored_without_qv", _params(qv=0, qv_row_stride=4), OK),
    ("k_stride_8", _params(k_head_stride=72), BAD_STRIDE),   # 16 bytes = 16 e4m3 elements
    ("k_stride_16", _params(k_head_stride=80), OK),
    ("v_stride_8", _params(v_row_stride=520), BAD_STRIDE),
    ("k_row_stride_2_24", _params(k_row_stride=1 << 24), BAD_STRIDE),
    ("v_row_stride_below_2_24", _params(v_row_stride=(1 << 24) - 16), OK),
    ("v_row_stride_negative", _params(v_row_stride=-16), BAD_STRIDE),
    ("k_pointer", _params(k=ADDR + 8), BAD_STRIDE),
    ("qv_pointer", _params(qv=ADDR + 8), BAD_STRIDE),
    ("descale_stride_negative", _params(k_descale=ADDR, k_descale_batch_stride=-1), BAD_STRIDE),
    ("descale_stride_wide", _params(v_descale=ADDR, v_descale_head_stride=1 << 31), BAD_STRIDE),
    ("descale_pointer", _params(v_descale=ADDR + 2), BAD_STRIDE),
    ("descales", _params(k_descale=ADDR, v_descale=ADDR + 4, k_descale_batch_stride=1, v_descale_batch_stride=1), OK),
    ("splits_negative", _params(num_splits=-1), BAD_SHAPE),
    ("splits_without_workspace", _params(num_splits=3, workspace=0), WORKSPACE),
    ("splits_small_workspace", _params(num_splits=3, workspace_bytes=1024), WORKSPACE),
    ("softcap", _params(softcap=30.0), OK),
    ("softcap_negative", _params(softcap=-1.0), BAD_SHAPE),
]


@pytest.mark.parametrize("name,p,status", VALIDATE, ids=[r[0] for r in VALIDATE])
def test_qv8_validate(name, p, status):
    assert _lib.load().fa_fwd_qv8_validate(p) == status
    if status != OK:
        assert _lib.load().fa_fwd_qv8_plan_name(p, 256) is None


def test_qv8_validate_null_and_abi():
    lib = _lib.load()
    assert lib.fa_fwd_qv8_validate(None) == NULLP
    p = _params()
    p.abi_version = 12
    assert lib.fa_fwd_qv8_validate(p) == BAD_ABI
    assert lib.fa_fwd_qv8_workspace_size(p) == BAD_ABI
    assert _lib.FA_ABI_VERSION == 13 and lib.fa_abi_version() == 13


def test_the_other_entry_points_keep_refusing_the_shape():
    """fa_fwd_kv8_validate is untouched: qv and a wide V stay FA_ERR_UNSUPPORTED there; fa_fwd still refuses fp8 beside qv."""
    lib = _lib.load()
    assert lib.fa_fwd_kv8_validate(_params()) == UNSUPPORTED
    assert lib.fa_fwd_kv8_validate(_params(qv=0)) == UNSUPPORTED             # a wide V alone
    same = _params(d=64, dv=64, qv=ADDR)
    assert lib.fa_fwd_kv8_validate(same) == UNSUPPORTED                      # qv alone
    assert lib.fa_fwd_validate(_params(dtype=FP8)) == UNSUPPORTED


def _plan(dvt, splits=1, softcap=False):
    return f"qv8_fwd_kernel DVT={dvt} waves=4{' SOFTCAP' if softcap else ''} block_m=32 splits={splits}"


PLANS = [
    ("decode", _params(), _plan(512)),
    ("fp16", _params(dtype=_lib.FA_DTYPE_FP16), _plan(512)),
    ("dv256", _params(dv=256), _plan(256)),
    ("dv272", _params(dv=272), _plan(512)),
    ("dv320_d48", _params(d=48, dv=320), _plan(512)),
    ("without_qv", _params(qv=0, dv=256), _plan(256)),
    ("softcap", _params(softcap=30.0), _plan(512, softcap=True)),
    ("dv256_softcap", _params(dv=256, softcap=30.0), _plan(256, softcap=True)),
    ("splits_3", _params(num_splits=3), _plan(512, 3)),
    ("splits_3_dv256_softcap", _params(num_splits=3, dv=256, softcap=20.0), _plan(256, 3, softcap=True)),
    # N parts never exceed the 64-key blocks of the capacity
    ("splits_clamped", _params(num_splits=9), _plan(512, 5)),
    ("ragged_split", _ragged(num_splits=2), _plan(512, 2)),
    ("paged_16", _paged(16), _plan(512)),
    ("heuristic_short", _params(b=1, sk=320, num_splits=0), _plan(512)),
]


@pytest.mark.parametrize("name,p,plan", PLANS, ids=[r[0] for r in PLANS])
def test_qv8_plan_name(name, p, plan):
    got = _lib.load().fa_fwd_qv8_plan_name(p, 256)
    assert got is not None and got.decode() == plan
    assert _lib.load().fa_fwd_qv8_plan_name(p, 64).decode() == plan  # the CU count decides nothing


def _as_16bit(p, sk, h_k, d, dv):
    """The 16-bit call of the same shape: k / v strides in elements of a 16-bit cache."""
    for t, w in (("k", d), ("v", dv)):
        setattr(p, f"{t}_head_stride", w)
        setattr(p, f"{t}_row_stride", h_k * w)
        setattr(p, f"{t}_batch_stride", sk * h_k * w)
    return p


def test_qv8_heuristic_equals_the_qv_plan_of_fa_fwd():
    """num_splits = 0 is split_plan_qv's count: the 16-bit qv call of the same shape plans the same parts."""
    lib = _lib.load()
    seen = set()
    for b, h, sq, sk in ((1, 16, 1, 8192), (4, 16, 1, 8192), (32, 128, 1, 8192), (128, 16, 2, 8192), (2, 16, 1, 320), (600, 16, 1, 8192)):
        p8 = _params(b=b, h=h, sq=sq, sk=sk, num_splits=0)
        p16 = _as_16bit(_params(b=b, h=h, sq=sq, sk=sk, num_splits=0), sk, 1, 64, 512)
        n8 = re.search(r"splits=(\d+)", lib.fa_fwd_qv8_plan_name(p8, 256).decode()).group(1)
        name16 = lib.fa_fwd_plan_name(p16, 256).decode()
        assert name16.startswith("fwd_kernel_qv DVT=512") and re.search(r"splits=(\d+)", name16).group(1) == n8, (b, sk, name16)
        seen.add(int(n8))
    assert 1 in seen and len(seen) >= 3, seen  # the shapes above cross the heuristic's thresholds


def _align256(x):
    return (x + 255) & ~255


def test_qv8_workspace_size():
    """0 unsplit; split: the fp32 partials fa_fwd_combine merges -- O (splits, rows, h, d_v) and LSE (splits, rows, h), each rounded
    up to 256 bytes; ragged queries count total_q rows."""
    lib = _lib.load()
    assert lib.fa_fwd_qv8_workspace_size(_params()) == 0
    assert lib.fa_fwd_qv8_workspace_size(_params(sq=0)) == 0
    assert lib.fa_fwd_qv8_workspace_size(_params(sq=0, num_splits=3)) == 0
    p = _params(b=2, h=6, h_k=2, sq=3, sk=320, d=48, dv=320, num_splits=3)
    assert lib.fa_fwd_qv8_workspace_size(p) == _align256(3 * 2 * 3 * 6 * 320 * 4) + _align256(3 * 2 * 3 * 6 * 4)
    p = _ragged(num_splits=2)  # total_q = 6
    assert lib.fa_fwd_qv8_workspace_size(p) == _align256(2 * 6 * 16 * 512 * 4) + _align256(2 * 6 * 16 * 4)
    p = _params(b=1, sk=2048, num_splits=0)  # the heuristic: 1 group, 32 key blocks -> 8 parts of 4 blocks
    assert lib.fa_fwd_qv8_plan_name(p, 256).decode() == _plan(512, 8)
    assert lib.fa_fwd_qv8_workspace_size(p) == _align256(8 * 16 * 512 * 4) + _align256(8 * 16 * 4)
    assert lib.fa_fwd_qv8_workspace_size(_params(dtype=FP8)) == UNSUPPORTED
    assert lib.fa_fwd_qv8_workspace_size(_params(dv=128)) == UNSUPPORTED
    assert lib.fa_fwd_qv8_workspace_size(None) == NULLP


def test_qv8_large_cache_entries_are_served_not_refused():
    """The kernel rebuilds a 64-bit base per 64-key tile, so a V of 4 GiB per cache entry validates; what is bounded is the row
    stride, which the 32-bit lane offset inside a tile multiplies by up to 63."""
    lib = _lib.load()
    sk, h_k, dv = 1 << 20, 8, 512                      # 4 GiB of V per cache entry
    p = _params(b=4, h=16, h_k=h_k, sk=sk, dv=dv)
    assert p.v_batch_stride == 1 << 32
    assert lib.fa_fwd_qv8_validate(p) == OK
    assert lib.fa_fwd_qv8_plan_name(p, 256).decode() == _plan(512)
    paged = _paged(64, b=4, h=16, h_k=h_k, sk=sk, k_batch_stride=64 * h_k * 64, v_batch_stride=64 * h_k * dv)
    assert lib.fa_fwd_qv8_validate(paged) == OK        # 2^14 pages per sequence: the page offset is 64-bit


def test_qv8_symbols_are_exported():
    lib = _lib.load()
    for name in ("fa_fwd_qv8", "fa_fwd_qv8_validate", "fa_fwd_qv8_workspace_size", "fa_fwd_qv8_plan_name"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)


def _qv8_kernels():
    """{(type, DVT, SOFTCAP): private segment bytes} of the device code of fa_fwd_qv8_api.hip (any other kernel in it is an error)."""
    from device_asm import fp8_cache_kernels
    return fp8_cache_kernels("fa_fwd_qv8_api.hip", "qv8_fwd_kernel", "QvParams")


def test_qv8_instantiations_and_no_scratch():
    """The translation unit holds exactly {bf16, fp16} x {256, 512} x {plain, SOFTCAP} of qv8_fwd_kernel and nothing else (the
    merge is fa_fwd_combine's kernel, in fa_fwd_api.hip), and none of them has a private segment: nothing spills."""
    kernels = _qv8_kernels()
    assert set(kernels) == {(t, d, s) for t in ("bf16", "fp16") for d in (256, 512) for s in (False, True)}
    assert len(kernels) == 8
    assert all(v == 0 for v in kernels.values()), kernels
