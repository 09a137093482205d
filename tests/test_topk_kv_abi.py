"""CPU tests of the top-k token-sparse MLA decode at the C-ABI (include/fa_fwd.h: fa_fwd_topk_kv_validate, fa_fwd_topk_kv_plan_name,
fa_fwd_topk_kv_workspace_size) and of the kernel set of its translation unit, csrc/fa_fwd_topk_kv_api.hip.  Nothing here touches
a device; tests/test_topk_kv_gpu.py checks what the kernel computes."""
import re

import pytest

from flash_attention_annotated_amd import _lib

ADDR = 0x10000  # an aligned dummy address: nothing is dereferenced
OK, NULLP, BAD_SHAPE, BAD_STRIDE, UNSUPPORTED, BAD_ABI, WORKSPACE = 0, -1, -5, -6, -7, -9, -11


def _pair(params=None, topk=None, b=2, sq=1, h=16, h_k=1, sk=4096, d=64, dv=512, k=2048):
    """MLA decode params (q (b, sq, h, d), qv / o (b, sq, h, dv), a dense cache (b, sk, h_k, d | dv)), a dummy workspace, and a
    contiguous list (b, sq, h_k, k)."""
    p = _lib.new_params()
    for f in ("q", "k", "v", "o", "softmax_lse", "qv", "workspace"):
        setattr(p, f, ADDR)
    p.workspace_bytes = 1 << 40
    p.b, p.seqlen_q, p.seqlen_k, p.h, p.h_k, p.d, p.d_v, p.dtype = b, sq, sk, h, h_k, d, dv, _lib.FA_DTYPE_BF16
    for t, rows, heads, width in (("q", sq, h, d), ("qv", sq, h, dv), ("o", sq, h, dv), ("k", sk, h_k, d), ("v", sk, h_k, dv)):
        setattr(p, f"{t}_head_stride", width)
        setattr(p, f"{t}_row_stride", heads * width)
        setattr(p, f"{t}_batch_stride", rows * heads * width)
    p.softmax_scale = (d + dv) ** -0.5
    p.window_size_left = p.window_size_right = -1
    p.num_splits = 1
    for name, value in (params or {}).items():
        setattr(p, name, value)
    s = _lib.new_topk_kv_params()
    s.indices, s.topk, s.head_stride, s.row_stride, s.batch_stride = ADDR, k, k, h_k * k, sq * h_k * k
    for name, value in (topk or {}).items():
        setattr(s, name, value)
    return p, s


def _plan(dvt, k, splits=1):
    return f"tk_fwd_kernel DVT={dvt} waves=4 topk={k} splits={splits}"


PAGED = dict(block_table=ADDR, page_block_size=16, block_table_batch_stride=256)
CASES = [
    # accepted forms, with their plan text
    ("bf16", _pair(), _plan(512, 2048)),
    ("fp16_dv256", _pair(dict(dtype=_lib.FA_DTYPE_FP16), dv=256), _plan(256, 2048)),
    ("d24_dv264_is_tile_512", _pair(d=24, dv=264), _plan(512, 2048)),
    ("no_qv", _pair(dict(qv=0)), _plan(512, 2048)),
    ("topk_1", _pair(k=1), _plan(512, 1)),
    ("broadcast_heads_two_tokens", _pair(topk=dict(head_stride=0), sq=2, h=32, h_k=2), _plan(512, 2048)),
    ("paged_16", _pair(dict(PAGED, seqused_k=ADDR)), _plan(512, 2048)),
    ("batch_idx", _pair(dict(kv_batch_idx=ADDR, seqused_k=ADDR)), _plan(512, 2048)),
    ("empty_cache_still_runs", _pair(dict(k=0, v=0), sk=0), _plan(512, 2048)),
    ("splits_3", _pair(dict(num_splits=3)), _plan(512, 2048, 3)),
    ("splits_4_of_3_tiles", _pair(dict(num_splits=4), k=130), _plan(512, 130, 4)),  # as asked for: one part is empty
    ("heuristic_short_list", _pair(dict(num_splits=0), k=256), _plan(512, 256)),
    ("unsplit_without_workspace", _pair(dict(workspace=0)), _plan(512, 2048)),
    # the refusals, one row each: what is unsupported is said before what the params lack
    ("fp8_dtype", _pair(dict(dtype=_lib.FA_DTYPE_FP8_E4M3)), UNSUPPORTED),
    ("d128", _pair(d=128), UNSUPPORTED),
    ("dv128", _pair(dv=128), UNSUPPORTED),
    ("dv576", _pair(dv=576), UNSUPPORTED),
    ("causal", _pair(dict(is_causal=1)), UNSUPPORTED),
    ("window_left", _pair(dict(window_size_left=100)), UNSUPPORTED),
    ("window_right", _pair(dict(window_size_right=0)), UNSUPPORTED),
    ("chunk", _pair(dict(attention_chunk=64)), UNSUPPORTED),
    ("softcap", _pair(dict(softcap=30.0)), UNSUPPORTED),
    ("alibi", _pair(dict(alibi_slopes=ADDR)), UNSUPPORTED),
    ("dropout", _pair(dict(p_dropout=0.1, rng_state=ADDR)), UNSUPPORTED),
    ("leftpad", _pair(dict(leftpad_k=ADDR, seqused_k=ADDR)), UNSUPPORTED),
    ("cu_seqlens_q", _pair(dict(cu_seqlens_q=ADDR, seqused_k=ADDR, total_q=2)), UNSUPPORTED),
    ("cu_seqlens_k", _pair(dict(cu_seqlens_k=ADDR)), UNSUPPORTED),
    ("paged_batch_idx", _pair(dict(PAGED, kv_batch_idx=ADDR)), UNSUPPORTED),
    ("unsupported_first", _pair(dict(is_causal=1, q=0, h=7), dict(indices=0)), UNSUPPORTED),
    ("null_indices", _pair(topk=dict(indices=0)), NULLP),
    ("topk_0", _pair(k=0), BAD_SHAPE),
    ("head_stride_negative", _pair(topk=dict(head_stride=-1)), BAD_STRIDE),
    ("row_stride_negative", _pair(topk=dict(row_stride=-8)), BAD_STRIDE),
    ("splits_without_workspace", _pair(dict(num_splits=3, workspace=0)), WORKSPACE),
    ("splits_small_workspace", _pair(dict(num_splits=3, workspace_bytes=1024)), WORKSPACE),
]


@pytest.mark.parametrize("name,pair,want", CASES, ids=[c[0] for c in CASES])
def test_topk_kv_validate_and_plan(name, pair, want):
    """An accepted call names its plan; a refused one gives its status from validate and from the launch entry (no stream is
    touched: the refusal comes first), and no plan."""
    lib = _lib.load()
    p, s = pair
    if isinstance(want, str):
        assert lib.fa_fwd_topk_kv_validate(p, s) == OK
        assert lib.fa_fwd_topk_kv_plan_name(p, s, 256).decode() == want == lib.fa_fwd_topk_kv_plan_name(p, s, 64).decode()
    else:
        assert lib.fa_fwd_topk_kv_validate(p, s) == want == lib.fa_fwd_topk_kv(p, s, None)
        assert lib.fa_fwd_topk_kv_plan_name(p, s, 256) is None


def test_topk_kv_struct_symbols_and_abi():
    lib = _lib.load()
    for name in ("fa_fwd_topk_kv", "fa_fwd_topk_kv_validate", "fa_fwd_topk_kv_workspace_size", "fa_fwd_topk_kv_plan_name",
                 "fa_topk_kv_params_size"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert lib.fa_topk_kv_params_size() == 48 and lib.fa_abi_version() == 13 == _lib.FA_ABI_VERSION
    assert [n for n, _ in _lib.FaTopkKvParams._fields_] == ["abi_version", "struct_size", "indices", "batch_stride", "row_stride",
                                                           "head_stride", "topk", "reserved"]
    p, s = _pair()
    assert lib.fa_fwd_topk_kv_validate(None, s) == NULLP == lib.fa_fwd_topk_kv_validate(p, None)
    s.struct_size -= 8
    assert lib.fa_fwd_topk_kv_validate(p, s) == BAD_ABI == lib.fa_fwd_topk_kv_workspace_size(p, s)


@pytest.mark.parametrize("b,sq,h,k", [(1, 1, 16, 2048), (1, 1, 128, 2048), (8, 2, 16, 512), (64, 1, 128, 2048), (1, 1, 16, 8192)])
def test_topk_kv_heuristic_is_a_function_of_shapes(b, sq, h, k):
    """num_splits = 0 is the qv kernel's heuristic for b * sq single-token queries over a key length of topk: the dense qv call
    of that shape plans the same parts, whatever the capacity, the paging and the pointers of this call are."""
    lib = _lib.load()
    parts = set()
    for params, sk in ((dict(num_splits=0), 32768), (dict(PAGED, num_splits=0, seqused_k=ADDR, k=ADDR + 4096), 1 << 20)):
        p, s = _pair(params, b=b, sq=sq, h=h, sk=sk, k=k)
        parts.add(re.search(r"splits=(\d+)$", lib.fa_fwd_topk_kv_plan_name(p, s, 256).decode()).group(1))
    dense, _ = _pair(dict(num_splits=0), b=b * sq, sq=1, h=h, sk=k)
    parts.add(re.search(r"splits=(\d+)", lib.fa_fwd_plan_name(dense, 256).decode()).group(1))
    assert len(parts) == 1, parts


def test_topk_kv_workspace_size():
    """0 unsplit; split: fp32 O (splits, b, sq, h, d_v) and LSE (splits, b, h, sq), each rounded up to 256 bytes."""
    lib = _lib.load()
    align = lambda x: (x + 255) & ~255
    assert lib.fa_fwd_topk_kv_workspace_size(*_pair()) == 0
    assert lib.fa_fwd_topk_kv_workspace_size(*_pair(dict(num_splits=3), sq=0)) == 0
    pair = _pair(dict(num_splits=3), b=2, sq=2, h=40, dv=264, d=24)
    assert lib.fa_fwd_topk_kv_workspace_size(*pair) == align(3 * 2 * 2 * 40 * 264 * 4) + align(3 * 2 * 2 * 40 * 4)
    assert lib.fa_fwd_topk_kv_workspace_size(*_pair(dict(is_causal=1))) == UNSUPPORTED
    assert lib.fa_fwd_topk_kv_workspace_size(*_pair(k=0)) == BAD_SHAPE


def test_topk_kv_unit_holds_exactly_the_four_instantiations():
    from device_asm import kernel_bodies
    symbols = sorted(sym for sym, _ in kernel_bodies("fa_fwd_topk_kv_api.hip"))
    assert symbols == sorted(f"_ZN2fa13tk_fwd_kernelI{t}Li{dvt}EEEvNS_8TkParamsE" for t in ("DF16b", "DF16_") for dvt in (256, 512))
