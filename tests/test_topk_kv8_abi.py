"""CPU tests of the top-k token-sparse MLA decode over the fp8 latent cache at the C-ABI (include/fa_fwd.h: fa_fwd_topk_kv8_validate,
fa_fwd_topk_kv8_plan_name, fa_fwd_topk_kv8_workspace_size).  Nothing here touches a device; tests/test_topk_kv8_gpu.py checks
what the kernel computes."""
import pytest

from flash_attention_annotated_amd import _lib

ADDR = 0x10000  # an aligned dummy address: nothing is dereferenced
OK, NULLP, BAD_SHAPE, BAD_STRIDE, UNSUPPORTED, WORKSPACE = 0, -1, -5, -6, -7, -11


def _pair(params=None, topk=None, b=2, sq=1, h=16, h_k=1, sk=4096, d=64, dv=512, k=2048):
    """MLA decode params (16-bit q (b, sq, h, d), qv / o (b, sq, h, dv), a dense e4m3 cache (b, sk, h_k, d | dv) with byte
    strides and both descales), a dummy workspace, and a contiguous list (b, sq, h_k, k)."""
    p = _lib.new_params()
    for f in ("q", "k", "v", "o", "softmax_lse", "qv", "workspace", "k_descale", "v_descale"):
        setattr(p, f, ADDR)
    p.workspace_bytes = 1 << 40
    p.b, p.seqlen_q, p.seqlen_k, p.h, p.h_k, p.d, p.d_v, p.dtype = b, sq, sk, h, h_k, d, dv, _lib.FA_DTYPE_BF16
    for t, rows, heads, width in (("q", sq, h, d), ("qv", sq, h, dv), ("o", sq, h, dv), ("k", sk, h_k, d), ("v", sk, h_k, dv)):
        setattr(p, f"{t}_head_stride", width)
        setattr(p, f"{t}_row_stride", heads * width)
        setattr(p, f"{t}_batch_stride", rows * heads * width)
    p.k_descale_batch_stride = p.v_descale_batch_stride = h_k
    p.k_descale_head_stride = p.v_descale_head_stride = 1
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
    return f"tk8_fwd_kernel DVT={dvt} waves=4 topk={k} splits={splits}"


PAGED = dict(block_table=ADDR, page_block_size=16, block_table_batch_stride=256)
CASES = [
    # accepted forms, with their plan text
    ("bf16", _pair(), _plan(512, 2048)),
    ("fp16_dv256", _pair(dict(dtype=_lib.FA_DTYPE_FP16), dv=256), _plan(256, 2048)),
    ("d16_dv272_is_tile_512", _pair(d=16, dv=272), _plan(512, 2048)),
    ("no_qv_null_descales", _pair(dict(qv=0, k_descale=0, v_descale=0)), _plan(512, 2048)),
    ("paged_16", _pair(dict(PAGED, seqused_k=ADDR)), _plan(512, 2048)),
    ("batch_idx", _pair(dict(kv_batch_idx=ADDR, seqused_k=ADDR)), _plan(512, 2048)),
    ("empty_cache_still_runs", _pair(dict(k=0, v=0), sk=0), _plan(512, 2048)),
    ("splits_3", _pair(dict(num_splits=3)), _plan(512, 2048, 3)),
    ("splits_4_of_3_tiles", _pair(dict(num_splits=4), k=130), _plan(512, 130, 4)),  # as asked for: one part is empty
    ("heuristic_short_list", _pair(dict(num_splits=0), k=256), _plan(512, 256)),
    # the refusals, one row each: what is unsupported is said before what the params lack
    ("fp8_q", _pair(dict(dtype=_lib.FA_DTYPE_FP8_E4M3)), UNSUPPORTED),
    ("d24", _pair(d=24), UNSUPPORTED),
    ("dv264", _pair(dv=264), UNSUPPORTED),
    ("dv576", _pair(dv=576), UNSUPPORTED),
    ("causal", _pair(dict(is_causal=1)), UNSUPPORTED),
    ("window_left", _pair(dict(window_size_left=100)), UNSUPPORTED),
    ("softcap", _pair(dict(softcap=30.0)), UNSUPPORTED),
    ("alibi", _pair(dict(alibi_slopes=ADDR)), UNSUPPORTED),
    ("dropout", _pair(dict(p_dropout=0.1, rng_state=ADDR)), UNSUPPORTED),
    ("leftpad", _pair(dict(leftpad_k=ADDR, seqused_k=ADDR)), UNSUPPORTED),
    ("cu_seqlens_q", _pair(dict(cu_seqlens_q=ADDR, seqused_k=ADDR, total_q=2)), UNSUPPORTED),
    ("unsupported_first", _pair(dict(is_causal=1, q=0, h=7), dict(indices=0)), UNSUPPORTED),
    ("null_indices", _pair(topk=dict(indices=0)), NULLP),
    ("topk_0", _pair(k=0), BAD_SHAPE),
    ("k_row_stride_misaligned", _pair(dict(k_row_stride=72)), BAD_STRIDE),
    ("v_base_misaligned", _pair(dict(v=ADDR + 8)), BAD_STRIDE),
    ("v_row_stride_2_24", _pair(dict(v_row_stride=1 << 24)), BAD_STRIDE),
    ("descale_stride_negative", _pair(dict(k_descale_batch_stride=-1)), BAD_STRIDE),
    ("splits_without_workspace", _pair(dict(num_splits=3, workspace=0)), WORKSPACE),
]


@pytest.mark.parametrize("name,pair,want", CASES, ids=[c[0] for c in CASES])
def test_topk_kv8_validate_and_plan(name, pair, want):
    """An accepted call names its plan; a refused one gives its status from validate and from the launch entry (no stream is
    touched: the refusal comes first), and no plan."""
    lib = _lib.load()
    p, s = pair
    if isinstance(want, str):
        assert lib.fa_fwd_topk_kv8_validate(p, s) == OK
        assert lib.fa_fwd_topk_kv8_plan_name(p, s, 256).decode() == want
    else:
        assert lib.fa_fwd_topk_kv8_validate(p, s) == want == lib.fa_fwd_topk_kv8(p, s, None)
        assert lib.fa_fwd_topk_kv8_plan_name(p, s, 256) is None


@pytest.mark.parametrize("params,shape", [(dict(), dict()), (dict(num_splits=3), dict(b=2, sq=2, h=40, dv=272, d=16)),
                                          (dict(num_splits=0), dict(b=1, h=128)), (dict(num_splits=4), dict(k=130))])
def test_topk_kv8_workspace_is_the_16_bit_calls(params, shape):
    """The parts and the workspace come from shapes alone: what fa_fwd_topk_kv plans for the same shapes over a 16-bit cache."""
    lib = _lib.load()
    p8, s = _pair(params, **shape)
    p16, _ = _pair(params, **shape)
    assert lib.fa_fwd_topk_kv8_workspace_size(p8, s) == lib.fa_fwd_topk_kv_workspace_size(p16, s) >= 0
    assert (lib.fa_fwd_topk_kv8_workspace_size(p8, s) > 0) == (not lib.fa_fwd_topk_kv8_plan_name(p8, s, 256).decode().endswith("splits=1"))
