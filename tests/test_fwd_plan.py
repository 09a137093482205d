"""CPU tests of the forward routing: fa_fwd_plan_name() names the kernel plan_fwd() (csrc/fa_fwd_api.hip) picks -- family,
template shape and forms, block_m, split-KV, fp8 expansion, 256-column calls.  One row per branch of the routing, on a
device of 256 CUs; tests/test_persistent_gpu.py and the GPU suite check that the named kernels compute the right thing."""
import ctypes

import pytest

from flash_attention_annotated_amd import _lib

ADDR = 0x10000  # an aligned dummy address: nothing is dereferenced


def _params(b=2, h=16, h_k=None, sq=4096, sk=None, d=128, d_v=0, dtype=_lib.FA_DTYPE_BF16, **fields):
    """Dense contiguous (b, s, h, d) tensors; a dummy workspace large enough for any split or fp8 expansion."""
    h_k, sk, dv = h_k or h, sk or sq, d_v or d
    p = _lib.new_params()
    for f in ("q", "k", "v", "o", "softmax_lse", "workspace"):
        setattr(p, f, ADDR)
    p.workspace_bytes = 1 << 40
    p.b, p.seqlen_q, p.seqlen_k, p.h, p.h_k, p.d, p.d_v, p.dtype = b, sq, sk, h, h_k, d, d_v, dtype
    for t, rows, heads, width in (("q", sq, h, d), ("k", sk, h_k, d), ("v", sk, h_k, dv), ("o", sq, h, dv)):
        setattr(p, f"{t}_head_stride", width)
        setattr(p, f"{t}_row_stride", heads * width)
        setattr(p, f"{t}_batch_stride", rows * heads * width)
    p.softmax_scale = d ** -0.5
    p.window_size_left = p.window_size_right = -1
    for k, v in fields.items():
        setattr(p, k, v)
    return p


def _paged(**kw):
    return _params(block_table=ADDR, page_block_size=256, block_table_batch_stride=16, **kw)


def _qv(d=64, d_v=512, **kw):
    return _params(d=d, d_v=d_v, qv=ADDR, qv_head_stride=d, qv_row_stride=16 * d, qv_batch_stride=4096 * 16 * d, **kw)


FP8 = _lib.FA_DTYPE_FP8_E4M3
ROWS = [  # (id, params, persist mode, plan name)
    ("c2", _params(b=4, sq=8192), 0,
     "fwd_kernel_w64 D=128 DEFF=128 waves=4 PERSIST block_m=256 splits=1"),
    ("c2_handover", _params(b=4, sq=8192), -1,
     "fwd_kernel_w64 D=128 DEFF=128 waves=4 block_m=256 splits=1"),
    ("c3", _params(b=4, sq=16384, is_causal=1), 0,
     "fwd_kernel_w64 D=128 DEFF=128 waves=4 PERSIST block_m=256 splits=1"),
    ("d96", _params(d=96), 0,
     "fwd_kernel_w64 D=128 DEFF=96 waves=4 block_m=256 splits=1"),
    ("d64_short_causal", _params(b=16, sq=1024, d=64, is_causal=1), 0,
     "fwd_kernel D=64 waves=4 block_m=128 splits=1"),
    ("d64", _params(h=32, sq=8192, d=64), 0,
     "fwd_kernel_w64 D=64 DEFF=64 waves=4 block_m=256 splits=1"),
    ("decode", _params(b=8, h=32, h_k=8, sq=1, sk=8192), 0,
     "fwd_kernel D=128 waves=4 block_m=128 splits=4"),
    ("d128_paged", _paged(), 0,
     "fwd_kernel D=128 waves=8 block_m=256 splits=1"),
    ("d128_softcap", _params(b=4, softcap=30.0), 0,
     "fwd_kernel_d256 W=128 waves=4 SOFTCAP block_m=128 splits=1"),
    ("d64_alibi", _params(d=64, alibi_slopes=ADDR), 0,
     "fwd_kernel_d256 W=64 waves=4 ALIBI block_m=128 splits=1"),
    ("d128_softcap_alibi", _params(softcap=30.0, alibi_slopes=ADDR), 0,
     "fwd_kernel_w64 D=128 DEFF=128 waves=4 SOFTCAP block_m=256 splits=1"),
    ("d192", _params(d=192), 0,
     "fwd_kernel_d256 W=192 waves=4 block_m=128 splits=1"),
    ("d256_paged", _paged(d=256), 0,
     "fwd_kernel D=256 waves=4 block_m=128 splits=1"),
    ("d192_dv128", _params(d=192, d_v=128), 0,
     "fwd_kernel_d256 W=192 waves=4 block_m=128 splits=1"),
    ("d128_chunk", _params(attention_chunk=1024), 0,
     "fwd_kernel D=128 waves=8 EXTRA block_m=256 splits=1"),
    ("d128_dropout", _params(p_dropout=0.1, rng_state=ADDR), 0,
     "fwd_kernel D=128 waves=8 DROPOUT block_m=256 splits=1"),
    ("c5_fp8", _params(b=4, sq=8192, dtype=FP8), 0,
     "fwd_kernel_fp8 D=128 waves=4 block_m=256 splits=1"),
    ("fp8_d64", _params(d=64, dtype=FP8), 0,
     "fwd_kernel_w64 D=64 DEFF=64 waves=4 block_m=256 splits=1 fp8_expand"),
    ("qv_dv512", _qv(), 0,
     "fwd_kernel_qv DVT=512 waves=4 block_m=128 splits=1"),
    ("dv512_columns", _params(d=64, d_v=512), 0,
     "fwd_kernel_d256 W=256 waves=4 block_m=128 splits=1 cols=2"),
    ("dv384_paged", _paged(d=64, d_v=384), 0,
     "fwd_kernel_qv DVT=512 waves=4 block_m=128 splits=1"),
]


@pytest.mark.parametrize("params,persist,name", [r[1:] for r in ROWS], ids=[r[0] for r in ROWS])
def test_plan_name(built_lib, params, persist, name):
    assert built_lib.fa_fwd_validate(ctypes.byref(params)) == 0
    built_lib.fa_set_persist_mode(persist)
    try:
        assert built_lib.fa_fwd_plan_name(ctypes.byref(params), 256) == name.encode()
    finally:
        built_lib.fa_set_persist_mode(0)


def test_plan_name_follows_validation(built_lib):
    p = _params()
    p.h_k = 3
    assert built_lib.fa_fwd_validate(ctypes.byref(p)) == -4
    assert built_lib.fa_fwd_plan_name(ctypes.byref(p), 256) is None
    p = _params(b=8, h=32, h_k=8, sq=1, sk=8192)  # the decode row splits: without a workspace fa_fwd refuses it
    p.workspace = None
    assert built_lib.fa_fwd_plan_name(ctypes.byref(p), 256) is None


def test_persistent_form_needs_the_cu_count(built_lib):
    """The persistent form takes chains of at least two items per CU: c2 has 2048 work items."""
    p = _params(b=4, sq=8192)
    assert b" PERSIST " in built_lib.fa_fwd_plan_name(ctypes.byref(p), 256)
    assert b" PERSIST " not in built_lib.fa_fwd_plan_name(ctypes.byref(p), 2048)
    assert b" PERSIST " not in built_lib.fa_fwd_plan_name(ctypes.byref(p), 0)
