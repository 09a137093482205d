"""CPU tests of the learnable-sink entry points at the C-ABI (include/fa_fwd.h fa_fwd_sink / fa_sink_params, include/fa_bwd.h
fa_sink_grad): struct mirrors, the unchanged ABI version and fa_fwd_params size, validation, the refusals the reference's
sink surface does not have either, and that a sink never changes the plan.  No kernel is launched."""
import ctypes

import pytest

from flash_attention_annotated_amd import _lib
from plan_universe import UNIVERSE

ADDR = 0x100000  # aligned dummy address: nothing is dereferenced
KEYS = {form for _, form, _ in UNIVERSE}
UNSUPPORTED, NULL_POINTER, BAD_DTYPE, BAD_SHAPE, BAD_STRIDE, BAD_ABI = -7, -1, -2, -5, -6, -9


def _dense(b=2, sq=300, sk=715, h=4, h_k=2, d=128, d_v=0, **fields):
    dv = d_v or d
    p = _lib.new_params()
    for f in ("q", "k", "v", "o", "softmax_lse"):
        setattr(p, f, ADDR)
    p.b, p.seqlen_q, p.seqlen_k, p.h, p.h_k, p.d, p.d_v = b, sq, sk, h, h_k, d, d_v
    p.dtype = _lib.FA_DTYPE_BF16
    p.q_batch_stride, p.q_row_stride, p.q_head_stride = sq * h * d, h * d, d
    p.o_batch_stride, p.o_row_stride, p.o_head_stride = sq * h * dv, h * dv, dv
    p.k_batch_stride, p.k_row_stride, p.k_head_stride = sk * h_k * d, h_k * d, d
    p.v_batch_stride, p.v_row_stride, p.v_head_stride = sk * h_k * dv, h_k * dv, dv
    p.softmax_scale = d ** -0.5
    p.window_size_left = p.window_size_right = -1
    p.num_splits = 1
    p.flags = _lib.FA_FLAG_FA3_WINDOW
    for k, v in fields.items():
        setattr(p, k, v)
    return p


def _paged(page=256, **kw):
    p = _dense(**kw)
    p.block_table, p.block_table_batch_stride, p.page_block_size = ADDR, (p.seqlen_k + page - 1) // page, page
    p.seqlen_k = p.block_table_batch_stride * page
    p.k_batch_stride, p.v_batch_stride = page * p.h_k * p.d, page * p.h_k * p.d
    p.seqused_k = ADDR
    return p


def _varlen(**kw):
    p = _dense(cu_seqlens_q=ADDR, cu_seqlens_k=ADDR, total_q=900, total_k=1400, **kw)
    return p


def _sink(**fields):
    s = _lib.new_sink_params()
    s.learnable_sink = ADDR
    for k, v in fields.items():
        setattr(s, k, v)
    return s


def _with_workspace(lib, p):
    need = lib.fa_fwd_workspace_size(ctypes.byref(p))
    assert need >= 0
    if need:
        p.workspace, p.workspace_bytes = 0x10000000, need
    return need


def test_struct_mirrors_and_pinned_sizes(built_lib):
    assert built_lib.fa_sink_params_size() == ctypes.sizeof(_lib.FaSinkParams) == 32
    assert built_lib.fa_sink_grad_params_size() == ctypes.sizeof(_lib.FaSinkGradParams)
    assert built_lib.fa_abi_version() == _lib.FA_ABI_VERSION == 13
    assert built_lib.fa_fwd_params_size() == ctypes.sizeof(_lib.FaFwdParams) == 464


def test_bad_abi_and_null(built_lib):
    p = _dense()
    assert built_lib.fa_fwd_sink_validate(ctypes.byref(p), ctypes.byref(_sink())) == 0
    assert built_lib.fa_fwd_sink_validate(ctypes.byref(p), ctypes.byref(_sink(abi_version=12))) == BAD_ABI
    assert built_lib.fa_fwd_sink_validate(ctypes.byref(p), ctypes.byref(_sink(struct_size=24))) == BAD_ABI
    assert built_lib.fa_fwd_sink_validate(ctypes.byref(_dense(abi_version=12)), ctypes.byref(_sink())) == BAD_ABI
    assert built_lib.fa_fwd_sink_validate(ctypes.byref(p), ctypes.byref(_sink(learnable_sink=None))) == NULL_POINTER
    assert built_lib.fa_fwd_sink_validate(ctypes.byref(p), None) == NULL_POINTER
    assert built_lib.fa_fwd_sink_validate(None, ctypes.byref(_sink())) == NULL_POINTER
    # nothing is launched before validation: a NULL sink struct or a bad one never reaches a kernel
    assert built_lib.fa_fwd_sink(ctypes.byref(p), None, None) == NULL_POINTER
    assert built_lib.fa_fwd_sink(ctypes.byref(p), ctypes.byref(_sink(abi_version=12)), None) == BAD_ABI


def test_sink_fields_are_validated(built_lib):
    p = _dense()
    ok = lambda s, q=p: built_lib.fa_fwd_sink_validate(ctypes.byref(q), ctypes.byref(s))  # noqa: E731
    assert ok(_sink(sink_dtype=_lib.FA_DTYPE_FP32)) == 0
    assert ok(_sink(sink_dtype=_lib.FA_DTYPE_FP16)) == BAD_DTYPE
    assert ok(_sink(sink_dtype=_lib.FA_DTYPE_FP32, learnable_sink=ADDR + 2)) == BAD_STRIDE
    assert ok(_sink(learnable_sink=ADDR + 1)) == BAD_STRIDE
    assert ok(_sink(sink_head_stride=-1)) == BAD_STRIDE
    # the folded decode step: (b, 1, 16, d) viewed as (b, 8, 2, d), head stride = the group size, row stride 1
    fold = _dense(sq=8, h=2, h_k=2, sk=4096)
    assert ok(_sink(sink_head_stride=8, sink_row_stride=1), fold) == 0
    assert ok(_sink(sink_head_stride=8, sink_row_stride=1), _varlen()) == BAD_STRIDE
    # what fa_fwd_validate refuses stays refused
    assert ok(_sink(), _dense(h=4, h_k=3)) == -4


@pytest.mark.parametrize("what", ["fp8", "qv", "dropout", "alibi", "s_dmask", "qv_kernel_without_qv"])
def test_unsupported_with_a_sink(built_lib, what):
    p = {
        "fp8": lambda: _dense(dtype=_lib.FA_DTYPE_FP8_E4M3),
        "qv": lambda: _dense(d=64, d_v=512, qv=ADDR, qv_batch_stride=300 * 4 * 512, qv_row_stride=4 * 512, qv_head_stride=512),
        "dropout": lambda: _dense(p_dropout=0.1, rng_state=ADDR),
        "alibi": lambda: _dense(alibi_slopes=ADDR),
        "s_dmask": lambda: _dense(p_dropout=0.1, rng_state=ADDR, s_dmask=ADDR),
        "qv_kernel_without_qv": lambda: _paged(d=64, d_v=512),  # q/k <= 64 beside a paged 512-wide V runs fwd_kernel_qv
    }[what]()
    if what == "qv_kernel_without_qv":
        p.v_batch_stride = 256 * p.h_k * 512
        assert built_lib.fa_fwd_validate(ctypes.byref(p)) == 0
    assert built_lib.fa_fwd_sink_validate(ctypes.byref(p), ctypes.byref(_sink())) == UNSUPPORTED


FAMILIES = {
    "w64_d128": (lambda: _dense(is_causal=1), "fwd_kernel_w64 D=128 DEFF=128 waves=4"),
    "w64_d96": (lambda: _dense(d=96, is_causal=1), "fwd_kernel_w64 D=128 DEFF=96 waves=4"),
    "w64_d64_window": (lambda: _dense(d=64, window_size_left=400, window_size_right=100), "fwd_kernel_w64 D=64 DEFF=64 waves=4"),
    "persist": (lambda: _dense(b=16, h=16, h_k=4, sk=1024, is_causal=1), "fwd_kernel_w64 D=128 DEFF=128 waves=4 PERSIST"),
    "generic_short_q": (lambda: _dense(sq=100, is_causal=1), "fwd_kernel D=128 waves=4"),
    "generic_paged": (lambda: _paged(is_causal=1), "fwd_kernel D=128 waves=8"),
    "generic_chunk": (lambda: _dense(attention_chunk=300), "fwd_kernel D=128 waves=8 EXTRA"),
    "d256_192": (lambda: _dense(d=192, is_causal=1), "fwd_kernel_d256 W=192 waves=4"),
    "d256_256": (lambda: _dense(d=256, is_causal=1), "fwd_kernel_d256 W=256 waves=4"),
    "d256_softcap": (lambda: _dense(softcap=5.0, is_causal=1), "fwd_kernel_d256 W=128 waves=4 SOFTCAP"),
    "own_dv": (lambda: _dense(d=192, d_v=128), "fwd_kernel_d256 W=192 waves=4"),
    "splits3": (lambda: _dense(is_causal=1, num_splits=3), "fwd_kernel_w64 D=128 DEFF=128 waves=4"),
    "paged_splits3": (lambda: _paged(is_causal=1, num_splits=3), "fwd_kernel D=128 waves=8"),
    "decode_folded": (lambda: _paged(sq=8, h=2, h_k=2, sk=4096, d=64, num_splits=0), "fwd_kernel D=64 waves=8"),
    "varlen": (lambda: _varlen(is_causal=1), "fwd_kernel_w64 D=128 DEFF=128 waves=4"),
    "ragged_cache": (lambda: _dense(cu_seqlens_q=ADDR, seqused_k=ADDR, total_q=900, sk=4096), "fwd_kernel_w64 D=128 DEFF=128 waves=4"),
}


@pytest.mark.parametrize("form", list(FAMILIES))
def test_a_sink_never_changes_the_plan(built_lib, form):
    """fa_fwd_plan_name and fa_fwd_workspace_size read fa_fwd_params alone; the params a sink rides with are accepted as they
    are (same workspace), are not written to, and name the plan they named before -- a key of the plan universe, so no forward
    instantiation was added for the sink."""
    make, want = FAMILIES[form]
    p = make()
    need = _with_workspace(built_lib, p)
    before = bytes(p)
    assert built_lib.fa_fwd_validate(ctypes.byref(p)) == 0
    plan = built_lib.fa_fwd_plan_name(ctypes.byref(p), 256).decode()
    s = _sink(sink_head_stride=8, sink_row_stride=1) if form == "decode_folded" else _sink()
    assert built_lib.fa_fwd_sink_validate(ctypes.byref(p), ctypes.byref(s)) == 0
    assert bytes(p) == before
    assert built_lib.fa_fwd_workspace_size(ctypes.byref(p)) == need
    assert built_lib.fa_fwd_plan_name(ctypes.byref(p), 256).decode() == plan
    key = plan.split(" block_m=")[0]
    assert key == want and key in KEYS


def _grad(**fields):
    g = _lib.new_sink_grad_params()
    for f in ("softmax_lse", "softmax_d", "learnable_sink", "dsink"):
        setattr(g, f, ADDR)
    g.b, g.seqlen_q, g.h, g.softmax_d_row_len = 2, 300, 4, 384
    for k, v in fields.items():
        setattr(g, k, v)
    return g


def test_sink_grad_validation(built_lib):
    v = lambda g: built_lib.fa_sink_grad_validate(ctypes.byref(g))  # noqa: E731
    assert v(_grad()) == 0
    assert v(_grad(sink_dtype=_lib.FA_DTYPE_FP32)) == 0
    assert v(_grad(cu_seqlens_q=ADDR, total_q=900, softmax_d_row_len=900 + 256)) == 0
    assert built_lib.fa_sink_grad_validate(None) == NULL_POINTER
    assert v(_grad(abi_version=12)) == BAD_ABI
    assert v(_grad(struct_size=8)) == BAD_ABI
    assert v(_grad(sink_dtype=_lib.FA_DTYPE_FP16)) == BAD_DTYPE
    assert v(_grad(b=0)) == BAD_SHAPE
    assert v(_grad(h=0)) == BAD_SHAPE
    assert v(_grad(softmax_d_row_len=299)) == BAD_SHAPE
    assert v(_grad(cu_seqlens_q=ADDR, total_q=900, softmax_d_row_len=384)) == BAD_SHAPE
    for f in ("softmax_lse", "softmax_d", "learnable_sink", "dsink"):
        assert v(_grad(**{f: None})) == NULL_POINTER
    assert v(_grad(dsink=ADDR + 2)) == BAD_STRIDE
    assert built_lib.fa_sink_grad(ctypes.byref(_grad(abi_version=12)), None) == BAD_ABI
