"""CPU tests of the block-sparse entry points at the C-ABI (include/fa_fwd.h fa_fwd_block_sparse / fa_block_sparse_params):
the struct mirror, the unchanged ABI version and fa_fwd_params size, validation and every refusal, that plain params keep
their plan, and that every instantiation of the new kernel runs without scratch memory.  No kernel is launched."""
import ctypes
import re

import pytest

from device_asm import device_asm
from flash_attention_annotated_amd import _lib

ADDR = 0x100000  # aligned dummy address: nothing is dereferenced
UNSUPPORTED, NULL_POINTER, BAD_STRIDE, BAD_ABI, BAD_HEADS = -7, -1, -6, -9, -4
B, SQ, SK, H, HK = 2, 300, 715, 4, 2
NM, NK = 3, 6


def _dense(d=128, d_v=0, **fields):
    dv = d_v or d
    p = _lib.new_params()
    for f in ("q", "k", "v", "o", "softmax_lse"):
        setattr(p, f, ADDR)
    p.b, p.seqlen_q, p.seqlen_k, p.h, p.h_k, p.d, p.d_v = B, SQ, SK, H, HK, d, d_v
    p.dtype = _lib.FA_DTYPE_BF16
    p.q_batch_stride, p.q_row_stride, p.q_head_stride = SQ * H * d, H * d, d
    p.o_batch_stride, p.o_row_stride, p.o_head_stride = SQ * H * dv, H * dv, dv
    p.k_batch_stride, p.k_row_stride, p.k_head_stride = SK * HK * d, HK * d, d
    p.v_batch_stride, p.v_row_stride, p.v_head_stride = SK * HK * dv, HK * dv, dv
    p.softmax_scale = d ** -0.5
    p.window_size_left = p.window_size_right = -1
    p.num_splits = 1
    p.flags = _lib.FA_FLAG_FA3_WINDOW
    for k, v in fields.items():
        setattr(p, k, v)
    return p


def _sparse(full=True, **fields):
    s = _lib.new_block_sparse_params()
    s.mask_block_cnt, s.mask_block_idx = ADDR, ADDR + 4096
    s.mask_cnt_stride[:] = [H * NM, NM, 1, 0]
    s.mask_idx_stride[:] = [H * NM * NK, NM * NK, NK, 1]
    if full:
        s.full_block_cnt, s.full_block_idx = ADDR + 8192, ADDR + 12288
        s.full_cnt_stride[:] = [0, 0, 1, 0]  # broadcast over batch and heads
        s.full_idx_stride[:] = [0, 0, NK, 1]
    for k, v in fields.items():
        setattr(s, k, v)
    return s


def _sink():
    s = _lib.new_sink_params()
    s.learnable_sink = ADDR
    return s


def _validate(lib, p, s, sink=None):
    return lib.fa_fwd_block_sparse_validate(ctypes.byref(p), ctypes.byref(s), ctypes.byref(sink) if sink is not None else None)


def test_struct_mirror_and_pinned_sizes(built_lib):
    assert built_lib.fa_block_sparse_params_size() == ctypes.sizeof(_lib.FaBlockSparseParams) == 8 + 4 * 8 + 16 * 8 + 8
    assert built_lib.fa_abi_version() == _lib.FA_ABI_VERSION == 13
    assert built_lib.fa_fwd_params_size() == ctypes.sizeof(_lib.FaFwdParams) == 464
    assert built_lib.fa_sink_params_size() == ctypes.sizeof(_lib.FaSinkParams) == 32
    for sym in ("fa_fwd_block_sparse", "fa_fwd_block_sparse_validate", "fa_block_sparse_params_size"):
        assert sym in _lib.EXPORTED_SYMBOLS and hasattr(built_lib, sym)


@pytest.mark.parametrize("kw", [dict(), dict(is_causal=1), dict(window_size_left=200, window_size_right=50), dict(softcap=5.0),
                                dict(d=64), dict(d=256), dict(d=192, d_v=128), dict(dtype=_lib.FA_DTYPE_FP16),
                                dict(num_splits=0)], ids=str)
def test_accepted(built_lib, kw):
    assert _validate(built_lib, _dense(**kw), _sparse()) == 0
    assert _validate(built_lib, _dense(**kw), _sparse(full=False)) == 0
    assert _validate(built_lib, _dense(**kw), _sparse(), _sink()) == 0


def test_bad_abi_and_null(built_lib):
    p, s = _dense(), _sparse()
    assert built_lib.fa_fwd_block_sparse_validate(None, ctypes.byref(s), None) == NULL_POINTER
    assert built_lib.fa_fwd_block_sparse_validate(ctypes.byref(p), None, None) == NULL_POINTER
    assert _validate(built_lib, _dense(abi_version=12), s) == BAD_ABI
    assert _validate(built_lib, p, _sparse(abi_version=12)) == BAD_ABI
    assert _validate(built_lib, p, _sparse(struct_size=64)) == BAD_ABI
    # the mask list is required; cnt and idx of the full list come together
    assert _validate(built_lib, p, _sparse(mask_block_cnt=None)) == NULL_POINTER
    assert _validate(built_lib, p, _sparse(mask_block_idx=None)) == NULL_POINTER
    assert _validate(built_lib, p, _sparse(mask_block_cnt=None, mask_block_idx=None)) == NULL_POINTER
    assert _validate(built_lib, p, _sparse(full_block_idx=None)) == NULL_POINTER
    assert _validate(built_lib, p, _sparse(full_block_cnt=None)) == NULL_POINTER
    assert _validate(built_lib, p, _sparse(mask_block_idx=ADDR + 2)) == BAD_STRIDE
    bad = _sparse()
    bad.mask_idx_stride[1] = -1
    assert _validate(built_lib, p, bad) == BAD_STRIDE
    # what fa_fwd_validate refuses stays refused, a bad sink too
    assert _validate(built_lib, _dense(h_k=3), s) == BAD_HEADS
    sink = _sink()
    sink.sink_dtype = _lib.FA_DTYPE_FP16
    assert _validate(built_lib, p, s, sink) == -2
    # nothing is launched before validation
    assert built_lib.fa_fwd_block_sparse(ctypes.byref(p), ctypes.byref(_sparse(abi_version=12)), None, None) == BAD_ABI
    assert built_lib.fa_fwd_block_sparse(ctypes.byref(p), ctypes.byref(_sparse(mask_block_cnt=None)), None, None) == NULL_POINTER


@pytest.mark.parametrize("block", [dict(block_m=64), dict(block_n=64), dict(block_m=256, block_n=256), dict(block_m=0)], ids=str)
def test_block_size_other_than_128(built_lib, block):
    assert _validate(built_lib, _dense(), _sparse(**block)) == UNSUPPORTED


REFUSED = {
    "cu_seqlens_q": dict(cu_seqlens_q=ADDR, total_q=600),
    "cu_seqlens_qk": dict(cu_seqlens_q=ADDR, cu_seqlens_k=ADDR, total_q=600, total_k=1430),
    "cu_seqlens_k": dict(cu_seqlens_k=ADDR),
    "seqused_q": dict(seqused_q=ADDR),
    "seqused_k": dict(seqused_k=ADDR),
    "page_table": dict(block_table=ADDR, block_table_batch_stride=3, page_block_size=256),
    "kv_batch_idx": dict(kv_batch_idx=ADDR),
    "leftpad_k": dict(leftpad_k=ADDR),
    "fp8": dict(dtype=_lib.FA_DTYPE_FP8_E4M3),
    "qv": dict(d=64, d_v=256, qv=ADDR, qv_batch_stride=SQ * H * 256, qv_row_stride=H * 256, qv_head_stride=256),
    "dropout": dict(p_dropout=0.1, rng_state=ADDR),
    "s_dmask": dict(p_dropout=0.1, rng_state=ADDR, s_dmask=ADDR),
    "alibi": dict(alibi_slopes=ADDR),
    "attention_chunk": dict(attention_chunk=256),
    "num_splits": dict(num_splits=2, workspace=0x10000000, workspace_bytes=1 << 30),
    "d_v_above_256": dict(d=64, d_v=512),
}


@pytest.mark.parametrize("what", list(REFUSED))
def test_refused_combinations(built_lib, what):
    p = _dense(**REFUSED[what])
    assert _validate(built_lib, p, _sparse()) == UNSUPPORTED
    assert _validate(built_lib, p, _sparse(), _sink()) == UNSUPPORTED
    # ... before anything the params may lack: no tensors, and no mask list either
    bare = _dense(**REFUSED[what])
    for f in ("q", "k", "v", "o", "softmax_lse"):
        setattr(bare, f, None)
    assert _validate(built_lib, bare, _sparse(mask_block_cnt=None, mask_block_idx=None)) == UNSUPPORTED
    assert built_lib.fa_fwd_block_sparse(ctypes.byref(p), ctypes.byref(_sparse()), None, None) == UNSUPPORTED


@pytest.mark.parametrize("kw", [dict(is_causal=1), dict(d=64, window_size_left=400, window_size_right=100), dict(d=192, d_v=128),
                                dict(softcap=5.0)], ids=str)
def test_plain_params_keep_their_plan(built_lib, kw):
    """fa_fwd_plan_name / fa_fwd_workspace_size read fa_fwd_params alone: validating them for a block-sparse call neither
    writes to them nor changes what they name."""
    p = _dense(**kw)
    before = bytes(p)
    plan = built_lib.fa_fwd_plan_name(ctypes.byref(p), 256)
    need = built_lib.fa_fwd_workspace_size(ctypes.byref(p))
    assert plan is not None and plan.startswith(b"fwd_kernel") and need == 0
    assert _validate(built_lib, p, _sparse()) == 0
    assert bytes(p) == before
    assert built_lib.fa_fwd_plan_name(ctypes.byref(p), 256) == plan
    assert built_lib.fa_fwd_workspace_size(ctypes.byref(p)) == need


def test_new_kernel_has_zero_scratch():
    """Every instantiation of fa::bs_fwd_kernel -- 2 element types x head-dim tiles 64 / 128 / 256 x softcap -- keeps its
    registers: .amdhsa_private_segment_fixed_size 0."""
    text = open(device_asm("fa_fwd_api.hip")).read()
    scratch = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", text, re.S):
        if m.group(1).startswith("_ZN2fa13bs_fwd_kernel"):
            scratch[m.group(1)] = int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", m.group(2)).group(1))
    assert len(scratch) == 12, sorted(scratch)
    assert {k for k, v in scratch.items() if v != 0} == set()
