"""CPU tests of the block-sparse backward at the C-ABI (include/fa_bwd.h fa_bwd_block_sparse / fa_block_sparse_bwd_params): the
struct mirror, the unchanged ABI version and fa_bwd_params size, the accepted set and every refusal, that plain params keep
their plan, and the device code of the new translation unit: exactly its 16 kernels, none with scratch memory, clean under
tools/isa_hazards.py.  No kernel is launched."""
import ctypes
import os
import re
import sys

import pytest

from device_asm import device_asm
from flash_attention_annotated_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ADDR = 0x100000  # aligned dummy address: nothing is dereferenced
UNSUPPORTED, NULL_POINTER, BAD_STRIDE, BAD_ABI, BAD_HEADS = -7, -1, -6, -9, -4
B, SQ, SK, H, HK = 2, 300, 715, 4, 2
NM, NK = 3, 6


def _dense(d=128, **fields):
    p = _lib.new_bwd_params()
    for f in ("q", "k", "v", "o", "dout", "softmax_lse", "dq", "dk", "dv", "softmax_d"):
        setattr(p, f, ADDR)
    p.b, p.seqlen_q, p.seqlen_k, p.h, p.h_k, p.d = B, SQ, SK, H, HK, d
    p.dtype = _lib.FA_DTYPE_BF16
    for t, s, heads in (("q", SQ, H), ("o", SQ, H), ("do", SQ, H), ("dq", SQ, H), ("k", SK, HK), ("v", SK, HK), ("dk", SK, HK),
                        ("dv", SK, HK)):
        setattr(p, f"{t}_batch_stride", s * heads * d)
        setattr(p, f"{t}_row_stride", heads * d)
        setattr(p, f"{t}_head_stride", d)
    p.softmax_d_row_len = 384
    p.softmax_scale = d ** -0.5
    p.window_size_left = p.window_size_right = -1
    p.flags = _lib.FA_FLAG_FA3_WINDOW
    for k, v in fields.items():
        setattr(p, k, v)
    return p


def _fwd_lists(full=True, **fields):
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


def _key_lists(**fields):
    s = _lib.new_block_sparse_bwd_params()
    s.q_block_cnt, s.q_block_idx = ADDR + 16384, ADDR + 20480
    s.q_cnt_stride[:] = [H * NK, NK, 1, 0]
    s.q_idx_stride[:] = [H * NK * NM, NK * NM, NM, 1]
    for k, v in fields.items():
        setattr(s, k, v)
    return s


def _validate(lib, p, s, kl):
    return lib.fa_bwd_block_sparse_validate(ctypes.byref(p), ctypes.byref(s), ctypes.byref(kl))


def test_struct_mirror_and_pinned_sizes(built_lib):
    assert built_lib.fa_block_sparse_bwd_params_size() == ctypes.sizeof(_lib.FaBlockSparseBwdParams) == 8 + 2 * 8 + 8 * 8 + 8
    assert built_lib.fa_abi_version() == _lib.FA_ABI_VERSION == 13
    assert built_lib.fa_bwd_params_size() == ctypes.sizeof(_lib.FaBwdParams) == 408
    assert built_lib.fa_block_sparse_params_size() == ctypes.sizeof(_lib.FaBlockSparseParams)
    for sym in ("fa_bwd_block_sparse", "fa_bwd_block_sparse_validate", "fa_block_sparse_bwd_params_size"):
        assert sym in _lib.EXPORTED_SYMBOLS and hasattr(built_lib, sym)
    kl = _lib.new_block_sparse_bwd_params()
    assert (kl.abi_version, kl.struct_size, kl.block_m, kl.block_n) == (13, ctypes.sizeof(kl), 128, 128)


@pytest.mark.parametrize("kw", [dict(), dict(is_causal=1), dict(window_size_left=200, window_size_right=50), dict(softcap=5.0),
                                dict(d=64), dict(d=32), dict(d=96), dict(d=128, d_v=128), dict(dtype=_lib.FA_DTYPE_FP16),
                                dict(h_k=H), dict(h_k=1)], ids=str)
def test_accepted(built_lib, kw):
    assert _validate(built_lib, _dense(**kw), _fwd_lists(), _key_lists()) == 0
    assert _validate(built_lib, _dense(**kw), _fwd_lists(full=False), _key_lists()) == 0
    broadcast = _key_lists()
    broadcast.q_cnt_stride[:] = [0, 0, 1, 0]
    broadcast.q_idx_stride[:] = [0, 0, NM, 1]
    assert _validate(built_lib, _dense(**kw), _fwd_lists(), broadcast) == 0


def test_bad_abi_null_and_strides(built_lib):
    p, s, kl = _dense(), _fwd_lists(), _key_lists()
    f = built_lib.fa_bwd_block_sparse_validate
    assert f(None, ctypes.byref(s), ctypes.byref(kl)) == NULL_POINTER
    assert f(ctypes.byref(p), None, ctypes.byref(kl)) == NULL_POINTER
    assert f(ctypes.byref(p), ctypes.byref(s), None) == NULL_POINTER
    assert _validate(built_lib, _dense(abi_version=12), s, kl) == BAD_ABI
    assert _validate(built_lib, p, _fwd_lists(abi_version=12), kl) == BAD_ABI
    assert _validate(built_lib, p, s, _key_lists(abi_version=12)) == BAD_ABI
    assert _validate(built_lib, p, s, _key_lists(struct_size=64)) == BAD_ABI
    # the forward's codes: the mask list and the key-major list are required, cnt and idx of the full list come together
    assert _validate(built_lib, p, _fwd_lists(mask_block_cnt=None), kl) == NULL_POINTER
    assert _validate(built_lib, p, _fwd_lists(mask_block_idx=None), kl) == NULL_POINTER
    assert _validate(built_lib, p, _fwd_lists(full_block_idx=None), kl) == NULL_POINTER
    assert _validate(built_lib, p, s, _key_lists(q_block_cnt=None)) == NULL_POINTER
    assert _validate(built_lib, p, s, _key_lists(q_block_idx=None)) == NULL_POINTER
    assert _validate(built_lib, p, _fwd_lists(mask_block_idx=ADDR + 2), kl) == BAD_STRIDE
    assert _validate(built_lib, p, s, _key_lists(q_block_cnt=ADDR + 2)) == BAD_STRIDE
    assert _validate(built_lib, p, s, _key_lists(q_block_idx=ADDR + 1)) == BAD_STRIDE
    for field in ("q_cnt_stride", "q_idx_stride"):
        bad = _key_lists()
        getattr(bad, field)[1] = -1
        assert _validate(built_lib, p, s, bad) == BAD_STRIDE
    bad = _fwd_lists()
    bad.mask_idx_stride[3] = -1
    assert _validate(built_lib, p, bad, kl) == BAD_STRIDE
    # what fa_bwd_validate refuses stays refused
    assert _validate(built_lib, _dense(h_k=3), s, kl) == BAD_HEADS
    assert _validate(built_lib, _dense(dq=None), s, kl) == NULL_POINTER
    # nothing is launched before validation
    assert built_lib.fa_bwd_block_sparse(ctypes.byref(p), ctypes.byref(s), ctypes.byref(_key_lists(abi_version=12)), None) == BAD_ABI
    assert built_lib.fa_bwd_block_sparse(ctypes.byref(p), ctypes.byref(s), ctypes.byref(_key_lists(q_block_cnt=None)), None) == NULL_POINTER


@pytest.mark.parametrize("block", [dict(block_m=64), dict(block_n=64), dict(block_m=256, block_n=256), dict(block_m=0)], ids=str)
def test_block_size_other_than_128(built_lib, block):
    assert _validate(built_lib, _dense(), _fwd_lists(**block), _key_lists()) == UNSUPPORTED
    assert _validate(built_lib, _dense(), _fwd_lists(), _key_lists(**block)) == UNSUPPORTED


REFUSED = {
    "cu_seqlens_q": dict(cu_seqlens_q=ADDR, total_q=600),
    "cu_seqlens_qk": dict(cu_seqlens_q=ADDR, cu_seqlens_k=ADDR, total_q=600, total_k=1430),
    "cu_seqlens_k": dict(cu_seqlens_k=ADDR),
    "alibi": dict(alibi_slopes=ADDR),
    "dropout": dict(p_dropout=0.1, rng_state=ADDR),
    "d_192": dict(d=192),
    "d_256": dict(d=256),
    "d_v_differs": dict(d=128, d_v=64),
    "d_v_wide": dict(d=192, d_v=128),
}


@pytest.mark.parametrize("what", list(REFUSED))
def test_refused_combinations(built_lib, what):
    p = _dense(**REFUSED[what])
    assert _validate(built_lib, p, _fwd_lists(), _key_lists()) == UNSUPPORTED
    # ... before anything the params may lack: no tensors, and no lists either
    bare = _dense(**REFUSED[what])
    for f in ("q", "k", "v", "o", "dout", "softmax_lse", "dq", "dk", "dv", "softmax_d"):
        setattr(bare, f, None)
    assert _validate(built_lib, bare, _fwd_lists(mask_block_cnt=None, mask_block_idx=None),
                     _key_lists(q_block_cnt=None, q_block_idx=None)) == UNSUPPORTED
    assert built_lib.fa_bwd_block_sparse(ctypes.byref(p), ctypes.byref(_fwd_lists()), ctypes.byref(_key_lists()), None) == UNSUPPORTED


@pytest.mark.parametrize("kw", [dict(), dict(is_causal=1), dict(d=64, softcap=5.0), dict(d=96)], ids=str)
def test_plain_params_keep_their_plan(built_lib, kw):
    """fa_bwd_plan_name reads fa_bwd_params alone: validating them for a block-sparse call neither writes to them nor changes
    what they name -- the dense kernels."""
    p = _dense(**kw)
    before = bytes(p)
    plan = built_lib.fa_bwd_plan_name(ctypes.byref(p))
    assert plan is not None and plan.startswith(b"bwd_dot LPR=") and b"bs_bwd" not in plan and b"| bwd_dkdv D=" in plan
    assert _validate(built_lib, p, _fwd_lists(), _key_lists()) == 0
    assert bytes(p) == before
    assert built_lib.fa_bwd_plan_name(ctypes.byref(p)) == plan


@pytest.fixture(scope="module")
def unit_asm():
    return device_asm("fa_bwd_bs_api.hip")


def test_new_unit_holds_exactly_its_16_kernels_without_scratch(unit_asm):
    """2 kernels x 2 element types x head-dim tiles 64 / 128 x softcap, nothing else (bwd_dot_kernel stays in fa_bwd_api.hip),
    every one with .amdhsa_private_segment_fixed_size 0."""
    text = open(unit_asm).read()
    scratch = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", text, re.S):
        scratch[m.group(1)] = int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", m.group(2)).group(1))
    want = {f"_ZN2fa{len(k)}{k}I{t}Li{d}ELb{sc}EEEvNS_11BsBwdParamsE"
            for k in ("bs_bwd_dq_kernel", "bs_bwd_dkdv_kernel") for t in ("DF16b", "DF16_") for d in (64, 128) for sc in (0, 1)}
    assert len(want) == 16 and set(scratch) == want, sorted(set(scratch) ^ want)
    assert {k for k, v in scratch.items() if v != 0} == set()


def test_new_unit_has_no_unpadded_mfma_or_trans_hazards(unit_asm):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_hazards
    violations = isa_hazards.scan(str(unit_asm))
    assert not violations, violations[:5]
