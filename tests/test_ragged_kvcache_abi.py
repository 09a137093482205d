"""CPU tests of the ragged-queries-over-a-KV-cache form at the C-ABI (include/fa_fwd.h): fa_fwd takes cu_seqlens_q without
cu_seqlens_k when seqused_k gives the fill levels of a batched or paged cache, plans it like any varlen problem (every plan
text an existing key of tests/plan_universe.py), splits the key range on request, and refuses fp8 / dropout / ALiBi on it.
The two ragged entry points (fa_kvcache_append_varlen, fa_rotary_apply_varlen) exist, mirror their ctypes structs and
validate like their dense twins.  ABI version and the sizes of the three older structs are unchanged.  No kernel is launched."""
import ctypes
import os
import re

import pytest

from flash_attention_annotated_amd import _lib
from plan_universe import UNIVERSE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ADDR = 0x100000  # aligned dummy address: nothing is dereferenced
KEYS = {form for _, form, _ in UNIVERSE}


def _ragged(b=6, total_q=900, max_sq=512, h=8, h_k=2, cap=4096, d=128, d_v=0, b_cache=None, **fields):
    """q / o (total_q, h, .) with cu_seqlens_q, k / v a (b_cache, cap, h_k, .) cache with its fill levels in seqused_k."""
    dv = d_v or d
    p = _lib.new_params()
    for f in ("q", "k", "v", "o", "softmax_lse", "cu_seqlens_q", "seqused_k"):
        setattr(p, f, ADDR)
    p.b, p.seqlen_q, p.seqlen_k, p.h, p.h_k, p.d, p.d_v, p.total_q = b, max_sq, cap, h, h_k, d, d_v, total_q
    p.dtype = _lib.FA_DTYPE_BF16
    p.q_row_stride, p.q_head_stride = h * d, d
    p.o_row_stride, p.o_head_stride = h * dv, dv
    p.k_batch_stride, p.k_row_stride, p.k_head_stride = cap * h_k * d, h_k * d, d
    p.v_batch_stride, p.v_row_stride, p.v_head_stride = cap * h_k * dv, h_k * dv, dv
    p.softmax_scale = d ** -0.5
    p.window_size_left = p.window_size_right = -1
    p.num_splits = 1
    p.flags = _lib.FA_FLAG_FA3_WINDOW
    for k, v in fields.items():
        setattr(p, k, v)
    return p


def _paged(page=64, **kw):
    p = _ragged(**kw)
    p.block_table, p.block_table_batch_stride, p.page_block_size = ADDR, p.seqlen_k // page, page
    dv = p.d_v or p.d
    p.k_batch_stride, p.v_batch_stride = page * p.h_k * p.d, page * p.h_k * dv
    return p


def _qv(**kw):
    p = _paged(d=64, d_v=512, h=16, h_k=1, **kw)
    p.qv, p.qv_row_stride, p.qv_head_stride = ADDR, 16 * 512, 512
    p.softmax_scale = (64 + 512) ** -0.5
    return p


def _with_workspace(lib, p):
    need = lib.fa_fwd_workspace_size(ctypes.byref(p))
    assert need >= 0
    if need:
        p.workspace, p.workspace_bytes = 0x10000000, need
    return need


FORMS = {
    "plain": (lambda: _ragged(), "fwd_kernel_w64 D=128 DEFF=128 waves=4 block_m=256 splits=1"),
    "causal_d64": (lambda: _ragged(d=64, is_causal=1), "fwd_kernel_w64 D=64 DEFF=64 waves=4 block_m=256 splits=1"),
    "paged": (lambda: _paged(), "fwd_kernel D=128 waves=8 block_m=256 splits=1"),
    "kv_batch_idx": (lambda: _ragged(b_cache=9, kv_batch_idx=ADDR), "fwd_kernel_w64 D=128 DEFF=128 waves=4 block_m=256 splits=1"),
    "leftpad": (lambda: _ragged(leftpad_k=ADDR), "fwd_kernel_w64 D=128 DEFF=128 waves=4 block_m=256 splits=1"),
    "softcap": (lambda: _ragged(softcap=30.0), "fwd_kernel_d256 W=128 waves=4 SOFTCAP block_m=128 splits=1"),
    "d256": (lambda: _ragged(d=256), "fwd_kernel_d256 W=256 waves=4 block_m=128 splits=1"),
    "qv": (lambda: _qv(), "fwd_kernel_qv DVT=512 waves=4 block_m=128 splits=1"),
    "splits4": (lambda: _ragged(num_splits=4), "fwd_kernel_w64 D=128 DEFF=128 waves=4 block_m=256 splits=4"),
    "paged_splits4": (lambda: _paged(num_splits=4), "fwd_kernel D=128 waves=8 block_m=256 splits=4"),
    "qv_splits4": (lambda: _qv(num_splits=4), "fwd_kernel_qv DVT=512 waves=4 block_m=128 splits=4"),
}


@pytest.mark.parametrize("form", list(FORMS))
def test_ragged_cache_form_is_planned(built_lib, form):
    """fa_fwd_plan_name is non-NULL for the mixed form (NULL before it existed), and its text is a plan-universe key."""
    make, want = FORMS[form]
    p = make()
    _with_workspace(built_lib, p)
    assert built_lib.fa_fwd_validate(ctypes.byref(p)) == 0
    name = built_lib.fa_fwd_plan_name(ctypes.byref(p), 256)
    assert name is not None
    name = name.decode()
    assert name == want
    assert re.sub(r" (block_m|splits|cols)=\d+| fp8_expand", "", name) in KEYS
    assert " PERSIST" not in name


def test_split_workspace_formula(built_lib):
    """splits x (total_q h d_v + h total_q) x 4 bytes, each part rounded up to 256 as the plan rounds."""
    rnd = lambda x: (x + 255) // 256 * 256  # noqa: E731
    for make, dv in ((lambda **kw: _ragged(**kw), 128), (lambda **kw: _paged(**kw), 128), (lambda **kw: _qv(**kw), 512)):
        for total_q, splits in ((900, 4), (77, 2), (1, 5)):
            p = make(total_q=total_q, num_splits=splits)
            want = rnd(splits * total_q * p.h * dv * 4) + rnd(splits * p.h * total_q * 4)
            assert built_lib.fa_fwd_workspace_size(ctypes.byref(p)) == want
            p.workspace, p.workspace_bytes = 0x10000000, want - 256
            assert built_lib.fa_fwd_validate(ctypes.byref(p)) == -11
            p.workspace_bytes = want
            assert built_lib.fa_fwd_validate(ctypes.byref(p)) == 0
    # num_splits = 1: nothing; the cu_seqlens_q + cu_seqlens_k training path never splits, whatever is asked
    assert built_lib.fa_fwd_workspace_size(ctypes.byref(_ragged())) == 0
    p = _ragged(num_splits=4, cu_seqlens_k=ADDR, total_k=900)
    p.k_batch_stride = p.v_batch_stride = 0
    assert built_lib.fa_fwd_workspace_size(ctypes.byref(p)) == 0
    assert built_lib.fa_fwd_plan_name(ctypes.byref(p), 256).decode().endswith("splits=1")


def test_split_heuristic_counts_tiles_from_total_q(built_lib):
    """num_splits = 0: a decode-heavy ragged step (few row blocks) splits, a prefill-heavy one does not; no device data is read
    (the pointers are dummies)."""
    few = _ragged(b=4, total_q=4, max_sq=1, cap=8192, num_splits=0)
    assert built_lib.fa_fwd_workspace_size(ctypes.byref(few)) > 0
    many = _ragged(b=64, total_q=64 * 2048, max_sq=2048, h=32, cap=8192, num_splits=0)
    assert built_lib.fa_fwd_workspace_size(ctypes.byref(many)) == 0
    # total_q bounds the tiles even when max_seqlen_q x b would not: one long sequence among single tokens
    mixed = _ragged(b=128, total_q=127 + 2048, max_sq=2048, h=32, cap=8192, num_splits=0)
    assert built_lib.fa_fwd_workspace_size(ctypes.byref(mixed)) == 0


@pytest.mark.parametrize("mutate", [
    lambda p: setattr(p, "dtype", _lib.FA_DTYPE_FP8_E4M3),
    lambda p: (setattr(p, "p_dropout", 0.1), setattr(p, "rng_state", ADDR)),
    lambda p: setattr(p, "alibi_slopes", ADDR),
], ids=["fp8", "dropout", "alibi"])
def test_ragged_cache_form_unsupported(built_lib, mutate):
    p = _ragged()
    mutate(p)
    assert built_lib.fa_fwd_validate(ctypes.byref(p)) == -7
    assert built_lib.fa_fwd_plan_name(ctypes.byref(p), 256) is None


def test_ragged_cache_form_shape_rules(built_lib):
    p = _ragged()
    p.cu_seqlens_q = None  # cu_seqlens_k alone
    p.cu_seqlens_k = ADDR
    assert built_lib.fa_fwd_validate(ctypes.byref(p)) == -5
    p = _ragged()
    p.seqused_k = None     # the fill levels are required
    assert built_lib.fa_fwd_validate(ctypes.byref(p)) == -5
    p = _ragged()
    p.k_batch_stride += 4  # the cache's batch stride counts on this form
    assert built_lib.fa_fwd_validate(ctypes.byref(p)) == -6
    p = _ragged(cu_seqlens_k=ADDR, total_k=900, kv_batch_idx=ADDR)  # kv_batch_idx stays a dense-K/V argument
    assert built_lib.fa_fwd_validate(ctypes.byref(p)) == -7
    p = _paged(kv_batch_idx=ADDR)
    assert built_lib.fa_fwd_validate(ctypes.byref(p)) == -7


def _struct_fields(name):
    text = open(os.path.join(ROOT, "include", "fa_fwd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        base = re.match(r"(?:const\s+)?\w+\s*\**\s*", decl).group(0)
        fields += [part.strip().lstrip("*").strip() for part in decl[len(base):].split(",")]
    return fields


def test_new_entry_points_and_struct_mirrors(built_lib):
    assert _lib.FA_ABI_VERSION == 13 and built_lib.fa_abi_version() == 13
    for sym in ("fa_kvcache_append_varlen", "fa_kvcache_append_varlen_params_size", "fa_rotary_apply_varlen",
                "fa_rotary_varlen_params_size"):
        assert hasattr(built_lib, sym) and sym in _lib.EXPORTED_SYMBOLS
    assert built_lib.fa_kvcache_append_varlen_params_size() == ctypes.sizeof(_lib.FaKvcacheAppendVarlenParams)
    assert built_lib.fa_rotary_varlen_params_size() == ctypes.sizeof(_lib.FaRotaryVarlenParams)
    assert [f[0] for f in _lib.FaKvcacheAppendVarlenParams._fields_] == _struct_fields("fa_kvcache_append_varlen_params")
    assert [f[0] for f in _lib.FaRotaryVarlenParams._fields_] == _struct_fields("fa_rotary_varlen_params")


def test_old_struct_sizes_unchanged(built_lib):
    """ABI 13 as released: new work has entry points and structs of its own."""
    assert built_lib.fa_fwd_params_size() == ctypes.sizeof(_lib.FaFwdParams) == 464
    assert built_lib.fa_kvcache_append_params_size() == ctypes.sizeof(_lib.FaKvcacheAppendParams) == 240
    assert built_lib.fa_rotary_params_size() == ctypes.sizeof(_lib.FaRotaryParams) == 128


def _append(b=3, total=40, h_k=2, d=128, cap=1024):
    p = _lib.FaKvcacheAppendVarlenParams()
    p.abi_version, p.struct_size = _lib.FA_ABI_VERSION, ctypes.sizeof(p)
    for f in ("k_new", "v_new", "k_cache", "v_cache", "cu_seqlens_k_new", "cache_seqlens", "seqused_out"):
        setattr(p, f, ADDR)
    p.b, p.total_k_new, p.seqlen_cache, p.h_k, p.d, p.dtype = b, total, cap, h_k, d, _lib.FA_DTYPE_BF16
    p.knew_row_stride = p.vnew_row_stride = p.kcache_row_stride = p.vcache_row_stride = h_k * d
    p.knew_head_stride = p.vnew_head_stride = p.kcache_head_stride = p.vcache_head_stride = d
    p.kcache_batch_stride = p.vcache_batch_stride = cap * h_k * d
    return p


@pytest.mark.parametrize("mutate,code", [
    (lambda p: setattr(p, "abi_version", 12), -9),
    (lambda p: setattr(p, "struct_size", 8), -9),
    (lambda p: setattr(p, "dtype", _lib.FA_DTYPE_FP8_E4M3), -2),
    (lambda p: setattr(p, "k_new", ADDR + 8), -6),
    (lambda p: setattr(p, "vcache_row_stride", 4), -6),
    (lambda p: setattr(p, "d", 132), -3),
    (lambda p: setattr(p, "d_v", 520), -3),
    (lambda p: setattr(p, "b", 0), -5),
    (lambda p: setattr(p, "seqused_out", None), -1),
    (lambda p: setattr(p, "cu_seqlens_k_new", None), -1),
    (lambda p: (setattr(p, "block_table", ADDR), setattr(p, "page_block_size", 16), setattr(p, "cache_batch_idx", ADDR)), -5),
    (lambda p: (setattr(p, "rotary_cos", ADDR), setattr(p, "rotary_sin", ADDR), setattr(p, "rotary_dim", 24)), -5),
    (lambda p: (setattr(p, "rotary_cos", ADDR + 2), setattr(p, "rotary_sin", ADDR), setattr(p, "rotary_dim", 32)), -6),
])
def test_append_varlen_rejects(built_lib, mutate, code):
    p = _append()
    mutate(p)
    assert built_lib.fa_kvcache_append_varlen(ctypes.byref(p), None) == code
    assert built_lib.fa_kvcache_append_varlen(None, None) == -1


def _rotary(b=3, total=40, h=4, d=128):
    p = _lib.FaRotaryVarlenParams()
    p.abi_version, p.struct_size = _lib.FA_ABI_VERSION, ctypes.sizeof(p)
    for f in ("src", "dst", "rotary_cos", "rotary_sin", "cu_seqlens_q", "offsets"):
        setattr(p, f, ADDR)
    p.b, p.total_q, p.h, p.d, p.dtype, p.rotary_dim = b, total, h, d, _lib.FA_DTYPE_FP16, 64
    p.src_row_stride = p.dst_row_stride = h * d
    p.src_head_stride = p.dst_head_stride = d
    return p


@pytest.mark.parametrize("mutate,code", [
    (lambda p: setattr(p, "abi_version", 12), -9),
    (lambda p: setattr(p, "dtype", _lib.FA_DTYPE_FP8_E4M3), -2),
    (lambda p: setattr(p, "dst", ADDR + 4), -6),
    (lambda p: setattr(p, "src_head_stride", 12), -6),
    (lambda p: setattr(p, "rotary_dim", 8), -5),
    (lambda p: setattr(p, "rotary_dim", 256), -5),
    (lambda p: setattr(p, "d", 260), -3),
    (lambda p: setattr(p, "offsets", None), -1),
    (lambda p: setattr(p, "total_q", 0), 0),  # nothing to do: no launch
])
def test_rotary_varlen_rejects(built_lib, mutate, code):
    p = _rotary()
    mutate(p)
    assert built_lib.fa_rotary_apply_varlen(ctypes.byref(p), None) == code


def test_ragged_cache_call_traces_on_meta_tensors():
    """The FA3 forward op has a shape-only implementation: the ragged cache call traces with out (total_q, h, d_v) and LSE
    (h, total_q), the dense decode call with (b, s, h, d_v) and (b, h, s)."""
    import torch
    from flash_attention_annotated_amd import hopper_interface as fa3
    bf = dict(device="meta", dtype=torch.bfloat16)
    i32 = dict(device="meta", dtype=torch.int32)
    kc, vc = torch.empty(8, 64, 1, 64, **bf), torch.empty(8, 64, 1, 512, **bf)
    out, lse, *_ = fa3.flash_attn_with_kvcache(
        torch.empty(10, 4, 64, **bf), kc, vc, k=torch.empty(3, 1, 64, **bf), v=torch.empty(3, 1, 512, **bf),
        qv=torch.empty(10, 4, 512, **bf), cache_seqlens=torch.empty(2, **i32), cu_seqlens_q=torch.empty(3, **i32),
        cu_seqlens_k_new=torch.empty(3, **i32), max_seqlen_q=7, page_table=torch.empty(2, 4, **i32), return_softmax_lse=True)
    assert tuple(out.shape) == (10, 4, 512) and out.dtype == torch.bfloat16
    assert tuple(lse.shape) == (4, 10) and lse.dtype == torch.float32
    out, lse, *_ = fa3.flash_attn_with_kvcache(torch.empty(2, 3, 4, 64, **bf), kc, vc, cache_seqlens=torch.empty(2, **i32),
                                               page_table=torch.empty(2, 4, **i32), return_softmax_lse=True)
    assert tuple(out.shape) == (2, 3, 4, 512) and tuple(lse.shape) == (2, 4, 3)
