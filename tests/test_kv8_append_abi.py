"""CPU tests of the quantising append to an fp8 KV cache (include/fa_fwd.h: fa_kvcache_append_kv8, _validate, _params_size) and
of the device code of its translation unit, csrc/fa_kvcache_append_kv8.hip.  Nothing here touches a device;
tests/test_kv8_append_gpu.py checks what the kernel writes."""
import ctypes
import os
import re

import pytest

from flash_attention_annotated_amd import _lib

ADDR = 0x10000  # an aligned dummy address: nothing is dereferenced
OK, NULLP, BAD_DTYPE, BAD_HEAD_DIM, BAD_SHAPE, BAD_STRIDE, BAD_ABI = 0, -1, -2, -3, -5, -6, -9
SYMBOLS = ("fa_kvcache_append_kv8", "fa_kvcache_append_kv8_validate", "fa_kvcache_append_kv8_params_size")


def _dense(b=2, s_new=3, cap=320, h_k=2, d=128, dtype=_lib.FA_DTYPE_BF16, **fields):
    """Dense new rows (b, s_new, h_k, d) of 16-bit elements into a dense e4m3 cache (b, cap, h_k, d) of bytes."""
    p = _lib.new_kvcache_append_kv8_params()
    for f in ("k_new", "v_new", "k_cache", "v_cache", "cache_seqlens", "k_descale", "v_descale"):
        setattr(p, f, ADDR)
    p.b, p.seqlen_new, p.seqlen_cache, p.h_k, p.d, p.dtype = b, s_new, cap, h_k, d, dtype
    for t, rows in (("knew", s_new), ("vnew", s_new), ("kcache", cap), ("vcache", cap)):
        setattr(p, f"{t}_head_stride", d)
        setattr(p, f"{t}_row_stride", h_k * d)
        setattr(p, f"{t}_batch_stride", rows * h_k * d)
    p.k_descale_batch_stride = p.v_descale_batch_stride = h_k
    p.k_descale_head_stride = p.v_descale_head_stride = 1
    for k, v in fields.items():
        setattr(p, k, v)
    return p


def _ragged(**kw):
    return _dense(**{**dict(cu_seqlens_k_new=ADDR, seqused_out=ADDR + 64, total_k_new=7, max_seqlen_k_new=5, s_new=0), **kw})


def _rotary(**kw):
    return _dense(**{**dict(rotary_cos=ADDR, rotary_sin=ADDR, rotary_dim=64), **kw})


VALIDATE = [
    ("bf16", _dense(), OK),
    ("fp16", _dense(dtype=_lib.FA_DTYPE_FP16), OK),
    ("ragged", _ragged(), OK),
    ("ragged_search", _ragged(max_seqlen_k_new=0), OK),
    ("no_descales_means_one", _dense(k_descale=0, v_descale=0), OK),
    ("dense_with_fill_levels", _dense(seqused_out=ADDR + 64), OK),
    ("no_rows", _dense(s_new=0, k_new=0, v_new=0), OK),
    # ABI and size
    ("abi_version", _dense(abi_version=12), BAD_ABI),
    ("struct_size", _dense(struct_size=8), BAD_ABI),
    # dtype of the new rows
    ("fp8_rows", _dense(dtype=_lib.FA_DTYPE_FP8_E4M3), BAD_DTYPE),
    ("fp32_rows", _dense(dtype=_lib.FA_DTYPE_FP32), BAD_DTYPE),
    # shapes
    ("b0", _dense(b=0), BAD_SHAPE),
    ("negative_rows", _dense(s_new=-1), BAD_SHAPE),
    ("negative_total", _ragged(total_k_new=-1), BAD_SHAPE),
    # head dims: what the read route serves
    ("d16", _dense(d=16), OK),
    ("d80", _dense(d=80), OK),
    ("d72", _dense(d=72), BAD_HEAD_DIM),
    ("d8", _dense(d=8), BAD_HEAD_DIM),
    ("d192", _dense(d=192), BAD_HEAD_DIM),
    ("d_v_same", _dense(d_v=128), OK),
    ("d_v_own", _dense(d_v=64), BAD_HEAD_DIM),
    # 16-byte aligned new rows
    ("knew_pointer", _dense(k_new=ADDR + 8), BAD_STRIDE),
    ("vnew_head_stride", _dense(vnew_head_stride=132), BAD_STRIDE),
    ("knew_batch_stride", _dense(knew_batch_stride=3 * 2 * 128 + 4), BAD_STRIDE),
    ("knew_batch_stride_unread_when_ragged", _ragged(knew_batch_stride=4), OK),
    # 8-byte aligned cache rows, heads and strides (bytes)
    ("cache_pointer_8", _dense(k_cache=ADDR + 8), OK),
    ("cache_pointer_4", _dense(v_cache=ADDR + 4), BAD_STRIDE),
    ("cache_head_stride_8", _dense(kcache_head_stride=136), OK),
    ("cache_head_stride_4", _dense(kcache_head_stride=132), BAD_STRIDE),
    ("cache_row_stride_4", _dense(vcache_row_stride=2 * 128 + 4), BAD_STRIDE),
    # rotary
    ("rotary", _rotary(), OK),
    ("rotary_full", _rotary(rotary_dim=128), OK),
    ("rotary_dim_24", _rotary(rotary_dim=24), BAD_SHAPE),
    ("rotary_dim_above_d", _rotary(d=64, rotary_dim=128), BAD_SHAPE),
    ("rotary_cos_alone", _rotary(rotary_sin=0), NULLP),
    ("rotary_sin_alone", _rotary(rotary_cos=0), NULLP),
    ("rotary_cos_pointer", _rotary(rotary_cos=ADDR + 8), BAD_STRIDE),
    # cache selection
    ("paged", _dense(block_table=ADDR, page_block_size=16, block_table_batch_stride=20), OK),
    ("paged_0", _dense(block_table=ADDR, page_block_size=0, block_table_batch_stride=20), BAD_SHAPE),
    ("paged_batch_idx", _dense(block_table=ADDR, page_block_size=16, block_table_batch_stride=20, cache_batch_idx=ADDR), BAD_SHAPE),
    ("batch_idx", _dense(cache_batch_idx=ADDR), OK),
    # seqused_out
    ("ragged_without_seqused_out", _ragged(seqused_out=0), NULLP),
    ("seqused_out_aliases_cache_seqlens", _ragged(seqused_out=ADDR), BAD_SHAPE),
    # required pointers
    ("null_k_new", _dense(k_new=0), NULLP),
    ("null_v_cache", _dense(v_cache=0), NULLP),
    ("null_cache_seqlens", _dense(cache_seqlens=0), NULLP),
]


@pytest.mark.parametrize("name,p,status", VALIDATE, ids=[r[0] for r in VALIDATE])
def test_append_kv8_validate(name, p, status):
    lib = _lib.load()
    assert lib.fa_kvcache_append_kv8_validate(p) == status
    if status != OK:  # the launch entry refuses the same way before it launches anything
        assert lib.fa_kvcache_append_kv8(p, None) == status


def test_append_kv8_validate_null():
    assert _lib.load().fa_kvcache_append_kv8_validate(None) == NULLP
    assert _lib.load().fa_kvcache_append_kv8(None, None) == NULLP


def test_append_kv8_cache_entry_of_4_gib_validates():
    """Strides are 64-bit and the kernel builds a 64-bit base per row: 2^20 rows x 32 heads x 128 bytes = 4 GiB per entry."""
    cap, h_k, d = 1 << 20, 32, 128
    p = _dense(b=4, cap=cap, h_k=h_k, d=d)
    assert p.kcache_batch_stride == 1 << 32
    assert _lib.load().fa_kvcache_append_kv8_validate(p) == OK
    assert _lib.load().fa_kvcache_append_kv8_validate(_ragged(b=4, cap=cap, h_k=h_k, d=d)) == OK


def test_append_kv8_symbols_and_sizes():
    lib = _lib.load()
    header = open(os.path.join(_lib.INCLUDE, "fa_fwd.h")).read()
    for name in SYMBOLS:
        assert re.search(rf"\b{name}\(", header), name
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert lib.fa_kvcache_append_kv8_params_size() == ctypes.sizeof(_lib.FaKvcacheAppendKv8Params)
    # additive: the ABI version and the structs of the 16-bit appends are what they were
    assert lib.fa_abi_version() == 13 == _lib.FA_ABI_VERSION
    assert lib.fa_kvcache_append_params_size() == ctypes.sizeof(_lib.FaKvcacheAppendParams) == 240
    assert lib.fa_kvcache_append_varlen_params_size() == ctypes.sizeof(_lib.FaKvcacheAppendVarlenParams) == 240
    assert lib.fa_fwd_params_size() == ctypes.sizeof(_lib.FaFwdParams)


def test_append_kv8_device_code():
    """The translation unit holds kvcache_append_kv8_kernel for bf16 and fp16 and nothing else; neither form has a private
    segment (nothing spills, nothing is called) or static LDS (the cu_seqlens image is the launch's dynamic LDS)."""
    from device_asm import device_asm
    text = open(device_asm("fa_kvcache_append_kv8.hip")).read()
    kernels = {}
    for m in re.finditer(r"^\s*\.amdhsa_kernel (\S+)$(.*?)^\s*\.end_amdhsa_kernel", text, re.M | re.S):
        k = re.match(r"_ZN\d+_GLOBAL__N_125kvcache_append_kv8_kernelI(DF16b|DF16_)EEv28fa_kvcache_append_kv8_params$", m.group(1))
        assert k, f"a kernel in fa_kvcache_append_kv8.hip that is no kvcache_append_kv8_kernel: {m.group(1)}"
        assert k.group(1) not in kernels
        kernels[k.group(1)] = (int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", m.group(2)).group(1)),
                               int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", m.group(2)).group(1)))
    assert set(kernels) == {"DF16b", "DF16_"}
    assert all(v == (0, 0) for v in kernels.values()), kernels
    assert "v_cvt_pk_fp8_f32" in text and "v_med3_f32" in text
    assert "global_store_dwordx2" in text and not re.search(r"global_store_(byte|short)\b", text)  # 8-byte stores of 8 elements
