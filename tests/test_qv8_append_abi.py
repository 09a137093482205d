"""CPU tests of the quantising append to an fp8 KV cache of the MLA shape (include/fa_fwd.h: fa_kvcache_append_qv8, _validate)
and of the device code of its translation unit, csrc/fa_kvcache_append_qv8.hip.  The struct is fa_kvcache_append_kv8_params,
unchanged; the rules are those of fa_kvcache_append_kv8_validate (tests/test_kv8_append_abi.py) with the head-dim rule of
fa_fwd_qv8: d <= 64, d_v in [256, 512], both multiples of 16.  Nothing here touches a device; tests/test_qv8_append_gpu.py
checks what the kernel writes."""
import ctypes
import os
import re

import pytest

from flash_attention_annotated_amd import _lib

ADDR = 0x10000  # an aligned dummy address: nothing is dereferenced
OK, NULLP, BAD_DTYPE, BAD_HEAD_DIM, BAD_SHAPE, BAD_STRIDE, BAD_ABI = 0, -1, -2, -3, -5, -6, -9
SYMBOLS = ("fa_kvcache_append_qv8", "fa_kvcache_append_qv8_validate")


def _dense(b=2, s_new=3, cap=320, h_k=1, d=64, d_v=512, dtype=_lib.FA_DTYPE_BF16, **fields):
    """Dense new rows (b, s_new, h_k, d) / (b, s_new, h_k, d_v) of 16-bit elements into dense e4m3 caches (b, cap, h_k, d) /
    (b, cap, h_k, d_v) of bytes."""
    p = _lib.new_kvcache_append_kv8_params()
    for f in ("k_new", "v_new", "k_cache", "v_cache", "cache_seqlens", "k_descale", "v_descale"):
        setattr(p, f, ADDR)
    p.b, p.seqlen_new, p.seqlen_cache, p.h_k, p.d, p.d_v, p.dtype = b, s_new, cap, h_k, d, d_v, dtype
    for t, rows, w in (("knew", s_new, d), ("vnew", s_new, d_v), ("kcache", cap, d), ("vcache", cap, d_v)):
        setattr(p, f"{t}_head_stride", w)
        setattr(p, f"{t}_row_stride", h_k * w)
        setattr(p, f"{t}_batch_stride", rows * h_k * w)
    p.k_descale_batch_stride = p.v_descale_batch_stride = h_k
    p.k_descale_head_stride = p.v_descale_head_stride = 1
    for k, v in fields.items():
        setattr(p, k, v)
    return p


def _ragged(**kw):
    return _dense(**{**dict(cu_seqlens_k_new=ADDR, seqused_out=ADDR + 64, total_k_new=7, max_seqlen_k_new=5, s_new=0), **kw})


def _rotary(**kw):
    return _dense(**{**dict(rotary_cos=ADDR, rotary_sin=ADDR, rotary_dim=32), **kw})


VALIDATE = [
    ("bf16", _dense(), OK),
    ("fp16", _dense(dtype=_lib.FA_DTYPE_FP16), OK),
    ("ragged", _ragged(), OK),
    ("ragged_search", _ragged(max_seqlen_k_new=0), OK),
    ("no_descales_means_one", _dense(k_descale=0, v_descale=0), OK),
    ("dense_with_fill_levels", _dense(seqused_out=ADDR + 64), OK),
    ("no_rows", _dense(s_new=0, k_new=0, v_new=0), OK),
    ("two_kv_heads", _dense(h_k=2), OK),
    # ABI and size
    ("abi_version", _dense(abi_version=12), BAD_ABI),
    ("struct_size", _dense(struct_size=8), BAD_ABI),
    # dtype of the new rows
    ("fp8_rows", _dense(dtype=_lib.FA_DTYPE_FP8_E4M3), BAD_DTYPE),
    ("fp32_rows", _dense(dtype=_lib.FA_DTYPE_FP32), BAD_DTYPE),
    # shapes
    ("b0", _dense(b=0), BAD_SHAPE),
    ("h_k0", _dense(h_k=0), BAD_SHAPE),
    ("negative_rows", _dense(s_new=-1), BAD_SHAPE),
    ("negative_total", _ragged(total_k_new=-1), BAD_SHAPE),
    ("negative_max_len", _ragged(max_seqlen_k_new=-1), BAD_SHAPE),
    # head dims: what fa_fwd_qv8 reads
    ("d16_d_v256", _dense(d=16, d_v=256), OK),
    ("d32_d_v272", _dense(d=32, d_v=272), OK),
    ("d48_d_v320", _dense(d=48, d_v=320), OK),
    ("d0", _dense(d=0), BAD_HEAD_DIM),
    ("d8", _dense(d=8), BAD_HEAD_DIM),
    ("d40", _dense(d=40), BAD_HEAD_DIM),
    ("d80", _dense(d=80), BAD_HEAD_DIM),
    ("d128", _dense(d=128), BAD_HEAD_DIM),
    ("d_v0_is_required", _dense(d_v=0), BAD_HEAD_DIM),
    ("d_v_of_d", _dense(d_v=64), BAD_HEAD_DIM),
    ("d_v128", _dense(d_v=128), BAD_HEAD_DIM),
    ("d_v248", _dense(d_v=248), BAD_HEAD_DIM),
    ("d_v264", _dense(d_v=264), BAD_HEAD_DIM),  # a multiple of 8, not of 16
    ("d_v520", _dense(d_v=520), BAD_HEAD_DIM),
    ("d_v528", _dense(d_v=528), BAD_HEAD_DIM),
    # 16-byte aligned new rows
    ("knew_pointer", _dense(k_new=ADDR + 8), BAD_STRIDE),
    ("vnew_pointer", _dense(v_new=ADDR + 8), BAD_STRIDE),
    ("vnew_head_stride", _dense(vnew_head_stride=516), BAD_STRIDE),
    ("knew_batch_stride", _dense(knew_batch_stride=3 * 64 + 4), BAD_STRIDE),
    ("knew_batch_stride_unread_when_ragged", _ragged(knew_batch_stride=4), OK),
    # 8-byte aligned cache rows, heads and strides (bytes)
    ("cache_pointer_8", _dense(v_cache=ADDR + 8), OK),
    ("cache_pointer_4", _dense(v_cache=ADDR + 4), BAD_STRIDE),
    ("cache_head_stride_8", _dense(vcache_head_stride=520), OK),
    ("cache_head_stride_4", _dense(kcache_head_stride=68), BAD_STRIDE),
    ("cache_row_stride_4", _dense(vcache_row_stride=512 + 4), BAD_STRIDE),
    # rotary: against d, not d_v
    ("rotary", _rotary(), OK),
    ("rotary_full", _rotary(rotary_dim=64), OK),
    ("rotary_dim_24", _rotary(rotary_dim=24), BAD_SHAPE),
    ("rotary_dim_0", _rotary(rotary_dim=0), BAD_SHAPE),
    ("rotary_dim_above_d", _rotary(rotary_dim=80), BAD_SHAPE),
    ("rotary_dim_of_d_v", _rotary(rotary_dim=512), BAD_SHAPE),
    ("rotary_dim_above_d32", _rotary(d=32, d_v=256, rotary_dim=48), BAD_SHAPE),
    ("rotary_cos_alone", _rotary(rotary_sin=0), NULLP),
    ("rotary_sin_alone", _rotary(rotary_cos=0), NULLP),
    ("rotary_cos_pointer", _rotary(rotary_cos=ADDR + 8), BAD_STRIDE),
    # cache selection
    ("paged", _dense(block_table=ADDR, page_block_size=16, block_table_batch_stride=20), OK),
    ("paged_0", _dense(block_table=ADDR, page_block_size=0, block_table_batch_stride=20), BAD_SHAPE),
    ("paged_batch_idx", _dense(block_table=ADDR, page_block_size=16, block_table_batch_stride=20, cache_batch_idx=ADDR), BAD_SHAPE),
    ("paged_table_stride", _dense(block_table=ADDR, page_block_size=16, block_table_batch_stride=-1), BAD_STRIDE),
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
def test_append_qv8_validate(name, p, status):
    lib = _lib.load()
    assert lib.fa_kvcache_append_qv8_validate(p) == status
    if status != OK:  # the launch entry refuses the same way before it launches anything
        assert lib.fa_kvcache_append_qv8(p, None) == status


def test_append_qv8_validate_null():
    assert _lib.load().fa_kvcache_append_qv8_validate(None) == NULLP
    assert _lib.load().fa_kvcache_append_qv8(None, None) == NULLP


@pytest.mark.parametrize("name,p,status", [r for r in VALIDATE if r[2] == OK], ids=[r[0] for r in VALIDATE if r[2] == OK])
def test_append_kv8_validate_still_refuses_the_mla_shape(name, p, status):
    """Every params block the new entry accepts is FA_ERR_BAD_HEAD_DIM to fa_kvcache_append_kv8_validate: d_v != d stays refused
    there, and its launch entry refuses alike."""
    lib = _lib.load()
    assert lib.fa_kvcache_append_kv8_validate(p) == BAD_HEAD_DIM
    assert lib.fa_kvcache_append_kv8(p, None) == BAD_HEAD_DIM


def test_append_qv8_cache_entry_of_4_gib_validates():
    """Strides are 64-bit and the kernel builds a 64-bit base per row: 2^23 rows x 512 bytes = 4 GiB per V entry."""
    cap = 1 << 23
    p = _dense(b=4, cap=cap)
    assert p.vcache_batch_stride == 1 << 32
    assert _lib.load().fa_kvcache_append_qv8_validate(p) == OK
    assert _lib.load().fa_kvcache_append_qv8_validate(_ragged(b=4, cap=cap)) == OK


def test_append_qv8_symbols_and_sizes():
    lib = _lib.load()
    header = open(os.path.join(_lib.INCLUDE, "fa_fwd.h")).read()
    for name in SYMBOLS:
        assert re.search(rf"\b{name}\(", header), name
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
    # additive: the ABI version and the struct are what they were
    assert lib.fa_abi_version() == 13 == _lib.FA_ABI_VERSION
    assert lib.fa_kvcache_append_kv8_params_size() == ctypes.sizeof(_lib.FaKvcacheAppendKv8Params)
    assert not hasattr(lib, "fa_kvcache_append_qv8_params_size")  # (one struct, one size query)


def test_append_qv8_device_code():
    """The translation unit holds kvcache_append_qv8_kernel for bf16 and fp16 and nothing else; neither form has a private
    segment (nothing spills, nothing is called) or static LDS (the cu_seqlens image is the launch's dynamic LDS)."""
    from device_asm import device_asm
    text = open(device_asm("fa_kvcache_append_qv8.hip")).read()
    kernels = {}
    for m in re.finditer(r"^\s*\.amdhsa_kernel (\S+)$(.*?)^\s*\.end_amdhsa_kernel", text, re.M | re.S):
        k = re.match(r"_ZN\d+_GLOBAL__N_125kvcache_append_qv8_kernelI(DF16b|DF16_)EEv28fa_kvcache_append_kv8_params$", m.group(1))
        assert k, f"a kernel in fa_kvcache_append_qv8.hip that is no kvcache_append_qv8_kernel: {m.group(1)}"
        assert k.group(1) not in kernels
        kernels[k.group(1)] = (int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", m.group(2)).group(1)),
                               int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", m.group(2)).group(1)))
    assert set(kernels) == {"DF16b", "DF16_"}
    assert all(v == (0, 0) for v in kernels.values()), kernels
    assert "v_cvt_pk_fp8_f32" in text and "v_med3_f32" in text
    assert "global_load_dwordx4" in text  # 16-byte loads
    assert "global_store_dwordx2" in text and not re.search(r"global_store_(byte|short)\b", text)  # 8-byte stores of 8 elements
    assert not re.search(r"\b(global|flat|ds|buffer)_atomic", text) and "scratch_" not in text
