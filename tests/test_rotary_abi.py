"""CPU tests of the rotary embedding layer's C-ABI (include/fa_rotary.h: fa_rotary_emb, _validate, _params_size) and of the
device code of its translation unit, csrc/fa_rotary_emb.hip.  Nothing here touches a device; tests/test_rotary_gpu.py checks what
the kernel writes."""
import ctypes
import os
import re

import pytest

from flash_attention_annotated_amd import _lib

ADDR = 0x10000  # an aligned dummy address: nothing is dereferenced
OK, NULLP, BAD_DTYPE, BAD_HEAD_DIM, BAD_SHAPE, BAD_STRIDE, BAD_ABI = 0, -1, -2, -3, -5, -6, -9
SYMBOLS = ("fa_rotary_emb", "fa_rotary_emb_validate", "fa_rotary_emb_params_size")


def _dense(b=2, s=37, h=3, d=128, rd=64, dtype=_lib.FA_DTYPE_BF16, cs=None, **fields):
    """A contiguous (b, s, h, d) tensor rotated into another one, tables of x's dtype unless `cs` says otherwise."""
    p = _lib.new_rotary_emb_params()
    for f in ("x", "out", "cos", "sin"):
        setattr(p, f, ADDR)
    p.b, p.seqlen, p.h, p.d, p.rotary_dim, p.seqlen_ro = b, s, h, d, rd, s + 8
    p.dtype = dtype
    p.cos_dtype = p.sin_dtype = dtype if cs is None else cs
    for t in ("x", "out"):
        setattr(p, f"{t}_dim_stride", 1)
        setattr(p, f"{t}_head_stride", d)
        setattr(p, f"{t}_row_stride", h * d)
        setattr(p, f"{t}_batch_stride", s * h * d)
    for k, v in fields.items():
        setattr(p, k, v)
    return p


def _ragged(**kw):
    return _dense(**{**dict(cu_seqlens=ADDR, seqlen=0, total=51, max_seqlen=33, seqlen_offsets=ADDR), **kw})


VALIDATE = [
    # accepted: every dtype, both paths
    ("bf16_vector", _dense(), OK),
    ("fp16_vector", _dense(dtype=_lib.FA_DTYPE_FP16), OK),
    ("fp32_element", _dense(dtype=_lib.FA_DTYPE_FP32), OK),
    ("bf16_element_rotary_dim_20", _dense(d=40, rd=20), OK),
    ("fp16_element_last_stride_2", _dense(dtype=_lib.FA_DTYPE_FP16, x_dim_stride=2), OK),
    ("bf16_element_base_8_bytes", _dense(x=ADDR + 8), OK),
    ("bf16_fp32_tables", _dense(cs=_lib.FA_DTYPE_FP32), OK),
    ("in_place", _dense(out=ADDR), OK),
    ("ragged", _ragged(), OK),
    ("ragged_int64_offsets", _ragged(offsets_int64=1), OK),
    ("d256", _dense(d=256, rd=256), OK),
    ("no_rows", _dense(s=0), OK),
    ("conjugate_interleaved", _dense(conjugate=1, interleaved=1), OK),
    # ABI and size
    ("abi_version", _dense(abi_version=12), BAD_ABI),
    ("struct_size", _dense(struct_size=8), BAD_ABI),
    # null pointers
    ("null_x", _dense(x=0), NULLP),
    ("null_out", _dense(out=0), NULLP),
    ("null_cos", _dense(cos=0), NULLP),
    ("null_sin", _dense(sin=0), NULLP),
    # dtypes
    ("fp8_x", _dense(dtype=_lib.FA_DTYPE_FP8_E4M3), BAD_DTYPE),
    ("dtype_out_of_range", _dense(dtype=7), BAD_DTYPE),
    ("cos_sin_differ", _dense(cos_dtype=_lib.FA_DTYPE_FP32), BAD_DTYPE),
    ("tables_of_another_16_bit_type", _dense(cs=_lib.FA_DTYPE_FP16), BAD_DTYPE),
    ("fp32_x_16_bit_tables", _dense(dtype=_lib.FA_DTYPE_FP32, cs=_lib.FA_DTYPE_BF16), BAD_DTYPE),
    # head dim and rotary_dim
    ("d_above_256", _dense(d=264, rd=64), BAD_HEAD_DIM),
    ("d_0", _dense(d=0, rd=0), BAD_HEAD_DIM),
    ("rotary_dim_odd", _dense(rd=63), BAD_SHAPE),
    ("rotary_dim_above_d", _dense(d=64, rd=66), BAD_SHAPE),
    ("rotary_dim_negative", _dense(rd=-2), BAD_SHAPE),
    # cu_seqlens needs the bound of the lengths
    ("cu_seqlens_without_max_seqlen", _ragged(max_seqlen=0), BAD_SHAPE),
    # negative sizes
    ("negative_b", _dense(b=-1), BAD_SHAPE),
    ("negative_seqlen", _dense(s=-1), BAD_SHAPE),
    ("negative_total", _ragged(total=-1), BAD_SHAPE),
    ("negative_max_seqlen", _ragged(max_seqlen=-3), BAD_SHAPE),
    ("negative_h", _dense(h=-1), BAD_SHAPE),
    ("negative_seqlen_ro", _dense(seqlen_ro=-1), BAD_SHAPE),
    # scalar accesses keep their natural alignment
    ("x_odd_address", _dense(x=ADDR + 1), BAD_STRIDE),
    ("fp32_out_2_bytes", _dense(dtype=_lib.FA_DTYPE_FP32, out=ADDR + 2), BAD_STRIDE),
    ("int64_offsets_4_bytes", _ragged(offsets_int64=1, seqlen_offsets=ADDR + 4), BAD_STRIDE),
]


@pytest.mark.parametrize("name,p,status", VALIDATE, ids=[r[0] for r in VALIDATE])
def test_rotary_emb_validate(name, p, status):
    lib = _lib.load()
    assert lib.fa_rotary_emb_validate(p) == status
    if status != OK:  # the launch entry refuses the same way before it launches anything
        assert lib.fa_rotary_emb(p, None) == status


def test_rotary_emb_validate_null():
    assert _lib.load().fa_rotary_emb_validate(None) == NULLP
    assert _lib.load().fa_rotary_emb(None, None) == NULLP


def test_rotary_emb_tensor_of_2_31_elements_validates():
    """Strides are 64-bit and the kernel builds a 64-bit base per row: 65552 rows x 128 heads x 256 = 2^31 + 2^19 elements."""
    p = _dense(b=1, s=65552, h=128, d=256, rd=256, out=ADDR)
    assert p.x_batch_stride > 1 << 31
    assert _lib.load().fa_rotary_emb_validate(p) == OK


def test_rotary_emb_symbols_and_sizes():
    lib = _lib.load()
    header = open(os.path.join(_lib.INCLUDE, "fa_rotary.h")).read()
    declared = re.findall(r"^\w[\w ]*?\b(fa_\w+)\(", header, re.M)
    assert sorted(declared) == sorted(SYMBOLS) == sorted(_lib.ROTARY_EMB_SYMBOLS)
    for name in SYMBOLS:
        assert hasattr(lib, name)
    assert lib.fa_rotary_emb_params_size() == ctypes.sizeof(_lib.FaRotaryEmbParams) == 184
    # additive: a header of its own; the ABI version, the forward params and the inference rotary structs are what they were
    assert lib.fa_abi_version() == 13 == _lib.FA_ABI_VERSION
    assert not set(SYMBOLS) & set(_lib.EXPORTED_SYMBOLS)
    assert "fa_rotary_emb" not in open(os.path.join(_lib.INCLUDE, "fa_fwd.h")).read()
    assert lib.fa_rotary_params_size() == ctypes.sizeof(_lib.FaRotaryParams)
    assert lib.fa_fwd_params_size() == ctypes.sizeof(_lib.FaFwdParams)


def test_rotary_emb_device_code():
    """The translation unit holds rotary_emb_kernel<T, CS, VEC> and nothing else: the vector path for the two 16-bit types, the
    element path for them with tables of their own type and of fp32, and for fp32.  No form has a private segment (nothing
    spills, nothing is called) or static LDS."""
    from device_asm import kernel_bodies
    types = {"DF16b": "bf16", "DF16_": "fp16", "f": "fp32"}
    kernels = {}
    for sym, body in kernel_bodies("fa_rotary_emb.hip"):
        k = re.match(r"_ZN\d+_GLOBAL__N_117rotary_emb_kernelI(DF16b|DF16_|f)(DF16b|DF16_|f)Lb([01])EEEv20fa_rotary_emb_params$", sym)
        assert k, f"a kernel in fa_rotary_emb.hip that is no rotary_emb_kernel: {sym}"
        key = (types[k.group(1)], types[k.group(2)], bool(int(k.group(3))))
        assert key not in kernels
        kernels[key] = (int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body).group(1)),
                        int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", body).group(1)))
    assert set(kernels) == {("bf16", "bf16", True), ("fp16", "fp16", True), ("bf16", "bf16", False), ("fp16", "fp16", False),
                            ("bf16", "fp32", False), ("fp16", "fp32", False), ("fp32", "fp32", False)}
    assert all(v == (0, 0) for v in kernels.values()), kernels
