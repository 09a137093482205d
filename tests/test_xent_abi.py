"""CPU tests of the fused cross-entropy's C-ABI (include/fa_xent.h: fa_xent_fwd / fa_xent_bwd, their _validate and
_params_size) and of the device code of its translation unit, csrc/fa_xent.hip.  Nothing here touches a device;
tests/test_xent_gpu.py checks what the kernels write."""
import ctypes
import os
import re

import pytest

from flash_attention_annotated_amd import _lib

ADDR = 0x10000  # an aligned dummy address: nothing is dereferenced
OK, NULLP, BAD_DTYPE, BAD_SHAPE, BAD_STRIDE, BAD_ABI = 0, -1, -2, -5, -6, -9
BF16, FP16, FP32, FP8 = _lib.FA_DTYPE_BF16, _lib.FA_DTYPE_FP16, _lib.FA_DTYPE_FP32, _lib.FA_DTYPE_FP8_E4M3
INT64, INT32 = _lib.FA_XENT_LABELS_INT64, _lib.FA_XENT_LABELS_INT32
GIVEN, SPLIT = _lib.FA_XENT_PRECOMPUTED_LSE, _lib.FA_XENT_SPLIT
SYMBOLS = ("fa_xent_fwd", "fa_xent_fwd_validate", "fa_xent_fwd_params_size", "fa_xent_bwd", "fa_xent_bwd_validate",
           "fa_xent_bwd_params_size", "fa_xent_fwd_plan", "fa_xent_bwd_plan")


def _fwd(M=37, N=4096, **fields):
    """A contiguous bf16 (M, N) with int64 labels, everything present."""
    p = _lib.new_xent_fwd_params()
    for f in ("logits", "labels", "losses", "lse", "z_losses"):
        setattr(p, f, ADDR)
    p.M, p.N, p.logits_row_stride, p.total_classes = M, N, N, N
    for k, v in fields.items():
        setattr(p, k, v)
    if "total_classes" not in fields:
        p.total_classes = p.N
    return p


def _bwd(M=37, N=4096, **fields):
    p = _lib.new_xent_bwd_params()
    for f in ("logits", "labels", "lse", "dloss"):
        setattr(p, f, ADDR)
    p.dlogits = ADDR + (1 << 30)
    p.M, p.N, p.logits_row_stride, p.dlogits_row_stride, p.dloss_stride = M, N, N, N, 1
    for k, v in fields.items():
        setattr(p, k, v)
    if "total_classes" not in fields:
        p.total_classes = p.N
    return p


FWD = [
    ("bf16_int64", _fwd(), OK),
    ("fp16", _fwd(logits_dtype=FP16), OK),
    ("fp32", _fwd(logits_dtype=FP32), OK),
    ("int32_labels", _fwd(labels_dtype=INT32, labels=ADDR + 4), OK),
    ("no_rows", _fwd(M=0), OK),
    ("one_column", _fwd(N=1), OK),
    ("odd_width_odd_base", _fwd(N=50257, logits=ADDR + 2), OK),
    ("odd_width_odd_base_fp32", _fwd(N=50257, logits=ADDR + 4, logits_dtype=FP32), OK),
    ("rows_2_31_of_them", _fwd(M=1 << 31), OK),
    ("past_2_31_elements", _fwd(M=32768, N=128256), OK),
    ("widest_row", _fwd(M=1, N=(1 << 31) - 1), OK),
    ("row_stride_above_n", _fwd(logits_row_stride=4099), OK),
    ("smoothing_scale_z", _fwd(smoothing=0.1, logit_scale=0.7, lse_square_scale=1e-2), OK),
    ("smoothing_1", _fwd(smoothing=1.0), OK),
    ("lse_given", _fwd(flags=GIVEN), OK),
    ("lse_given_with_z", _fwd(flags=GIVEN, lse_square_scale=1e-2), OK),
    ("split_without_z_losses", _fwd(flags=SPLIT, z_losses=0, class_start_idx=4096, total_classes=8192), OK),
    ("abi_version", _fwd(abi_version=12), BAD_ABI),
    ("struct_size", _fwd(struct_size=8), BAD_ABI),
    ("null_logits", _fwd(logits=0), NULLP),
    ("null_labels", _fwd(labels=0), NULLP),
    ("null_losses", _fwd(losses=0), NULLP),
    ("null_lse", _fwd(lse=0), NULLP),
    ("null_lse_given", _fwd(lse=0, flags=GIVEN), NULLP),
    ("null_z_losses", _fwd(z_losses=0), NULLP),
    ("logits_fp8", _fwd(logits_dtype=FP8), BAD_DTYPE),
    ("logits_dtype_unknown", _fwd(logits_dtype=7), BAD_DTYPE),
    ("labels_dtype_unknown", _fwd(labels_dtype=2), BAD_DTYPE),
    ("n_0", _fwd(N=0), BAD_SHAPE),
    ("n_negative", _fwd(N=-8), BAD_SHAPE),
    ("m_negative", _fwd(M=-1), BAD_SHAPE),
    ("logit_scale_0", _fwd(logit_scale=0.0), BAD_SHAPE),
    ("logit_scale_negative", _fwd(logit_scale=-1.0), BAD_SHAPE),
    ("logit_scale_nan", _fwd(logit_scale=float("nan")), BAD_SHAPE),
    ("smoothing_negative", _fwd(smoothing=-0.1), BAD_SHAPE),
    ("smoothing_above_1", _fwd(smoothing=1.5), BAD_SHAPE),
    ("total_classes_below_n", _fwd(total_classes=4095), BAD_SHAPE),
    ("lse_given_with_smoothing", _fwd(flags=GIVEN, smoothing=0.1), BAD_SHAPE),
    ("lse_given_with_a_scale", _fwd(flags=GIVEN, logit_scale=0.7), BAD_SHAPE),
    ("logits_odd_address", _fwd(logits=ADDR + 1), BAD_STRIDE),
    ("fp32_logits_2_bytes", _fwd(logits=ADDR + 2, logits_dtype=FP32), BAD_STRIDE),
    ("int64_labels_4_bytes", _fwd(labels=ADDR + 4), BAD_STRIDE),
    ("lse_2_bytes", _fwd(lse=ADDR + 2), BAD_STRIDE),
    ("losses_2_bytes", _fwd(losses=ADDR + 2), BAD_STRIDE),
]

BWD = [
    ("bf16_int64", _bwd(), OK),
    ("fp16", _bwd(logits_dtype=FP16), OK),
    ("fp32", _bwd(logits_dtype=FP32), OK),
    ("int32_labels", _bwd(labels_dtype=INT32, labels=ADDR + 4), OK),
    ("no_rows", _bwd(M=0), OK),
    ("one_column", _bwd(N=1), OK),
    ("odd_width_odd_base", _bwd(N=50257, logits=ADDR + 2, dlogits=ADDR + 2), OK),
    ("dloss_stride_0", _bwd(dloss_stride=0), OK),
    ("in_place", _bwd(dlogits=ADDR), OK),
    ("another_phase", _bwd(dlogits=ADDR + (1 << 30) + 6), OK),
    ("rows_2_31_of_them", _bwd(M=1 << 31), OK),
    ("past_2_31_elements", _bwd(M=32768, N=128256), OK),
    ("split_flag", _bwd(flags=SPLIT, class_start_idx=4096, total_classes=8192), OK),
    ("one_row_any_stride", _bwd(M=1, dlogits_row_stride=0), OK),
    ("abi_version", _bwd(abi_version=12), BAD_ABI),
    ("struct_size", _bwd(struct_size=8), BAD_ABI),
    ("null_logits", _bwd(logits=0), NULLP),
    ("null_labels", _bwd(labels=0), NULLP),
    ("null_lse", _bwd(lse=0), NULLP),
    ("null_dloss", _bwd(dloss=0), NULLP),
    ("null_dlogits", _bwd(dlogits=0), NULLP),
    ("logits_fp8", _bwd(logits_dtype=FP8), BAD_DTYPE),
    ("labels_dtype_unknown", _bwd(labels_dtype=-1), BAD_DTYPE),
    ("n_0", _bwd(N=0), BAD_SHAPE),
    ("m_negative", _bwd(M=-1), BAD_SHAPE),
    ("logit_scale_0", _bwd(logit_scale=0.0), BAD_SHAPE),
    ("smoothing_above_1", _bwd(smoothing=1.5), BAD_SHAPE),
    ("smoothing_nan", _bwd(smoothing=float("nan")), BAD_SHAPE),
    ("total_classes_below_n", _bwd(total_classes=100), BAD_SHAPE),
    ("dlogits_odd_address", _bwd(dlogits=ADDR + 1), BAD_STRIDE),
    ("dloss_2_bytes", _bwd(dloss=ADDR + 2), BAD_STRIDE),
    ("dlogits_rows_overlap", _bwd(dlogits_row_stride=4095), BAD_STRIDE),
]


@pytest.mark.parametrize("name,p,status", FWD, ids=[r[0] for r in FWD])
def test_xent_fwd_validate(name, p, status):
    lib = _lib.load()
    assert lib.fa_xent_fwd_validate(p) == status
    if status != OK:  # the launch entry refuses the same way before it launches anything
        assert lib.fa_xent_fwd(p, None) == status


@pytest.mark.parametrize("name,p,status", BWD, ids=[r[0] for r in BWD])
def test_xent_bwd_validate(name, p, status):
    lib = _lib.load()
    assert lib.fa_xent_bwd_validate(p) == status
    if status != OK:
        assert lib.fa_xent_bwd(p, None) == status


def test_xent_validate_null():
    lib = _lib.load()
    assert lib.fa_xent_fwd_validate(None) == NULLP and lib.fa_xent_fwd(None, None) == NULLP
    assert lib.fa_xent_bwd_validate(None) == NULLP and lib.fa_xent_bwd(None, None) == NULLP


def test_xent_no_rows_launches_nothing():
    """M = 0 returns before any launch: FA_OK without a device."""
    lib = _lib.load()
    assert lib.fa_xent_fwd(_fwd(M=0), None) == OK and lib.fa_xent_fwd(_fwd(M=0, flags=GIVEN), None) == OK
    assert lib.fa_xent_bwd(_bwd(M=0), None) == OK


def test_xent_symbols_and_sizes():
    lib = _lib.load()
    header = open(os.path.join(_lib.INCLUDE, "fa_xent.h")).read()
    declared = re.findall(r"^\w[\w ]*?\b(fa_\w+)\(", header, re.M)
    assert sorted(declared) == sorted(SYMBOLS) == sorted(_lib.XENT_SYMBOLS)
    for name in SYMBOLS:
        assert hasattr(lib, name)
    assert lib.fa_xent_fwd_params_size() == ctypes.sizeof(_lib.FaXentFwdParams) == 120
    assert lib.fa_xent_bwd_params_size() == ctypes.sizeof(_lib.FaXentBwdParams) == 136
    for struct in (_lib.FaXentFwdParams, _lib.FaXentBwdParams):  # both begin like every other params struct
        assert [f[0] for f in struct._fields_[:2]] == ["abi_version", "struct_size"]
    # additive: a header of its own; the ABI version, the other symbol sets and the existing structs are what they were
    assert lib.fa_abi_version() == 13 == _lib.FA_ABI_VERSION
    for other in (_lib.EXPORTED_SYMBOLS, _lib.ROTARY_EMB_SYMBOLS, _lib.NORM_SYMBOLS):
        assert not set(SYMBOLS) & set(other)
    for other in ("fa_fwd.h", "fa_bwd.h", "fa_rotary.h", "fa_norm.h"):
        assert "fa_xent" not in open(os.path.join(_lib.INCLUDE, other)).read()
    sizes = {"fa_fwd_params_size": (_lib.FaFwdParams, 464), "fa_bwd_params_size": (_lib.FaBwdParams, 408),
             "fa_rotary_emb_params_size": (_lib.FaRotaryEmbParams, 184), "fa_norm_fwd_params_size": (_lib.FaNormFwdParams, 160),
             "fa_norm_bwd_params_size": (_lib.FaNormBwdParams, 232)}
    for fn, (struct, size) in sizes.items():
        assert getattr(lib, fn)() == ctypes.sizeof(struct) == size, fn


# the kernels of csrc/fa_xent.hip, by the elements of one access (8 x 16-bit or 4 x fp32 in 16 bytes; 1: elements)
FORMS = {("xent_fwd_kernel", 8), ("xent_fwd_kernel", 4), ("xent_fwd_lse_given_kernel",),
         ("xent_bwd_kernel", 8), ("xent_bwd_kernel", 4), ("xent_bwd_kernel", 1)}


def test_xent_device_code():
    """The translation unit holds exactly the kernels DESIGN 4.23 lists, and none has a private segment: nothing spills,
    nothing is called."""
    from device_asm import kernel_bodies
    found = {}
    for sym, body in kernel_bodies("fa_xent.hip"):
        k = re.match(r"_ZN\d+_GLOBAL__N_1\d+(xent_\w+?_kernel)(?:I((?:Li\d+E)+)E)?(?:Ev|v)?\w*$", sym)
        assert k, f"a kernel in fa_xent.hip of no known family: {sym}"
        key = (k.group(1), *(int(v) for v in re.findall(r"Li(\d+)E", k.group(2) or "")))
        assert key not in found, sym
        found[key] = int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body).group(1))
    assert set(found) == FORMS
    assert all(v == 0 for v in found.values()), found
