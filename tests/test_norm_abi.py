"""CPU tests of the fused norm's C-ABI (include/fa_norm.h: fa_norm_fwd / fa_norm_bwd, their _validate and _params_size, and
fa_norm_bwd_workspace_bytes) and of the device code of its translation unit, csrc/fa_norm.hip.  Nothing here touches a device;
tests/test_norm_gpu.py checks what the kernels write."""
import ctypes
import os
import re

import pytest

from flash_attention_annotated_amd import _lib

ADDR = 0x10000  # an aligned dummy address: nothing is dereferenced
OK, NULLP, BAD_DTYPE, BAD_SHAPE, BAD_STRIDE, BAD_ABI, WORKSPACE = 0, -1, -2, -5, -6, -9, -11
BF16, FP16, FP32, FP8 = _lib.FA_DTYPE_BF16, _lib.FA_DTYPE_FP16, _lib.FA_DTYPE_FP32, _lib.FA_DTYPE_FP8_E4M3
SYMBOLS = ("fa_norm_fwd", "fa_norm_fwd_validate", "fa_norm_fwd_params_size", "fa_norm_bwd", "fa_norm_bwd_validate",
           "fa_norm_bwd_params_size", "fa_norm_bwd_workspace_bytes", "fa_norm_fwd_plan", "fa_norm_bwd_plan")


def _fwd(M=111, N=192, **fields):
    """LayerNorm of a contiguous bf16 (M, N) with a bf16 residual, everything present."""
    p = _lib.new_norm_fwd_params()
    for f in ("x", "residual", "weight", "bias", "rowscale", "y", "residual_out", "mean", "rstd"):
        setattr(p, f, ADDR)
    p.M, p.N = M, N
    for t in ("x", "residual", "y", "residual_out"):
        setattr(p, f"{t}_row_stride", N)
    for k, v in fields.items():
        setattr(p, k, v)
    return p


def _bwd(M=111, N=192, sized=True, **fields):
    p = _lib.new_norm_bwd_params()
    for f in ("x", "dy", "weight", "bias", "dresidual", "rowscale", "mean", "rstd", "dx", "dresidual_in", "dw", "db", "y"):
        setattr(p, f, ADDR)
    p.M, p.N = M, N
    for t in ("x", "dy", "dresidual", "dx", "dresidual_in", "y"):
        setattr(p, f"{t}_row_stride", N)
    if sized:  # the workspace, a function of M and N alone
        p.workspace, p.workspace_bytes = ADDR, _lib.load().fa_norm_bwd_workspace_bytes(p)
    for k, v in fields.items():
        setattr(p, k, v)
    return p


ALL_FP32 = {f"{t}_dtype": FP32 for t in ("x", "y", "residual", "residual_out")}
FWD = [
    ("bf16", _fwd(), OK),
    ("fp16_fp32_residual_fp32_weight", _fwd(x_dtype=FP16, y_dtype=FP16, residual_dtype=FP32, residual_out_dtype=FP32, weight_dtype=FP32), OK),
    ("fp32", _fwd(**ALL_FP32), OK),
    ("rms_without_mean", _fwd(flags=_lib.FA_NORM_RMS, mean=0), OK),
    ("nothing_optional", _fwd(residual=0, bias=0, rowscale=0, residual_out=0), OK),
    ("absent_tensors_have_no_dtype", _fwd(residual=0, bias=0, rowscale=0, residual_out=0, residual_dtype=9, bias_dtype=9, rowscale_dtype=9), OK),
    ("in_place_residual", _fwd(residual_out=ADDR), OK),
    ("odd_width_odd_base", _fwd(N=203, x=ADDR + 2), OK),
    ("one_column", _fwd(N=1), OK),
    ("no_rows", _fwd(M=0), OK),
    ("bf16_row_of_64_kib", _fwd(M=16, N=32768), OK),
    ("fp32_row_of_64_kib", _fwd(N=16384, **ALL_FP32), OK),
    ("abi_version", _fwd(abi_version=12), BAD_ABI),
    ("struct_size", _fwd(struct_size=8), BAD_ABI),
    ("null_x", _fwd(x=0), NULLP),
    ("null_weight", _fwd(weight=0), NULLP),
    ("null_y", _fwd(y=0), NULLP),
    ("null_rstd", _fwd(rstd=0), NULLP),
    ("null_mean_layer_norm", _fwd(mean=0), NULLP),
    ("n_0", _fwd(N=0), BAD_SHAPE),
    ("n_negative", _fwd(N=-8), BAD_SHAPE),
    ("m_negative", _fwd(M=-1), BAD_SHAPE),
    ("bf16_row_above_64_kib", _fwd(M=16, N=32776), BAD_SHAPE),
    ("wide_rows_2_31_of_them", _fwd(M=1 << 31, N=32768), BAD_SHAPE),
    ("rows_2_31_of_them", _fwd(M=1 << 31, N=8), OK),
    ("fp32_row_above_64_kib", _fwd(N=16388, **ALL_FP32), BAD_SHAPE),
    ("x_fp8", _fwd(x_dtype=FP8), BAD_DTYPE),
    ("x_dtype_unknown", _fwd(x_dtype=7), BAD_DTYPE),
    ("weight_dtype_unknown", _fwd(weight_dtype=-1), BAD_DTYPE),
    ("bias_dtype_unknown", _fwd(bias_dtype=5), BAD_DTYPE),
    ("y_fp8", _fwd(y_dtype=FP8), BAD_DTYPE),
    ("rowscale_dtype_unknown", _fwd(rowscale_dtype=4), BAD_DTYPE),
    ("residual_of_the_other_16_bit_type", _fwd(residual_dtype=FP16), BAD_DTYPE),
    ("residual_out_of_the_other_16_bit_type", _fwd(residual_out_dtype=FP16), BAD_DTYPE),
    ("fp32_x_16_bit_residual", _fwd(x_dtype=FP32, N=64), BAD_DTYPE),
    ("x_odd_address", _fwd(x=ADDR + 1), BAD_STRIDE),
    ("fp32_residual_2_bytes", _fwd(residual_dtype=FP32, residual=ADDR + 2), BAD_STRIDE),
    ("rstd_2_bytes", _fwd(rstd=ADDR + 2), BAD_STRIDE),
]

BWD = [
    ("bf16", _bwd(), OK),
    ("fp32_stream_bf16_dx", _bwd(x_dtype=FP32, dresidual_dtype=FP32, dresidual_in_dtype=FP32, weight_dtype=FP32, bias_dtype=FP32), OK),
    ("rms_without_mean", _bwd(flags=_lib.FA_NORM_RMS, mean=0), OK),
    ("nothing_optional", _bwd(bias=0, dresidual=0, rowscale=0, dresidual_in=0, db=0, y=0), OK),
    ("odd_width", _bwd(N=203), OK),
    ("wide_row", _bwd(M=16, N=32768), OK),
    ("no_rows_no_workspace", _bwd(M=0, sized=False), OK),
    ("abi_version", _bwd(abi_version=12), BAD_ABI),
    ("struct_size", _bwd(struct_size=8), BAD_ABI),
    ("null_x", _bwd(x=0), NULLP),
    ("null_dy", _bwd(dy=0), NULLP),
    ("null_weight", _bwd(weight=0), NULLP),
    ("null_rstd", _bwd(rstd=0), NULLP),
    ("null_mean_layer_norm", _bwd(mean=0), NULLP),
    ("null_dx", _bwd(dx=0), NULLP),
    ("null_dw", _bwd(dw=0), NULLP),
    ("n_0", _bwd(N=0, sized=False), BAD_SHAPE),
    ("m_negative", _bwd(M=-1, sized=False), BAD_SHAPE),
    ("bf16_row_above_64_kib", _bwd(M=16, N=32776), BAD_SHAPE),
    ("wide_rows_2_31_of_them", _bwd(M=1 << 31, N=8200, sized=False), BAD_SHAPE),
    ("fp32_stream_row_above_64_kib", _bwd(M=16, N=16392, x_dtype=FP32, dresidual_dtype=FP32, dresidual_in_dtype=FP32), BAD_SHAPE),
    ("x_fp8", _bwd(x_dtype=FP8), BAD_DTYPE),
    ("dy_dtype_unknown", _bwd(dy_dtype=6), BAD_DTYPE),
    ("dx_dtype_unknown", _bwd(dx_dtype=6), BAD_DTYPE),
    ("stream_of_the_other_16_bit_type", _bwd(x_dtype=FP16, dresidual_dtype=FP16, dresidual_in_dtype=FP16), BAD_DTYPE),
    ("dresidual_not_of_the_streams_dtype", _bwd(dresidual_dtype=FP32), BAD_DTYPE),
    ("dresidual_in_not_of_the_streams_dtype", _bwd(dresidual_in_dtype=FP32), BAD_DTYPE),
    ("workspace_missing", _bwd(sized=False), WORKSPACE),
    ("workspace_null", _bwd(workspace=0), WORKSPACE),
    ("workspace_too_small", _bwd(workspace_bytes=1024), WORKSPACE),
    ("workspace_misaligned", _bwd(workspace=ADDR + 4), BAD_STRIDE),
    ("dy_odd_address", _bwd(dy=ADDR + 1), BAD_STRIDE),
]


@pytest.mark.parametrize("name,p,status", FWD, ids=[r[0] for r in FWD])
def test_norm_fwd_validate(name, p, status):
    lib = _lib.load()
    assert lib.fa_norm_fwd_validate(p) == status
    if status != OK:  # the launch entry refuses the same way before it launches anything
        assert lib.fa_norm_fwd(p, None) == status


@pytest.mark.parametrize("name,p,status", BWD, ids=[r[0] for r in BWD])
def test_norm_bwd_validate(name, p, status):
    lib = _lib.load()
    assert lib.fa_norm_bwd_validate(p) == status
    if status != OK:
        assert lib.fa_norm_bwd(p, None) == status


def test_norm_validate_null():
    lib = _lib.load()
    assert lib.fa_norm_fwd_validate(None) == NULLP and lib.fa_norm_fwd(None, None) == NULLP
    assert lib.fa_norm_bwd_validate(None) == NULLP and lib.fa_norm_bwd(None, None) == NULLP
    assert lib.fa_norm_bwd_workspace_bytes(None) == 0


def test_norm_no_rows_launches_nothing_forward():
    """M = 0 returns before any launch: FA_OK without a device."""
    assert _lib.load().fa_norm_fwd(_fwd(M=0), None) == OK


def test_norm_2_31_elements_validate():
    """Rows are addressed in 64 bits: M * N = 2^31 + N."""
    n = 4096
    m = (1 << 31) // n + 1
    assert m * n >= 1 << 31
    lib = _lib.load()
    assert lib.fa_norm_fwd_validate(_fwd(M=m, N=n)) == OK
    assert lib.fa_norm_bwd_validate(_bwd(M=m, N=n)) == OK


def test_norm_bwd_workspace_depends_on_the_shape_only():
    """One fp32 partial row of dw and one of db per workgroup; the count is a function of M (at most 1024 + a remainder, at least
    16 rows each), never of dtypes, strides or pointers.  Wide rows add two floats per row."""
    lib = _lib.load()

    def partials(m, n):
        return lib.fa_norm_bwd_workspace_bytes(_bwd(M=m, N=n, sized=False)) // (2 * 4 * n)
    assert partials(1, 192) == 1 and partials(16, 192) == 1 and partials(17, 192) == 2 and partials(111, 192) == 7
    assert partials(65536, 4096) == 1024 and partials(1 << 20, 8) == 1024
    for n in (8, 203, 4096, 8192):
        a = _bwd(M=3000, N=n, sized=False)
        b = _bwd(M=3000, N=n, sized=False, x_dtype=FP32, dresidual_dtype=FP32, dresidual_in_dtype=FP32, x=ADDR + 4, x_row_stride=n + 3)
        assert lib.fa_norm_bwd_workspace_bytes(a) == lib.fa_norm_bwd_workspace_bytes(b) == partials(3000, n) * 8 * n
    wide = lib.fa_norm_bwd_workspace_bytes(_bwd(M=16, N=32768, sized=False))
    assert wide == 1 * 8 * 32768 + 16 * 8
    assert lib.fa_norm_bwd_workspace_bytes(_bwd(M=0, sized=False)) == 0


def test_norm_symbols_and_sizes():
    lib = _lib.load()
    header = open(os.path.join(_lib.INCLUDE, "fa_norm.h")).read()
    declared = re.findall(r"^\w[\w ]*?\b(fa_\w+)\(", header, re.M)
    assert sorted(declared) == sorted(SYMBOLS) == sorted(_lib.NORM_SYMBOLS)
    for name in SYMBOLS:
        assert hasattr(lib, name)
    assert lib.fa_norm_fwd_params_size() == ctypes.sizeof(_lib.FaNormFwdParams) == 160
    assert lib.fa_norm_bwd_params_size() == ctypes.sizeof(_lib.FaNormBwdParams) == 232
    # additive: a header of its own; the ABI version, the other symbol sets and the existing structs are what they were
    assert lib.fa_abi_version() == 13 == _lib.FA_ABI_VERSION
    assert not set(SYMBOLS) & set(_lib.EXPORTED_SYMBOLS) and not set(SYMBOLS) & set(_lib.ROTARY_EMB_SYMBOLS)
    for other in ("fa_fwd.h", "fa_bwd.h", "fa_rotary.h"):
        assert "fa_norm" not in open(os.path.join(_lib.INCLUDE, other)).read()
    sizes = {"fa_fwd_params_size": (_lib.FaFwdParams, 464), "fa_bwd_params_size": (_lib.FaBwdParams, 408),
             "fa_rotary_emb_params_size": (_lib.FaRotaryEmbParams, 184), "fa_rotary_params_size": (_lib.FaRotaryParams, None),
             "fa_combine_params_size": (_lib.FaCombineParams, None), "fa_kvcache_append_params_size": (_lib.FaKvcacheAppendParams, None)}
    for fn, (struct, size) in sizes.items():
        assert getattr(lib, fn)() == ctypes.sizeof(struct)
        if size is not None:
            assert ctypes.sizeof(struct) == size, fn


# the kernel forms of csrc/fa_norm.hip, by access shape (CW columns per access) and columns per thread
FORMS = {("norm_fwd_kernel", 8, 2), ("norm_fwd_kernel", 4, 4), ("norm_fwd_kernel", 1, 16),
         ("norm_fwd_wide_kernel", 8), ("norm_fwd_wide_kernel", 1),
         ("norm_bwd_kernel", 8, 1), ("norm_bwd_kernel", 4, 2), ("norm_bwd_kernel", 1, 8),
         ("norm_bwd_row_sums_kernel", 8), ("norm_bwd_row_sums_kernel", 4), ("norm_bwd_row_sums_kernel", 1),
         ("norm_reduce_kernel",)}


def test_norm_device_code():
    """The translation unit holds exactly the forms DESIGN 4.22 lists, and none has a private segment: nothing spills, nothing
    is called."""
    from device_asm import kernel_bodies
    found = {}
    for sym, body in kernel_bodies("fa_norm.hip"):
        k = re.match(r"_ZN\d+_GLOBAL__N_1\d+(norm_\w+?_kernel)(?:I((?:Li\d+E)+)E)?(?:Ev|v)?\w*$", sym)
        assert k, f"a kernel in fa_norm.hip of no known family: {sym}"
        key = (k.group(1), *(int(v) for v in re.findall(r"Li(\d+)E", k.group(2) or "")))
        assert key not in found, sym
        found[key] = int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body).group(1))
    assert set(found) == FORMS
    assert all(v == 0 for v in found.values()), found
