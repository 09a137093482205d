"""CPU tests of the fused dropout-add-norm's C-ABI (include/fa_dropout_norm.h: fa_dropout_norm_fwd / _bwd, their _validate,
_params_size and _plan, and fa_dropout_norm_bwd_workspace_bytes) and of the device code of its translation unit,
csrc/fa_dropout_norm.hip.  Nothing here touches a device; tests/test_dropout_norm_gpu.py checks what the kernels write."""
import ctypes
import os
import re

import pytest

import dropout_norm_plan_universe as U
from flash_attention_annotated_amd import _lib

ADDR = 0x10000  # an aligned dummy address: nothing is dereferenced
OK, NULLP, BAD_DTYPE, BAD_SHAPE, BAD_STRIDE, UNSUPPORTED, BAD_ABI, WORKSPACE = 0, -1, -2, -5, -6, -7, -9, -11
BF16, FP16, FP32, FP8 = _lib.FA_DTYPE_BF16, _lib.FA_DTYPE_FP16, _lib.FA_DTYPE_FP32, _lib.FA_DTYPE_FP8_E4M3
RMS = _lib.FA_DROPOUT_NORM_RMS
SYMBOLS = ("fa_dropout_norm_fwd", "fa_dropout_norm_fwd_validate", "fa_dropout_norm_fwd_params_size", "fa_dropout_norm_bwd",
           "fa_dropout_norm_bwd_validate", "fa_dropout_norm_bwd_params_size", "fa_dropout_norm_bwd_workspace_bytes",
           "fa_dropout_norm_fwd_plan", "fa_dropout_norm_bwd_plan")
FWD_ROWS = ("x0", "x1", "residual", "z0", "z1", "x")
BWD_ROWS = ("dz0", "dz1", "dx", "x", "x0", "dx0", "dx1", "dresidual")


def _fwd(M=111, N=192, **fields):
    """The one-weight LayerNorm of a contiguous bf16 (M, N) with a bf16 residual, both scales, p = 0.1 and the mask."""
    p = _lib.new_dropout_norm_fwd_params()
    for f in ("x0", "residual", "weight0", "bias0", "rowscale", "colscale", "rng_state", "z0", "x", "dmask0", "mu", "rsigma"):
        setattr(p, f, ADDR)
    p.M, p.N, p.p_dropout = M, N, 0.1
    for t in FWD_ROWS:
        setattr(p, f"{t}_row_stride", N)
    for k, v in fields.items():
        setattr(p, k, v)
    return p


PARALLEL = dict(rowscale=0, colscale=0, x1=ADDR, weight1=ADDR, bias1=ADDR, z1=ADDR, dmask1=ADDR)


def _bwd(M=111, N=192, sized=True, **fields):
    p = _lib.new_dropout_norm_bwd_params()
    for f in ("dz0", "dx", "x", "x0", "weight0", "rowscale", "colscale", "rng_state", "mu", "rsigma", "dx0", "dresidual", "dw0", "db0",
              "dcolscale"):
        setattr(p, f, ADDR)
    p.M, p.N, p.p_dropout = M, N, 0.1
    for t in BWD_ROWS:
        setattr(p, f"{t}_row_stride", N)
    for k, v in fields.items():
        setattr(p, k, v)
    if sized:  # the workspace, a function of M, N and the sums there are
        p.workspace, p.workspace_bytes = ADDR, _lib.load().fa_dropout_norm_bwd_workspace_bytes(p)
        for k in ("workspace", "workspace_bytes"):
            if k in fields:
                setattr(p, k, fields[k])
    return p


BWD_PARALLEL = dict(rowscale=0, colscale=0, x0=0, dcolscale=0, dz1=ADDR, weight1=ADDR, dx1=ADDR, dw1=ADDR, db1=ADDR)
FP32_STREAM = dict(residual_dtype=FP32, x_dtype=FP32)
FWD = [
    ("bf16", _fwd(), OK),
    ("parallel", _fwd(**PARALLEL), OK),
    ("weight1_without_x1", _fwd(**{**PARALLEL, "x1": 0, "dmask1": 0}), OK),
    ("fp16_fp32_stream_fp32_weight", _fwd(x0_dtype=FP16, z_dtype=FP16, weight_dtype=FP32, **FP32_STREAM), OK),
    ("fp32", _fwd(x0_dtype=FP32, z_dtype=FP32, **FP32_STREAM), OK),
    ("rms_without_mu", _fwd(flags=RMS, mu=0), OK),
    ("nothing_optional", _fwd(residual=0, bias0=0, rowscale=0, colscale=0, x=0, dmask0=0), OK),
    ("absent_tensors_have_no_dtype", _fwd(rowscale=0, colscale=0, rowscale_dtype=9, colscale_dtype=9), OK),
    ("p_0_without_rng_state", _fwd(p_dropout=0.0, rng_state=0, dmask0=0), OK),
    ("p_just_below_1", _fwd(p_dropout=0.999), OK),
    ("odd_width_odd_base", _fwd(N=203, x0=ADDR + 2), OK),
    ("one_column", _fwd(N=1), OK),
    ("no_rows", _fwd(M=0), OK),
    ("bf16_row_of_64_kib", _fwd(M=16, N=32768), OK),
    ("fp32_row_of_64_kib", _fwd(N=16384, x0_dtype=FP32, **FP32_STREAM), OK),
    ("rows_2_31_of_them", _fwd(M=1 << 31, N=8), OK),
    ("abi_version", _fwd(abi_version=12), BAD_ABI),
    ("struct_size", _fwd(struct_size=8), BAD_ABI),
    ("null_x0", _fwd(x0=0), NULLP),
    ("null_weight0", _fwd(weight0=0), NULLP),
    ("null_z0", _fwd(z0=0), NULLP),
    ("null_rsigma", _fwd(rsigma=0), NULLP),
    ("null_mu_layer_norm", _fwd(mu=0), NULLP),
    ("null_z1_with_weight1", _fwd(**{**PARALLEL, "z1": 0}), NULLP),
    ("null_rng_state_with_dropout", _fwd(rng_state=0), NULLP),
    ("n_0", _fwd(N=0), BAD_SHAPE),
    ("n_negative", _fwd(N=-8), BAD_SHAPE),
    ("m_negative", _fwd(M=-1), BAD_SHAPE),
    ("bf16_row_above_64_kib", _fwd(M=16, N=32776), BAD_SHAPE),
    ("fp32_stream_row_above_64_kib", _fwd(M=16, N=16392, **FP32_STREAM), BAD_SHAPE),
    ("wide_rows_2_31_of_them", _fwd(M=1 << 31, N=32768), BAD_SHAPE),
    ("p_1", _fwd(p_dropout=1.0), BAD_SHAPE),
    ("p_negative", _fwd(p_dropout=-0.1), BAD_SHAPE),
    ("p_nan", _fwd(p_dropout=float("nan")), BAD_SHAPE),
    ("x0_fp8", _fwd(x0_dtype=FP8), BAD_DTYPE),
    ("x0_dtype_unknown", _fwd(x0_dtype=7), BAD_DTYPE),
    ("weight_dtype_unknown", _fwd(weight_dtype=-1), BAD_DTYPE),
    ("z_fp8", _fwd(z_dtype=FP8), BAD_DTYPE),
    ("rowscale_dtype_unknown", _fwd(rowscale_dtype=4), BAD_DTYPE),
    ("colscale_dtype_unknown", _fwd(colscale_dtype=4), BAD_DTYPE),
    ("stream_of_the_other_16_bit_type", _fwd(x_dtype=FP16, residual_dtype=FP16), BAD_DTYPE),
    ("residual_not_of_the_streams_dtype", _fwd(residual_dtype=FP32), BAD_DTYPE),
    ("fp32_x0_16_bit_stream", _fwd(x0_dtype=FP32, N=64), BAD_DTYPE),
    ("rowscale_with_x1", _fwd(**{**PARALLEL, "rowscale": ADDR}), UNSUPPORTED),
    ("colscale_with_weight1", _fwd(**{**PARALLEL, "x1": 0, "dmask1": 0, "colscale": ADDR}), UNSUPPORTED),
    ("bias1_without_weight1", _fwd(bias1=ADDR), UNSUPPORTED),
    ("mask_without_dropout", _fwd(p_dropout=0.0), UNSUPPORTED),
    ("dmask1_without_x1", _fwd(dmask1=ADDR), UNSUPPORTED),
    ("x0_odd_address", _fwd(x0=ADDR + 1), BAD_STRIDE),
    ("fp32_residual_2_bytes", _fwd(residual=ADDR + 2, **FP32_STREAM), BAD_STRIDE),
    ("rsigma_2_bytes", _fwd(rsigma=ADDR + 2), BAD_STRIDE),
    ("rng_state_4_bytes", _fwd(rng_state=ADDR + 4), BAD_STRIDE),
]

BWD = [
    ("bf16", _bwd(), OK),
    ("parallel", _bwd(**BWD_PARALLEL), OK),
    ("fp32_stream_bf16_dx0", _bwd(x_dtype=FP32, weight_dtype=FP32), OK),
    ("rms_without_mu", _bwd(flags=RMS, mu=0), OK),
    ("nothing_optional", _bwd(dx=0, x0=0, rowscale=0, colscale=0, dcolscale=0, dresidual=0, db0=0), OK),
    ("p_0_without_rng_state", _bwd(p_dropout=0.0, rng_state=0), OK),
    ("odd_width", _bwd(N=203), OK),
    ("wide_row", _bwd(M=16, N=32768), OK),
    ("no_rows_no_workspace", _bwd(M=0, sized=False), OK),
    ("abi_version", _bwd(abi_version=12), BAD_ABI),
    ("struct_size", _bwd(struct_size=8), BAD_ABI),
    ("null_x", _bwd(x=0), NULLP),
    ("null_dz0", _bwd(dz0=0), NULLP),
    ("null_weight0", _bwd(weight0=0), NULLP),
    ("null_rsigma", _bwd(rsigma=0), NULLP),
    ("null_mu_layer_norm", _bwd(mu=0), NULLP),
    ("null_dx0", _bwd(dx0=0), NULLP),
    ("null_dw0", _bwd(dw0=0), NULLP),
    ("null_dz1_with_weight1", _bwd(**{**BWD_PARALLEL, "dz1": 0}), NULLP),
    ("null_dw1_with_weight1", _bwd(**{**BWD_PARALLEL, "dw1": 0}), NULLP),
    ("null_x0_with_colscale", _bwd(x0=0), NULLP),
    ("null_dcolscale_with_colscale", _bwd(dcolscale=0), NULLP),
    ("null_rng_state_with_dropout", _bwd(rng_state=0), NULLP),
    ("n_0", _bwd(N=0, sized=False), BAD_SHAPE),
    ("m_negative", _bwd(M=-1, sized=False), BAD_SHAPE),
    ("bf16_row_above_64_kib", _bwd(M=16, N=32776), BAD_SHAPE),
    ("wide_rows_2_31_of_them", _bwd(M=1 << 31, N=8200, sized=False), BAD_SHAPE),
    ("fp32_stream_row_above_64_kib", _bwd(M=16, N=16392, x_dtype=FP32), BAD_SHAPE),
    ("p_1", _bwd(p_dropout=1.0), BAD_SHAPE),
    ("p_negative", _bwd(p_dropout=-0.5), BAD_SHAPE),
    ("x_fp8", _bwd(x_dtype=FP8), BAD_DTYPE),
    ("dz_dtype_unknown", _bwd(dz_dtype=6), BAD_DTYPE),
    ("x0_dtype_unknown", _bwd(x0_dtype=6), BAD_DTYPE),
    ("stream_of_the_other_16_bit_type", _bwd(x_dtype=FP16), BAD_DTYPE),
    ("rowscale_with_dx1", _bwd(**{**BWD_PARALLEL, "rowscale": ADDR}), UNSUPPORTED),
    ("dw1_without_weight1", _bwd(dw1=ADDR), UNSUPPORTED),
    ("dcolscale_without_colscale", _bwd(colscale=0, x0=0), UNSUPPORTED),
    ("workspace_missing", _bwd(sized=False), WORKSPACE),
    ("workspace_null", _bwd(workspace=0), WORKSPACE),
    ("workspace_too_small", _bwd(workspace_bytes=1024), WORKSPACE),
    ("workspace_misaligned", _bwd(workspace=ADDR + 4), BAD_STRIDE),
    ("dz0_odd_address", _bwd(dz0=ADDR + 1), BAD_STRIDE),
]


@pytest.mark.parametrize("name,p,status", FWD, ids=[r[0] for r in FWD])
def test_dropout_norm_fwd_validate(name, p, status):
    lib = _lib.load()
    assert lib.fa_dropout_norm_fwd_validate(p) == status
    if status != OK:  # the launch entry refuses the same way before it launches anything
        assert lib.fa_dropout_norm_fwd(p, None) == status


@pytest.mark.parametrize("name,p,status", BWD, ids=[r[0] for r in BWD])
def test_dropout_norm_bwd_validate(name, p, status):
    lib = _lib.load()
    assert lib.fa_dropout_norm_bwd_validate(p) == status
    if status != OK:
        assert lib.fa_dropout_norm_bwd(p, None) == status


def test_dropout_norm_validate_null():
    lib = _lib.load()
    assert lib.fa_dropout_norm_fwd_validate(None) == NULLP and lib.fa_dropout_norm_fwd(None, None) == NULLP
    assert lib.fa_dropout_norm_bwd_validate(None) == NULLP and lib.fa_dropout_norm_bwd(None, None) == NULLP
    assert lib.fa_dropout_norm_bwd_workspace_bytes(None) == 0


def test_dropout_norm_no_rows_launches_nothing_forward():
    """M = 0 returns before any launch: FA_OK without a device."""
    assert _lib.load().fa_dropout_norm_fwd(_fwd(M=0), None) == OK


def test_dropout_norm_2_31_elements_validate():
    """Rows are addressed in 64 bits: M * N = 2^31 + 3 N."""
    m, n = (1 << 18) + 3, 8192
    lib = _lib.load()
    assert lib.fa_dropout_norm_fwd_validate(_fwd(M=m, N=n)) == OK
    assert lib.fa_dropout_norm_bwd_validate(_bwd(M=m, N=n)) == OK


def test_dropout_norm_bwd_workspace_depends_on_the_shape_and_the_sums_only():
    """One fp32 partial row per column sum and workgroup; the workgroup count is a function of M (at most 1024 + a remainder,
    at least 16 rows each), the sums 2 (dw0, db0), 3 (and dcolscale) or 4 (two weights); never of dtypes, strides or pointers.
    Rows that some access shape takes as wide (N > 2048) add two floats per row."""
    lib = _lib.load()
    plain = dict(colscale=0, x0=0, dcolscale=0)

    def bytes_of(m, n, **kw):
        return lib.fa_dropout_norm_bwd_workspace_bytes(_bwd(M=m, N=n, sized=False, **kw))
    for m, parts in ((1, 1), (16, 1), (17, 2), (111, 7), (65536, 1024), (1 << 20, 1024)):
        assert bytes_of(m, 192, **plain) == parts * 192 * 2 * 4 == U.bwd_workspace_bytes(m, 192, 2)
        assert bytes_of(m, 192) == parts * 192 * 3 * 4
        assert bytes_of(m, 192, **BWD_PARALLEL) == parts * 192 * 4 * 4
    for n in (8, 203, 2048, 2049, 4096, 8192, 32768):
        a = bytes_of(3000, n)
        b = bytes_of(3000, n, x_dtype=FP32, x=ADDR + 4, x_row_stride=n + 3, p_dropout=0.0) if n * 4 <= 65536 else a
        assert a == b == U.bwd_workspace_bytes(3000, n, 3) == 188 * n * 12 + (3000 * 8 if n > 2048 else 0)
    assert bytes_of(0, 192) == 0


def test_dropout_norm_symbols_and_sizes():
    lib = _lib.load()
    header = open(os.path.join(_lib.INCLUDE, "fa_dropout_norm.h")).read()
    declared = re.findall(r"^\w[\w ]*?\b(fa_\w+)\(", header, re.M)
    assert sorted(declared) == sorted(SYMBOLS) == sorted(_lib.DROPOUT_NORM_SYMBOLS)
    for name in SYMBOLS:
        assert hasattr(lib, name)
    assert lib.fa_dropout_norm_fwd_params_size() == ctypes.sizeof(_lib.FaDropoutNormFwdParams) == 248
    assert lib.fa_dropout_norm_bwd_params_size() == ctypes.sizeof(_lib.FaDropoutNormBwdParams) == 296
    assert ctypes.sizeof(_lib.FaDropoutNormPlan) == 36
    # additive: a header of its own; the ABI version, the other symbol sets and the existing structs are what they were
    assert lib.fa_abi_version() == 13 == _lib.FA_ABI_VERSION
    for others in (_lib.EXPORTED_SYMBOLS, _lib.ROTARY_EMB_SYMBOLS, _lib.NORM_SYMBOLS, _lib.XENT_SYMBOLS, _lib.ACT_SYMBOLS,
                   _lib.GEMM_ACT_SYMBOLS):
        assert not set(SYMBOLS) & set(others)
    for other in os.listdir(_lib.INCLUDE):
        if other != "fa_dropout_norm.h":
            assert "fa_dropout_norm" not in open(os.path.join(_lib.INCLUDE, other)).read(), other
    assert lib.fa_norm_fwd_params_size() == ctypes.sizeof(_lib.FaNormFwdParams) == 160
    assert lib.fa_norm_bwd_params_size() == ctypes.sizeof(_lib.FaNormBwdParams) == 232


def test_dropout_norm_device_code():
    """The translation unit holds exactly the kernels DESIGN 4.26 lists, and none has a private segment: nothing spills, nothing
    is called."""
    from device_asm import kernel_bodies
    found = {}
    for sym, body in kernel_bodies("fa_dropout_norm.hip"):
        k = re.match(r"_ZN\d+_GLOBAL__N_1\d+(dropout_norm_\w+?_kernel)(?:I((?:L[ib]\d+E)+)E)?(?:Ev|v|E)?\w*$", sym)
        assert k, f"a kernel in fa_dropout_norm.hip of no known family: {sym}"
        args = re.findall(r"L([ib])(\d+)E", k.group(2) or "")
        key = (k.group(1), *(bool(int(v)) if t == "b" else int(v) for t, v in args))
        assert key not in found, sym
        found[key] = int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body).group(1))
    assert set(found) == U.KERNELS and len(found) == 16
    assert all(v == 0 for v in found.values()), found
