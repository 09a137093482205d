"""CPU tests of the fused GEMM's C-ABI (include/fa_gemm_act.h: fa_gemm_act_fwd / fa_gemm_act_dgrad, their _validate,
_params_size, _plan and _workspace_bytes) and of the device code of its translation unit, csrc/fa_gemm_act.hip.  Nothing here
touches a device; tests/test_gemm_act_gpu.py checks what the kernels write."""
import ctypes
import os
import re

import pytest

from flash_attention_annotated_amd import _lib

ADDR = 0x10000  # an aligned dummy address: nothing is dereferenced
OK, NULLP, BAD_DTYPE, BAD_SHAPE, BAD_STRIDE, UNSUPPORTED, BAD_ABI, WORKSPACE = 0, -1, -2, -5, -6, -7, -9, -11
BF16, FP16, FP32, FP8 = _lib.FA_DTYPE_BF16, _lib.FA_DTYPE_FP16, _lib.FA_DTYPE_FP32, _lib.FA_DTYPE_FP8_E4M3
SYMBOLS = ("fa_gemm_act_fwd", "fa_gemm_act_fwd_validate", "fa_gemm_act_fwd_params_size", "fa_gemm_act_dgrad",
           "fa_gemm_act_dgrad_validate", "fa_gemm_act_dgrad_params_size", "fa_gemm_act_dgrad_workspace_bytes",
           "fa_gemm_act_fwd_plan", "fa_gemm_act_dgrad_plan")
FWD_DTYPES = ("x", "weight", "bias", "out", "act_input")
DGRAD_DTYPES = ("grad_out", "weight", "act_input", "grad_in", "dbias")


def _fwd(M=300, N=264, K=200, dtype=None, **fields):
    """contiguous bf16 x (M, K) and weight (N, K), no bias, no act_input"""
    p = _lib.new_gemm_act_fwd_params()
    p.x, p.weight, p.out = ADDR, ADDR + (1 << 40), ADDR + (2 << 40)
    p.M, p.N, p.K, p.activation = M, N, K, _lib.FA_ACT_SQRELU
    p.x_row_stride, p.weight_row_stride, p.out_row_stride, p.act_input_row_stride = K, K, N, N
    for t in FWD_DTYPES if dtype is not None else ():
        setattr(p, f"{t}_dtype", dtype)
    for k, v in fields.items():
        setattr(p, k, v)
    return p


def _dgrad(M=300, N=264, K=200, dbias=False, dtype=None, **fields):
    """contiguous bf16 grad_out (M, K), weight (K, N) and act_input (M, N)"""
    p = _lib.new_gemm_act_dgrad_params()
    p.grad_out, p.weight, p.act_input, p.grad_in = ADDR, ADDR + (1 << 40), ADDR + (2 << 40), ADDR + (3 << 40)
    p.M, p.N, p.K, p.activation = M, N, K, _lib.FA_ACT_SQRELU
    p.grad_out_row_stride, p.weight_row_stride, p.act_input_row_stride, p.grad_in_row_stride = K, N, N, N
    if dbias:  # (True: at an aligned address; an address: there)
        p.dbias, p.workspace, p.workspace_bytes = ADDR + (4 << 40) if dbias is True else dbias, ADDR + (5 << 40), 1 << 50
    for t in DGRAD_DTYPES if dtype is not None else ():
        setattr(p, f"{t}_dtype", dtype)
    for k, v in fields.items():
        setattr(p, k, v)
    return p


BIG_M = (1 << 31) // 8 + 1  # M * N passes 2^31 at N = 8

FWD = [
    ("bf16", _fwd(), OK),
    ("fp16", _fwd(dtype=FP16), OK),
    ("bias", _fwd(bias=ADDR + (3 << 40)), OK),
    ("act_input", _fwd(act_input=ADDR + (4 << 40)), OK),
    ("bias_and_act_input", _fwd(bias=ADDR + (3 << 40), act_input=ADDR + (4 << 40)), OK),
    ("every_activation_6", _fwd(activation=_lib.FA_ACT_IDENTITY), OK),
    ("relu", _fwd(activation=_lib.FA_ACT_RELU), OK),
    ("no_rows", _fwd(M=0), OK),
    ("k_8", _fwd(K=8), OK),
    ("n_8", _fwd(N=8), OK),
    ("past_2_31_elements", _fwd(M=BIG_M, N=8, K=8), OK),
    ("pitch_above_k", _fwd(x_row_stride=208, weight_row_stride=216, out_row_stride=272), OK),
    ("one_row_any_pitch", _fwd(M=1, x_row_stride=0, out_row_stride=0), OK),
    ("abi_version", _fwd(abi_version=12), BAD_ABI),
    ("struct_size", _fwd(struct_size=8), BAD_ABI),
    ("null_x", _fwd(x=0), NULLP),
    ("null_weight", _fwd(weight=0), NULLP),
    ("null_out", _fwd(out=0), NULLP),
    ("fp32", _fwd(dtype=FP32), BAD_DTYPE),
    ("fp8", _fwd(dtype=FP8), BAD_DTYPE),
    ("weight_of_another_dtype", _fwd(weight_dtype=FP16), BAD_DTYPE),
    ("out_of_another_dtype", _fwd(out_dtype=FP16), BAD_DTYPE),
    ("bias_fp32_beside_bf16", _fwd(bias=ADDR, bias_dtype=FP32), BAD_DTYPE),
    ("act_input_of_another_dtype", _fwd(act_input=ADDR, act_input_dtype=FP16), BAD_DTYPE),
    ("activation_unknown", _fwd(activation=7), UNSUPPORTED),
    ("activation_negative", _fwd(activation=-1), UNSUPPORTED),
    ("n_130", _fwd(N=130), BAD_SHAPE),
    ("k_36", _fwd(K=36), BAD_SHAPE),
    ("n_0", _fwd(N=0), BAD_SHAPE),
    ("k_0", _fwd(K=0), BAD_SHAPE),
    ("m_negative", _fwd(M=-1), BAD_SHAPE),
    ("x_odd_base", _fwd(x=ADDR + 2), BAD_STRIDE),
    ("weight_8_byte_base", _fwd(weight=ADDR + 8), BAD_STRIDE),
    ("out_odd_base", _fwd(out=ADDR + 6), BAD_STRIDE),
    ("bias_odd_base", _fwd(bias=ADDR + 2), BAD_STRIDE),
    ("act_input_odd_base", _fwd(act_input=ADDR + 4), BAD_STRIDE),
    ("x_pitch_below_k", _fwd(x_row_stride=192), BAD_STRIDE),
    ("x_pitch_no_multiple_of_8", _fwd(x_row_stride=204), BAD_STRIDE),
    ("weight_pitch_no_multiple_of_8", _fwd(weight_row_stride=201), BAD_STRIDE),
    ("out_pitch_below_n", _fwd(out_row_stride=256), BAD_STRIDE),
    ("act_input_pitch_no_multiple_of_8", _fwd(act_input=ADDR, act_input_row_stride=268), BAD_STRIDE),
]

DGRAD = [
    ("bf16", _dgrad(), OK),
    ("fp16", _dgrad(dtype=FP16), OK),
    ("dbias", _dgrad(dbias=True), OK),
    ("identity_without_act_input", _dgrad(activation=_lib.FA_ACT_IDENTITY, act_input=0), OK),
    ("identity_with_act_input", _dgrad(activation=_lib.FA_ACT_IDENTITY), OK),
    ("no_rows", _dgrad(M=0), OK),
    ("no_rows_dbias_no_workspace", _dgrad(M=0, dbias=True, workspace=0, workspace_bytes=0), OK),
    ("k_8", _dgrad(K=8), OK),
    ("past_2_31_elements", _dgrad(M=BIG_M, N=8, K=8, dbias=True), OK),
    ("workspace_exact", _dgrad(dbias=True, workspace_bytes=3 * 264 * 4), OK),
    ("abi_version", _dgrad(abi_version=12), BAD_ABI),
    ("struct_size", _dgrad(struct_size=8), BAD_ABI),
    ("null_grad_out", _dgrad(grad_out=0), NULLP),
    ("null_weight", _dgrad(weight=0), NULLP),
    ("null_grad_in", _dgrad(grad_in=0), NULLP),
    ("null_act_input_with_an_activation", _dgrad(act_input=0), NULLP),
    ("fp32", _dgrad(dtype=FP32), BAD_DTYPE),
    ("weight_of_another_dtype", _dgrad(weight_dtype=FP16), BAD_DTYPE),
    ("act_input_of_another_dtype", _dgrad(act_input_dtype=FP16), BAD_DTYPE),
    ("grad_in_fp32", _dgrad(grad_in_dtype=FP32), BAD_DTYPE),
    ("dbias_fp32_beside_bf16", _dgrad(dbias=True, dbias_dtype=FP32), BAD_DTYPE),
    ("activation_unknown", _dgrad(activation=99), UNSUPPORTED),
    ("n_130", _dgrad(N=130), BAD_SHAPE),
    ("k_36", _dgrad(K=36), BAD_SHAPE),
    ("m_negative", _dgrad(M=-1), BAD_SHAPE),
    ("grad_out_odd_base", _dgrad(grad_out=ADDR + 2), BAD_STRIDE),
    ("act_input_odd_base", _dgrad(act_input=ADDR + (2 << 40) + 8), BAD_STRIDE),
    ("dbias_odd_base", _dgrad(dbias=ADDR + 2), BAD_STRIDE),
    ("grad_out_pitch_below_k", _dgrad(grad_out_row_stride=192), BAD_STRIDE),
    ("weight_pitch_below_n", _dgrad(weight_row_stride=200), BAD_STRIDE),
    ("grad_in_pitch_no_multiple_of_8", _dgrad(grad_in_row_stride=268), BAD_STRIDE),
    ("act_input_pitch_below_n", _dgrad(act_input_row_stride=8), BAD_STRIDE),
    ("workspace_8_bytes", _dgrad(dbias=True, workspace=ADDR + 8), BAD_STRIDE),
    ("workspace_missing", _dgrad(dbias=True, workspace=0), WORKSPACE),
    ("workspace_short", _dgrad(dbias=True, workspace_bytes=3 * 264 * 4 - 1), WORKSPACE),
]


@pytest.mark.parametrize("name,p,status", FWD, ids=[r[0] for r in FWD])
def test_gemm_act_fwd_validate(name, p, status):
    lib = _lib.load()
    assert lib.fa_gemm_act_fwd_validate(p) == status
    if status != OK:  # the launch entry refuses the same way before it launches anything
        assert lib.fa_gemm_act_fwd(p, None) == status


@pytest.mark.parametrize("name,p,status", DGRAD, ids=[r[0] for r in DGRAD])
def test_gemm_act_dgrad_validate(name, p, status):
    lib = _lib.load()
    assert lib.fa_gemm_act_dgrad_validate(p) == status
    if status != OK:
        assert lib.fa_gemm_act_dgrad(p, None) == status


def test_gemm_act_validate_null():
    lib = _lib.load()
    assert lib.fa_gemm_act_fwd_validate(None) == NULLP and lib.fa_gemm_act_fwd(None, None) == NULLP
    assert lib.fa_gemm_act_dgrad_validate(None) == NULLP and lib.fa_gemm_act_dgrad(None, None) == NULLP


def test_gemm_act_no_rows_launches_nothing():
    """M = 0 returns before any launch: FA_OK without a device."""
    lib = _lib.load()
    assert lib.fa_gemm_act_fwd(_fwd(M=0), None) == OK
    assert lib.fa_gemm_act_dgrad(_dgrad(M=0, dbias=True), None) == OK


def test_gemm_act_workspace_is_a_function_of_the_shape():
    lib = _lib.load()
    need = lambda **kw: lib.fa_gemm_act_dgrad_workspace_bytes(_dgrad(dbias=True, **kw))  # noqa: E731
    assert lib.fa_gemm_act_dgrad_workspace_bytes(_dgrad()) == 0 and need(M=0) == 0
    assert lib.fa_gemm_act_dgrad_workspace_bytes(None) == 0
    assert need() == 3 * 264 * 4  # (three row tiles of 128)
    assert need(M=64) == need(M=1) == 264 * 4 and need(M=65) == 264 * 4 and need(M=129) == 2 * 264 * 4
    assert need(M=BIG_M, N=8) == ((BIG_M + 127) // 128) * 8 * 4
    # nothing but M, N and the presence of dbias is read
    assert need(K=8) == need(dtype=FP16) == need(activation=_lib.FA_ACT_IDENTITY) == need(grad_out=0, grad_out_row_stride=1) == need()


def test_gemm_act_symbols_and_sizes():
    lib = _lib.load()
    header = open(os.path.join(_lib.INCLUDE, "fa_gemm_act.h")).read()
    declared = re.findall(r"^\w[\w ]*?\b(fa_\w+)\(", header, re.M)
    assert sorted(declared) == sorted(SYMBOLS) == sorted(_lib.GEMM_ACT_SYMBOLS)
    for name in SYMBOLS:
        assert hasattr(lib, name)
    assert lib.fa_gemm_act_fwd_params_size() == ctypes.sizeof(_lib.FaGemmActFwdParams) == 120
    assert lib.fa_gemm_act_dgrad_params_size() == ctypes.sizeof(_lib.FaGemmActDgradParams) == 136
    assert ctypes.sizeof(_lib.FaGemmActPlan) == 64
    for struct in (_lib.FaGemmActFwdParams, _lib.FaGemmActDgradParams):  # both begin like every other params struct
        assert [f[0] for f in struct._fields_[:2]] == ["abi_version", "struct_size"]
    # additive: a header of its own; the ABI version, the other symbol sets and the existing structs are what they were
    assert lib.fa_abi_version() == 13 == _lib.FA_ABI_VERSION
    for other in (_lib.EXPORTED_SYMBOLS, _lib.ROTARY_EMB_SYMBOLS, _lib.NORM_SYMBOLS, _lib.XENT_SYMBOLS, _lib.ACT_SYMBOLS):
        assert not set(SYMBOLS) & set(other)
    for other in ("fa_fwd.h", "fa_bwd.h", "fa_rotary.h", "fa_norm.h", "fa_xent.h", "fa_act.h"):
        assert "fa_gemm_act" not in open(os.path.join(_lib.INCLUDE, other)).read()
    sizes = {"fa_fwd_params_size": (_lib.FaFwdParams, 464), "fa_bwd_params_size": (_lib.FaBwdParams, 408),
             "fa_rotary_emb_params_size": (_lib.FaRotaryEmbParams, 184), "fa_norm_fwd_params_size": (_lib.FaNormFwdParams, 160),
             "fa_norm_bwd_params_size": (_lib.FaNormBwdParams, 232), "fa_xent_fwd_params_size": (_lib.FaXentFwdParams, 120),
             "fa_xent_bwd_params_size": (_lib.FaXentBwdParams, 136), "fa_act_fwd_params_size": (_lib.FaActFwdParams, 96),
             "fa_act_bwd_params_size": (_lib.FaActBwdParams, 176)}
    for fn, (struct, size) in sizes.items():
        assert getattr(lib, fn)() == ctypes.sizeof(struct) == size, fn


# the kernels of csrc/fa_gemm_act.hip, by (dtype code, rows of the tile): fp16 = 0, bf16 = 1
FORMS = ({(k, dt, bm) for k in ("gemm_act_fwd_kernel", "gemm_act_dgrad_kernel") for dt in (FP16, BF16) for bm in (64, 128)}
         | {("gemm_act_dbias_reduce_kernel",)})


def test_gemm_act_device_code():
    """The translation unit holds exactly the kernels DESIGN 4.25 lists, and none has a private segment: nothing spills,
    nothing is called."""
    from device_asm import kernel_bodies
    found = {}
    for sym, body in kernel_bodies("fa_gemm_act.hip"):
        k = re.match(r"_ZN\d+_GLOBAL__N_1\d+(gemm_act_\w+?_kernel)(?:I((?:Li\d+E)+)E)?(?:Ev|v)?\w*$", sym)
        assert k, f"a kernel in fa_gemm_act.hip of no known family: {sym}"
        key = (k.group(1), *(int(v) for v in re.findall(r"Li(\d+)E", k.group(2) or "")))
        assert key not in found, sym
        found[key] = int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body).group(1))
    assert set(found) == FORMS
    assert all(v == 0 for v in found.values()), found
