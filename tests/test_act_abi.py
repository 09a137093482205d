"""CPU tests of the fused activations' C-ABI (include/fa_act.h: fa_act_fwd / fa_act_bwd, their _validate, _params_size and
_workspace_bytes) and of the device code of its translation unit, csrc/fa_act.hip.  Nothing here touches a device;
tests/test_act_gpu.py checks what the kernels write."""
import ctypes
import os
import re

import pytest

from flash_attention_annotated_amd import _lib

ADDR = 0x10000  # an aligned dummy address: nothing is dereferenced
OK, NULLP, BAD_DTYPE, BAD_SHAPE, BAD_STRIDE, UNSUPPORTED, BAD_ABI, WORKSPACE = 0, -1, -2, -5, -6, -7, -9, -11
BF16, FP16, FP32, FP8 = _lib.FA_DTYPE_BF16, _lib.FA_DTYPE_FP16, _lib.FA_DTYPE_FP32, _lib.FA_DTYPE_FP8_E4M3
GATED = _lib.FA_ACT_GATED
SYMBOLS = ("fa_act_fwd", "fa_act_fwd_validate", "fa_act_fwd_params_size", "fa_act_bwd", "fa_act_bwd_validate",
           "fa_act_bwd_params_size", "fa_act_bwd_workspace_bytes", "fa_act_fwd_plan", "fa_act_bwd_plan")
FWD_DTYPES = ("pre", "up", "bias", "out")
BWD_DTYPES = ("pre", "up", "bias", "dout", "dpre", "dup", "dbias", "out")


def _fwd(M=37, H=4096, gated=False, dtype=None, **fields):
    """A contiguous bf16 (M, H) without a bias; gated: the two halves of a (M, 2H) tensor."""
    p = _lib.new_act_fwd_params()
    p.pre, p.out = ADDR, ADDR + (1 << 40)
    p.M, p.H, p.pre_row_stride, p.out_row_stride = M, H, H, H
    p.activation = _lib.FA_ACT_GELU_TANH
    if gated:
        p.flags, p.up, p.pre_row_stride, p.activation = GATED, ADDR + 2 * H, 2 * H, _lib.FA_ACT_SILU
    for t in FWD_DTYPES if dtype is not None else ():
        setattr(p, f"{t}_dtype", dtype)
    for k, v in fields.items():
        setattr(p, k, v)
    return p


def _bwd(M=37, H=4096, gated=False, dbias=False, dtype=None, **fields):
    p = _lib.new_act_bwd_params()
    p.pre, p.dout, p.dpre = ADDR, ADDR + (1 << 40), ADDR + (2 << 40)
    p.M, p.H, p.pre_row_stride, p.dout_row_stride, p.dpre_row_stride, p.out_row_stride = M, H, H, H, H, H
    p.activation = _lib.FA_ACT_GELU_TANH
    if gated:
        p.flags, p.up, p.pre_row_stride, p.activation = GATED, ADDR + 2 * H, 2 * H, _lib.FA_ACT_SILU
        p.dup, p.dpre_row_stride = ADDR + (2 << 40) + 2 * H, 2 * H
    if dbias:
        p.bias, p.dbias, p.workspace, p.workspace_bytes = ADDR + (3 << 40), ADDR + (4 << 40), ADDR + (5 << 40), 1 << 40
    for t in BWD_DTYPES if dtype is not None else ():
        setattr(p, f"{t}_dtype", dtype)
    for k, v in fields.items():
        setattr(p, k, v)
    return p


FWD = [
    ("bf16", _fwd(), OK),
    ("fp16", _fwd(dtype=FP16), OK),
    ("fp32", _fwd(dtype=FP32), OK),
    ("every_activation_6", _fwd(activation=_lib.FA_ACT_IDENTITY), OK),
    ("bias", _fwd(bias=ADDR), OK),
    ("bias_fp32", _fwd(bias=ADDR, bias_dtype=FP32), OK),
    ("gated_packed", _fwd(gated=True), OK),
    ("gated_203_in_406", _fwd(H=203, gated=True), OK),
    ("no_rows", _fwd(M=0), OK),
    ("one_column", _fwd(H=1), OK),
    ("odd_base", _fwd(pre=ADDR + 2, out=ADDR + 6), OK),
    ("rows_2_31_of_them", _fwd(M=1 << 31), OK),
    ("past_2_31_elements", _fwd(M=16400, H=65536, gated=True), OK),
    ("pitch_above_h", _fwd(pre_row_stride=4099, out_row_stride=5000), OK),
    ("one_row_any_pitch", _fwd(M=1, pre_row_stride=0, out_row_stride=0), OK),
    ("abi_version", _fwd(abi_version=12), BAD_ABI),
    ("struct_size", _fwd(struct_size=8), BAD_ABI),
    ("null_pre", _fwd(pre=0), NULLP),
    ("null_out", _fwd(out=0), NULLP),
    ("null_up_gated", _fwd(gated=True, up=0), NULLP),
    ("pre_fp8", _fwd(dtype=FP8), BAD_DTYPE),
    ("pre_dtype_unknown", _fwd(pre_dtype=7), BAD_DTYPE),
    ("out_of_another_dtype", _fwd(out_dtype=FP32), BAD_DTYPE),
    ("up_of_another_dtype", _fwd(gated=True, up_dtype=FP16), BAD_DTYPE),
    ("bias_fp16_beside_bf16", _fwd(bias=ADDR, bias_dtype=FP16), BAD_DTYPE),
    ("activation_unknown", _fwd(activation=7), UNSUPPORTED),
    ("activation_negative", _fwd(activation=-1), UNSUPPORTED),
    ("h_0", _fwd(H=0), BAD_SHAPE),
    ("m_negative", _fwd(M=-1), BAD_SHAPE),
    ("flags_unknown", _fwd(flags=2), BAD_SHAPE),
    ("bias_with_gated", _fwd(gated=True, bias=ADDR), BAD_SHAPE),
    ("pitch_below_h", _fwd(pre_row_stride=4095), BAD_STRIDE),
    ("out_pitch_below_h", _fwd(out_row_stride=4095), BAD_STRIDE),
    ("pre_odd_address", _fwd(pre=ADDR + 1), BAD_STRIDE),
    ("fp32_out_2_bytes", _fwd(dtype=FP32, out=ADDR + 2), BAD_STRIDE),
    ("fp32_bias_2_bytes", _fwd(bias=ADDR + 2, bias_dtype=FP32), BAD_STRIDE),
]

BWD = [
    ("bf16", _bwd(), OK),
    ("fp16", _bwd(dtype=FP16), OK),
    ("fp32", _bwd(dtype=FP32), OK),
    ("dbias", _bwd(dbias=True), OK),
    ("dbias_fp32", _bwd(dbias=True, bias_dtype=FP32, dbias_dtype=FP32), OK),
    ("dbias_without_bias", _bwd(dbias=True, bias=0), OK),
    ("recompute", _bwd(recompute_out=ADDR + (6 << 40)), OK),
    ("gated_packed", _bwd(gated=True), OK),
    ("gated_recompute", _bwd(gated=True, recompute_out=ADDR + (6 << 40)), OK),
    ("gated_203_in_406", _bwd(H=203, gated=True), OK),
    ("no_rows", _bwd(M=0), OK),
    ("no_rows_dbias_no_workspace", _bwd(M=0, dbias=True, workspace=0, workspace_bytes=0), OK),
    ("rows_2_31_of_them", _bwd(M=1 << 31, dbias=True), OK),
    ("past_2_31_elements", _bwd(M=16400, H=65536, gated=True), OK),
    ("another_phase", _bwd(dpre=ADDR + (2 << 40) + 6), OK),
    ("abi_version", _bwd(abi_version=12), BAD_ABI),
    ("struct_size", _bwd(struct_size=8), BAD_ABI),
    ("null_pre", _bwd(pre=0), NULLP),
    ("null_dout", _bwd(dout=0), NULLP),
    ("null_dpre", _bwd(dpre=0), NULLP),
    ("null_up_gated", _bwd(gated=True, up=0), NULLP),
    ("null_dup_gated", _bwd(gated=True, dup=0), NULLP),
    ("dout_of_another_dtype", _bwd(dout_dtype=FP16), BAD_DTYPE),
    ("dpre_fp8", _bwd(dpre_dtype=FP8), BAD_DTYPE),
    ("dup_of_another_dtype", _bwd(gated=True, dup_dtype=FP32), BAD_DTYPE),
    ("recompute_of_another_dtype", _bwd(recompute_out=ADDR, out_dtype=FP32), BAD_DTYPE),
    ("dbias_fp16_beside_bf16", _bwd(dbias=True, dbias_dtype=FP16), BAD_DTYPE),
    ("activation_unknown", _bwd(activation=99), UNSUPPORTED),
    ("h_negative", _bwd(H=-8), BAD_SHAPE),
    ("m_negative", _bwd(M=-1), BAD_SHAPE),
    ("bias_with_gated", _bwd(gated=True, bias=ADDR), BAD_SHAPE),
    ("dbias_with_gated", _bwd(gated=True, dbias=True, bias=0), BAD_SHAPE),
    ("pitch_below_h", _bwd(pre_row_stride=100), BAD_STRIDE),
    ("dout_pitch_below_h", _bwd(dout_row_stride=4095), BAD_STRIDE),
    ("dpre_pitch_below_h", _bwd(dpre_row_stride=4095), BAD_STRIDE),
    ("recompute_pitch_below_h", _bwd(recompute_out=ADDR, out_row_stride=7), BAD_STRIDE),
    ("dpre_odd_address", _bwd(dpre=ADDR + 1), BAD_STRIDE),
    ("workspace_8_bytes", _bwd(dbias=True, workspace=ADDR + 8), BAD_STRIDE),
    ("workspace_missing", _bwd(dbias=True, workspace=0), WORKSPACE),
    ("workspace_short", _bwd(dbias=True, workspace_bytes=2 * 4096 * 4 - 1), WORKSPACE),
]


@pytest.mark.parametrize("name,p,status", FWD, ids=[r[0] for r in FWD])
def test_act_fwd_validate(name, p, status):
    lib = _lib.load()
    assert lib.fa_act_fwd_validate(p) == status
    if status != OK:  # the launch entry refuses the same way before it launches anything
        assert lib.fa_act_fwd(p, None) == status


@pytest.mark.parametrize("name,p,status", BWD, ids=[r[0] for r in BWD])
def test_act_bwd_validate(name, p, status):
    lib = _lib.load()
    assert lib.fa_act_bwd_validate(p) == status
    if status != OK:
        assert lib.fa_act_bwd(p, None) == status


def test_act_validate_null():
    lib = _lib.load()
    assert lib.fa_act_fwd_validate(None) == NULLP and lib.fa_act_fwd(None, None) == NULLP
    assert lib.fa_act_bwd_validate(None) == NULLP and lib.fa_act_bwd(None, None) == NULLP


def test_act_no_rows_launches_nothing():
    """M = 0 returns before any launch: FA_OK without a device."""
    lib = _lib.load()
    assert lib.fa_act_fwd(_fwd(M=0), None) == OK and lib.fa_act_fwd(_fwd(M=0, gated=True), None) == OK
    assert lib.fa_act_bwd(_bwd(M=0, dbias=True), None) == OK and lib.fa_act_bwd(_bwd(M=0, gated=True), None) == OK


def test_act_workspace_is_a_function_of_m_and_h():
    lib = _lib.load()
    need = lambda **kw: lib.fa_act_bwd_workspace_bytes(_bwd(dbias=True, **kw))  # noqa: E731
    assert lib.fa_act_bwd_workspace_bytes(_bwd()) == 0 and need(M=0) == 0 and lib.fa_act_bwd_workspace_bytes(None) == 0
    assert need(M=37) == 2 * 4096 * 4 and need(M=32) == 4096 * 4 and need(M=33) == 2 * 4096 * 4
    assert need(M=37, H=203) == 2 * 204 * 4  # (partial rows are padded to 16 bytes)
    assert need(M=32 * 1024) == need(M=1 << 31) == 1024 * 4096 * 4  # (at most 1024 partial rows)
    assert need(M=37, dtype=FP32) == need(M=37)


def test_act_symbols_and_sizes():
    lib = _lib.load()
    header = open(os.path.join(_lib.INCLUDE, "fa_act.h")).read()
    declared = re.findall(r"^\w[\w ]*?\b(fa_\w+)\(", header, re.M)
    assert sorted(declared) == sorted(SYMBOLS) == sorted(_lib.ACT_SYMBOLS)
    for name in SYMBOLS:
        assert hasattr(lib, name)
    assert lib.fa_act_fwd_params_size() == ctypes.sizeof(_lib.FaActFwdParams) == 96
    assert lib.fa_act_bwd_params_size() == ctypes.sizeof(_lib.FaActBwdParams) == 176
    assert ctypes.sizeof(_lib.FaActPlan) == 20
    for struct in (_lib.FaActFwdParams, _lib.FaActBwdParams):  # both begin like every other params struct
        assert [f[0] for f in struct._fields_[:2]] == ["abi_version", "struct_size"]
    codes = [getattr(_lib, f"FA_ACT_{n}") for n in ("GELU_TANH", "GELU_ERF", "RELU", "SQRELU", "SILU", "SIGMOID", "IDENTITY")]
    assert codes == list(range(7)) == [int(re.search(rf"#define FA_ACT_{n} (\d+)", header).group(1))
                                       for n in ("GELU_TANH", "GELU_ERF", "RELU", "SQRELU", "SILU", "SIGMOID", "IDENTITY")]
    # additive: a header of its own; the ABI version, the other symbol sets and the existing structs are what they were
    assert lib.fa_abi_version() == 13 == _lib.FA_ABI_VERSION
    for other in (_lib.EXPORTED_SYMBOLS, _lib.ROTARY_EMB_SYMBOLS, _lib.NORM_SYMBOLS, _lib.XENT_SYMBOLS):
        assert not set(SYMBOLS) & set(other)
    for other in ("fa_fwd.h", "fa_bwd.h", "fa_rotary.h", "fa_norm.h", "fa_xent.h"):
        assert "fa_act" not in open(os.path.join(_lib.INCLUDE, other)).read()
    sizes = {"fa_fwd_params_size": (_lib.FaFwdParams, 464), "fa_bwd_params_size": (_lib.FaBwdParams, 408),
             "fa_rotary_emb_params_size": (_lib.FaRotaryEmbParams, 184), "fa_norm_fwd_params_size": (_lib.FaNormFwdParams, 160),
             "fa_norm_bwd_params_size": (_lib.FaNormBwdParams, 232), "fa_xent_fwd_params_size": (_lib.FaXentFwdParams, 120),
             "fa_xent_bwd_params_size": (_lib.FaXentBwdParams, 136)}
    for fn, (struct, size) in sizes.items():
        assert getattr(lib, fn)() == ctypes.sizeof(struct) == size, fn


# the kernels of csrc/fa_act.hip, by the elements of one access (8 x 16-bit or 4 x fp32 in 16 bytes; 1: elements)
FORMS = {("act_fwd_kernel", 8), ("act_fwd_kernel", 4), ("act_fwd_kernel", 1),
         ("act_bwd_kernel", 8), ("act_bwd_kernel", 4), ("act_bwd_kernel", 1), ("act_dbias_reduce_kernel",)}


def test_act_device_code():
    """The translation unit holds exactly the kernels DESIGN 4.24 lists, and none has a private segment: nothing spills,
    nothing is called."""
    from device_asm import kernel_bodies
    found = {}
    for sym, body in kernel_bodies("fa_act.hip"):
        k = re.match(r"_ZN\d+_GLOBAL__N_1\d+(act_\w+?_kernel)(?:I((?:Li\d+E)+)E)?(?:Ev|v)?\w*$", sym)
        assert k, f"a kernel in fa_act.hip of no known family: {sym}"
        key = (k.group(1), *(int(v) for v in re.findall(r"Li(\d+)E", k.group(2) or "")))
        assert key not in found, sym
        found[key] = int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body).group(1))
    assert set(found) == FORMS
    assert all(v == 0 for v in found.values()), found
