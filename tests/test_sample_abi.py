"""CPU tests of the token sampling's C-ABI (include/fa_sample.h: fa_sample, fa_sample_validate, fa_sample_params_size,
fa_sample_plan) and of the device code of its translation unit, csrc/fa_sample.hip.  Nothing here touches a device;
tests/test_sample_gpu.py checks what the kernels write."""
import ctypes
import os
import re

import pytest

import sample_plan_universe as U
from flash_attention_annotated_amd import _lib

ADDR = 0x10000  # an aligned dummy address: nothing is dereferenced
OK, NULLP, BAD_DTYPE, BAD_SHAPE, BAD_STRIDE, BAD_ABI = 0, -1, -2, -5, -6, -9
BF16, FP16, FP32, FP8 = _lib.FA_DTYPE_BF16, _lib.FA_DTYPE_FP16, _lib.FA_DTYPE_FP32, _lib.FA_DTYPE_FP8_E4M3
DRAW, FILTER = _lib.FA_SAMPLE_DRAW, _lib.FA_SAMPLE_FILTER
SYMBOLS = ("fa_sample", "fa_sample_validate", "fa_sample_params_size", "fa_sample_plan")


def _p(B=5, V=4096, **fields):
    """A contiguous bf16 (B, V) drawn with uniforms: top_k 50, top_p 0.9."""
    p = _lib.new_sample_params()
    p.logits, p.u, p.token = ADDR, ADDR, ADDR
    p.B, p.V, p.logits_row_stride, p.top_k, p.top_p = B, V, V, 50, 0.9
    for k, v in fields.items():
        setattr(p, k, v)
    return p


CASES = [
    ("bf16_u", _p(), OK),
    ("fp16", _p(logits_dtype=FP16), OK),
    ("fp32", _p(logits_dtype=FP32), OK),
    ("rng_state", _p(u=0, rng_state=ADDR), OK),
    ("kept_and_mass", _p(kept=ADDR, mass=ADDR), OK),
    ("no_rows", _p(B=0), OK),
    ("one_column", _p(V=1), OK),
    ("odd_width_odd_base", _p(V=50257, logits=ADDR + 2), OK),
    ("widest_row", _p(B=1, V=(1 << 31) - 1), OK),
    ("past_2_31_elements", _p(B=32768, V=128256), OK),
    ("row_stride_above_v", _p(logits_row_stride=4099), OK),
    ("row_stride_0_in_a_draw", _p(logits_row_stride=0), OK),
    ("top_k_0", _p(top_k=0), OK),
    ("top_k_above_v", _p(top_k=5000), OK),
    ("top_p_0", _p(top_p=0.0), OK),
    ("top_p_1", _p(top_p=1.0), OK),
    ("temperature", _p(temperature=0.7), OK),
    ("greedy_needs_no_uniforms", _p(top_k=1, u=0), OK),
    ("filter", _p(mode=FILTER, u=0, token=0), OK),
    ("filter_top_k_1", _p(mode=FILTER, u=0, token=0, top_k=1, kept=ADDR, mass=ADDR), OK),
    ("abi_version", _p(abi_version=12), BAD_ABI),
    ("struct_size", _p(struct_size=8), BAD_ABI),
    ("logits_fp8", _p(logits_dtype=FP8), BAD_DTYPE),
    ("logits_dtype_unknown", _p(logits_dtype=7), BAD_DTYPE),
    ("v_0", _p(V=0), BAD_SHAPE),
    ("v_negative", _p(V=-8), BAD_SHAPE),  # (what 2^31 and above are in the field)
    ("b_negative", _p(B=-1), BAD_SHAPE),
    ("mode_unknown", _p(mode=2), BAD_SHAPE),
    ("temperature_0", _p(temperature=0.0), BAD_SHAPE),
    ("temperature_negative", _p(temperature=-1.0), BAD_SHAPE),
    ("temperature_nan", _p(temperature=float("nan")), BAD_SHAPE),
    ("top_p_negative", _p(top_p=-0.1), BAD_SHAPE),
    ("top_p_above_1", _p(top_p=1.5), BAD_SHAPE),
    ("top_p_nan", _p(top_p=float("nan")), BAD_SHAPE),
    ("top_k_negative", _p(top_k=-1), BAD_SHAPE),
    ("null_logits", _p(logits=0), NULLP),
    ("null_token", _p(token=0), NULLP),
    ("neither_u_nor_rng_state", _p(u=0), NULLP),
    ("both_u_and_rng_state", _p(rng_state=ADDR), BAD_SHAPE),
    ("greedy_with_kept", _p(top_k=1, kept=ADDR), BAD_SHAPE),
    ("logits_odd_address", _p(logits=ADDR + 1), BAD_STRIDE),
    ("fp32_logits_2_bytes", _p(logits=ADDR + 2, logits_dtype=FP32), BAD_STRIDE),
    ("u_2_bytes", _p(u=ADDR + 2), BAD_STRIDE),
    ("rng_state_4_bytes", _p(u=0, rng_state=ADDR + 4), BAD_STRIDE),
    ("token_4_bytes", _p(token=ADDR + 4), BAD_STRIDE),
    ("kept_2_bytes", _p(kept=ADDR + 2), BAD_STRIDE),
    ("filter_rows_overlap", _p(mode=FILTER, u=0, logits_row_stride=4095), BAD_STRIDE),
]


@pytest.mark.parametrize("name,p,status", CASES, ids=[r[0] for r in CASES])
def test_sample_validate(name, p, status):
    lib = _lib.load()
    assert lib.fa_sample_validate(p) == status
    if status != OK:  # the launch entry refuses the same way before it launches anything
        assert lib.fa_sample(p, None) == status


def test_sample_validate_null_and_no_rows():
    """A NULL params is refused; B = 0 returns before any launch: FA_OK without a device."""
    lib = _lib.load()
    assert lib.fa_sample_validate(None) == NULLP and lib.fa_sample(None, None) == NULLP
    assert lib.fa_sample(_p(B=0), None) == OK and lib.fa_sample(_p(B=0, mode=FILTER, u=0), None) == OK
    assert lib.fa_sample(_p(B=0, top_k=1), None) == OK


def test_sample_symbols_and_sizes():
    lib = _lib.load()
    header = open(os.path.join(_lib.INCLUDE, "fa_sample.h")).read()
    declared = re.findall(r"^\w[\w ]*?\b(fa_\w+)\(", header, re.M)
    assert sorted(declared) == sorted(SYMBOLS) == sorted(_lib.SAMPLE_SYMBOLS)
    for name in SYMBOLS:
        assert hasattr(lib, name)
    assert lib.fa_sample_params_size() == ctypes.sizeof(_lib.FaSampleParams) == 96
    assert ctypes.sizeof(_lib.FaSampleForm) == 56
    assert [f[0] for f in _lib.FaSampleParams._fields_[:2]] == ["abi_version", "struct_size"]
    # additive: a header of its own; the ABI version, the other symbol sets and the existing structs are what they were
    assert lib.fa_abi_version() == 13 == _lib.FA_ABI_VERSION
    for other in (_lib.EXPORTED_SYMBOLS, _lib.ROTARY_EMB_SYMBOLS, _lib.NORM_SYMBOLS, _lib.XENT_SYMBOLS, _lib.ACT_SYMBOLS,
                  _lib.GEMM_ACT_SYMBOLS, _lib.DROPOUT_NORM_SYMBOLS):
        assert not set(SYMBOLS) & set(other)
    headers = sorted(f for f in os.listdir(_lib.INCLUDE) if f.endswith(".h"))
    assert "fa_sample.h" in headers and len(headers) >= 9
    for other in headers:
        if other != "fa_sample.h":
            assert "fa_sample" not in open(os.path.join(_lib.INCLUDE, other)).read(), other
    sizes = {"fa_fwd_params_size": (_lib.FaFwdParams, 464), "fa_bwd_params_size": (_lib.FaBwdParams, 408),
             "fa_xent_fwd_params_size": (_lib.FaXentFwdParams, 120), "fa_xent_bwd_params_size": (_lib.FaXentBwdParams, 136),
             "fa_norm_fwd_params_size": (_lib.FaNormFwdParams, 160), "fa_norm_bwd_params_size": (_lib.FaNormBwdParams, 232)}
    for fn, (struct, size) in sizes.items():
        assert getattr(lib, fn)() == ctypes.sizeof(struct) == size, fn


def test_sample_plan_struct_is_the_mirror():
    """fa_sample_plan fills every field of the mirror: a form whose fields are all distinct comes back in order."""
    lib = _lib.load()
    form = _lib.FaSampleForm()
    assert lib.fa_sample_plan(_p(B=70000, V=4099, logits_dtype=FP16, temperature=0.7, top_k=37, top_p=0.5), form) == OK
    got = U.Plan(*(getattr(form, f) for f in U.Plan._fields))
    assert got == U.Plan(cw=1, threads=1024, mode=0, greedy=0, topk=1, topp=1, draw=1, k=37, key_bits=32, key_passes=3, index_bits=13,
                         index_passes=2, frac_bits=40, grid_x=65535)
    assert [f[0] for f in _lib.FaSampleForm._fields_] == list(U.Plan._fields)


def test_sample_device_code():
    """The translation unit holds exactly the kernels of the universe, and none has a private segment: nothing spills, nothing
    is called."""
    from device_asm import kernel_bodies
    found = {}
    for sym, body in kernel_bodies("fa_sample.hip"):
        k = re.match(r"_ZN\d+_GLOBAL__N_1\d+(sample_(?:\w+_)?kernel)I((?:Li\d+E)+)EEv16fa_sample_params14fa_sample_form$", sym)
        assert k, f"a kernel in fa_sample.hip of no known family: {sym}"
        args = [int(v) for v in re.findall(r"Li(\d+)E", k.group(2))]
        key = (k.group(1), args[0], args[1] if len(args) > 1 else None)
        assert key not in found, sym
        found[key] = int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body).group(1))
    assert set(found) == U.KERNELS
    assert all(v == 0 for v in found.values()), found
    assert {U.kernel_of(U.case_plan(c)) for c in U.CASES} == U.KERNELS  # the GPU cases run every one of them
