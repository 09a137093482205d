"""CPU tests of the C-ABI of the tree-shaped speculative-sampling verification (include/fa_tree_sample.h: fa_tree_sample,
fa_tree_sample_validate, fa_tree_sample_params_size, fa_tree_sample_workspace_size, fa_tree_sample_plan) and of the device code
of its translation unit, csrc/fa_tree_sample.hip.  Nothing here touches a device; tests/test_sample_tree_gpu.py checks what the
kernels write."""
import ctypes
import os
import re

import pytest

import sample_tree_plan_universe as U
from flash_attention_annotated_amd import _lib

ADDR = 0x10000  # an aligned dummy address: nothing is dereferenced
OK, NULLP, BAD_DTYPE, BAD_SHAPE, BAD_STRIDE, BAD_ABI, WORKSPACE = 0, -1, -2, -5, -6, -9, -11
BF16, FP16, FP32, FP8 = _lib.FA_DTYPE_BF16, _lib.FA_DTYPE_FP16, _lib.FA_DTYPE_FP32, _lib.FA_DTYPE_FP8_E4M3
SYMBOLS = ("fa_tree_sample", "fa_tree_sample_validate", "fa_tree_sample_params_size", "fa_tree_sample_workspace_size",
           "fa_tree_sample_plan")


def _p(B=5, T=13, V=4096, **fields):
    """Contiguous bf16 logits and drafts (B, T, V), int64 tokens, uniforms given: top_k 50, top_p 0.9."""
    p = _lib.new_tree_sample_params()
    for name in ("logits", "logits_draft", "tokens_draft", "parents", "u_acc", "u_res", "workspace", "path", "path_len", "tokens",
                 "num_generated"):
        setattr(p, name, ADDR)
    p.B, p.T, p.V, p.top_k, p.top_p = B, T, V, 50, 0.9
    p.logits_batch_stride, p.logits_node_stride, p.draft_batch_stride, p.draft_node_stride = T * V, V, T * V, V
    p.tokens_draft_batch_stride = p.parents_batch_stride = T
    p.workspace_bytes = 24 * max(B, 0) * 2 * max(T, 0)
    for k, v in fields.items():
        setattr(p, k, v)
    return p


CASES = [
    ("bf16_u", _p(), OK),
    ("fp16", _p(logits_dtype=FP16), OK),
    ("fp32", _p(logits_dtype=FP32), OK),
    ("int32_tokens", _p(tokens_dtype=_lib.FA_TREE_TOKENS_INT32), OK),
    ("rng_state", _p(u_acc=0, u_res=0, rng_state=ADDR), OK),
    ("one_hot", _p(logits_draft=0), OK),
    ("stats", _p(p_tok=ADDR, q_tok=ADDR, visited=ADDR, accepted=ADDR), OK),
    ("no_sequences", _p(B=0), OK),
    ("no_sequences_no_workspace", _p(B=0, workspace=0), OK),
    ("one_node", _p(T=1), OK),
    ("one_node_no_u_acc", _p(T=1, u_acc=0), OK),
    ("64_nodes", _p(T=64), OK),
    ("one_column", _p(V=1), OK),
    ("odd_width_odd_base", _p(V=50257, logits=ADDR + 2), OK),
    ("strides_0", _p(logits_batch_stride=0, draft_node_stride=0, parents_batch_stride=0), OK),
    ("top_k_0", _p(top_k=0), OK),
    ("top_k_1", _p(top_k=1), OK),
    ("top_k_above_v", _p(top_k=5000), OK),
    ("top_p_0", _p(top_p=0.0), OK),
    ("top_p_1", _p(top_p=1.0), OK),
    ("temperature", _p(temperature=0.7), OK),
    ("workspace_larger", _p(workspace_bytes=1 << 20), OK),
    ("abi_version", _p(abi_version=12), BAD_ABI),
    ("struct_size", _p(struct_size=8), BAD_ABI),
    ("logits_fp8", _p(logits_dtype=FP8), BAD_DTYPE),
    ("logits_dtype_unknown", _p(logits_dtype=7), BAD_DTYPE),
    ("tokens_dtype_unknown", _p(tokens_dtype=2), BAD_DTYPE),
    ("v_0", _p(V=0), BAD_SHAPE),
    ("v_negative", _p(V=-8), BAD_SHAPE),  # (what 2^31 and above are in the field)
    ("b_negative", _p(B=-1), BAD_SHAPE),
    ("t_0", _p(T=0), BAD_SHAPE),
    ("t_negative", _p(T=-1), BAD_SHAPE),
    ("t_65", _p(T=65, workspace_bytes=1 << 20), BAD_SHAPE),
    ("too_many_rows", _p(B=1 << 27, T=8, workspace_bytes=1 << 40), BAD_SHAPE),
    ("just_enough_rows", _p(B=(1 << 27) - 1, T=8, workspace_bytes=1 << 40), OK),
    ("temperature_0", _p(temperature=0.0), BAD_SHAPE),
    ("temperature_negative", _p(temperature=-1.0), BAD_SHAPE),
    ("temperature_nan", _p(temperature=float("nan")), BAD_SHAPE),
    ("top_p_negative", _p(top_p=-0.1), BAD_SHAPE),
    ("top_p_above_1", _p(top_p=1.5), BAD_SHAPE),
    ("top_p_nan", _p(top_p=float("nan")), BAD_SHAPE),
    ("top_k_negative", _p(top_k=-1), BAD_SHAPE),
    ("null_logits", _p(logits=0), NULLP),
    ("null_tokens_draft", _p(tokens_draft=0), NULLP),
    ("null_parents", _p(parents=0), NULLP),
    ("null_path", _p(path=0), NULLP),
    ("null_path_len", _p(path_len=0), NULLP),
    ("null_tokens", _p(tokens=0), NULLP),
    ("null_num_generated", _p(num_generated=0), NULLP),
    ("no_uniforms", _p(u_acc=0, u_res=0), NULLP),
    ("u_res_without_u_acc", _p(u_acc=0), NULLP),
    ("u_acc_without_u_res", _p(u_res=0), NULLP),
    ("both_u_and_rng_state", _p(rng_state=ADDR), BAD_SHAPE),
    ("u_acc_and_rng_state", _p(u_res=0, rng_state=ADDR), BAD_SHAPE),
    ("logits_odd_address", _p(logits=ADDR + 1), BAD_STRIDE),
    ("draft_odd_address", _p(logits_draft=ADDR + 1), BAD_STRIDE),
    ("fp32_logits_2_bytes", _p(logits=ADDR + 2, logits_dtype=FP32), BAD_STRIDE),
    ("int64_tokens_4_bytes", _p(tokens_draft=ADDR + 4), BAD_STRIDE),
    ("int64_out_4_bytes", _p(tokens=ADDR + 4), BAD_STRIDE),
    ("parents_2_bytes", _p(parents=ADDR + 2), BAD_STRIDE),
    ("path_2_bytes", _p(path=ADDR + 2), BAD_STRIDE),
    ("path_len_2_bytes", _p(path_len=ADDR + 2), BAD_STRIDE),
    ("u_acc_2_bytes", _p(u_acc=ADDR + 2), BAD_STRIDE),
    ("u_res_2_bytes", _p(u_res=ADDR + 2), BAD_STRIDE),
    ("rng_state_4_bytes", _p(u_acc=0, u_res=0, rng_state=ADDR + 4), BAD_STRIDE),
    ("num_generated_4_bytes", _p(num_generated=ADDR + 4), BAD_STRIDE),
    ("p_tok_2_bytes", _p(p_tok=ADDR + 2), BAD_STRIDE),
    ("visited_2_bytes", _p(visited=ADDR + 2), BAD_STRIDE),
    ("accepted_2_bytes", _p(accepted=ADDR + 2), BAD_STRIDE),
    ("workspace_4_bytes", _p(workspace=ADDR + 4), BAD_STRIDE),
    ("null_workspace", _p(workspace=0), WORKSPACE),
    ("workspace_one_byte_short", _p(workspace_bytes=24 * 5 * 26 - 1), WORKSPACE),
]


@pytest.mark.parametrize("name,p,status", CASES, ids=[r[0] for r in CASES])
def test_tree_sample_validate(name, p, status):
    lib = _lib.load()
    assert lib.fa_tree_sample_validate(p) == status
    if status != OK:  # the launch entry refuses the same way before it launches anything
        assert lib.fa_tree_sample(p, None) == status


def test_tree_sample_null_and_no_sequences():
    """A NULL params is refused; B = 0 returns before any launch: FA_OK without a device."""
    lib = _lib.load()
    assert lib.fa_tree_sample_validate(None) == NULLP and lib.fa_tree_sample(None, None) == NULLP
    assert lib.fa_tree_sample(_p(B=0), None) == OK and lib.fa_tree_sample(_p(B=0, T=1), None) == OK


def test_tree_sample_workspace_size():
    lib = _lib.load()
    assert _lib.FA_TREE_RECORD_BYTES == 24 and _lib.FA_TREE_SAMPLE_MAX_NODES == 64
    for b, t in ((1, 1), (1, 2), (5, 13), (64, 64), (1 << 20, 16)):
        assert lib.fa_tree_sample_workspace_size(b, t) == 24 * b * 2 * t  # a target and a draft record per node
    assert lib.fa_tree_sample_workspace_size(0, 4) == 0 and lib.fa_tree_sample_workspace_size(-1, 4) == 0
    assert lib.fa_tree_sample_workspace_size(4, 0) == 0 and lib.fa_tree_sample_workspace_size(4, -1) == 0


def test_tree_sample_symbols_and_sizes():
    lib = _lib.load()
    header = open(os.path.join(_lib.INCLUDE, "fa_tree_sample.h")).read()
    declared = re.findall(r"^\w[\w ]*?\b(fa_\w+)\(", header, re.M)
    assert sorted(declared) == sorted(SYMBOLS) == sorted(_lib.TREE_SAMPLE_SYMBOLS)
    for name in SYMBOLS:
        assert hasattr(lib, name)
    assert lib.fa_tree_sample_params_size() == ctypes.sizeof(_lib.FaTreeSampleParams) == 232
    assert ctypes.sizeof(_lib.FaTreeSampleForm) == 52
    assert [f[0] for f in _lib.FaTreeSampleParams._fields_[:2]] == ["abi_version", "struct_size"]
    # additive: a header of its own; the ABI version, the other symbol sets and the other sampling units' structs are what they were
    assert lib.fa_abi_version() == 13 == _lib.FA_ABI_VERSION
    for other in (_lib.EXPORTED_SYMBOLS, _lib.ROTARY_EMB_SYMBOLS, _lib.NORM_SYMBOLS, _lib.XENT_SYMBOLS, _lib.ACT_SYMBOLS,
                  _lib.GEMM_ACT_SYMBOLS, _lib.DROPOUT_NORM_SYMBOLS, _lib.SAMPLE_SYMBOLS, _lib.SPEC_SAMPLE_SYMBOLS, _lib.BLOCK_SELECT_SYMBOLS,
                  _lib.BLOCK_PATTERN_SYMBOLS):
        assert not set(SYMBOLS) & set(other)
    for other in os.listdir(_lib.INCLUDE):
        if other != "fa_tree_sample.h":
            assert "fa_tree_sample" not in open(os.path.join(_lib.INCLUDE, other)).read(), other
    assert lib.fa_sample_params_size() == ctypes.sizeof(_lib.FaSampleParams) == 96 and ctypes.sizeof(_lib.FaSampleForm) == 56
    assert lib.fa_spec_sample_params_size() == ctypes.sizeof(_lib.FaSpecSampleParams) == 192 and ctypes.sizeof(_lib.FaSpecSampleForm) == 48


def test_tree_sample_plan_struct_is_the_mirror():
    """fa_tree_sample_plan fills every field of the mirror: a form whose fields are all distinct comes back in order."""
    lib = _lib.load()
    form = _lib.FaTreeSampleForm()
    p = _p(B=30000, T=3, V=4099, logits_dtype=FP16, temperature=0.7, top_k=37, top_p=0.5, workspace_bytes=1 << 30)
    assert lib.fa_tree_sample_plan(p, form) == OK
    got = U.Plan(*(getattr(form, f) for f in U.Plan._fields))
    assert got == U.Plan(cw=1, threads=1024, drafts=1, topk=1, topp=1, k=37, key_bits=32, key_passes=3, index_bits=13, index_passes=2,
                         frac_bits=40, grid_a=65535, grid_b=30000)
    assert [f[0] for f in _lib.FaTreeSampleForm._fields_] == list(U.Plan._fields)
    assert lib.fa_tree_sample_plan(_p(V=0), form) == BAD_SHAPE and lib.fa_tree_sample_plan(_p(), None) == NULLP


def test_tree_sample_device_code():
    """The translation unit holds exactly the kernels of the universe, and none has a private segment: nothing spills, nothing
    is called."""
    from device_asm import kernel_bodies
    found = {}
    for sym, body in kernel_bodies("fa_tree_sample.hip"):
        k = re.match(r"_ZN\d+_GLOBAL__N_1\d+(tree_\w+_kernel)ILi(\d+)EEEv21fa_tree_sample_params19fa_tree_sample_form$", sym)
        assert k, f"a kernel in fa_tree_sample.hip of no known family: {sym}"
        key = (k.group(1), int(k.group(2)))
        assert key not in found, sym
        found[key] = int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body).group(1))
    assert set(found) == U.KERNELS
    assert all(v == 0 for v in found.values()), found
    assert set().union(*(U.kernels_of(U.case_plan(c)) for c in U.CASES)) == U.KERNELS  # the GPU cases run every one of them
