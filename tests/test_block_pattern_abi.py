"""CPU tests of the C-ABI of the block-sparse prefill pattern (include/fa_block_pattern.h) and of the device code of its
translation unit, csrc/fa_block_pattern.hip: every refusal of _validate one by one, the plan name and the workspace size of every
form against tests/block_pattern_plan_universe.py, the struct size against the ctypes mirror, the kernels of the unit.  Nothing
here touches a device; tests/test_block_pattern_gpu.py checks what the kernels write."""
import ctypes
import os
import re

import pytest

import block_pattern_plan_universe as U
from flash_attention_annotated_amd import _lib

ADDR = 0x10000  # an aligned dummy address: nothing is dereferenced
OK, NULLP, BAD_DTYPE, BAD_HEAD_DIM, BAD_HEADS, BAD_SHAPE, BAD_STRIDE, BAD_ABI, WORKSPACE = 0, -1, -2, -3, -4, -5, -6, -9, -11
BF16, FP16, FP32, FP8 = _lib.FA_DTYPE_BF16, _lib.FA_DTYPE_FP16, _lib.FA_DTYPE_FP32, _lib.FA_DTYPE_FP8_E4M3
SYMBOLS = ("fa_block_pattern", "fa_block_pattern_validate", "fa_block_pattern_workspace_size", "fa_block_pattern_plan_name",
           "fa_block_pattern_params_size")
LISTS = ("full_block_cnt", "full_block_idx", "mask_block_cnt", "mask_block_idx")


def _p(b=2, sq=300, sk=700, h=4, h_k=2, d=128, num_blocks=3, bwd=False, want_scores=False, **fields):
    """Contiguous bf16 q and k, every output given, a workspace of the right size: sink 1, local 1, no mask."""
    p = _lib.new_block_pattern_params()
    for name in ("q", "k", "workspace") + LISTS + (("q_block_cnt", "q_block_idx") if bwd else ()) + (("scores",) if want_scores else ()):
        setattr(p, name, ADDR)
    p.b, p.sq, p.sk, p.h, p.h_k, p.d, p.num_blocks = b, sq, sk, h, h_k, d, num_blocks
    p.q_head_stride, p.q_row_stride, p.q_batch_stride = d, h * d, sq * h * d
    p.k_head_stride, p.k_row_stride, p.k_batch_stride = d, h_k * d, sk * h_k * d
    p.workspace_bytes = U.workspace_size(b, sq, sk, h, h_k, d, bwd)
    for k, v in fields.items():
        setattr(p, k, v)
    return p


CASES = [
    ("bf16", _p(), OK),
    ("fp16", _p(dtype=FP16), OK),
    ("key_major_lists", _p(bwd=True), OK),
    ("scores", _p(want_scores=True), OK),
    ("causal", _p(is_causal=1), OK),
    ("window", _p(window_size_left=256, window_size_right=0), OK),
    ("d_16", _p(d=16), OK),
    ("mqa", _p(h_k=1), OK),
    ("8192_blocks", _p(sk=8192 * 128), OK),
    ("one_row_one_key", _p(sq=1, sk=1), OK),
    ("forced_only", _p(num_blocks=2), OK),
    ("nothing_forced", _p(num_blocks=0, sink_blocks=0, local_blocks=0), OK),
    ("more_places_than_blocks", _p(num_blocks=0x7fffffff), OK),
    ("no_entries", _p(b=0, workspace=0, workspace_bytes=0), OK),
    ("q_2_bytes", _p(q=ADDR + 2), OK),  # (the element loads)
    ("k_row_stride_odd", _p(k_row_stride=2 * 128 + 1), OK),
    ("larger_workspace", _p(workspace_bytes=1 << 30), OK),
    ("abi_version", _p(abi_version=12), BAD_ABI),
    ("struct_size", _p(struct_size=8), BAD_ABI),
    ("fp32", _p(dtype=FP32), BAD_DTYPE),
    ("e4m3", _p(dtype=FP8), BAD_DTYPE),
    ("d_136", _p(d=136), BAD_HEAD_DIM),
    ("d_24", _p(d=24), BAD_HEAD_DIM),
    ("d_0", _p(d=0), BAD_HEAD_DIM),
    ("heads", _p(h=5), BAD_HEADS),
    ("h_k_0", _p(h_k=0), BAD_HEADS),
    ("8193_blocks", _p(sk=8192 * 128 + 1), BAD_SHAPE),
    ("sq_0", _p(sq=0), BAD_SHAPE),
    ("sk_0", _p(sk=0), BAD_SHAPE),
    ("b_negative", _p(b=-1), BAD_SHAPE),
    ("num_blocks_below_sink_plus_local", _p(num_blocks=4, sink_blocks=2, local_blocks=3), BAD_SHAPE),
    ("num_blocks_1", _p(num_blocks=1), BAD_SHAPE),
    ("sink_negative", _p(sink_blocks=-1), BAD_SHAPE),
    ("local_negative", _p(local_blocks=-1), BAD_SHAPE),
    ("null_q", _p(q=0), NULLP),
    ("null_k", _p(k=0), NULLP),
] + [(f"null_{name}", _p(**{name: 0}), NULLP) for name in LISTS] + [
    ("q_block_cnt_alone", _p(q_block_cnt=ADDR), NULLP),
    ("q_block_idx_alone", _p(q_block_idx=ADDR), NULLP),
    ("q_odd_address", _p(q=ADDR + 1), BAD_STRIDE),
    ("k_odd_address", _p(k=ADDR + 1), BAD_STRIDE),
    ("list_2_bytes", _p(mask_block_idx=ADDR + 2), BAD_STRIDE),
    ("scores_2_bytes", _p(scores=ADDR + 2), BAD_STRIDE),
    ("workspace_8_bytes", _p(workspace=ADDR + 8), BAD_STRIDE),
    ("null_workspace", _p(workspace=0), WORKSPACE),
    ("workspace_too_small", _p(workspace_bytes=U.workspace_size(2, 300, 700, 4, 2, 128, False) - 1), WORKSPACE),
    ("workspace_without_the_bitmap", _p(bwd=True, workspace_bytes=U.workspace_size(2, 300, 700, 4, 2, 128, False)), WORKSPACE),
]


@pytest.mark.parametrize("name,p,status", CASES, ids=[r[0] for r in CASES])
def test_validate(name, p, status):
    lib = _lib.load()
    assert lib.fa_block_pattern_validate(p) == status
    if status != OK:  # the launch entry refuses the same way before it launches anything
        assert lib.fa_block_pattern(p, None) == status
    if status in (OK, WORKSPACE) or name == "workspace_8_bytes":  # the size and the name do not look at the workspace
        bwd = bool(p.q_block_cnt)
        assert lib.fa_block_pattern_workspace_size(p) == U.workspace_size(p.b, p.sq, p.sk, p.h, p.h_k, p.d, bwd)
        assert lib.fa_block_pattern_plan_name(p) is not None
    else:
        assert lib.fa_block_pattern_workspace_size(p) == status and lib.fa_block_pattern_plan_name(p) is None


def test_null_and_no_entries():
    """A NULL params is refused; b = 0 returns before any launch: FA_OK without a device."""
    lib = _lib.load()
    assert lib.fa_block_pattern_validate(None) == NULLP and lib.fa_block_pattern(None, None) == NULLP
    assert lib.fa_block_pattern_workspace_size(None) == NULLP and lib.fa_block_pattern_plan_name(None) is None
    assert lib.fa_block_pattern(_p(b=0), None) == OK


def test_symbols_and_sizes():
    lib = _lib.load()
    header = open(os.path.join(_lib.INCLUDE, "fa_block_pattern.h")).read()
    declared = re.findall(r"^\w[\w *]*?\b(fa_\w+)\(", header, re.M)
    assert sorted(declared) == sorted(SYMBOLS) == sorted(_lib.BLOCK_PATTERN_SYMBOLS)
    for name in SYMBOLS:
        assert hasattr(lib, name)
    assert lib.fa_block_pattern_params_size() == ctypes.sizeof(_lib.FaBlockPatternParams) == 200
    assert [f[0] for f in _lib.FaBlockPatternParams._fields_[:2]] == ["abi_version", "struct_size"]
    assert (_lib.FA_BLOCK_PATTERN_BLOCK, _lib.FA_BLOCK_PATTERN_MAX_BLOCKS) == (U.BLOCK, U.MAX_BLOCKS) == (128, 8192)
    # additive: a header of its own; the ABI version, the other symbol sets and the structs of the readers are what they were
    assert lib.fa_abi_version() == 13 == _lib.FA_ABI_VERSION
    for other in (_lib.EXPORTED_SYMBOLS, _lib.ROTARY_EMB_SYMBOLS, _lib.NORM_SYMBOLS, _lib.XENT_SYMBOLS, _lib.ACT_SYMBOLS,
                  _lib.GEMM_ACT_SYMBOLS, _lib.DROPOUT_NORM_SYMBOLS, _lib.SAMPLE_SYMBOLS, _lib.SPEC_SAMPLE_SYMBOLS, _lib.BLOCK_SELECT_SYMBOLS):
        assert not set(SYMBOLS) & set(other)
    for other in os.listdir(_lib.INCLUDE):
        if other != "fa_block_pattern.h":
            assert "fa_block_pattern" not in open(os.path.join(_lib.INCLUDE, other)).read(), other
    assert lib.fa_block_sparse_params_size() == ctypes.sizeof(_lib.FaBlockSparseParams) == 176
    assert lib.fa_block_sparse_bwd_params_size() == ctypes.sizeof(_lib.FaBlockSparseBwdParams) == 96
    assert lib.fa_fwd_params_size() == ctypes.sizeof(_lib.FaFwdParams) == 464


@pytest.mark.parametrize("form", sorted(U.FORMS), ids=str)
def test_plan_name_and_workspace_of_every_form(form):
    lib = _lib.load()
    pool, threads, transpose = form
    vec = pool == "16B"
    sks = (1, 700, 1024 * 128) if threads == U.SMALL_THREADS else (1024 * 128 + 1, 8192 * 128)  # both sides of the boundary
    for sk in sks:
        assert U.form(vec, sk, transpose) == form
        for b, sq, h, h_k, d in ((1, 1, 1, 1, 16), (2, 300, 4, 2, 64), (3, 1000, 8, 8, 80), (2, 129, 6, 2, 128)):
            for odd in (() if vec else ("q", "k_row_stride", "q_head_stride")):
                p = _p(b=b, sq=sq, sk=sk, h=h, h_k=h_k, d=d, bwd=transpose)
                setattr(p, odd, getattr(p, odd) + (2 if odd == "q" else 4))
                assert lib.fa_block_pattern_plan_name(p).decode() == U.plan(b, sq, sk, h, h_k, d, False, transpose)
            if vec:
                p = _p(b=b, sq=sq, sk=sk, h=h, h_k=h_k, d=d, bwd=transpose, q_row_stride=3 * h * d, k_batch_stride=8 * sk * h_k * d)
                assert lib.fa_block_pattern_plan_name(p).decode() == U.plan(b, sq, sk, h, h_k, d, True, transpose)
            assert lib.fa_block_pattern_workspace_size(p) == U.workspace_size(b, sq, sk, h, h_k, d, transpose)
    assert "L=8" in U.plan(1, 1, 1, 1, 1, 64, True, False) and "L=16" in U.plan(1, 1, 1, 1, 1, 80, True, False)


def test_the_gpu_cases_run_every_form():
    assert {U.case_form(c) for c in U.GPU_CASES} == U.FORMS
    assert {c.d for c in U.GPU_CASES} >= {16, 64, 128} and {c.dtype for c in U.GPU_CASES} == {"bf16", "fp16"}


def test_device_code():
    """The translation unit holds exactly the kernels of the universe, and none has a private segment: nothing spills, nothing
    is called."""
    from device_asm import kernel_bodies
    found = {}
    for sym, body in kernel_bodies("fa_block_pattern.hip"):
        k = re.match(r"_ZN\d+_GLOBAL__N_1\d+(pool_kernel)I(Lb[01])EEEv\d+fa_block_pattern_params", sym)
        plain = re.match(r"_ZN\d+_GLOBAL__N_1\d+(pattern_kernel|transpose_kernel)E\d+fa_block_pattern_params", sym)
        assert k or plain, f"a kernel in fa_block_pattern.hip of no known family: {sym}"
        key = (k.group(1), k.group(2)) if k else (plain.group(1), None)
        assert key not in found, sym
        found[key] = int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body).group(1))
    assert set(found) == U.KERNELS
    assert all(v == 0 for v in found.values()), found
