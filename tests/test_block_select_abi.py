"""CPU tests of the C-ABI of the block summaries and the Quest block selection (include/fa_block_select.h) and of the device code
of its translation unit, csrc/fa_block_select.hip: every refusal of the two _validate functions one by one, the plan names of
every form against tests/block_select_plan_universe.py, the struct sizes against the ctypes mirror, the kernels of the unit.
Nothing here touches a device; tests/test_block_select_gpu.py checks what the kernels write."""
import ctypes
import os
import re

import pytest

import block_select_plan_universe as U
from flash_attention_annotated_amd import _lib

ADDR = 0x10000  # an aligned dummy address: nothing is dereferenced
OK, NULLP, BAD_DTYPE, BAD_HEAD_DIM, BAD_HEADS, BAD_SHAPE, BAD_STRIDE, UNSUPPORTED, BAD_ABI = 0, -1, -2, -3, -4, -5, -6, -7, -9
BF16, FP16, FP32, FP8 = _lib.FA_DTYPE_BF16, _lib.FA_DTYPE_FP16, _lib.FA_DTYPE_FP32, _lib.FA_DTYPE_FP8_E4M3
SYMBOLS = ("fa_block_summary_update", "fa_block_summary_update_validate", "fa_block_summary_update_workspace_size",
           "fa_block_summary_update_plan_name", "fa_block_summary_params_size", "fa_block_select", "fa_block_select_validate",
           "fa_block_select_workspace_size", "fa_block_select_plan_name", "fa_block_select_params_size")


def _s(b=3, h_k=2, d=128, capacity=512, max_blocks=4, block=128, page=0, **fields):
    """A contiguous bf16 summary over a dense bf16 cache (page: a paged one of that page size)."""
    p = _lib.new_block_summary_params()
    for name in ("k_summary", "k_cache", "seqlens_old", "seqlens_new"):
        setattr(p, name, ADDR)
    p.b, p.h_k, p.d, p.capacity, p.max_blocks, p.block_size, p.max_seqlen_new = b, h_k, d, capacity, max_blocks, block, capacity
    p.sum_head_stride, p.sum_side_stride = d, h_k * d
    p.sum_block_stride, p.sum_slot_stride = 2 * h_k * d, max_blocks * 2 * h_k * d
    p.cache_head_stride, p.cache_row_stride = d, h_k * d
    p.cache_batch_stride = (page or capacity) * h_k * d
    if page:
        p.page_table, p.page_size, p.page_table_batch_stride = ADDR, page, capacity // page
    for k, v in fields.items():
        setattr(p, k, v)
    return p


def _q(b=3, s_q=1, h=8, h_k=2, d=128, max_blocks=64, num_blocks=8, width=None, **fields):
    """Contiguous bf16 queries and summary, contiguous outputs: sink 1, local 1, "max"."""
    p = _lib.new_block_select_params()
    for name in ("q", "k_summary", "cache_seqlens", "scores", "block_cnt", "block_idx"):
        setattr(p, name, ADDR)
    width = num_blocks if width is None else width
    p.b, p.s_q, p.h, p.h_k, p.d, p.max_blocks, p.num_blocks, p.list_width = b, s_q, h, h_k, d, max_blocks, num_blocks, width
    p.q_head_stride, p.q_row_stride, p.q_batch_stride = d, h * d, s_q * h * d
    p.sum_head_stride, p.sum_side_stride = d, h_k * d
    p.sum_block_stride, p.sum_slot_stride = 2 * h_k * d, max_blocks * 2 * h_k * d
    p.scores_head_stride, p.scores_batch_stride = max_blocks, h_k * max_blocks
    p.cnt_head_stride, p.cnt_batch_stride, p.idx_head_stride, p.idx_batch_stride = 1, h_k, width, h_k * width
    for k, v in fields.items():
        setattr(p, k, v)
    return p


SUMMARY_CASES = [
    ("bf16_dense", _s(), OK),
    ("fp16", _s(summary_dtype=FP16, cache_dtype=FP16), OK),
    ("e4m3_cache", _s(cache_dtype=FP8), OK),
    ("e4m3_cache_8_bytes", _s(cache_dtype=FP8, k_cache=ADDR + 8), OK),
    ("rebuild", _s(seqlens_old=0), OK),
    ("cache_batch_idx", _s(cache_batch_idx=ADDR), OK),
    ("paged_16", _s(page=16), OK),
    ("paged_256_block_64", _s(page=256, block=64, max_blocks=8), OK),
    ("max_blocks_larger", _s(max_blocks=9), OK),
    ("d_16", _s(d=16), OK),
    ("no_entries", _s(b=0), OK),
    ("max_seqlen_new_1", _s(max_seqlen_new=1), OK),
    ("abi_version", _s(abi_version=12), BAD_ABI),
    ("struct_size", _s(struct_size=8), BAD_ABI),
    ("summary_fp32", _s(summary_dtype=FP32, cache_dtype=FP32), BAD_DTYPE),
    ("summary_e4m3", _s(summary_dtype=FP8, cache_dtype=FP8), BAD_DTYPE),
    ("cache_of_the_other_16_bit_type", _s(cache_dtype=FP16), BAD_DTYPE),
    ("d_136", _s(d=136), BAD_HEAD_DIM),
    ("d_72", _s(d=72), BAD_HEAD_DIM),
    ("d_0", _s(d=0), BAD_HEAD_DIM),
    ("leftpad", _s(cache_leftpad=ADDR), UNSUPPORTED),
    ("ragged_new_rows", _s(cu_seqlens_k_new=ADDR), UNSUPPORTED),
    ("block_96", _s(block=96, max_blocks=6), BAD_SHAPE),
    ("block_0", _s(block=0), BAD_SHAPE),
    ("max_blocks_too_small_for_the_capacity", _s(max_blocks=3), BAD_SHAPE),
    ("b_negative", _s(b=-1), BAD_SHAPE),
    ("h_k_0", _s(h_k=0), BAD_SHAPE),
    ("max_seqlen_new_negative", _s(max_seqlen_new=-1), BAD_SHAPE),
    ("page_size_0", _s(page=16, page_size=0), BAD_SHAPE),
    ("capacity_no_multiple_of_the_page", _s(page=16, capacity=500), BAD_SHAPE),
    ("paged_with_cache_batch_idx", _s(page=16, cache_batch_idx=ADDR), BAD_SHAPE),
    ("null_summary", _s(k_summary=0), NULLP),
    ("null_cache", _s(k_cache=0), NULLP),
    ("null_seqlens_new", _s(seqlens_new=0), NULLP),
    ("summary_8_bytes", _s(k_summary=ADDR + 8), BAD_STRIDE),
    ("cache_8_bytes", _s(k_cache=ADDR + 8), BAD_STRIDE),
    ("e4m3_cache_4_bytes", _s(cache_dtype=FP8, k_cache=ADDR + 4), BAD_STRIDE),
    ("seqlens_2_bytes", _s(seqlens_new=ADDR + 2), BAD_STRIDE),
    ("summary_block_stride", _s(sum_block_stride=2 * 2 * 128 + 4), BAD_STRIDE),
    ("cache_row_stride", _s(cache_row_stride=2 * 128 + 2), BAD_STRIDE),
]

SELECT_CASES = [
    ("bf16", _q(), OK),
    ("fp16", _q(dtype=FP16), OK),
    ("cache_batch_idx", _q(cache_batch_idx=ADDR), OK),
    ("sum", _q(group_reduce=_lib.FA_BLOCK_REDUCE_SUM), OK),
    ("128_rows", _q(s_q=32), OK),
    ("8192_blocks", _q(max_blocks=8192), OK),
    ("wider_list", _q(width=64), OK),
    ("forced_only", _q(num_blocks=2), OK),
    ("nothing_forced", _q(num_blocks=0, sink_blocks=0, local_blocks=0), OK),
    ("block_64", _q(block_size=64), OK),
    ("no_entries", _q(b=0), OK),
    ("abi_version", _q(abi_version=12), BAD_ABI),
    ("struct_size", _q(struct_size=8), BAD_ABI),
    ("fp32", _q(dtype=FP32), BAD_DTYPE),
    ("e4m3", _q(dtype=FP8), BAD_DTYPE),
    ("d_136", _q(d=136), BAD_HEAD_DIM),
    ("d_24", _q(d=24), BAD_HEAD_DIM),
    ("heads", _q(h=7), BAD_HEADS),
    ("h_k_0", _q(h_k=0), BAD_HEADS),
    ("ragged_q", _q(cu_seqlens_q=ADDR), UNSUPPORTED),
    ("leftpad", _q(cache_leftpad=ADDR), UNSUPPORTED),
    ("group_reduce_unknown", _q(group_reduce=2), UNSUPPORTED),
    ("block_96", _q(block_size=96), BAD_SHAPE),
    ("129_rows", _q(s_q=33), BAD_SHAPE),
    ("s_q_0", _q(s_q=0), BAD_SHAPE),
    ("8193_blocks", _q(max_blocks=8193), BAD_SHAPE),
    ("max_blocks_0", _q(max_blocks=0), BAD_SHAPE),
    ("list_narrower_than_num_blocks", _q(width=7), BAD_SHAPE),
    ("num_blocks_below_sink_plus_local", _q(num_blocks=4, sink_blocks=2, local_blocks=3), BAD_SHAPE),
    ("sink_negative", _q(sink_blocks=-1), BAD_SHAPE),
    ("b_negative", _q(b=-1), BAD_SHAPE),
    ("null_q", _q(q=0), NULLP),
    ("null_summary", _q(k_summary=0), NULLP),
    ("null_cache_seqlens", _q(cache_seqlens=0), NULLP),
    ("null_scores", _q(scores=0), NULLP),
    ("null_block_cnt", _q(block_cnt=0), NULLP),
    ("null_block_idx", _q(block_idx=0), NULLP),
    ("q_8_bytes", _q(q=ADDR + 8), BAD_STRIDE),
    ("summary_8_bytes", _q(k_summary=ADDR + 8), BAD_STRIDE),
    ("scores_2_bytes", _q(scores=ADDR + 2), BAD_STRIDE),
    ("q_row_stride", _q(q_row_stride=8 * 128 + 4), BAD_STRIDE),
]


@pytest.mark.parametrize("name,p,status", SUMMARY_CASES, ids=[r[0] for r in SUMMARY_CASES])
def test_block_summary_update_validate(name, p, status):
    lib = _lib.load()
    assert lib.fa_block_summary_update_validate(p) == status
    if status != OK:  # the launch entry refuses the same way before it launches anything; so do the size and the name
        assert lib.fa_block_summary_update(p, None) == status
        assert lib.fa_block_summary_update_workspace_size(p) == status and lib.fa_block_summary_update_plan_name(p) is None
    else:
        assert lib.fa_block_summary_update_workspace_size(p) == 0


@pytest.mark.parametrize("name,p,status", SELECT_CASES, ids=[r[0] for r in SELECT_CASES])
def test_block_select_validate(name, p, status):
    lib = _lib.load()
    assert lib.fa_block_select_validate(p) == status
    if status != OK:
        assert lib.fa_block_select(p, None) == status
        assert lib.fa_block_select_workspace_size(p) == status and lib.fa_block_select_plan_name(p) is None
    else:
        assert lib.fa_block_select_workspace_size(p) == 4 * p.b * p.h_k * p.max_blocks


def test_null_and_no_entries():
    """A NULL params is refused; b = 0 returns before any launch: FA_OK without a device."""
    lib = _lib.load()
    assert lib.fa_block_summary_update_validate(None) == NULLP and lib.fa_block_summary_update(None, None) == NULLP
    assert lib.fa_block_select_validate(None) == NULLP and lib.fa_block_select(None, None) == NULLP
    assert lib.fa_block_summary_update(_s(b=0), None) == OK and lib.fa_block_select(_q(b=0), None) == OK


def test_symbols_and_sizes():
    lib = _lib.load()
    header = open(os.path.join(_lib.INCLUDE, "fa_block_select.h")).read()
    declared = re.findall(r"^\w[\w *]*?\b(fa_\w+)\(", header, re.M)
    assert sorted(declared) == sorted(SYMBOLS) == sorted(_lib.BLOCK_SELECT_SYMBOLS)
    for name in SYMBOLS:
        assert hasattr(lib, name)
    assert lib.fa_block_summary_params_size() == ctypes.sizeof(_lib.FaBlockSummaryParams) == 176
    assert lib.fa_block_select_params_size() == ctypes.sizeof(_lib.FaBlockSelectParams) == 240
    for struct in (_lib.FaBlockSummaryParams, _lib.FaBlockSelectParams):
        assert [f[0] for f in struct._fields_[:2]] == ["abi_version", "struct_size"]
    assert (_lib.FA_BLOCK_SELECT_MAX_BLOCKS, _lib.FA_BLOCK_SELECT_MAX_ROWS) == (U.MAX_BLOCKS, U.MAX_ROWS) == (8192, 128)
    # additive: a header of its own; the ABI version, the other symbol sets and the sparse read's struct are what they were
    assert lib.fa_abi_version() == 13 == _lib.FA_ABI_VERSION
    for other in (_lib.EXPORTED_SYMBOLS, _lib.ROTARY_EMB_SYMBOLS, _lib.NORM_SYMBOLS, _lib.XENT_SYMBOLS, _lib.ACT_SYMBOLS,
                  _lib.GEMM_ACT_SYMBOLS, _lib.DROPOUT_NORM_SYMBOLS, _lib.SAMPLE_SYMBOLS, _lib.SPEC_SAMPLE_SYMBOLS):
        assert not set(SYMBOLS) & set(other)
    for other in os.listdir(_lib.INCLUDE):
        if other != "fa_block_select.h":
            text = open(os.path.join(_lib.INCLUDE, other)).read()
            assert "fa_block_select" not in text and "fa_block_summary" not in text, other
    assert lib.fa_sparse_kv_params_size() == ctypes.sizeof(_lib.FaSparseKvParams) == 72
    assert lib.fa_fwd_params_size() == ctypes.sizeof(_lib.FaFwdParams) == 464


@pytest.mark.parametrize("form", sorted(U.UPDATE_FORMS), ids=str)
def test_update_plan_name_of_every_form(form):
    lib = _lib.load()
    L, cache, side = form
    d, fp8, paged = 128 if L == 16 else 64, cache == "e4m3", side == "paged"
    assert U.update_form(d, fp8, paged) == form
    for b, h_k, block, max_blocks, bound in ((3, 2, 128, 4, 512), (1, 1, 64, 9, 1), (6, 2, 64, 8, 64), (6, 2, 128, 4, 129), (2, 1, 128, 4, 0)):
        p = _s(b=b, h_k=h_k, d=d, block=block, max_blocks=max_blocks, page=64 if paged else 0, max_seqlen_new=bound,
               cache_dtype=FP8 if fp8 else BF16)
        assert lib.fa_block_summary_update_plan_name(p).decode() == U.update_plan(b, h_k, d, max_blocks, block, bound, fp8, paged)


@pytest.mark.parametrize("form", sorted(U.SELECT_FORMS), ids=str)
def test_select_plan_name_of_every_form(form):
    lib = _lib.load()
    L, reduce, threads = form
    d = 128 if L == 16 else 64
    sizes = (1, 40, 1024) if threads == U.SMALL_THREADS else (1025, 4096, 8192)  # both sides of the workgroup's boundary
    for max_blocks in sizes:
        assert U.select_form(d, max_blocks, reduce) == form
        for b, h_k in ((1, 1), (5, 2)):
            p = _q(b=b, h=4 * h_k, h_k=h_k, d=d, max_blocks=max_blocks, group_reduce=("max", "sum").index(reduce))
            assert lib.fa_block_select_plan_name(p).decode() == U.select_plan(b, h_k, d, max_blocks, reduce)
    # the lanes' boundary: d 64 has 8 lanes per row, d 80 has 16; the scoring is split from 1 block on
    assert U.lanes(64) == 8 and U.lanes(80) == 16 and U.lanes(16) == 8
    p = _q(b=1, h=8, h_k=8, d=128, max_blocks=8192)
    assert "split=128 grid=(128,8,1)" in lib.fa_block_select_plan_name(p).decode()  # batch 1: 1024 workgroups score


def test_the_gpu_cases_run_every_form():
    got = {U.update_form(c.d, c.cache == "e4m3", c.form != "dense") for c in U.SUMMARY_CASES}
    assert got == U.UPDATE_FORMS
    got = {U.select_form(c.d, c.max_blocks, c.reduce) for c in U.SELECT_CASES + U.LARGE_CASES}
    assert got == U.SELECT_FORMS
    assert {U.lanes(d) for d in (64, 128)} == {lanes for _, lanes in U.KERNELS if lanes}


def test_device_code():
    """The translation unit holds exactly the kernels of the universe, and none has a private segment: nothing spills, nothing
    is called."""
    from device_asm import kernel_bodies
    found = {}
    for sym, body in kernel_bodies("fa_block_select.hip"):
        k = re.match(r"_ZN\d+_GLOBAL__N_1\d+(summary_update_kernel|block_score_kernel)ILi(\d+)EEEv\d+fa_block_(?:summary|select)_params$", sym)
        plain = re.match(r"_ZN\d+_GLOBAL__N_1\d+(block_select_kernel)E\d+fa_block_select_params$", sym)
        assert k or plain, f"a kernel in fa_block_select.hip of no known family: {sym}"
        key = (k.group(1), int(k.group(2))) if k else (plain.group(1), None)
        assert key not in found, sym
        found[key] = int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body).group(1))
    assert set(found) == U.KERNELS
    assert all(v == 0 for v in found.values()), found
