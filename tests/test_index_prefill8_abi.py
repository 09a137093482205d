"""CPU tests of the C-ABI of the prefill-sized lightning indexer over an e4m3 index-key cache (include/fa_index_prefill8.h): the
refusals of _validate one by one, the struct size against the ctypes mirrors, the declared names, the plan texts, and the CPU route
of kvcache_index_topk_prefill(k_index_scale=).  No device is touched."""
import ctypes
import os
import re

import pytest
import torch

from flash_attention_annotated_amd import _lib, hopper_interface as H

ADDR = 0x10000  # an aligned dummy address: nothing is dereferenced
OK, NULLP, BAD_DTYPE, BAD_HEAD_DIM, BAD_HEADS, BAD_SHAPE, BAD_STRIDE, UNSUPPORTED, BAD_ABI = 0, -1, -2, -3, -4, -5, -6, -7, -9
BF16, FP16, FP32 = _lib.FA_DTYPE_BF16, _lib.FA_DTYPE_FP16, _lib.FA_DTYPE_FP32
BLOCK, TILE = _lib.FA_INDEX_PREFILL_BLOCK, _lib.FA_INDEX_PREFILL8_TILE


def _p(b=3, s_q=4096, h_i=64, d_i=128, capacity=8192, topk=2048, page=0, rows=BLOCK, **fields):
    p = _lib.new_index_prefill8_params()
    for name in ("q_index", "k_index_cache", "k_index_scale", "weights", "cache_seqlens", "workspace", "indices"):
        setattr(p, name, ADDR)
    p.b, p.s_q, p.h_i, p.d_i, p.capacity, p.topk, p.list_width = b, s_q, h_i, d_i, capacity, topk, topk
    p.workspace_rows, p.workspace_width, p.workspace_row_stride = rows, capacity, capacity
    p.q_head_stride, p.q_row_stride, p.q_batch_stride = d_i, h_i * d_i, s_q * h_i * d_i
    p.cache_row_stride, p.cache_batch_stride, p.scale_batch_stride = d_i, (page or capacity) * d_i, page or capacity
    p.w_row_stride, p.w_batch_stride, p.idx_row_stride, p.idx_batch_stride = h_i, s_q * h_i, topk, s_q * topk
    if page:
        p.page_table, p.page_size, p.page_table_batch_stride = ADDR, page, capacity // page
    for k, v in fields.items():
        setattr(p, k, v)
    return p


CASES = [
    ("bf16_dense", _p(), OK),
    ("fp16_d64_h16", _p(dtype=FP16, d_i=64, h_i=16), OK),
    *[(f"s_q_{n}", _p(s_q=n), OK) for n in (1, 17, 70000)],
    ("h48_not_causal", _p(h_i=48, is_causal=0), OK),
    ("paged_48", _p(page=48, capacity=48 * 100), OK),
    ("131072_keys_wider_buffers", _p(capacity=131072, list_width=4096, workspace_width=140000, workspace_row_stride=140000), OK),
    ("padded_rows_and_one_scale_row", _p(cache_row_stride=128 + 16, scale_batch_stride=0), OK),
    ("no_entries", _p(b=0), OK),
    ("abi_version", _p(abi_version=12), BAD_ABI),
    ("struct_size_of_the_16_bit_struct", _p(struct_size=232), BAD_ABI),
    ("fp32_queries", _p(dtype=FP32), BAD_DTYPE),
    ("16_bit_cache", _p(cache_dtype=BF16), UNSUPPORTED),
    ("d_96", _p(d_i=96), BAD_HEAD_DIM),
    *[(f"h_{h}", _p(h_i=h), BAD_HEADS) for h in (8, 40, 80)],
    *[(n, _p(**{n: ADDR}), UNSUPPORTED) for n in ("cu_seqlens_q", "cache_leftpad")],
    ("s_q_0", _p(s_q=0), BAD_SHAPE),
    ("topk_0", _p(topk=0), BAD_SHAPE),
    ("workspace_narrower_than_the_capacity", _p(workspace_width=8191), BAD_SHAPE),
    ("workspace_below_a_block", _p(rows=BLOCK - 1), BAD_SHAPE),
    ("capacity_no_multiple_of_the_page", _p(page=48), BAD_SHAPE),
    ("paged_with_cache_batch_idx", _p(page=64, cache_batch_idx=ADDR), BAD_SHAPE),
    *[(f"null_{n}", _p(**{n: 0}), NULLP)
      for n in ("q_index", "k_index_cache", "k_index_scale", "weights", "cache_seqlens", "workspace", "indices")],
    *[(f"{n}_8_bytes", _p(**{n: ADDR + 8}), BAD_STRIDE) for n in ("q_index", "k_index_cache")],
    *[(f"{n}_2_bytes", _p(**{n: ADDR + 2}), BAD_STRIDE) for n in ("k_index_scale", "weights", "workspace", "indices")],
    ("q_head_stride", _p(q_head_stride=128 + 4), BAD_STRIDE),
    ("cache_row_stride_8_bytes", _p(cache_row_stride=128 + 8), BAD_STRIDE),
    ("cache_batch_stride_8_bytes", _p(cache_batch_stride=8192 * 128 + 8), BAD_STRIDE),
    ("scale_stride_negative", _p(scale_batch_stride=-8192), BAD_STRIDE),
]


@pytest.mark.parametrize("name,p,status", CASES, ids=[r[0] for r in CASES])
def test_index_prefill8_validate(name, p, status):
    lib = _lib.load()
    assert lib.fa_index_prefill8_validate(p) == status
    # the launch entry refuses the same way before it launches anything; so does the name
    assert status == OK or (lib.fa_index_prefill8(p, None) == status and lib.fa_index_prefill8_plan_name(p) is None)


def test_symbols_sizes_and_plan_texts():
    lib = _lib.load()
    header = open(os.path.join(_lib.INCLUDE, "fa_index_prefill8.h")).read()
    declared = re.findall(r"^\w[\w *]*?\b(fa_\w+)\(", header, re.M)
    assert sorted(declared) == sorted(_lib.INDEX_PREFILL8_SYMBOLS) and all(hasattr(lib, name) for name in declared)
    assert not set(declared) & (set(_lib.INDEX_TOPK_SYMBOLS) | set(_lib.INDEX_PREFILL_SYMBOLS) | set(_lib.INDEX_TOPK8_SYMBOLS))
    # the struct is the 16-bit one's fields, the scale pointer and its batch stride
    assert lib.fa_index_prefill8_params_size() == ctypes.sizeof(_lib.FaIndexPrefill8Params) == ctypes.sizeof(_lib.FaIndexPrefillParams) + 16 == 248
    assert [f for f in _lib.FaIndexPrefill8Params._fields_ if f[0] not in ("k_index_scale", "scale_batch_stride")] == _lib.FaIndexPrefillParams._fields_
    assert TILE == int(re.search(r"#define FA_INDEX_PREFILL8_TILE (\d+)", header).group(1))
    assert lib.fa_index_prefill8_validate(None) == NULLP and lib.fa_index_prefill8(_p(b=0), None) == OK  # b = 0: no launch, no device
    assert lib.fa_index_prefill8_workspace_size(_p(workspace=0, rows=0, workspace_width=0), 1) == 4 * 8192 * 3 * 4096
    # one prompt of 4096 tokens over 32768 keys in one round: 512 blocks, the chunk grows to 4096 keys (8 chunks)
    assert lib.fa_index_prefill8_plan_name(_p(b=1, capacity=32768, rows=4096)).decode() == \
        f"index_logits_prefill8_kernel d=128 heads=64 sq=4096 block=8 tile={TILE} chunk=4096 grid=4096 | index_select_prefill_kernel " \
        "threads=1024 passes=4 grid=4096 | rounds=1"
    # 3 x 17 tokens on the least workspace: 9 blocks, a round each; the chunk does not depend on the rows
    assert lib.fa_index_prefill8_plan_name(_p(s_q=17, h_i=16, d_i=64, capacity=768, topk=64, dtype=FP16)).decode() == \
        f"index_logits_prefill8_kernel d=64 heads=16 sq=17 block=8 tile={TILE} chunk=256 grid=3 | index_select_prefill_kernel threads=256 " \
        "passes=4 grid=8 | rounds=9"


def test_cpu_route_is_the_rule_on_the_dequantised_keys():
    """s_q 18: bytes -4 .. 4 with a scale of 1/8, 1/4 or 1/2 per key, key s a copy of key s % 3; the mixed forms are refused."""
    g = torch.Generator().manual_seed(0)
    q = (torch.randint(-8, 9, (2, 18, 16, 64), generator=g).float() / 4).bfloat16()
    k8 = torch.randint(-4, 5, (2, 3, 64), generator=g).float()[:, torch.arange(24) % 3].to(torch.float8_e4m3fn)
    scale = (2.0 ** -torch.randint(1, 4, (2, 3), generator=g).float())[:, torch.arange(24) % 3]
    w, fills = torch.randint(-4, 5, (2, 18, 16), generator=g).float() / 2, torch.tensor([21, 5])
    for causal in (True, False):
        ref = H.index_topk_prefill_ref(q, k8.float() * scale[..., None], w, fills, 4, causal=causal)
        idx, logits = H.kvcache_index_topk_prefill(q, k8, w, fills, 4, causal=causal, return_logits=True, k_index_scale=scale)
        assert torch.equal(idx, ref.indices) and torch.equal(logits.double(), ref.logits)
    with pytest.raises(ValueError, match="needs k_index_scale"):
        H.kvcache_index_topk_prefill(q, k8, w, fills, 4)
    with pytest.raises(ValueError, match="16-bit k_index_cache has no scale"):
        H.kvcache_index_topk_prefill(q, k8.bfloat16(), w, fills, 4, k_index_scale=scale)
