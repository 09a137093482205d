"""CPU tests of the C-ABI of the lightning indexer over an e4m3 index-key cache and of its append (include/fa_index_topk8.h): every
refusal of the two _validate entries one by one, the struct sizes against the ctypes mirrors, the declared names, the plan texts,
and the CPU route of kvcache_index_topk(k_index_scale=) against a brute-force loop.  No device is touched."""
import ctypes
import os
import re

import pytest
import torch

from flash_attention_annotated_amd import _lib, hopper_interface as H

ADDR = 0x10000  # an aligned dummy address: nothing is dereferenced
OK, NULLP, BAD_DTYPE, BAD_HEAD_DIM, BAD_HEADS, BAD_SHAPE, BAD_STRIDE, UNSUPPORTED, BAD_ABI = 0, -1, -2, -3, -4, -5, -6, -7, -9
BF16, FP16, FP32, FP8 = _lib.FA_DTYPE_BF16, _lib.FA_DTYPE_FP16, _lib.FA_DTYPE_FP32, _lib.FA_DTYPE_FP8_E4M3


def _p(b=3, s_q=2, h_i=64, d_i=128, capacity=8192, topk=2048, page=0, **fields):
    p = _lib.new_index_topk8_params()
    for name in ("q_index", "k_index_cache", "k_index_scale", "weights", "cache_seqlens", "logits", "indices"):
        setattr(p, name, ADDR)
    p.b, p.s_q, p.h_i, p.d_i, p.capacity, p.topk, p.list_width, p.logits_width = b, s_q, h_i, d_i, capacity, topk, topk, capacity
    p.q_head_stride, p.q_row_stride, p.q_batch_stride = d_i, h_i * d_i, s_q * h_i * d_i
    p.cache_row_stride, p.cache_batch_stride, p.scale_batch_stride = d_i, (page or capacity) * d_i, page or capacity
    p.w_row_stride, p.w_batch_stride, p.idx_row_stride, p.idx_batch_stride = h_i, s_q * h_i, topk, s_q * topk
    p.logits_row_stride, p.logits_batch_stride = capacity, s_q * capacity
    if page:
        p.page_table, p.page_size, p.page_table_batch_stride = ADDR, page, capacity // page
    for k, v in fields.items():
        setattr(p, k, v)
    return p


def _a(b=3, s_new=5, d_i=128, capacity=8192, page=0, ragged=False, **fields):
    p = _lib.new_index_append8_params()
    for name in ("k_index_new", "k_index_cache", "k_index_scale", "cache_seqlens"):
        setattr(p, name, ADDR)
    p.seqused_out = ADDR + 64
    p.b, p.d_i, p.capacity = b, d_i, capacity
    p.new_row_stride, p.cache_row_stride, p.cache_batch_stride, p.scale_batch_stride = d_i, d_i, (page or capacity) * d_i, page or capacity
    if ragged:
        p.cu_seqlens_k_new, p.total_new = ADDR, b * s_new
    else:
        p.s_new, p.new_batch_stride = s_new, s_new * d_i
    if page:
        p.page_table, p.page_size, p.page_table_batch_stride = ADDR, page, capacity // page
    for k, v in fields.items():
        setattr(p, k, v)
    return p


READ = [
    ("bf16_dense", _p(), OK),
    ("fp16_d64_h16", _p(dtype=FP16, d_i=64, h_i=16), OK),
    ("h48_not_causal_s16", _p(h_i=48, is_causal=0, s_q=16), OK),
    ("cache_batch_idx", _p(cache_batch_idx=ADDR), OK),
    ("paged_48", _p(page=48, capacity=48 * 100), OK),
    ("131072_keys_wider_buffers", _p(capacity=131072, list_width=4096, logits_width=140000, logits_row_stride=140000), OK),
    ("padded_rows_and_one_scale_row", _p(cache_row_stride=128 + 16, scale_batch_stride=0), OK),
    ("no_entries", _p(b=0), OK),
    ("abi_version", _p(abi_version=12), BAD_ABI),
    ("struct_size_of_the_16_bit_struct", _p(struct_size=232), BAD_ABI),
    ("fp32_queries", _p(dtype=FP32), BAD_DTYPE),
    ("16_bit_cache", _p(cache_dtype=BF16), UNSUPPORTED),
    ("d_96", _p(d_i=96), BAD_HEAD_DIM),
    *[(f"h_{h}", _p(h_i=h), BAD_HEADS) for h in (8, 40, 80)],
    *[(n, _p(**{n: ADDR}), UNSUPPORTED) for n in ("cu_seqlens_q", "cache_leftpad")],
    ("s_q_17", _p(s_q=17), BAD_SHAPE),
    ("topk_0", _p(topk=0), BAD_SHAPE),
    ("list_narrower_than_topk", _p(list_width=2047), BAD_SHAPE),
    ("logits_narrower_than_the_capacity", _p(logits_width=8191), BAD_SHAPE),
    ("131073_keys", _p(capacity=131073), BAD_SHAPE),
    ("capacity_0", _p(capacity=0), BAD_SHAPE),
    ("capacity_no_multiple_of_the_page", _p(page=48), BAD_SHAPE),
    ("paged_with_cache_batch_idx", _p(page=64, cache_batch_idx=ADDR), BAD_SHAPE),
    *[(f"null_{n}", _p(**{n: 0}), NULLP)
      for n in ("q_index", "k_index_cache", "k_index_scale", "weights", "cache_seqlens", "logits", "indices")],
    *[(f"{n}_8_bytes", _p(**{n: ADDR + 8}), BAD_STRIDE) for n in ("q_index", "k_index_cache")],
    *[(f"{n}_2_bytes", _p(**{n: ADDR + 2}), BAD_STRIDE) for n in ("k_index_scale", "weights", "logits", "indices")],
    ("q_head_stride", _p(q_head_stride=128 + 4), BAD_STRIDE),
    ("cache_row_stride_8_bytes", _p(cache_row_stride=128 + 8), BAD_STRIDE),
    ("cache_batch_stride_8_bytes", _p(cache_batch_stride=8192 * 128 + 8), BAD_STRIDE),
    ("scale_stride_negative", _p(scale_batch_stride=-8192), BAD_STRIDE),
]

WRITE = [
    ("bf16_dense", _a(), OK),
    ("fp16_d64_ragged_paged_16", _a(dtype=FP16, d_i=64, ragged=True, page=16), OK),
    ("no_rows_no_tensors", _a(s_new=0, k_index_new=0, k_index_cache=0, k_index_scale=0), OK),
    ("cache_on_8_bytes", _a(k_index_cache=ADDR + 8, cache_row_stride=128 + 8), OK),
    ("abi_version", _a(abi_version=12), BAD_ABI),
    ("fp32_rows", _a(dtype=FP32), BAD_DTYPE),
    ("d_96", _a(d_i=96), BAD_HEAD_DIM),
    ("b_0", _a(b=0), BAD_SHAPE),
    ("s_new_negative", _a(s_new=-1), BAD_SHAPE),
    ("total_new_negative", _a(ragged=True, total_new=-1), BAD_SHAPE),
    ("131073_keys", _a(capacity=131073), BAD_SHAPE),
    ("capacity_no_multiple_of_the_page", _a(page=48), BAD_SHAPE),
    ("paged_with_cache_batch_idx", _a(page=64, cache_batch_idx=ADDR), BAD_SHAPE),
    ("fill_levels_in_place", _a(seqused_out=ADDR), BAD_SHAPE),
    *[(f"null_{n}", _a(**{n: 0}), NULLP) for n in ("k_index_new", "k_index_cache", "k_index_scale", "cache_seqlens", "seqused_out")],
    ("k_index_new_8_bytes", _a(k_index_new=ADDR + 8), BAD_STRIDE),
    ("k_index_cache_4_bytes", _a(k_index_cache=ADDR + 4), BAD_STRIDE),
    *[(f"{n}_2_bytes", _a(**{n: ADDR + 2}), BAD_STRIDE) for n in ("k_index_scale", "cache_seqlens", "seqused_out")],
    ("new_row_stride", _a(new_row_stride=128 + 4), BAD_STRIDE),
    ("new_batch_stride", _a(new_batch_stride=5 * 128 + 4), BAD_STRIDE),
    ("cache_row_stride_4_bytes", _a(cache_row_stride=128 + 4), BAD_STRIDE),
    ("scale_stride_negative", _a(scale_batch_stride=-1), BAD_STRIDE),
]
CASES = [("topk8", *r) for r in READ] + [("append8", *r) for r in WRITE]


@pytest.mark.parametrize("entry,name,p,status", CASES, ids=[f"{r[0]}-{r[1]}" for r in CASES])
def test_validate(entry, name, p, status):
    lib = _lib.load()
    launch, validate, plan_name = (getattr(lib, f"fa_index_{entry}{suffix}") for suffix in ("", "_validate", "_plan_name"))
    assert validate(p) == status
    # the launch entry refuses the same way before it launches anything; so do the name and the workspace size
    assert status == OK or (launch(p, None) == status and plan_name(p) is None)
    assert entry != "topk8" or lib.fa_index_topk8_workspace_size(p) == (4 * p.b * p.s_q * p.capacity if status == OK else status)


def test_symbols_sizes_and_plan_texts():
    lib = _lib.load()
    header = open(os.path.join(_lib.INCLUDE, "fa_index_topk8.h")).read()
    declared = re.findall(r"^\w[\w *]*?\b(fa_\w+)\(", header, re.M)
    assert sorted(declared) == sorted(_lib.INDEX_TOPK8_SYMBOLS) and all(hasattr(lib, name) for name in declared)
    # the read struct is the 16-bit one's fields, the scale pointer and its batch stride
    assert lib.fa_index_topk8_params_size() == ctypes.sizeof(_lib.FaIndexTopk8Params) == ctypes.sizeof(_lib.FaIndexTopkParams) + 16 == 248
    assert [f for f in _lib.FaIndexTopk8Params._fields_ if f[0] not in ("k_index_scale", "scale_batch_stride")] == _lib.FaIndexTopkParams._fields_
    assert lib.fa_index_append8_params_size() == ctypes.sizeof(_lib.FaIndexAppend8Params) == 152
    assert lib.fa_index_topk8_validate(None) == NULLP == lib.fa_index_append8_validate(None)
    assert lib.fa_index_topk8(_p(b=0), None) == OK  # b = 0: no launch, no device
    assert not set(_lib.INDEX_TOPK8_SYMBOLS) & (set(_lib.INDEX_TOPK_SYMBOLS) | set(_lib.INDEX_PREFILL_SYMBOLS))
    # batch 64 over 131072 keys: 256-key chunks would be 32768 workgroups, so the chunk is 1024
    assert lib.fa_index_topk8_plan_name(_p(b=64, s_q=1, capacity=131072)).decode() == \
        "index_logits8_kernel d=128 heads=64 sq=1 chunk=1024 grid=(128,64) | index_select_kernel threads=1024 passes=4"
    assert lib.fa_index_topk8_plan_name(_p(s_q=7, h_i=16, d_i=64, capacity=768, topk=64, dtype=FP16)).decode() == \
        "index_logits8_kernel d=64 heads=16 sq=7 chunk=256 grid=(3,3) | index_select_kernel threads=256 passes=4"
    # 15 rows of 128 channels: 4 rows per wave, 16 per workgroup; of 64 channels 8 and 32
    assert lib.fa_index_append8_plan_name(_a()).decode() == "index_append8_kernel d=128 rows_per_wave=4 grid=1"
    assert lib.fa_index_append8_plan_name(_a(d_i=64, ragged=True, total_new=33)).decode() == "index_append8_kernel d=64 rows_per_wave=8 grid=2"


def test_cpu_route_is_the_rule_on_the_dequantised_keys():
    """Bytes -4 .. 4 with a scale of 1/8, 1/4 or 1/2 per key, key s a copy of key s % 3: ties at the cut; the mixed forms are refused."""
    g = torch.Generator().manual_seed(0)
    q = (torch.randint(-8, 9, (2, 3, 16, 64), generator=g).float() / 4).bfloat16()
    k8 = torch.randint(-4, 5, (2, 3, 64), generator=g).float()[:, torch.arange(24) % 3].to(torch.float8_e4m3fn)
    scale = (2.0 ** -torch.randint(1, 4, (2, 3), generator=g).float())[:, torch.arange(24) % 3]
    w, fills, ties = torch.randint(-4, 5, (2, 3, 16), generator=g).float() / 2, (21, 5), 0
    idx, logits = H.kvcache_index_topk(q, k8, w, torch.tensor(fills), 4, k_index_scale=scale, return_logits=True)
    for b, sk in enumerate(fills):
        dots = torch.einsum("ihc,sc->ihs", q[b].double(), k8[b].double())
        for i in range(3):
            n = max(sk - (2 - i), 0)
            L = [float(scale[b, s]) * sum(float(w[b, i, j]) * max(0.0, float(dots[i, j, s])) for j in range(16)) for s in range(n)]
            assert logits[b, i, :n].tolist() == L and torch.all(logits[b, i, n:] == float("-inf"))
            chosen = sorted(sorted(range(n), key=lambda s: (-L[s], s))[:4])
            assert idx[b, i, 0].tolist() == chosen + [-1] * (4 - len(chosen))
            ties += n >= 8 and any(L[s] == sorted(L, reverse=True)[3] and s not in chosen for s in range(n))
    assert ties, "no tie at the cut"
    with pytest.raises(ValueError, match="needs k_index_scale"):
        H.kvcache_index_topk(q, k8, w, torch.tensor(fills), 4)
    with pytest.raises(ValueError, match="16-bit k_index_cache has no scale"):
        H.kvcache_index_topk(q, k8.bfloat16(), w, torch.tensor(fills), 4, k_index_scale=scale)
