"""CPU tests of the C-ABI of the lightning indexer (include/fa_index_topk.h): every refusal of _validate one by one, the struct
size against the ctypes mirror, the plan text, and the oracle index_topk_ref against a brute-force loop.  No device is touched."""
import ctypes
import os
import re

import pytest
import torch

from flash_attention_annotated_amd import _lib
from flash_attention_annotated_amd.hopper_interface import index_topk_ref

ADDR = 0x10000  # an aligned dummy address: nothing is dereferenced
OK, NULLP, BAD_DTYPE, BAD_HEAD_DIM, BAD_HEADS, BAD_SHAPE, BAD_STRIDE, UNSUPPORTED, BAD_ABI = 0, -1, -2, -3, -4, -5, -6, -7, -9
BF16, FP16, FP32, FP8 = _lib.FA_DTYPE_BF16, _lib.FA_DTYPE_FP16, _lib.FA_DTYPE_FP32, _lib.FA_DTYPE_FP8_E4M3


def _p(b=3, s_q=1, h_i=64, d_i=128, capacity=8192, topk=2048, page=0, **fields):
    p = _lib.new_index_topk_params()
    for name in ("q_index", "k_index_cache", "weights", "cache_seqlens", "logits", "indices"):
        setattr(p, name, ADDR)
    p.b, p.s_q, p.h_i, p.d_i, p.capacity, p.topk, p.list_width, p.logits_width = b, s_q, h_i, d_i, capacity, topk, topk, capacity
    p.q_head_stride, p.q_row_stride, p.q_batch_stride = d_i, h_i * d_i, s_q * h_i * d_i
    p.cache_row_stride, p.cache_batch_stride = d_i, (page or capacity) * d_i
    p.w_row_stride, p.w_batch_stride = h_i, s_q * h_i
    p.logits_row_stride, p.logits_batch_stride, p.idx_row_stride, p.idx_batch_stride = capacity, s_q * capacity, topk, s_q * topk
    if page:
        p.page_table, p.page_size, p.page_table_batch_stride = ADDR, page, capacity // page
    for k, v in fields.items():
        setattr(p, k, v)
    return p


CASES = [
    ("bf16_dense", _p(), OK),
    ("fp16_d64_h16", _p(dtype=FP16, cache_dtype=FP16, d_i=64, h_i=16), OK),
    ("h48_sq16_not_causal", _p(h_i=48, s_q=16, is_causal=0), OK),
    ("cache_batch_idx", _p(cache_batch_idx=ADDR), OK),
    ("paged_48", _p(page=48, capacity=48 * 100), OK),
    ("131072_keys_wider_buffers", _p(capacity=131072, list_width=4096, logits_width=140000), OK),
    ("no_entries", _p(b=0), OK),
    ("abi_version", _p(abi_version=12), BAD_ABI),
    ("struct_size", _p(struct_size=8), BAD_ABI),
    ("fp32", _p(dtype=FP32, cache_dtype=FP32), BAD_DTYPE),
    ("cache_of_the_other_16_bit_type", _p(cache_dtype=FP16), BAD_DTYPE),
    ("e4m3_cache", _p(cache_dtype=FP8), UNSUPPORTED),
    ("d_96", _p(d_i=96), BAD_HEAD_DIM),
    *[(f"h_{h}", _p(h_i=h), BAD_HEADS) for h in (8, 40, 80)],
    *[(n, _p(**{n: ADDR}), UNSUPPORTED) for n in ("cu_seqlens_q", "cache_leftpad")],
    *[(f"s_q_{n}", _p(s_q=n), BAD_SHAPE) for n in (0, 17)],
    ("topk_0", _p(topk=0), BAD_SHAPE),
    ("list_narrower_than_topk", _p(list_width=2047), BAD_SHAPE),
    ("logits_narrower_than_the_capacity", _p(logits_width=8191), BAD_SHAPE),
    ("131073_keys", _p(capacity=131073, logits_width=131073), BAD_SHAPE),
    ("capacity_0", _p(capacity=0), BAD_SHAPE),
    ("b_negative", _p(b=-1), BAD_SHAPE),
    ("page_size_0", _p(page=64, page_size=0), BAD_SHAPE),
    ("capacity_no_multiple_of_the_page", _p(page=48), BAD_SHAPE),
    ("paged_with_cache_batch_idx", _p(page=64, cache_batch_idx=ADDR), BAD_SHAPE),
    *[(f"null_{n}", _p(**{n: 0}), NULLP) for n in ("q_index", "k_index_cache", "weights", "cache_seqlens", "logits", "indices")],
    *[(f"{n}_8_bytes", _p(**{n: ADDR + 8}), BAD_STRIDE) for n in ("q_index", "k_index_cache")],
    *[(f"{n}_2_bytes", _p(**{n: ADDR + 2}), BAD_STRIDE) for n in ("weights", "logits", "indices")],
    ("q_head_stride", _p(q_head_stride=128 + 4), BAD_STRIDE),
    ("cache_row_stride", _p(cache_row_stride=128 + 2), BAD_STRIDE),
]


@pytest.mark.parametrize("name,p,status", CASES, ids=[r[0] for r in CASES])
def test_index_topk_validate(name, p, status):
    lib = _lib.load()
    assert lib.fa_index_topk_validate(p) == status
    # the launch entry refuses the same way before it launches anything; so do the size and the name
    assert status == OK or (lib.fa_index_topk(p, None) == status and lib.fa_index_topk_plan_name(p) is None)
    assert lib.fa_index_topk_workspace_size(p) == (status if status != OK else 4 * p.b * p.s_q * p.capacity)


def test_symbols_sizes_and_plan_text():
    lib = _lib.load()
    header = open(os.path.join(_lib.INCLUDE, "fa_index_topk.h")).read()
    declared = re.findall(r"^\w[\w *]*?\b(fa_\w+)\(", header, re.M)
    assert sorted(declared) == sorted(_lib.INDEX_TOPK_SYMBOLS) and all(hasattr(lib, name) for name in declared)
    assert lib.fa_index_topk_params_size() == ctypes.sizeof(_lib.FaIndexTopkParams) == 232
    assert lib.fa_index_topk_validate(None) == NULLP and lib.fa_index_topk(_p(b=0), None) == OK  # b = 0: no launch, no device
    # batch 1 over 32768 keys: 128 workgroups of 256 keys; 64 entries over 131072: the chunk grows to 1024, the grid stays 2-D
    assert lib.fa_index_topk_plan_name(_p(b=1, capacity=32768)).decode() == \
        "index_logits_kernel d=128 heads=64 sq=1 chunk=256 grid=(128,1) | index_select_kernel threads=1024 passes=4"
    assert lib.fa_index_topk_plan_name(_p(b=64, s_q=3, h_i=16, d_i=64, capacity=131072, dtype=FP16, cache_dtype=FP16)).decode() == \
        "index_logits_kernel d=64 heads=16 sq=3 chunk=1024 grid=(128,64) | index_select_kernel threads=1024 passes=4"


def test_index_topk_ref_is_the_rule():
    """Against a brute-force loop.  Key s is a copy of key s % 3: with 8 or 9 candidates the fourth place is a tie at the cut."""
    g = torch.Generator().manual_seed(0)
    q = torch.randint(-8, 9, (2, 2, 16, 64), generator=g).float() / 4
    k = torch.randint(-8, 9, (2, 3, 64), generator=g).float().div(4)[:, torch.arange(12) % 3]
    w = torch.randint(-4, 5, (2, 2, 16), generator=g).float() / 2
    for causal in (True, False):
        ref = index_topk_ref(q.bfloat16(), k.bfloat16(), w, torch.tensor([9, 3]), 4, causal=causal)
        for b, sk in enumerate((9, 3)):
            for i in range(2):
                n = max(sk - (1 - i), 0) if causal else sk
                L = [sum(float(w[b, i, j]) * max(0.0, sum(float(q[b, i, j, c]) * float(k[b, s, c]) for c in range(64))) for j in range(16))
                     for s in range(n)]
                assert ref.logits[b, i, :n].tolist() == L and torch.all(ref.logits[b, i, n:] == float("-inf"))
                chosen = sorted(sorted(range(n), key=lambda s: (-L[s], s))[:4])
                assert ref.indices[b, i, 0].tolist() == chosen + [-1] * (4 - len(chosen))
                if n >= 8:
                    cut = sorted(L, reverse=True)[3]
                    assert [s for s in range(n) if L[s] == cut and s not in chosen], "no tie at the cut"
        assert ref.A.min() >= 0 and torch.all(ref.A >= ref.logits.clamp_min(0).nan_to_num(0, 0, 0))
