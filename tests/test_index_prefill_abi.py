"""CPU tests of the C-ABI of the prefill-sized lightning indexer (include/fa_index_prefill.h): every refusal of _validate one by
one, the struct size against the ctypes mirror, the workspace sizes, the plan text, and the oracle index_topk_prefill_ref against
a brute-force loop.  No device is touched."""
import ctypes
import os
import re

import pytest
import torch

from flash_attention_annotated_amd import _lib, hopper_interface as H

ADDR = 0x10000  # an aligned dummy address: nothing is dereferenced
OK, NULLP, BAD_DTYPE, BAD_HEAD_DIM, BAD_HEADS, BAD_SHAPE, BAD_STRIDE, UNSUPPORTED, BAD_ABI = 0, -1, -2, -3, -4, -5, -6, -7, -9
BF16, FP16, FP32, FP8 = _lib.FA_DTYPE_BF16, _lib.FA_DTYPE_FP16, _lib.FA_DTYPE_FP32, _lib.FA_DTYPE_FP8_E4M3
BLOCK = _lib.FA_INDEX_PREFILL_BLOCK


def _p(b=3, s_q=4096, h_i=64, d_i=128, capacity=8192, topk=2048, page=0, rows=BLOCK, **fields):
    p = _lib.new_index_prefill_params()
    for name in ("q_index", "k_index_cache", "weights", "cache_seqlens", "workspace", "indices"):
        setattr(p, name, ADDR)
    p.b, p.s_q, p.h_i, p.d_i, p.capacity, p.topk, p.list_width = b, s_q, h_i, d_i, capacity, topk, topk
    p.workspace_rows, p.workspace_width, p.workspace_row_stride = rows, capacity, capacity
    p.q_head_stride, p.q_row_stride, p.q_batch_stride = d_i, h_i * d_i, s_q * h_i * d_i
    p.cache_row_stride, p.cache_batch_stride = d_i, (page or capacity) * d_i
    p.w_row_stride, p.w_batch_stride, p.idx_row_stride, p.idx_batch_stride = h_i, s_q * h_i, topk, s_q * topk
    if page:
        p.page_table, p.page_size, p.page_table_batch_stride = ADDR, page, capacity // page
    for k, v in fields.items():
        setattr(p, k, v)
    return p


CASES = [
    ("bf16_dense", _p(), OK),
    ("fp16_d64_h16", _p(dtype=FP16, cache_dtype=FP16, d_i=64, h_i=16), OK),
    *[(f"s_q_{n}", _p(s_q=n), OK) for n in (1, 16, 17, 70000)],
    ("h48_not_causal", _p(h_i=48, is_causal=0), OK),
    ("cache_batch_idx", _p(cache_batch_idx=ADDR), OK),
    ("paged_48", _p(page=48, capacity=48 * 100), OK),
    ("131072_keys_wider_buffers", _p(capacity=131072, list_width=4096, workspace_width=140000, workspace_row_stride=140000), OK),
    ("no_entries", _p(b=0), OK),
    ("abi_version", _p(abi_version=12), BAD_ABI),
    ("struct_size", _p(struct_size=8), BAD_ABI),
    ("fp32", _p(dtype=FP32, cache_dtype=FP32), BAD_DTYPE),
    ("cache_of_the_other_16_bit_type", _p(cache_dtype=FP16), BAD_DTYPE),
    ("e4m3_cache", _p(cache_dtype=FP8), UNSUPPORTED),
    ("d_96", _p(d_i=96), BAD_HEAD_DIM),
    *[(f"h_{h}", _p(h_i=h), BAD_HEADS) for h in (8, 40, 80)],
    *[(n, _p(**{n: ADDR}), UNSUPPORTED) for n in ("cu_seqlens_q", "cache_leftpad")],
    ("s_q_0", _p(s_q=0), BAD_SHAPE),
    ("2^31_tokens", _p(b=32768, s_q=65536), BAD_SHAPE),
    ("topk_0", _p(topk=0), BAD_SHAPE),
    ("list_narrower_than_topk", _p(list_width=2047), BAD_SHAPE),
    ("workspace_narrower_than_the_capacity", _p(workspace_width=8191), BAD_SHAPE),
    ("workspace_below_a_block", _p(rows=BLOCK - 1), BAD_SHAPE),
    ("131073_keys", _p(capacity=131073), BAD_SHAPE),
    ("capacity_0", _p(capacity=0), BAD_SHAPE),
    ("b_negative", _p(b=-1), BAD_SHAPE),
    ("page_size_0", _p(page=64, page_size=0), BAD_SHAPE),
    ("capacity_no_multiple_of_the_page", _p(page=48), BAD_SHAPE),
    ("paged_with_cache_batch_idx", _p(page=64, cache_batch_idx=ADDR), BAD_SHAPE),
    *[(f"null_{n}", _p(**{n: 0}), NULLP) for n in ("q_index", "k_index_cache", "weights", "cache_seqlens", "workspace", "indices")],
    *[(f"{n}_8_bytes", _p(**{n: ADDR + 8}), BAD_STRIDE) for n in ("q_index", "k_index_cache")],
    *[(f"{n}_2_bytes", _p(**{n: ADDR + 2}), BAD_STRIDE) for n in ("weights", "workspace", "indices")],
    ("q_head_stride", _p(q_head_stride=128 + 4), BAD_STRIDE),
    ("cache_row_stride", _p(cache_row_stride=128 + 2), BAD_STRIDE),
]


@pytest.mark.parametrize("name,p,status", CASES, ids=[r[0] for r in CASES])
def test_index_prefill_validate(name, p, status):
    lib = _lib.load()
    assert lib.fa_index_prefill_validate(p) == status
    # the launch entry refuses the same way before it launches anything; so does the name
    assert status == OK or (lib.fa_index_prefill(p, None) == status and lib.fa_index_prefill_plan_name(p) is None)
    if status == OK:  # the least workspace is one token block, the one-round one every block of the call (at least one)
        assert lib.fa_index_prefill_workspace_size(p, 0) == 4 * BLOCK * p.capacity
        assert lib.fa_index_prefill_workspace_size(p, 1) == 4 * BLOCK * p.capacity * max(p.b * -(-p.s_q // BLOCK), 1)


def test_symbols_sizes_and_plan_text():
    lib = _lib.load()
    header = open(os.path.join(_lib.INCLUDE, "fa_index_prefill.h")).read()
    declared = re.findall(r"^\w[\w *]*?\b(fa_\w+)\(", header, re.M)
    assert sorted(declared) == sorted(_lib.INDEX_PREFILL_SYMBOLS) and all(hasattr(lib, name) for name in declared)
    assert lib.fa_index_prefill_params_size() == ctypes.sizeof(_lib.FaIndexPrefillParams) == 232
    assert [f[0] for f in _lib.FaIndexPrefillParams._fields_[:2]] == ["abi_version", "struct_size"]
    assert BLOCK == H.INDEX_PREFILL_BLOCK == int(re.search(r"#define FA_INDEX_PREFILL_BLOCK (\d+)", header).group(1))
    assert lib.fa_index_prefill_validate(None) == NULLP and lib.fa_index_prefill(_p(b=0), None) == OK  # b = 0: no launch, no device
    # the workspace size looks at the call, not at the workspace it sizes
    assert lib.fa_index_prefill_workspace_size(_p(workspace=0, rows=0, workspace_width=0), 1) == 4 * 8192 * 3 * 4096
    assert lib.fa_index_prefill_workspace_size(_p(d_i=96), 0) == BAD_HEAD_DIM
    # additive: the ABI version, the decode unit's symbols and struct, and its refusal of 17 tokens are what they were
    assert lib.fa_abi_version() == 13 == _lib.FA_ABI_VERSION
    assert _lib.INDEX_TOPK_SYMBOLS == ("fa_index_topk", "fa_index_topk_validate", "fa_index_topk_workspace_size", "fa_index_topk_plan_name",
                                       "fa_index_topk_params_size") and not set(_lib.INDEX_TOPK_SYMBOLS) & set(_lib.INDEX_PREFILL_SYMBOLS)
    assert lib.fa_index_topk_params_size() == ctypes.sizeof(_lib.FaIndexTopkParams) == 232
    # one prompt of 4096 tokens over 32768 keys in one round: 512 blocks, the chunk grows to 4096 keys (8 chunks)
    assert lib.fa_index_prefill_plan_name(_p(b=1, capacity=32768, rows=4096)).decode() == \
        "index_logits_prefill_kernel d=128 heads=64 sq=4096 block=8 tile=64 chunk=4096 grid=4096 | index_select_prefill_kernel threads=1024 " \
        "passes=4 grid=4096 | rounds=1"
    # 3 x 17 tokens on the least workspace: 9 blocks, a round each; the chunk does not depend on the rows
    assert lib.fa_index_prefill_plan_name(_p(s_q=17, h_i=16, d_i=64, capacity=768, topk=64, dtype=FP16, cache_dtype=FP16)).decode() == \
        "index_logits_prefill_kernel d=64 heads=16 sq=17 block=8 tile=64 chunk=256 grid=3 | index_select_prefill_kernel threads=256 " \
        "passes=4 grid=8 | rounds=9"


def test_index_topk_prefill_ref_is_the_rule():
    """Against a brute-force loop at s_q 18, which index_topk_ref refuses.  Key s is a copy of key s % 3: the fourth place is a tie
    at the cut wherever 8 or more keys are visible.  CPU tensors take the oracle."""
    g = torch.Generator().manual_seed(0)
    q = (torch.randint(-8, 9, (2, 18, 16, 64), generator=g).float() / 4).bfloat16()
    k = (torch.randint(-8, 9, (2, 3, 64), generator=g).float().div(4)[:, torch.arange(24) % 3]).bfloat16()
    w, fills = torch.randint(-4, 5, (2, 18, 16), generator=g).float() / 2, torch.tensor([21, 5])
    with pytest.raises(AssertionError):
        H.index_topk_ref(q, k, w, fills, 4)
    for causal in (True, False):
        ref = H.index_topk_prefill_ref(q, k, w, fills, 4, causal=causal)
        idx, logits = H.kvcache_index_topk_prefill(q, k, w, fills, 4, causal=causal, return_logits=True)
        assert torch.equal(idx, ref.indices) and torch.equal(logits.double(), ref.logits)
        ties = 0
        for b, sk in enumerate((21, 5)):
            dots = torch.einsum("ihc,sc->ihs", q[b].double(), k[b].double())
            for i in range(18):
                n = max(sk - (17 - i), 0) if causal else sk
                L = [sum(float(w[b, i, j]) * max(0.0, float(dots[i, j, s])) for j in range(16)) for s in range(n)]
                assert ref.logits[b, i, :n].tolist() == L and torch.all(ref.logits[b, i, n:] == float("-inf"))
                chosen = sorted(sorted(range(n), key=lambda s: (-L[s], s))[:4])
                assert ref.indices[b, i, 0].tolist() == chosen + [-1] * (4 - len(chosen))
                ties += n >= 8 and any(L[s] == sorted(L, reverse=True)[3] and s not in chosen for s in range(n))
        assert ties, "no tie at the cut"
