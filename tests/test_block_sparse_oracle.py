"""CPU: the block-sparse oracle (tests/block_sparse_oracle.py) against independent statements of the same thing, and the
round trip of cute_interface.block_sparse_from_mask.  The GPU parity tests (tests/test_block_sparse_gpu.py) measure against
this oracle, so it is guarded here:
  * with every block listed it is the dense oracle (oracle/attention_ref.py), with a sink tests/sink_oracle.py, within 1e-5;
  * for random lists it is torch's scaled_dot_product_attention in fp32 under the same bool mask, on rows that see a key,
    within 1e-5;
  * mask -> lists -> mask is exact, with broadcast dims and with the full= split."""
import math

import pytest
import torch

import block_sparse_oracle as bso
import sink_oracle
from oracle import attention_ref as oracle
from flash_attention_annotated_amd.cute_interface import block_sparse_from_mask

B, H, HK, SQ, SK, D = 2, 4, 2, 300, 715, 32
NM, NK = 3, 6


def _qkv(seed=0, dtype=torch.bfloat16):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, SQ, H, D, generator=g).to(dtype), torch.randn(B, SK, HK, D, generator=g).to(dtype),
            torch.randn(B, SK, HK, D, generator=g).to(dtype))


def _random_lists(seed):
    return bso.random_lists(seed, B, H, NM, NK)


def _all_blocks(in_full):
    cnt = torch.full((1, 1, NM), NK, dtype=torch.int32)
    idx = torch.arange(NK, dtype=torch.int32).view(1, 1, 1, NK).expand(1, 1, NM, NK).contiguous()
    zc, zi = torch.zeros_like(cnt), torch.zeros_like(idx)
    return (cnt, idx, zc, zi) if in_full else (None, None, cnt, idx)


@pytest.mark.parametrize("in_full", [False, True])
@pytest.mark.parametrize("kw", [dict(), dict(causal=True), dict(window_size=(200, 50)), dict(causal=True, softcap=5.0)], ids=str)
def test_every_block_listed_is_the_dense_oracle(kw, in_full):
    """fp32 inputs, so that 1e-5 compares the math and not two roundings of the output to bf16."""
    q, k, v = (t.float() for t in _qkv())
    out, lse = bso.attention_block_sparse_ref(q, k, v, *_all_blocks(in_full), **kw)
    okw = dict(kw)
    okw["window_size"] = tuple(-1 if w is None else w for w in okw.pop("window_size", (None, None)))
    ref, _, lse_ref = oracle.attention_ref(q, k, v, return_lse=True, **okw)
    assert out.dtype == torch.float32
    assert (out - ref).abs().max().item() <= 1e-5
    assert (lse - lse_ref).abs().max().item() <= 1e-5
    # the input-precision path is tests/sink_oracle.py's (pinned to the reference there): all-zero bias, bit-equal
    qb, kb, vb = _qkv()
    pt, _ = bso.attention_block_sparse_ref(qb, kb, vb, *_all_blocks(in_full), upcast=False, reorder_ops=True, **kw)
    pt_ref, _ = sink_oracle.attention_sink_ref(qb, kb, vb, None, upcast=False, reorder_ops=True, **kw)
    assert pt.dtype == torch.bfloat16 and torch.equal(pt, pt_ref)


def test_every_block_listed_with_a_sink_is_the_sink_oracle():
    q, k, v = (t.float() for t in _qkv(1))
    sink = torch.linspace(-4, 4, H).to(torch.bfloat16)
    out, lse = bso.attention_block_sparse_ref(q, k, v, *_all_blocks(False), causal=True, learnable_sink=sink)
    ref, lse_ref = sink_oracle.attention_sink_ref(q, k, v, sink, causal=True)
    assert (out - ref).abs().max().item() <= 1e-5
    assert (lse - lse_ref).abs().max().item() <= 1e-5


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("seed", [0, 1])
def test_random_lists_are_sdpa_under_the_bool_mask(seed, causal):
    q, k, v = (t.float() for t in _qkv(2))
    lists, visited = _random_lists(seed)
    assert torch.equal(bso.block_mask_from_lists(*lists, B, H), visited)
    allowed = bso.dense_mask(visited, SQ, SK)
    if causal:
        i, j = torch.arange(SQ).view(-1, 1), torch.arange(SK).view(1, -1)
        allowed = allowed & (j <= i + SK - SQ)
    out, lse = bso.attention_block_sparse_ref(q, k, v, *lists, causal=causal)
    g = H // HK
    kk, vv = (t.repeat_interleave(g, dim=2).transpose(1, 2) for t in (k, v))
    ref = torch.nn.functional.scaled_dot_product_attention(q.transpose(1, 2), kk, vv, attn_mask=allowed).transpose(1, 2)
    seen = allowed.any(-1)                                       # (b, h, sq)
    assert seen.any() and not seen.all()                         # both kinds of row are in the case
    rows = seen.transpose(1, 2)                                  # (b, sq, h)
    assert (out[rows] - ref[rows]).abs().max().item() <= 1e-5
    assert (out[~rows] == 0).all()
    assert torch.equal(torch.isfinite(lse), seen)
    scores = torch.einsum("bthd,bhsd->bhts", q, kk) / math.sqrt(D)
    lse_ref = torch.logsumexp(scores.masked_fill(~allowed, float("-inf")), dim=-1)
    assert (lse[seen] - lse_ref[seen]).abs().max().item() <= 1e-5


@pytest.mark.parametrize("shape", [(B, H), (1, H), (B, 1), (1, 1)])
@pytest.mark.parametrize("split", [False, True])
def test_block_sparse_from_mask_round_trip(shape, split):
    g = torch.Generator().manual_seed(3)
    mask = torch.rand(*shape, NM, NK, generator=g) < 0.5
    mask[..., 1, :] = False  # a query block that visits nothing
    full = (torch.rand(*shape, NM, NK, generator=g) < 0.5) if split else None
    fc, fi, mc, mi = block_sparse_from_mask(mask, full)
    assert fc.dtype == fi.dtype == mc.dtype == mi.dtype == torch.int32
    assert fc.shape == mc.shape == (*shape, NM) and fi.shape == mi.shape == (*shape, NM, NK)
    back = bso.block_mask_from_lists(fc, fi, mc, mi, B, H)
    assert torch.equal(back, mask.expand(B, H, NM, NK))
    want_full = (mask & full) if split else torch.zeros_like(mask)
    assert torch.equal(bso.block_mask_from_lists(None, None, fc, fi, B, H), want_full.expand(B, H, NM, NK))
    assert torch.equal(fc + mc, mask.sum(-1, dtype=torch.int32))
    col = torch.arange(NK)
    for cnt, idx in ((fc, fi), (mc, mi)):
        used = col < cnt[..., None]
        assert (idx[~used] == 0).all()                                        # tails are zero
        asc = (idx[..., 1:] > idx[..., :-1]) | ~used[..., 1:]                  # indices ascend in front of the count
        assert asc.all()
