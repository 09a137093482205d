"""CPU: the oracle of the block-sparse backward (tests/block_sparse_bwd_oracle.py) and cute_interface.block_sparse_bwd_lists.
The GPU parity tests (tests/test_block_sparse_bwd_gpu.py) measure against these, so they are guarded here:
  * where no row is keyless, the guarded oracle IS block_sparse_oracle.attention_block_sparse_ref: same output and -- by
    autograd through both -- the same gradients, bit for bit, on the fp32 and on the low-precision reordered path;
  * with a query block that lists nothing and a key block nobody visits, the gradients are finite on both paths, dq of the
    empty query block and dk / dv of the unvisited key block are exactly 0;
  * with every block listed, the gradients are those of oracle/attention_ref.py;
  * block_sparse_bwd_lists is the transpose of block_mask_from_lists, for full, broadcast and shuffled lists, and equals
    block_sparse_from_mask of the transposed mask."""
import pytest
import torch

import block_sparse_bwd_oracle as bwo
import block_sparse_oracle as bso
from oracle import attention_ref as oracle
from flash_attention_annotated_amd.cute_interface import block_sparse_bwd_lists, block_sparse_from_mask

B, H, HK, SQ, SK, D = 2, 4, 2, 300, 715, 32
NM, NK = 3, 6


def _inputs(seed=0, dtype=torch.bfloat16):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, SQ, H, D, generator=g).to(dtype), torch.randn(B, SK, HK, D, generator=g).to(dtype),
            torch.randn(B, SK, HK, D, generator=g).to(dtype), torch.randn(B, SQ, H, D, generator=g).to(dtype))


def _all_blocks():
    cnt = torch.full((1, 1, NM), NK, dtype=torch.int32)
    idx = torch.arange(NK, dtype=torch.int32).flip(0).view(1, 1, 1, NK).expand(1, 1, NM, NK).contiguous()
    return None, None, cnt, idx


@pytest.mark.parametrize("kw,lists", [(dict(), "random"), (dict(softcap=5.0), "random"), (dict(causal=True), "all"),
                                      (dict(window_size=(200, 50)), "all")], ids=str)
def test_guarded_oracle_is_the_forward_oracle_where_every_row_sees_a_key(kw, lists):
    q, k, v, g = _inputs()
    lists = _all_blocks() if lists == "all" else bso.random_lists(3, B, H, NM, NK, min_visited=1)[0]
    mask_kw = {n: kw[n] for n in ("causal", "window_size") if n in kw}
    assert bwo.allowed_mask(lists, B, H, SQ, SK, **mask_kw).any(-1).all(), "the case must have no keyless row"
    old = bwo.grads(lambda a, b, c, **o: bso.attention_block_sparse_ref(a, b, c, *lists, **kw, **o)[0], [q, k, v], g)
    new = bwo.grads(lambda a, b, c, **o: bwo.attention_block_sparse_grad_ref(a, b, c, lists, **kw, **o)[0], [q, k, v], g)
    for path_old, path_new in zip(old, new):
        for a, b in zip(path_old, path_new):
            assert torch.isfinite(a).all() and torch.equal(a, b)
    for order in (dict(), dict(upcast=False, reorder_ops=True)):
        o1, l1 = bso.attention_block_sparse_ref(q, k, v, *lists, **kw, **order)
        o2, l2 = bwo.attention_block_sparse_grad_ref(q, k, v, lists, **kw, **order)
        assert torch.equal(o1, o2) and torch.equal(l1, l2)


@pytest.mark.parametrize("sink", [False, True], ids=["no_sink", "sink"])
def test_finite_with_an_empty_query_block_and_an_unvisited_key_block(sink):
    q, k, v, g = _inputs(1)
    _, visited = bso.random_lists(5, B, H, NM, NK, min_visited=2, max_visited=NK - 1)
    visited[:, :, 1] = False                            # query block 1 lists nothing
    visited[..., 4] = False                             # key block 4: nobody visits it
    # everything through the mask list: visited blocks first, the others (block 4 among them) behind the count
    mi = torch.sort((~visited).to(torch.int8), dim=-1, stable=True).indices.to(torch.int32)
    mc = visited.sum(-1, dtype=torch.int32)
    lists = (None, None, mc, mi)
    seen = bso.block_mask_from_lists(*lists, B, H)
    assert not seen[:, :, 1].any() and not seen[..., 4].any() and seen.any()
    s = torch.linspace(-4, 4, H).to(torch.bfloat16) if sink else None
    leaves = [q, k, v] + ([s] if sink else [])
    fn = lambda a, b, c, *z, **o: bwo.attention_block_sparse_grad_ref(a, b, c, lists, causal=True, learnable_sink=z[0] if z else None, **o)[0]  # noqa: E731
    for path in bwo.grads(fn, leaves, g):
        for t in path:
            assert torch.isfinite(t).all()
        dq, dk, dv = path[:3]
        assert (dq[:, 128:256] == 0).all() and dq[:, :128].abs().max() > 0
        assert (dk[:, 512:640] == 0).all() and (dv[:, 512:640] == 0).all() and dv[:, :512].abs().max() > 0
    out, lse = bwo.attention_block_sparse_grad_ref(q, k, v, lists, causal=True, learnable_sink=s)
    assert (out[:, 128:256] == 0).all()
    assert torch.equal(lse[:, :, 128:256], s.float().view(1, H, 1).expand(B, H, 128)) if sink else torch.isposinf(lse[:, :, 128:256]).all()


@pytest.mark.parametrize("kw", [dict(), dict(causal=True), dict(window_size=(200, 50)), dict(causal=True, softcap=5.0)], ids=str)
def test_every_block_listed_gives_the_dense_gradients(kw):
    lists = _all_blocks()
    dense_kw = dict(kw, window_size=kw.get("window_size", (-1, -1)))
    sparse = lambda a, b, c, **o: bwo.attention_block_sparse_grad_ref(a, b, c, lists, **kw, **o)[0]  # noqa: E731
    dense = lambda a, b, c, **o: oracle.attention_ref(a, b, c, **dense_kw, **o)[0]  # noqa: E731
    # fp32 leaves: the gradients themselves are fp32, nothing is rounded to the inputs' precision
    q, k, v, g = _inputs(2, torch.float32)
    for name, a, b in zip(("dq", "dk", "dv"), bwo.grads(sparse, [q, k, v], g)[0], bwo.grads(dense, [q, k, v], g)[0]):
        assert (a - b).abs().max().item() <= 1e-5, name
    # bf16 leaves: the fp32 paths agree to one rounding of the gradient to bf16 (eps x the largest magnitude), the low-precision paths differ by less than their
    # own distance from the fp32 gradients
    q, k, v, g = _inputs(2)
    (ref, pt), (dref, dpt) = bwo.grads(sparse, [q, k, v], g), bwo.grads(dense, [q, k, v], g)
    for name, a, b, p, dp in zip(("dq", "dk", "dv"), ref, dref, pt, dpt):
        a, b, p, dp = a.float(), b.float(), p.float(), dp.float()
        assert (a - b).abs().max().item() <= torch.finfo(q.dtype).eps * b.abs().max().item() + 1e-5, name
        assert (p - dp).abs().max().item() <= (dp - b).abs().max().item() + 1e-5, name


@pytest.mark.parametrize("shape", [(B, H), (1, 1), (1, H), (B, 1)], ids=str)
@pytest.mark.parametrize("seed", [0, 1])
def test_bwd_lists_are_the_transpose_of_the_forward_lists(shape, seed):
    b, h = shape
    lists, visited = bso.random_lists(seed, b, h, NM, NK)          # shuffled order, unvisited indices in the tails
    cnt, idx = block_sparse_bwd_lists(*lists)
    assert cnt.dtype == idx.dtype == torch.int32
    assert cnt.shape == (b, h, NK) and idx.shape == (b, h, NK, NM)   # broadcast dims of size 1 are kept
    want_cnt, want_idx = bwo.key_major_lists(lists, b, h)
    assert torch.equal(cnt, want_cnt) and torch.equal(idx, want_idx)  # ascending, tails zero
    back = bso.block_mask_from_lists(None, None, cnt, idx, b, h)      # (b, h, nk, nm)
    assert torch.equal(back, visited.transpose(-1, -2))
    from_mask = block_sparse_from_mask(visited.transpose(-1, -2))[2:]
    assert torch.equal(from_mask[0], cnt) and torch.equal(from_mask[1], idx)
    # without a full list, and with one list broadcast where the other is not
    only_mask = block_sparse_bwd_lists(None, None, lists[2], lists[3])
    assert torch.equal(bso.block_mask_from_lists(None, None, *only_mask, b, h),
                       bso.block_mask_from_lists(None, None, lists[2], lists[3], b, h).transpose(-1, -2))
    if (b, h) == (B, H):
        mixed = block_sparse_bwd_lists(lists[0][:1, :1], lists[1][:1, :1], lists[2], lists[3])
        want = bso.block_mask_from_lists(lists[0][:1, :1], lists[1][:1, :1], lists[2], lists[3], b, h)
        assert mixed[0].shape == (B, H, NK) and torch.equal(bso.block_mask_from_lists(None, None, *mixed, b, h), want.transpose(-1, -2))
