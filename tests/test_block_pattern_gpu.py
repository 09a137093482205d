"""GPU tests of cute_interface.block_sparse_select (csrc/fa_block_pattern.hip; include/fa_block_pattern.h states the rule), split
so that rounding cannot hide a wrong choice:
  scores   against the fp64 oracle, with the first-order bound of the rule:
           |u - u64| <= 2 (rq + rk + d) 2^-24 sum_c (sum_i |q_ic|) (mean_j |k_jc|), rq / rk the rows of the two blocks (the sums of
           rq and rk addends, the mean's two roundings and the d products and sums each cost at most 2^-24 relative to the sum
           of magnitudes; the factor 2 covers the second-order terms); -inf exactly where the mask hides a block;
  lists    bit-equal to block_sparse_select_ref(..., scores=<the kernel's own scores>): given the scores the rule is exact.
The cases are those of tests/block_pattern_plan_universe.py, which tests/test_block_pattern_abi.py holds to every launch form.
Then determinism, HIP-graph replay, torch.compile, and the lists fed to flash_attn_func forward and backward against the
block-sparse oracles with the tolerances of tests/test_block_sparse_gpu.py / tests/test_block_sparse_bwd_gpu.py."""
import functools

import pytest
import torch

import block_pattern_plan_universe as U

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}


def _cute():
    from flash_attention_annotated_amd import cute_interface
    return cute_interface


def _binding():
    from flash_attention_annotated_amd import _lib
    return _lib.binding()


@functools.lru_cache(maxsize=8)
def _values(b, h, h_k, d, sq, sk, dtype, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(b, sq, h, d, generator=g).to(DTYPES[dtype]).to(DEV), torch.randn(b, sk, h_k, d, generator=g).to(DTYPES[dtype]).to(DEV)


def _laid_out(q, k, layout):
    """q and k of these values in the layout: contiguous, or views of one packed qkv buffer (b, s, h + 2 h_k, D)."""
    if layout == "contiguous":
        return q, k
    (b, sq, h, d), (sk, h_k) = q.shape, k.shape[1:3]
    buf = torch.zeros(b, max(sq, sk), h + 2 * h_k, d + (0 if layout == "packed" else 4), dtype=q.dtype, device=DEV)
    qv, kv = buf[:, :sq, :h, :d], buf[:, :sk, h:h + h_k, :d]
    qv.copy_(q), kv.copy_(k)
    assert not qv.is_contiguous() and (qv.stride(2) % 8 == 0) == U.LAYOUTS[layout]
    return qv, kv


def _plan(q, k, sel, num_blocks, mask):
    C = _cute()
    left, right = C._window(mask.get("window_size", (None, None)))
    return _binding().block_pattern_plan(q, k, *sel[:4], sel.q_block_cnt, sel.q_block_idx, sel.scores, None, num_blocks,
                                         mask.get("causal", False), left, right, 1, 1)


@functools.lru_cache(maxsize=8)
def _oracle_scores(b, h, h_k, d, sq, sk, dtype, mask, seed=0):
    """(u64 (b, h, nm, nk) from the fp64 oracle, the bound of the docstring), on the device."""
    q, k = _values(b, h, h_k, d, sq, sk, dtype, seed)
    u64 = _cute().block_sparse_select_ref(q.double(), k.double(), 2, return_scores=True, **U.MASKS[mask]).scores
    nm, nk = U.blocks(sq), U.blocks(sk)

    def pooled(x, n):
        x = torch.nn.functional.pad(x.double().abs(), (0, 0, 0, 0, 0, n * 128 - x.shape[1]))
        return x.view(b, n, 128, x.shape[2], d).sum(2)

    rq = torch.clamp(sq - torch.arange(nm, device=DEV) * 128, max=128).double()
    rk = torch.clamp(sk - torch.arange(nk, device=DEV) * 128, max=128).double()
    mags = torch.einsum("bmhc,bnhc->bhmn", pooled(q, nm), (pooled(k, nk) / rk[None, :, None, None]).repeat_interleave(h // h_k, dim=2))
    return u64, 2 * (rq[:, None] + rk[None, :] + d) * 2.0 ** -24 * mags


def _check_case(c, seed=0, values=None):
    """One call held to the oracle; returns the selection."""
    C = _cute()
    mask = U.MASKS[c.mask]
    vq, vk = values or _values(c.b, c.h, c.h_k, c.d, c.sq, c.sk, c.dtype, seed)
    q, k = _laid_out(vq, vk, c.layout)
    sel = C.block_sparse_select(q, k, c.num_blocks, with_bwd_lists=c.bwd, return_scores=True, **mask)
    assert _plan(q, k, sel, c.num_blocks, mask) == U.plan(c.b, c.sq, c.sk, c.h, c.h_k, c.d, U.LAYOUTS[c.layout], c.bwd), c
    nm, nk = U.blocks(c.sq), U.blocks(c.sk)
    assert sel.scores.shape == (c.b, c.h, nm, nk) and sel.scores.dtype == torch.float32
    if values is None:
        u64, bound = _oracle_scores(c.b, c.h, c.h_k, c.d, c.sq, c.sk, c.dtype, c.mask, seed)
        hidden = torch.isneginf(u64)
        assert torch.equal(torch.isneginf(sel.scores), hidden), c
        err = torch.where(hidden, 0.0, (sel.scores.double() - u64).abs())
        assert (err <= bound).all(), f"{c}: score error {err.max().item():.3e}, worst error / bound {(err / bound.clamp_min(1e-300)).max().item():.3f}"
    ref = C.block_sparse_select_ref(vq, vk, c.num_blocks, with_bwd_lists=c.bwd, scores=sel.scores, **mask)
    for name, got, want in zip(sel._fields[:6], sel[:6], ref[:6]):
        if want is None:
            assert got is None, (c, name)
            continue
        assert got.dtype == torch.int32 and got.shape == want.shape, (c, name)
        assert torch.equal(got, want), f"{c}: {name} differs from the oracle on the kernel's own scores"
    visible = (~torch.isneginf(sel.scores)).sum(-1)
    assert torch.equal((sel.full_block_cnt + sel.mask_block_cnt).long(), visible.clamp(max=c.num_blocks)), c
    return sel


GROUPS = sorted({(c.d, c.dtype, c.layout) for c in U.GRID_CASES})


@pytest.mark.parametrize("d,dtype,layout", GROUPS, ids=[f"d{d}-{t}-{lay}" for d, t, lay in GROUPS])
def test_scores_and_lists_over_the_grid(d, dtype, layout):
    cases = [c for c in U.GRID_CASES if (c.d, c.dtype, c.layout) == (d, dtype, layout)]
    assert len(cases) == len(U.SHAPES) * len(U.MASKS) * 2 * 3
    for c in cases:
        _check_case(c)


def test_packed_qkv_views_with_16_byte_loads():
    for c in U.PACKED_CASES:
        _check_case(c)


@pytest.mark.parametrize("c", U.LONG_CASES, ids=[f"nk{U.blocks(c.sk)}-{c.mask}-{c.num_blocks}-{c.layout}-{'bwd' if c.bwd else 'fwd'}" for c in U.LONG_CASES])
def test_many_key_blocks(c):
    sel = _check_case(c)
    assert sel.full_block_idx.max().item() < U.blocks(c.sk)


def test_a_ragged_last_key_block_goes_to_the_mask_list():
    """sk = 300, every block chosen: key blocks 0 and 1 are full, block 2 (44 keys) is not, for the ragged query block as well."""
    c = U.Case(2, 4, 2, 64, 300, 300, "bf16", "full", 3, "contiguous", False)
    sel = _check_case(c)
    assert sel.full_block_cnt.unique().tolist() == [2] and sel.mask_block_cnt.unique().tolist() == [1]
    assert sel.mask_block_idx[..., 0].unique().tolist() == [2] and sel.full_block_idx[..., :2].unique().tolist() == [0, 1]


@pytest.mark.parametrize("what", ["constant_k", "zero_q"])
@pytest.mark.parametrize("mask", sorted(U.MASKS))
def test_ties_go_to_the_lowest_indices(what, mask):
    """Equal scores in a row: the free places go to the lowest unforced indices, as the oracle's stable sort gives them."""
    b, h, h_k, d, sq, sk = 2, 4, 2, 64, 300, 1290
    q, k = _values(b, h, h_k, d, sq, sk, "bf16", seed=2)
    q, k = (q, torch.full_like(k, 0.5)) if what == "constant_k" else (torch.zeros_like(q), k)
    for nb in (2, 5, 9):
        c = U.Case(b, h, h_k, d, sq, sk, "bf16", mask, nb, "contiguous", True)
        sel = _check_case(c, values=(q, k))
        if what == "zero_q":
            assert (sel.scores[~torch.isneginf(sel.scores)] == 0).all()
        if mask == "full" and nb == 5:  # sink 0, the ties 1, 2, 3, local 10
            both = torch.cat([sel.full_block_idx[..., :4], sel.mask_block_idx[..., :1]], -1)
            assert both.unique(dim=-2).flatten().tolist() == [0, 1, 2, 3, 10] * (b * h)


def test_two_calls_give_the_same_bits():
    q, k = _values(2, 4, 2, 128, 700, 700, "bf16", seed=3)
    runs = [_cute().block_sparse_select(q, k, 3, causal=True, with_bwd_lists=True, return_scores=True) for _ in range(2)]
    for name, a, e in zip(runs[0]._fields, *runs):
        assert torch.equal(a, e), name
    without = _cute().block_sparse_select(q, k, 3, causal=True)
    assert without.q_block_cnt is None and without.q_block_idx is None and without.scores is None
    assert all(torch.equal(a, e) for a, e in zip(without[:4], runs[0][:4]))


def test_graph_replay_after_q_and_k_change():
    C = _cute()
    q, k = (t.clone() for t in _values(2, 4, 2, 64, 300, 700, "fp16", seed=4))
    q2, k2 = _values(2, 4, 2, 64, 300, 700, "fp16", seed=5)
    call = lambda: C.block_sparse_select(q, k, 3, window_size=(256, 0), with_bwd_lists=True, return_scores=True)  # noqa: E731
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        first = call()  # (warm-up outside the capture: allocator and lazy initialisation)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        sel = call()
    q.copy_(q2), k.copy_(k2)
    graph.replay()
    torch.cuda.synchronize()
    fresh = C.block_sparse_select(q2, k2, 3, window_size=(256, 0), with_bwd_lists=True, return_scores=True)
    for name, a, e in zip(sel._fields, sel, fresh):
        assert torch.equal(a, e), name
    assert not torch.equal(first.scores, fresh.scores)


def test_torch_compile_fullgraph():
    C = _cute()
    q, k = _values(2, 4, 2, 64, 300, 700, "bf16", seed=6)

    def select(q, k):
        sel = C.block_sparse_select(q, k, 3, causal=True, with_bwd_lists=True)
        return sel.full_block_cnt + sel.mask_block_cnt, sel.mask_block_idx, sel.q_block_idx

    got = torch.compile(select, backend="aot_eager", fullgraph=True)(q, k)
    for a, e in zip(got, select(q, k)):
        assert torch.equal(a, e)


# ---- end to end: the lists feed the block-sparse forward and backward ---------------------------------------------------------
def _end_to_end(num_blocks):
    import test_block_sparse_bwd_gpu as bwd_t
    import test_block_sparse_gpu as fwd_t
    C = _cute()
    gen = torch.Generator().manual_seed(7)
    q, k, v, g = (torch.randn(1, 640, heads, 64, generator=gen).to(torch.bfloat16) for heads in (4, 2, 2, 4))
    leaves = [t.to(DEV).requires_grad_(True) for t in (q, k, v)]
    sel = C.block_sparse_select(leaves[0].detach(), leaves[1].detach(), num_blocks, causal=True, with_bwd_lists=True)
    out, lse = C.flash_attn_func(*leaves, causal=True, **{n: t for n, t in sel._asdict().items() if n != "scores"})
    grads = [t.detach().cpu() for t in torch.autograd.grad(out, leaves, g.to(DEV))]
    torch.cuda.synchronize()
    lists = tuple(t.cpu() for t in sel[:4])
    ref, pt, lse_ref = fwd_t._oracle(q, k, v, lists, causal=True)
    fwd_t._check(out.detach(), lse.detach(), ref, pt, lse_ref, f"end to end, num_blocks {num_blocks}")
    g_ref, g_pt = bwd_t._oracle((q, k, v, g), lists, causal=True)
    bwd_t._check(grads, g_ref, g_pt, f"end to end, num_blocks {num_blocks}")
    return sel, (q, k, v, g), (out.detach(), lse.detach(), grads), (ref, pt, lse_ref, g_ref, g_pt)


def test_lists_feed_forward_and_backward():
    sel, *_ = _end_to_end(3)
    assert (sel.full_block_cnt + sel.mask_block_cnt)[0, 0].tolist() == [1, 2, 3, 3, 3]
    assert torch.equal(sel.mask_block_idx[0, :, :, 0], torch.arange(5, device=DEV, dtype=torch.int32).expand(4, 5))  # the diagonal


def test_every_block_chosen_is_the_dense_causal_call():
    import test_block_sparse_bwd_gpu as bwd_t
    import test_block_sparse_gpu as fwd_t
    C = _cute()
    sel, (q, k, v, g), (out, lse, grads), (ref, pt, lse_ref, g_ref, g_pt) = _end_to_end(5)
    assert (sel.full_block_cnt + sel.mask_block_cnt)[0, 0].tolist() == [1, 2, 3, 4, 5]
    leaves = [t.to(DEV).requires_grad_(True) for t in (q, k, v)]
    dense, dense_lse = C.flash_attn_func(*leaves, causal=True)
    dense_grads = [t.detach().cpu() for t in torch.autograd.grad(dense, leaves, g.to(DEV))]
    # the oracle of the full lists is dense causal attention: the dense call passes the same check against it
    fwd_t._check(dense.detach(), dense_lse.detach(), ref, pt, lse_ref, "the dense causal call")
    bwd_t._check(dense_grads, g_ref, g_pt, "the dense causal call")
