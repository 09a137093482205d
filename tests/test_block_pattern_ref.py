"""CPU tests of cute_interface.block_sparse_select_ref, the torch oracle of the block-sparse prefill pattern
(include/fa_block_pattern.h states the rule): against a brute-force reading of the rule in Python loops over elements and blocks,
the tie rule, the degenerate choices, the rows without a visible block, and the key-major lists.  Nothing here touches a device;
tests/test_block_pattern_gpu.py holds the kernels to this oracle."""
import numpy as np
import pytest
import torch

from flash_attention_annotated_amd import cute_interface as cute

B = 128
MASKS = {"full": dict(), "causal": dict(causal=True), "window": dict(window_size=(256, 0))}
SHAPES = ((300, 300), (200, 700), (700, 200))


def element_mask(sq, sk, causal=False, window_size=(None, None)):
    """(sq, sk) bool: row i sees key j, bottom-right aligned."""
    left, right = window_size
    if causal:
        right = 0
    i, j = np.arange(sq)[:, None], np.arange(sk)[None, :]
    ok = np.ones((sq, sk), bool)
    if left is not None:
        ok &= j >= i + sk - sq - left
    if right is not None:
        ok &= j <= i + sk - sq + right
    return ok


def brute_force(q, k, num_blocks, sink_blocks=1, local_blocks=1, **mask):
    """The rule, block by block: (chosen (b, h, nm, nk) bool, full (nm, nk) bool, visible (nm, nk) bool, u (b, h, nm, nk) fp64)."""
    b, sq, h, d = q.shape
    sk, h_k = k.shape[1:3]
    nm, nk, g = -(-sq // B), -(-sk // B), h // h_k
    ok = element_mask(sq, sk, **mask)
    visible, full = np.zeros((nm, nk), bool), np.zeros((nm, nk), bool)
    for m in range(nm):
        for n in range(nk):
            tile = ok[m * B:(m + 1) * B, n * B:(n + 1) * B]
            visible[m, n] = tile.any()
            full[m, n] = tile.all() and (n + 1) * B <= sk  # a ragged last key block needs the seqlen_k bound: never full
    qn, kn = q.double().numpy(), k.double().numpy()
    u = np.full((b, h, nm, nk), -np.inf)
    chosen = np.zeros((b, h, nm, nk), bool)
    for bi in range(b):
        for hi in range(h):
            for m in range(nm):
                qs = qn[bi, m * B:(m + 1) * B, hi].sum(0)
                V = [n for n in range(nk) if visible[m, n]]
                for n in V:
                    u[bi, hi, m, n] = qs @ kn[bi, n * B:(n + 1) * B, hi // g].mean(0)
                K = min(num_blocks, len(V))
                forced = set(V[:min(sink_blocks, len(V))]) | set(V[len(V) - min(local_blocks, len(V)):])
                others = sorted((n for n in V if n not in forced), key=lambda n: (-u[bi, hi, m, n], n))
                for n in list(forced) + others[:K - len(forced)]:
                    chosen[bi, hi, m, n] = True
    return chosen, full, visible, u


def lists_of(chosen, full):
    """The four forward lists of a chosen set, written out by hand."""
    b, h, nm, nk = chosen.shape
    out = [np.zeros((b, h, nm), np.int32), np.zeros((b, h, nm, nk), np.int32), np.zeros((b, h, nm), np.int32), np.zeros((b, h, nm, nk), np.int32)]
    for bi, hi, m in np.ndindex(b, h, nm):
        for n in range(nk):
            if chosen[bi, hi, m, n]:
                cnt, idx = (out[0], out[1]) if full[m, n] else (out[2], out[3])
                idx[bi, hi, m, cnt[bi, hi, m]] = n
                cnt[bi, hi, m] += 1
    return out


def inputs(sq, sk, b=1, h=2, h_k=1, d=16, seed=0):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(b, sq, h, d, generator=gen, dtype=torch.float64), torch.randn(b, sk, h_k, d, generator=gen, dtype=torch.float64)


@pytest.mark.parametrize("mask", sorted(MASKS))
@pytest.mark.parametrize("sq,sk", SHAPES)
@pytest.mark.parametrize("num_blocks", (2, 3))
def test_against_the_rule_read_by_loops(sq, sk, mask, num_blocks):
    q, k = inputs(sq, sk)
    chosen, full, visible, u = brute_force(q, k, num_blocks, **MASKS[mask])
    got = cute.block_sparse_select_ref(q, k, num_blocks, with_bwd_lists=True, return_scores=True, **MASKS[mask])
    vis, ful = cute.block_sparse_visibility(sq, sk, **MASKS[mask])
    assert np.array_equal(vis.numpy(), visible) and np.array_equal(ful.numpy(), full & visible)
    assert got.scores.dtype == torch.float64
    assert np.array_equal(np.isneginf(got.scores.numpy()), ~np.broadcast_to(visible, u.shape))
    seen = np.broadcast_to(visible, u.shape)
    assert np.allclose(got.scores.numpy()[seen], u[seen], rtol=1e-12, atol=1e-12)
    for a, e in zip(got[:4], lists_of(chosen, full)):
        assert a.dtype == torch.int32 and np.array_equal(a.numpy(), e)
    # the counts: K = min(num_blocks, |V|) per row
    assert np.array_equal((got.full_block_cnt + got.mask_block_cnt).numpy()[0, 0], np.minimum(visible.sum(1), num_blocks))


def test_a_ragged_last_key_block_is_never_full():
    """sk = 300, no mask: blocks 0 and 1 are full, block 2 (44 keys) goes to the mask list, whatever its score."""
    q, k = inputs(300, 300)
    got = cute.block_sparse_select_ref(q, k, 3)
    assert got.full_block_cnt.unique().tolist() == [2] and got.mask_block_cnt.unique().tolist() == [1]
    assert got.full_block_idx[..., :2].unique().tolist() == [0, 1] and got.mask_block_idx[..., 0].unique().tolist() == [2]
    # a ragged last QUERY block may be full: block row 2 of sq = 300 over the complete key blocks of sk = 256
    _, full = cute.block_sparse_visibility(300, 256)
    assert full.all()


def test_ties_go_to_the_lowest_indices():
    """All keys equal: every score of a row is the same number, so the unforced places go to the lowest unforced indices; -0
    equals +0."""
    q = torch.randint(-3, 4, (1, 256, 2, 16), generator=torch.Generator().manual_seed(1)).double()  # (sums exact in any order)
    k = torch.ones(1, 1280, 1, 16, dtype=torch.float64)
    got = cute.block_sparse_select_ref(q, k, 5, sink_blocks=1, local_blocks=1)
    assert got.full_block_cnt.unique().tolist() == [5]
    assert got.full_block_idx[..., :5].unique(dim=-2).tolist() == [[[[0, 1, 2, 3, 9]]] * 2]
    zero = cute.block_sparse_select_ref(torch.zeros_like(q), k, 5, scores=torch.tensor([0.0, -0.0] * 5).expand(1, 2, 2, 10))
    assert zero.full_block_idx[..., :5].unique(dim=-2).tolist() == [[[[0, 1, 2, 3, 9]]] * 2]
    first = cute.block_sparse_select_ref(q, k, 4, sink_blocks=0, local_blocks=0, causal=True)
    assert first.mask_block_cnt.unique().tolist() == [0] and first.full_block_cnt.unique().tolist() == [4]
    assert first.full_block_idx[..., :4].unique(dim=-2).tolist() == [[[[0, 1, 2, 3]]] * 2]


def test_more_places_than_blocks_lists_every_visible_block():
    for mask in MASKS.values():
        q, k = inputs(300, 700)
        visible, full = cute.block_sparse_visibility(300, 700, **mask)
        for num_blocks in (6, 10):
            got = cute.block_sparse_select_ref(q, k, num_blocks, **mask)
            want = cute.block_sparse_from_mask(visible.expand(1, 2, 3, 6), full.expand(1, 2, 3, 6))
            assert all(torch.equal(a, e) for a, e in zip(got[:4], want))


def test_only_forced_blocks():
    """sink_blocks + local_blocks == num_blocks: the scores decide nothing."""
    q, k = inputs(700, 700)
    got = cute.block_sparse_select_ref(q, k, 3, causal=True, sink_blocks=1, local_blocks=2)
    again = cute.block_sparse_select_ref(-q, k, 3, causal=True, sink_blocks=1, local_blocks=2)
    assert all(torch.equal(a, e) for a, e in zip(got[:4], again[:4]))
    assert got.full_block_idx[0, 0, 5, :2].tolist() == [0, 4] and got.mask_block_idx[0, 0, 5, 0].item() == 5
    assert got.full_block_cnt[0, 0].tolist() == [0, 1, 2, 2, 2, 2] and got.mask_block_cnt[0, 0].tolist() == [1] * 6
    with pytest.raises(ValueError):
        cute.block_sparse_select_ref(q, k, 2, sink_blocks=1, local_blocks=2)


def test_rows_without_a_visible_block_have_counts_of_zero():
    """sq = 700 > sk = 200, causal: rows 0 .. 499 see no key, so query blocks 0 .. 2 list nothing."""
    q, k = inputs(700, 200)
    got = cute.block_sparse_select_ref(q, k, 2, causal=True, with_bwd_lists=True, return_scores=True)
    total = got.full_block_cnt + got.mask_block_cnt
    assert total[0, 0].tolist() == [0, 0, 0, 1, 2, 2]
    assert torch.isneginf(got.scores[:, :, :3]).all()
    assert (got.full_block_idx[:, :, :3] == 0).all() and (got.mask_block_idx[:, :, :3] == 0).all()
    assert got.q_block_cnt[0, 0].tolist() == [3, 2] and got.q_block_idx[0, 0, 0, :3].tolist() == [3, 4, 5]


@pytest.mark.parametrize("mask", sorted(MASKS))
def test_key_major_lists_are_those_of_block_sparse_bwd_lists(mask):
    q, k = inputs(700, 520, b=2)
    got = cute.block_sparse_select_ref(q, k, 3, with_bwd_lists=True, **MASKS[mask])
    cnt, idx = cute.block_sparse_bwd_lists(*got[:4])
    assert torch.equal(got.q_block_cnt, cnt) and torch.equal(got.q_block_idx, idx)
    assert got.q_block_cnt.shape == (2, 2, 5) and got.q_block_idx.shape == (2, 2, 5, 6) and got.q_block_idx.dtype == torch.int32
    chosen = brute_force(q, k, 3, **MASKS[mask])[0]
    for bi, hi, n in np.ndindex(2, 2, 5):
        rows = np.flatnonzero(chosen[bi, hi, :, n]).tolist()
        assert got.q_block_cnt[bi, hi, n].item() == len(rows) and got.q_block_idx[bi, hi, n, :len(rows)].tolist() == rows
    without = cute.block_sparse_select_ref(q, k, 3, **MASKS[mask])
    assert without.q_block_cnt is None and without.q_block_idx is None and without.scores is None


def test_given_scores_replace_the_pooled_ones():
    q, k = inputs(300, 700)
    scores = torch.arange(6.0).expand(1, 2, 3, 6).contiguous()
    got = cute.block_sparse_select_ref(q, k, 3, scores=scores, sink_blocks=0, local_blocks=0)
    assert got.full_block_idx[..., :2].unique().tolist() == [3, 4] and got.mask_block_idx[..., 0].unique().tolist() == [5]
    # fp32 inputs are pooled in fp32; the public call takes the oracle for CPU tensors
    sel = cute.block_sparse_select(q.float(), k.float(), 3, return_scores=True)
    ref = cute.block_sparse_select_ref(q.float(), k.float(), 3, return_scores=True)
    assert sel.scores.dtype == torch.float32 and all(torch.equal(a, e) for a, e in zip(sel[:4], ref[:4]))
