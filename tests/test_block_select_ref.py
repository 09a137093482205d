"""CPU tests of the torch oracles of the block summaries and the Quest block selection (hopper_interface.block_summary_ref /
select_blocks_ref, the rule of include/fa_block_select.h): hand-made cases of the list format, the Quest property in fp64, the tie
rule, incremental update against rebuild, and the CPU route of the two public calls.  No device, no library."""
import pytest
import torch

from flash_attention_annotated_amd import hopper_interface as H

BF = torch.bfloat16


def _summary(max_blocks, h_k=1, d=16, seed=0, slots=1):
    """A valid summary (min <= max) of multiples of 1/4"""
    g = torch.Generator().manual_seed(seed)
    a = torch.randint(-16, 17, (slots, max_blocks, 2, h_k, d), generator=g).float() / 4
    return torch.stack((a.amin(2), a.amax(2)), 2).to(BF)


def _q(b=1, s_q=1, h=1, d=16, seed=1):
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(-16, 17, (b, s_q, h, d), generator=g).float() / 4).to(BF)


def _lists(r, b=0, hk=0):
    return int(r.cnt[b, hk]), r.idx[b, hk].tolist()


def test_list_format_by_hand():
    """One kv head, d = 16, scores set by hand: q = e_0, so U of block j is max(min_0, max_0) = max_0 of the block."""
    s = torch.zeros(1, 8, 2, 1, 16, dtype=BF)
    s[0, :, 1, 0, 0] = torch.tensor([1.0, 7.0, 3.0, 7.0, 5.0, 2.0, 9.0, 4.0])
    s[0, :, 0, 0, 0] = -1.0
    q = torch.zeros(1, 1, 1, 16, dtype=BF)
    q[..., 0] = 1.0
    sel = lambda fill, k, **kw: _lists(H.select_blocks_ref(q, s, torch.tensor([fill], dtype=torch.int32), k, kv_block_size=64, width=6, **kw))
    assert sel(0, 4) == (0, [-1] * 6)                                            # n = 0
    assert sel(1, 4) == (1, [0, -1, -1, -1, -1, -1])                             # n = 1
    assert sel(2 * 64, 4) == (2, [0, 1, -1, -1, -1, -1])                         # n = sink + local
    assert sel(3 * 64, 5, sink_blocks=2, local_blocks=3) == (3, [0, 1, 2, -1, -1, -1])  # n < sink + local
    assert sel(4 * 64 - 5, 4) == (4, [0, 1, 2, 3, -1, -1])                       # n = K
    # forced 0 and 7; the free blocks 1..6 score 7, 3, 7, 5, 2, 9: two places go to 6 (9.0) and 1 (7.0, the lower index of the tie)
    assert sel(8 * 64, 4) == (4, [0, 1, 6, 7, -1, -1])
    r = H.select_blocks_ref(q, s, torch.tensor([8 * 64], dtype=torch.int32), 4, kv_block_size=64)
    assert _lists(r) == (4, [0, 1, 6, 7])
    assert r.scores[0, 0].tolist() == [1.0, 7.0, 3.0, 7.0, 5.0, 2.0, 9.0, 4.0] and r.scores.dtype == torch.float64
    r = H.select_blocks_ref(q, s, torch.tensor([8 * 64], dtype=torch.int32), 5, kv_block_size=64)
    assert _lists(r) == (5, [0, 1, 3, 6, 7])
    r = H.select_blocks_ref(q, s, torch.tensor([5 * 64 + 1], dtype=torch.int32), 3, kv_block_size=64, sink_blocks=0, local_blocks=0)
    assert _lists(r) == (3, [1, 3, 4]) and r.scores[0, 0, 6:].tolist() == [float("-inf")] * 2  # n = 6: block 6 is not filled
    r = H.select_blocks_ref(q, s, torch.tensor([10 ** 6], dtype=torch.int32), 8, kv_block_size=64)  # clamped to max_blocks * B
    assert _lists(r) == (8, list(range(8)))


def test_tie_rule_on_an_all_equal_row():
    s = torch.ones(1, 12, 2, 2, 16, dtype=BF)
    s[:, :, 0] = -0.0  # min = -0, max = 1; a q of zeros gives +-0 everywhere: -0 equals +0
    for q in (torch.ones(1, 2, 4, 16, dtype=BF), torch.zeros(1, 2, 4, 16, dtype=BF), -torch.zeros(1, 2, 4, 16, dtype=BF)):
        for reduce in ("max", "sum"):
            r = H.select_blocks_ref(q, s, torch.tensor([12 * 128], dtype=torch.int32), 6, group_reduce=reduce, sink_blocks=1, local_blocks=2)
            for hk in range(2):
                assert _lists(r, 0, hk) == (6, [0, 1, 2, 3, 10, 11])


@pytest.mark.parametrize("reduce", ["max", "sum"])
def test_quest_property(reduce):
    """U >= the largest q . k over the block's filled keys, for every row, in fp64; so is the reduced score of the reduced q . k"""
    torch.manual_seed(3)
    b, cap, h, h_k, d, B, s_q = 2, 512, 8, 2, 64, 64, 3
    g = h // h_k
    k = torch.randn(b, cap, h_k, d).to(BF)
    q = torch.randn(b, s_q, h, d).to(BF)
    fills = torch.tensor([200, 453], dtype=torch.int32)
    s = torch.full((b, cap // B, 2, h_k, d), 99.0, dtype=BF)
    H.block_summary_ref(s, k, None, fills, kv_block_size=B)
    r = H.select_blocks_ref(q, s, fills, 4, kv_block_size=B, group_reduce=reduce)
    for i in range(b):
        n = -(-int(fills[i]) // B)
        assert torch.all(r.scores[i, :, n:] == float("-inf")) and torch.all(r.U[i, :, :, n:] == 0)
        for hk in range(h_k):
            rows = q[i, :, hk * g:(hk + 1) * g].reshape(s_q * g, d).double()
            dots = rows @ k[i, :int(fills[i]), hk].double().T  # (rows, keys)
            for j in range(n):
                best = dots[:, j * B:(j + 1) * B].amax(1)
                assert torch.all(r.U[i, hk, :, j] >= best), (i, hk, j)
                assert torch.all(r.A[i, hk, :, j] >= r.U[i, hk, :, j].abs())
                assert r.scores[i, hk, j] >= (best.amax() if reduce == "max" else best.sum())


@pytest.mark.parametrize("form", ["dense", "p16", "p64"])
@pytest.mark.parametrize("cache", ["bf16", "e4m3"])
def test_incremental_update_equals_rebuild(form, cache):
    torch.manual_seed(4)
    b, cap, h_k, d, B = 3, 512, 2, 32, 128
    logical = torch.randn(b, cap, h_k, d)
    logical = logical.to(torch.float8_e4m3fn) if cache == "e4m3" else logical.to(BF)
    batch_idx = table = None
    if form == "dense":
        batch_idx = torch.tensor([3, 0, 2], dtype=torch.int32)
        store = torch.zeros(4, cap, h_k, d).to(logical.dtype)
        store.view(torch.uint8)[batch_idx.long()] = logical.view(torch.uint8)
        slots = 4
    else:
        page = int(form[1:])
        per = cap // page
        table = torch.randperm(b * per + 2)[:b * per].to(torch.int32).view(b, per)
        store = torch.zeros(b * per + 2, page, h_k, d).to(logical.dtype)
        store.view(torch.uint8)[table.flatten().long()] = logical.view(torch.uint8).reshape(b * per, page, h_k, -1)
        slots = b
    kw = dict(kv_block_size=B, cache_batch_idx=batch_idx, page_table=table)
    s = torch.full((slots, cap // B, 2, h_k, d), 77.0, dtype=BF)
    fills = torch.tensor([200, 0, 127], dtype=torch.int32)
    H.kvcache_block_summary_update(s, store, None, fills, **kw)  # (CPU tensors: the oracle)
    for step in (1, 1, 70, 1, 0):
        new = fills + torch.tensor([step, step, 2 * step], dtype=torch.int32)
        before = s.clone()
        H.block_summary_ref(s, store, fills, new, **kw)
        want = H.block_summary_ref(torch.full_like(s, 77.0), store, None, new, **kw)
        assert torch.equal(s, want), (step, fills)
        for i in range(b):  # blocks outside the range are what they were
            slot = i if batch_idx is None else int(batch_idx[i])
            lo, hi = int(fills[i]) // B, -(-int(new[i]) // B) if new[i] > fills[i] else 0
            keep = [j for j in range(cap // B) if not lo <= j < hi]
            assert torch.equal(s[slot, keep], before[slot, keep])
        fills = new
    # by hand: entry 0 holds 273 rows: block 0 and 1 full, block 2 of 17 rows, block 3 the sentinel
    slot = 0 if batch_idx is None else 3
    assert int(fills[0]) == 273
    rows = logical[0].float()
    assert torch.equal(s[slot, 2, 0].float(), rows[256:273].amin(0)) and torch.equal(s[slot, 1, 1].float(), rows[128:256].amax(0))
    assert torch.all(s[slot, 3] == 77.0)


def test_cpu_tensors_take_the_oracle():
    s, q = _summary(10, h_k=2, seed=5, slots=2), _q(b=2, s_q=2, h=4, seed=6)
    fills = torch.tensor([10 * 128, 300], dtype=torch.int32)
    cnt, idx, scores = H.kvcache_select_blocks(q, s, fills, 4, return_scores=True)
    r = H.select_blocks_ref(q, s, fills, 4)
    assert torch.equal(cnt, r.cnt) and torch.equal(idx, r.idx) and torch.equal(scores.double(), r.scores)
    assert cnt.dtype == idx.dtype == torch.int32 and scores.dtype == torch.float32 and idx.shape == (2, 2, 4)
    assert cnt.tolist() == [[4, 4], [3, 3]] and idx[1, 0].tolist() == [0, 1, 2, -1]
    buf_c, buf_i = torch.zeros(2, 2, dtype=torch.int32), torch.zeros(2, 2, 9, dtype=torch.int32)
    out = H.kvcache_select_blocks(q, s, fills, 4, kv_block_cnt=buf_c, kv_block_idx=buf_i, cache_batch_idx=torch.tensor([1, 0], dtype=torch.int32))
    assert out[0] is buf_c and out[1] is buf_i and torch.all(buf_i[:, :, 4:] == -1)
    r = H.select_blocks_ref(q, s.flip(0), fills, 4)
    assert torch.equal(buf_i[:, :, :4], r.idx)


@pytest.mark.parametrize("kw", [dict(kv_block_size=96), dict(group_reduce="mean"), dict(sink_blocks=3, local_blocks=2), dict(width=3)])
def test_oracle_refusals(kw):
    with pytest.raises(AssertionError):
        H.select_blocks_ref(_q(), _summary(4), torch.tensor([100], dtype=torch.int32), 4, **kw)
