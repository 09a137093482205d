"""GPU tests of the prefill-sized lightning indexer over an e4m3 index-key cache (hopper_interface.kvcache_index_topk_prefill(
k_index_scale=)) against the fp64 oracle index_topk_prefill_ref run on the CPU on the dequantised keys, and against the decode
entry kvcache_index_topk(k_index_scale=).  The exact data is test_index_topk8_gpu's (its header derives the 21 bits): every logit is
exact in fp32 in any order, the power-of-two scale is exact, and keys from six prototypes make ties at the cut the rule."""
import pytest
import torch
from test_index_topk8_gpu import BF, DEV, EPS, F8, FP, SENTINEL, _layout
from test_index_prefill_gpu import _same_logits  # (logits[b, i, :n] bit for bit, the sentinel at and behind n)
from test_index_topk_gpu import _tie_at_the_cut, _visible

from flash_attention_annotated_amd import _lib, hopper_interface as H

pytestmark = pytest.mark.gpu
BLOCK, TILE = _lib.FA_INDEX_PREFILL_BLOCK, _lib.FA_INDEX_PREFILL8_TILE


def _exact(b, s_q, h_i, d_i, cap, seed):
    """test_index_topk8_exact's data: (q, key bytes' values as e4m3, scales, weights) on the CPU."""
    g = torch.Generator().manual_seed(seed)
    q = (torch.randint(-16, 17, (b, s_q, h_i, d_i), generator=g).float() / 4).to(BF)
    w = torch.randint(-4, 5, (b, s_q, h_i), generator=g).float() / 2
    proto, proto_scale = torch.randint(-4, 5, (b, 6, d_i), generator=g).float(), 2.0 ** -torch.randint(1, 4, (b, 6), generator=g).float()
    pick = torch.randint(0, 6, (b, cap), generator=g)
    return q, torch.gather(proto, 1, pick[..., None].expand(b, cap, d_i)).to(F8), torch.gather(proto_scale, 1, pick), w


def _run(q, w, fills, topk, cache, causal=True, rows=0):
    """The call on sentinel-filled buffers 3 / 5 wider than needed (rows = 0: a workspace of one round) and its plan.  cache:
    (store, scales, kw) on the device.  indices and the logits view (zeros where the workspace does not hold every row) on the CPU."""
    (b, s_q), (store, scales, kw) = q.shape[:2], cache
    cap = kw["page_table"].shape[1] * store.shape[1] if kw["page_table"] is not None else store.shape[1]
    idx = torch.full((b, s_q, 1, topk + 3), SENTINEL, dtype=torch.int32, device=DEV)
    work = torch.full((rows or b * -(-s_q // BLOCK) * BLOCK, cap + 5), float(SENTINEL), dtype=torch.float32, device=DEV)
    args = (q.to(DEV), store.view(F8), w.to(DEV), fills.to(DEV), topk)
    got = H.kvcache_index_topk_prefill(*args, **kw, causal=causal, indices=idx, workspace=work, return_logits=not rows, k_index_scale=scales)
    plan = _lib.binding().kvcache_index_topk_prefill_fp8_plan(*args[:2], scales, *args[2:], *kw.values(), causal, idx, work)
    idx, logits = idx.cpu(), got[1].cpu() if not rows else torch.zeros(b, s_q, cap + 5)
    assert torch.all(idx[..., topk:] == SENTINEL) and torch.all(work[:, cap:] == SENTINEL), "written outside [0, topk) / [0, capacity)"
    return idx[..., :topk], logits[..., :cap], plan


def _exact_cache(k8, scale, form):
    store, scales, entry, row, _, kw = _layout(*k8.shape, form)
    store[entry, row], scales[entry, row] = k8.view(torch.uint8), scale
    return store.to(DEV), scales.to(DEV), kw


@pytest.mark.parametrize("form", ["dense", "p16", "p256"])
@pytest.mark.parametrize("s_q", [17, 2 * BLOCK + 3])
@pytest.mark.parametrize("d_i,h_i", [(64, 16), (128, 48), (128, 64)])
def test_index_prefill8_exact(d_i, h_i, s_q, form):
    """Capacity 768 = 3 chunks of 256 = 6 tiles of 128; three token blocks, the last one short; fill levels around the 32-key
    blocks and the tile, s_q - 1 (the first token sees nothing), 2 chunks + 1 and capacity + 5 (clamped) in one batch."""
    cap, fills = 768, torch.tensor([0, 1, 63, 65, 127, 129, s_q - 1, 2 * 256 + 1, 768 + 5], dtype=torch.int32)
    q, k8, scale, w = _exact(len(fills), s_q, h_i, d_i, cap, seed=d_i + s_q)
    cache, keys, ties = _exact_cache(k8, scale, form), k8.float() * scale[..., None], []
    for causal in (True, False):
        for topk in (1, 64, 100):
            ref = H.index_topk_prefill_ref(q, keys, w, fills, topk, causal=causal)
            idx, logits, plan = _run(q, w, fills, topk, cache, causal)
            assert plan == (f"index_logits_prefill8_kernel d={d_i} heads={h_i} sq={s_q} block={BLOCK} tile={TILE} chunk=256 grid=81 | "
                            f"index_select_prefill_kernel threads=256 passes=4 grid={9 * 3 * BLOCK} | rounds=1")
            _same_logits(logits, ref.logits, fills, causal)
            assert torch.equal(idx, ref.indices), (topk, causal)
            ties.append(_tie_at_the_cut(ref, fills, topk, causal))
    assert any(ties), "ties at the cut are the rule here by construction"


def test_index_prefill8_rounds_give_the_same_lists():
    """The least workspace (one token block a round: 27 rounds) against one round."""
    fills = torch.tensor([0, 1, 63, 65, 127, 129, 18, 513, 773], dtype=torch.int32)
    q, k8, scale, w = _exact(len(fills), 19, 64, 128, 768, seed=5)
    cache = _exact_cache(k8, scale, "p16")
    ref = H.index_topk_prefill_ref(q, k8.float() * scale[..., None], w, fills, 64)
    one, _, plan_one = _run(q, w, fills, 64, cache)
    many, _, plan_many = _run(q, w, fills, 64, cache, rows=BLOCK)
    assert torch.equal(one, many) and torch.equal(one, ref.indices)
    assert plan_one.endswith("grid=81 | index_select_prefill_kernel threads=256 passes=4 grid=216 | rounds=1")
    assert plan_many.endswith("grid=3 | index_select_prefill_kernel threads=256 passes=4 grid=8 | rounds=27")


def _appended(dtype, s_q, seed, b=3, h_i=64, d_i=128, cap=1024):
    """Normal data over randn rows that went through kvcache_index_append_fp8 into pages of 64 (one ragged append, fills 1024 / 517 /
    90): (q, w, fills, cache, table, what the cache holds) -- the rows behind a fill level are not read."""
    torch.manual_seed(seed)
    q, k, w = torch.randn(b, s_q, h_i, d_i).to(dtype), torch.randn(b, cap, d_i).to(dtype), torch.randn(b, s_q, h_i) * h_i ** -0.5
    fills = torch.tensor([cap, 517, 90], dtype=torch.int32)
    store, scales, _, _, table, kw = _layout(b, cap, d_i, "p64")
    store, scales = store.to(DEV), scales.to(DEV)
    cu = torch.cat([torch.zeros(1, dtype=torch.int32), fills.cumsum(0).int()]).to(DEV)
    H.kvcache_index_append_fp8(store.view(F8), scales, torch.cat([k[e, :fills[e]] for e in range(b)]).to(DEV),
                               torch.zeros(b, dtype=torch.int32, device=DEV), cu_seqlens_k_new=cu, page_table=kw["page_table"])
    return q, w, fills, (store, scales, kw), table, store.cpu().view(F8).float() * scales.cpu()[..., None]


@pytest.mark.parametrize("dtype", [BF, FP])
def test_index_prefill8_is_bit_equal_to_the_decode_entry(dtype):
    """16 tokens, h_i 64, d_i 128, pages of 64: logits[:n] and indices are kvcache_index_topk(k_index_scale=)'s, bit for bit."""
    q, w, fills, cache, _, _ = _appended(dtype, 16, seed=4)
    want_idx, want = H.kvcache_index_topk(q.to(DEV), cache[0].view(F8), w.to(DEV), fills.to(DEV), 128, k_index_scale=cache[1],
                                          page_table=cache[2]["page_table"], return_logits=True)
    idx, logits, _ = _run(q, w, fills, 128, cache)
    _same_logits(logits, want.cpu(), fills)
    assert torch.equal(idx, want_idx.cpu())


def test_index_prefill8_normal_data():
    """40 tokens.  Every logit within (d_i + h_i + 1) 2^-24 A of the fp64 logit on the dequantised cache contents (A from the oracle;
    + 1: the multiply by the scale), the bound test_index_topk8_normal_data_through_both_kernels derives, and a chosen set that is
    valid under twice that slack.  The worst ratio is printed; measured on MI355X: 0.001."""
    (b, s_q, h_i, d_i), cap, topk = (3, 40, 64, 128), 1024, 128
    q, w, fills, cache, table, keys = _appended(BF, s_q, seed=3)
    ref = H.index_topk_prefill_ref(q, keys, w, fills, topk, page_table=table)
    idx, logits, _ = _run(q, w, fills, topk, cache)
    worst = 0.0
    for e, i in ((e, i) for e in range(b) for i in range(s_q)):
        n = _visible(fills[e], cap, s_q, i)
        l32, l64, bound = logits[e, i, :n].double(), ref.logits[e, i, :n], (d_i + h_i + 1) * EPS * ref.A[e, i, :n]
        worst = max(worst, float(((l32 - l64).abs() / bound).max()))
        K = min(topk, n)
        got = idx[e, i, 0, :K].tolist()
        assert got == sorted(set(got)) and all(0 <= j < n for j in got) and torch.all(idx[e, i, 0, K:] == -1)
        if K < n:
            cut, slack = torch.sort(l64, descending=True).values[K - 1], 2 * bound.amax()
            assert torch.all(l64[got] >= cut - slack) and torch.all(l64[sorted(set(range(n)) - set(got))] <= cut + slack)
    print(f"index prefill8 logits: worst |l32 - l64| / ((d_i + h_i + 1) 2^-24 A) = {worst:.3f}")
    assert worst <= 1.0


def test_index_prefill8_replays_in_a_graph():
    """2 x 19 tokens = 6 token blocks on a workspace of 3: two rounds, captured once on one stream; replayed after the fill levels
    grew by one it equals the eager call and the oracle at the new levels."""
    b, s_q, cap, topk = 2, 19, 512, 96
    q, k8, scale, w = _exact(b, s_q, 16, 64, cap, seed=2)
    store, scales, kw = _exact_cache(k8, scale, "p64")
    fills, keys = torch.tensor([130, 383], dtype=torch.int32), k8.float() * scale[..., None]
    q_dev, w_dev, lens = q.to(DEV), w.to(DEV), fills.to(DEV)
    idx = torch.empty((b, s_q, 1, topk), dtype=torch.int32, device=DEV)
    work = torch.empty((3 * BLOCK, cap), dtype=torch.float32, device=DEV)

    def step():
        H.kvcache_index_topk_prefill(q_dev, store.view(F8), w_dev, lens, topk, **kw, indices=idx, workspace=work, k_index_scale=scales)

    step()  # (also the warm-up outside the capture)
    before = idx.cpu()
    assert torch.equal(before, H.index_topk_prefill_ref(q, keys, w, fills, topk).indices)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    lens.add_(1)
    for _ in range(3):
        graph.replay()
        replayed = idx.clone()
        step()
        assert torch.equal(replayed, idx)
    assert torch.equal(idx.cpu(), H.index_topk_prefill_ref(q, keys, w, fills + 1, topk).indices) and not torch.equal(idx.cpu(), before)
