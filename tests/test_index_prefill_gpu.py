"""GPU tests of the prefill-sized lightning indexer (hopper_interface.kvcache_index_topk_prefill) against the fp64 oracle
index_topk_prefill_ref run on the CPU, and against the decode entry.  The exact data is test_index_topk_gpu's: multiples of 1/4
and 1/2, keys from a few prototypes, so that every logit is exact in fp32 in any order and ties at the cut are the rule."""
import pytest
import torch

from flash_attention_annotated_amd import _lib, hopper_interface as H
from test_index_topk_gpu import BF, DEV, EPS, FP, SENTINEL, _exact_inputs, _store, _tie_at_the_cut, _visible

pytestmark = pytest.mark.gpu
BLOCK = _lib.FA_INDEX_PREFILL_BLOCK


def _run(q, k, w, fills, topk, form="dense", causal=True, rows=0, ref=None):
    """The call on sentinel-filled buffers 3 / 5 wider than needed (rows = 0: a workspace of one round), its plan, and the
    oracle (`ref` where the caller has one or compares with something else).  indices and the logits view (zeros where the
    workspace does not hold every row) on the CPU."""
    (b, s_q), cap = q.shape[:2], k.shape[1]
    store, batch_idx, table = _store(k, form)
    ref = ref or H.index_topk_prefill_ref(q, k, w, fills, topk, causal=causal)
    padded = -(-s_q // BLOCK) * BLOCK
    idx = torch.full((b, s_q, 1, topk + 3), SENTINEL, dtype=torch.int32, device=DEV)
    work = torch.full((rows or b * padded, cap + 5), float(SENTINEL), dtype=torch.float32, device=DEV)
    args = (q.to(DEV), store, w.to(DEV), fills.to(DEV), topk)
    got = H.kvcache_index_topk_prefill(*args, cache_batch_idx=batch_idx, page_table=table, causal=causal, indices=idx, workspace=work,
                                       return_logits=not rows)
    plan = _lib.binding().kvcache_index_topk_prefill_plan(*args, batch_idx, table, causal, idx, work)
    idx, logits = idx.cpu(), got[1].cpu() if not rows else torch.zeros(b, s_q, cap + 5)
    assert torch.all(idx[..., topk:] == SENTINEL) and torch.all(work[:, cap:] == SENTINEL), "written outside [0, topk) / [0, capacity)"
    return idx[..., :topk], logits[..., :cap], plan, ref


def _same_logits(logits, want, fills, causal=True):
    """logits[b, i, :n] are want's, bit for bit, and nothing is written at or behind n"""
    b, s_q, cap = logits.shape
    for e, i in ((e, i) for e in range(b) for i in range(s_q)):
        n = _visible(fills[e], cap, s_q, i, causal)
        assert torch.equal(logits[e, i, :n].double(), want[e, i, :n].double()) and torch.all(logits[e, i, n:] == SENTINEL), (e, i)


@pytest.mark.parametrize("form", ["dense", "p16", "p256"])
@pytest.mark.parametrize("s_q", [17, 2 * BLOCK + 3])
@pytest.mark.parametrize("d_i,h_i", [(64, 16), (128, 48), (128, 64)])
def test_index_prefill_exact(d_i, h_i, s_q, form):
    """Capacity 768 = 3 chunks of 256 = 12 tiles; three token blocks, the last one short; fill levels 0, 1, 63, 65, s_q - 1 (the
    first token sees nothing), 2 chunks + 1 and capacity + 5 (clamped) in one batch; topk 1, 64 and 100; causal and not."""
    cap, chunk = 768, 256
    fills = torch.tensor([0, 1, 63, 65, s_q - 1, 2 * chunk + 1, cap + 5], dtype=torch.int32)
    q, k, w = _exact_inputs(len(fills), s_q, h_i, d_i, cap, seed=d_i + s_q)
    ties = []
    for causal in (True, False):
        for topk in (1, 64, 100):
            idx, logits, plan, ref = _run(q, k, w, fills, topk, form, causal)
            assert plan == (f"index_logits_prefill_kernel d={d_i} heads={h_i} sq={s_q} block={BLOCK} tile=64 chunk={chunk} grid=63 | "
                            f"index_select_prefill_kernel threads=256 passes=4 grid={7 * 3 * BLOCK} | rounds=1")
            _same_logits(logits, ref.logits, fills, causal)
            assert torch.equal(idx, ref.indices), (topk, causal)
            ties.append(_tie_at_the_cut(ref, fills, topk, causal))
    assert any(ties), "ties at the cut are the rule here by construction"


def test_index_prefill_rounds_give_the_same_lists():
    """The least workspace (one token block a round: 21 rounds) against one round."""
    fills = torch.tensor([0, 1, 63, 65, 18, 513, 773], dtype=torch.int32)
    q, k, w = _exact_inputs(len(fills), 19, 64, 128, 768, seed=5)
    one, _, plan_one, ref = _run(q, k, w, fills, 64, "p16")
    many, _, plan_many, _ = _run(q, k, w, fills, 64, "p16", rows=BLOCK, ref=ref)
    assert torch.equal(one, many) and torch.equal(one, ref.indices)
    assert plan_one.endswith("grid=63 | index_select_prefill_kernel threads=256 passes=4 grid=168 | rounds=1")
    assert plan_many.endswith("grid=3 | index_select_prefill_kernel threads=256 passes=4 grid=8 | rounds=21")


@pytest.mark.parametrize("dtype", [BF, FP])
def test_index_prefill_is_bit_equal_to_the_decode_entry(dtype):
    """Normal data, 16 tokens, h_i 64, d_i 128, pages of 64: logits[:n] and indices are kvcache_index_topk's bit for bit."""
    torch.manual_seed(4)
    b, s_q, h_i, d_i, cap, topk = 3, 16, 64, 128, 1024, 128
    q, k, w = torch.randn(b, s_q, h_i, d_i).to(dtype), torch.randn(b, cap, d_i).to(dtype), torch.randn(b, s_q, h_i) * h_i ** -0.5
    fills = torch.tensor([cap, 517, 90], dtype=torch.int32)
    store, _, table = _store(k, "p64")
    args = (q.to(DEV), store, w.to(DEV), fills.to(DEV), topk)
    want_idx, want = H.kvcache_index_topk(*args, page_table=table, return_logits=True)
    idx, logits, _, _ = _run(q, k, w, fills, topk, "p64", ref=True)
    _same_logits(logits, want.cpu(), fills)
    assert torch.equal(idx, want_idx.cpu())


def test_index_prefill_normal_data():
    """40 tokens.  Every logit within (d_i + h_i) 2^-24 A of the fp64 logit, and a chosen set that is valid under the fp64 logits
    with twice that slack: test_index_topk_normal_data's rule and its derivation.  Measured on MI355X: worst ratio 0.001."""
    torch.manual_seed(3)
    b, s_q, h_i, d_i, cap, topk = 3, 40, 64, 128, 1024, 128
    q, k, w = torch.randn(b, s_q, h_i, d_i).to(BF), torch.randn(b, cap, d_i).to(BF), torch.randn(b, s_q, h_i) * h_i ** -0.5
    fills = torch.tensor([cap, 517, 90], dtype=torch.int32)
    idx, logits, _, ref = _run(q, k, w, fills, topk, "p64")
    worst = 0.0
    for e, i in ((e, i) for e in range(b) for i in range(s_q)):
        n = _visible(fills[e], cap, s_q, i)
        l32, l64, bound = logits[e, i, :n].double(), ref.logits[e, i, :n], (d_i + h_i) * EPS * ref.A[e, i, :n]
        worst = max(worst, float(((l32 - l64).abs() / bound).max()))
        K = min(topk, n)
        got = idx[e, i, 0, :K].tolist()
        assert got == sorted(set(got)) and all(0 <= j < n for j in got) and torch.all(idx[e, i, 0, K:] == -1)
        if K < n:
            cut, slack = torch.sort(l64, descending=True).values[K - 1], 2 * bound.amax()
            assert torch.all(l64[got] >= cut - slack) and torch.all(l64[sorted(set(range(n)) - set(got))] <= cut + slack)
    print(f"index prefill logits: worst |l32 - l64| / ((d_i + h_i) 2^-24 A) = {worst:.3f}")
    assert worst <= 1.0


def test_index_prefill_feeds_the_sparse_attention_and_replays_in_a_graph():
    """The MLA shape (h 16, h_k 1, d 64, d_v 512, pages of 64, batch 3, bf16), 40 query tokens: the indexer's lists give the sparse
    attention the bits the oracle's lists give; both calls captured in one graph see fill levels that grew by one row."""
    b, s_q, cap, page, topk = 3, 40, 512, 64, 96
    g = torch.Generator().manual_seed(0)
    q_i, k_i, w = _exact_inputs(b, s_q, 16, 64, cap, seed=2)
    kv, (store, _, table) = torch.randn(b, cap, 1, 576, generator=g).to(BF), _store(k_i, "p64", spare=0)
    cache = torch.zeros(b * cap // page, page, 1, 576, dtype=BF)
    cache[table.flatten().long().cpu()] = kv.reshape(-1, page, 1, 576)
    cache, qi_dev, w_dev = cache.to(DEV), q_i.to(DEV), w.to(DEV)
    q, qv = torch.randn(b, s_q, 16, 64, generator=g).to(BF).to(DEV), torch.randn(b, s_q, 16, 512, generator=g).to(BF).to(DEV)
    fills = torch.tensor([130, 384, 511], dtype=torch.int32)
    lens, idx = fills.to(DEV), torch.empty((b, s_q, 1, topk), dtype=torch.int32, device=DEV)
    work = torch.empty((2 * BLOCK, cap), dtype=torch.float32, device=DEV)  # 15 token blocks in 8 rounds
    kw = dict(qv=qv, cache_seqlens=lens, page_table=table, num_splits=1, return_softmax_lse=True)
    def step():
        H.kvcache_index_topk_prefill(qi_dev, store, w_dev, lens, topk, page_table=table, indices=idx, workspace=work)
        return H.flash_attn_with_kvcache_topk(q, cache[..., :64], cache[..., 64:], idx, **kw)

    out, lse = step()
    ref = H.index_topk_prefill_ref(q_i, k_i, w, fills, topk)
    want = H.flash_attn_with_kvcache_topk(q, cache[..., :64], cache[..., 64:], ref.indices.to(DEV), **kw)
    assert torch.equal(idx.cpu(), ref.indices) and torch.equal(out, want[0]) and torch.equal(lse, want[1])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()  # (warm-up outside the capture: allocator and lazy initialisation)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g_out, g_lse = step()
    lens.add_(1)
    for _ in range(3):
        graph.replay()
        g_idx = idx.clone()
        eager = step()
        assert torch.equal(g_idx, idx) and torch.equal(g_out, eager[0]) and torch.equal(g_lse, eager[1])
    assert torch.equal(idx.cpu(), H.index_topk_prefill_ref(q_i, k_i, w, fills + 1, topk).indices) and not torch.equal(g_out, out)
