"""GPU tests of the lightning indexer (hopper_interface.kvcache_index_topk) against the fp64 oracle index_topk_ref run on the CPU.
Exact data: q_index and keys are multiples of 1/4 in [-4, 4], weights multiples of 1/2 in [-2, 2].  A dot product over d_i <= 128
channels is a multiple of 1/16 below 2^11, a weighted term a multiple of 1/32 below 2^12, a sum over 64 heads stays below 2^18 at
a granularity of 2^-5: 23 bits, exact in fp32 in any order.  So logits and indices EQUAL the oracle's; the keys are drawn from a
few prototypes, which makes ties at the cut the rule."""
import pytest
import torch

from flash_attention_annotated_amd import _lib, hopper_interface as H

pytestmark = pytest.mark.gpu
DEV, BF, FP, EPS, SENTINEL = "cuda", torch.bfloat16, torch.float16, 2.0 ** -24, 77


def _store(logical, form, spare=2):
    """(store, cache_batch_idx, page_table) on the device for the logical rows (b, cap, d): dense, or pages of int(form[1:]) rows."""
    b, cap, d = logical.shape
    g = torch.Generator().manual_seed(0)
    if form == "dense":
        batch_idx = torch.randperm(b + spare, generator=g)[:b].to(torch.int32)
        store = torch.zeros((b + spare, cap, d), dtype=logical.dtype)
        store[batch_idx.long()] = logical
        return store.to(DEV), batch_idx.to(DEV), None
    page = int(form[1:])
    table = torch.randperm(b * cap // page + spare, generator=g)[:b * cap // page].to(torch.int32).view(b, cap // page)
    store = torch.zeros((b * cap // page + spare, page, d), dtype=logical.dtype)
    store[table.flatten().long()] = logical.reshape(-1, page, d)
    return store.to(DEV), None, table.to(DEV)


def _exact_inputs(b, s_q, h_i, d_i, cap, seed, distinct=6, dtype=BF):
    g = torch.Generator().manual_seed(seed)
    q = (torch.randint(-16, 17, (b, s_q, h_i, d_i), generator=g).float() / 4).to(dtype)
    protos = torch.randint(-16, 17, (b, distinct, d_i), generator=g).float() / 4
    k = torch.gather(protos, 1, torch.randint(0, distinct, (b, cap, 1), generator=g).expand(b, cap, d_i)).to(dtype)
    return q, k, torch.randint(-4, 5, (b, s_q, h_i), generator=g).float() / 2


def _run(q, k, w, fills, topk, form="dense", causal=True, width=0, extra=0):
    """The call on sentinel-filled buffers `width` / `extra` wider than needed, its plan, and the oracle.  Results on the CPU."""
    (b, s_q), cap = q.shape[:2], k.shape[1]
    store, batch_idx, table = _store(k, form)
    ref = H.index_topk_ref(q, k, w, fills, topk, causal=causal)
    idx = torch.full((b, s_q, 1, topk + width), SENTINEL, dtype=torch.int32, device=DEV)
    logits = torch.full((b, s_q, cap + extra), float(SENTINEL), dtype=torch.float32, device=DEV)
    args = (q.to(DEV), store, w.to(DEV), fills.to(DEV), topk)
    H.kvcache_index_topk(*args, cache_batch_idx=batch_idx, page_table=table, causal=causal, indices=idx, logits=logits)
    plan = _lib.binding().kvcache_index_topk_plan(*args, batch_idx, table, causal, idx, logits)
    idx, logits = idx.cpu(), logits.cpu()
    assert torch.all(idx[..., topk:] == SENTINEL) and torch.all(logits[..., cap:] == SENTINEL), "written outside [0, topk) / [0, capacity)"
    return idx[..., :topk], logits[..., :cap], plan, ref


def _visible(fill, cap, s_q, i, causal=True):
    sk = min(max(int(fill), 0), cap)
    return min(max(sk - (s_q - 1 - i), 0), sk) if causal else sk


def _tie_at_the_cut(ref, fills, topk, causal=True):
    """Some row's K-th logit equals one it did not choose."""
    b, s_q, cap = ref.logits.shape
    for e, i in ((e, i) for e in range(b) for i in range(s_q) if topk < _visible(fills[e], cap, s_q, i, causal)):
        L, chosen = ref.logits[e, i].clone(), ref.indices[e, i, 0].long()
        cut = L[chosen].min()
        L[chosen] = float("-inf")
        if (L == cut).any():
            return True
    return False


@pytest.mark.parametrize("form", ["dense", "p16", "p64", "p256"])
@pytest.mark.parametrize("s_q", [1, 3, 7])
@pytest.mark.parametrize("d_i,h_i", [(64, 16), (128, 64)])
def test_index_topk_exact(d_i, h_i, s_q, form):
    """Capacity 768 = 3 chunks of 256; fill levels 0, 1, 63, 64, 65, 2 chunk + 1 and capacity + 5 (clamped) in one batch; topk 1,
    64 and 100 (above n for five of the entries: the list is 0 .. n - 1, then -1).  s_q 7 at (128, 64) takes three token groups."""
    cap, chunk, causal = 768, 256, form != "p16"  # (pages of 16 run without the causal edge)
    fills = torch.tensor([0, 1, 63, 64, 65, 2 * chunk + 1, cap + 5], dtype=torch.int32)
    q, k, w = _exact_inputs(len(fills), s_q, h_i, d_i, cap, seed=d_i + s_q)
    ties = []
    for topk in (1, 64, 100):
        idx, logits, plan, ref = _run(q, k, w, fills, topk, form, causal, width=3, extra=5)
        assert plan == f"index_logits_kernel d={d_i} heads={h_i} sq={s_q} chunk={chunk} grid=(3,7) | index_select_kernel threads=256 passes=4"
        assert torch.equal(logits.double(), ref.logits) and torch.equal(idx, ref.indices), topk
        assert topk < 65 or idx[4, -1, 0].tolist() == list(range(65)) + [-1] * (topk - 65)  # topk > n: 0 .. n - 1, then -1
        ties.append(_tie_at_the_cut(ref, fills, topk, causal))
    assert any(ties), "ties at the cut are the rule here by construction"


def test_index_topk_exact_past_65536_keys():
    """b 1, capacity 70016 = 274 chunks, fill 70001, topk 2048: indices above 65535, the selection with 1024 threads"""
    q, k, w = _exact_inputs(1, 1, 16, 64, 70016, seed=9, distinct=300)
    fills = torch.tensor([70001], dtype=torch.int32)
    idx, logits, plan, ref = _run(q, k, w, fills, 2048)
    assert plan == "index_logits_kernel d=64 heads=16 sq=1 chunk=256 grid=(274,1) | index_select_kernel threads=1024 passes=4"
    assert torch.equal(logits.double(), ref.logits) and torch.equal(idx, ref.indices)
    assert int(idx.max()) > 65535 and _tie_at_the_cut(ref, fills, 2048)


@pytest.mark.parametrize("dtype", [BF, FP])
def test_index_topk_normal_data(dtype):
    """Every logit within (d_i + h_i) 2^-24 A of the fp64 logit (A = sum_j |w_j| sum_c |q_c k_c|, from the oracle), and a chosen
    set that is valid under the fp64 logits with that slack: with e the largest bound of the row and c the fp64 logit at the cut
    (the K-th largest), a chosen position below c - 2 e would have displaced an unchosen one at or above c, whose fp32 logit is
    larger by more than 0; likewise an unchosen one above c + 2 e."""
    torch.manual_seed(3)
    b, s_q, h_i, d_i, cap, topk = 3, 2, 64, 128, 1024, 128
    q, k, w = torch.randn(b, s_q, h_i, d_i).to(dtype), torch.randn(b, cap, d_i).to(dtype), torch.randn(b, s_q, h_i) * h_i ** -0.5
    fills = torch.tensor([cap, 517, 90], dtype=torch.int32)
    idx, logits, _, ref = _run(q, k, w, fills, topk, "p64")
    worst = 0.0  # (measured on MI355X: 0.001, both dtypes)
    for e, i in ((e, i) for e in range(b) for i in range(s_q)):
        n = _visible(fills[e], cap, s_q, i)
        assert torch.all(logits[e, i, n:] == float("-inf"))
        l32, l64, bound = logits[e, i, :n].double(), ref.logits[e, i, :n], (d_i + h_i) * EPS * ref.A[e, i, :n]
        worst = max(worst, float(((l32 - l64).abs() / bound).max()))
        K = min(topk, n)
        got = idx[e, i, 0, :K].tolist()
        assert got == sorted(set(got)) and all(0 <= j < n for j in got) and torch.all(idx[e, i, 0, K:] == -1)
        if K < n:
            cut, slack = torch.sort(l64, descending=True).values[K - 1], 2 * bound.amax()
            assert torch.all(l64[got] >= cut - slack) and torch.all(l64[sorted(set(range(n)) - set(got))] <= cut + slack)
    print(f"index logits {dtype}: worst |l32 - l64| / ((d_i + h_i) 2^-24 A) = {worst:.3f}")
    assert worst <= 1.0


def test_index_topk_nan_stays_inside():
    """NaN in q_index and in some keys: the choice is unspecified, every index written is in [0, n) or -1, the count is K"""
    q, k, w = _exact_inputs(2, 2, 16, 64, 512, seed=1)
    q[0, 1, 3, 5] = k[1, 7:300:11, 3] = float("nan")
    idx = _run(q, k, w, torch.tensor([512, 333], dtype=torch.int32), 40)[0]
    for e, i in ((e, i) for e in range(2) for i in range(2)):
        got = idx[e, i, 0].tolist()
        assert len(got) == 40 and got == sorted(set(got)) and 0 <= got[0] and got[-1] < _visible((512, 333)[e], 512, 2, i)


def test_index_topk_feeds_the_sparse_decode_and_replays_in_a_graph():
    """The MLA shape (h 16, h_k 1, d 64, d_v 512, pages of 64, batch 3, bf16): the indexer's list gives the sparse decode the bits the
    oracle's list gives; topk >= sk gives the dense call's; both calls captured in one graph see a fill level that grew by one row."""
    b, cap, page, topk = 3, 512, 64, 96
    g = torch.Generator().manual_seed(0)
    q_i, k_i, w = _exact_inputs(b, 1, 16, 64, cap, seed=2)
    kv, (store, _, table) = torch.randn(b, cap, 1, 576, generator=g).to(BF), _store(k_i, "p64", spare=0)
    cache = torch.zeros(b * cap // page, page, 1, 576, dtype=BF)
    cache[table.flatten().long().cpu()] = kv.reshape(-1, page, 1, 576)
    cache, qi_dev, w_dev = cache.to(DEV), q_i.to(DEV), w.to(DEV)
    q, qv = torch.randn(b, 1, 16, 64, generator=g).to(BF).to(DEV), torch.randn(b, 1, 16, 512, generator=g).to(BF).to(DEV)
    fills = torch.tensor([130, 384, 511], dtype=torch.int32)
    lens, idx = fills.to(DEV), torch.empty((b, 1, 1, topk), dtype=torch.int32, device=DEV)
    logits = torch.empty((b, 1, cap), dtype=torch.float32, device=DEV)
    kw = dict(qv=qv, cache_seqlens=lens, page_table=table, num_splits=1, return_softmax_lse=True)
    def step(k=topk, out_idx=idx):
        H.kvcache_index_topk(qi_dev, store, w_dev, lens, k, page_table=table, indices=out_idx, logits=logits)
        return H.flash_attn_with_kvcache_topk(q, cache[..., :64], cache[..., 64:], out_idx, **kw)

    out, lse = step()
    ref = H.index_topk_ref(q_i, k_i, w, fills, topk)
    want = H.flash_attn_with_kvcache_topk(q, cache[..., :64], cache[..., 64:], ref.indices.to(DEV), **kw)
    assert torch.equal(idx.cpu(), ref.indices) and torch.equal(out, want[0]) and torch.equal(lse, want[1])
    dense = H.flash_attn_with_kvcache(q, cache[..., :64], cache[..., 64:], **kw)[:2]
    listed = step(cap, torch.empty((b, 1, 1, cap), dtype=torch.int32, device=DEV))
    assert torch.equal(listed[0], dense[0]) and torch.equal(listed[1], dense[1])
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
    assert torch.equal(idx.cpu(), H.index_topk_ref(q_i, k_i, w, fills + 1, topk).indices) and not torch.equal(g_out, out)
