"""GPU tests of the lightning indexer over an e4m3 index-key cache (hopper_interface.kvcache_index_topk(k_index_scale=)) and of
its quantising append (kvcache_index_append_fp8).  The oracle is index_topk_ref on the CPU on the dequantised keys k8.float() * scale.
Exact data: q_index in multiples of 1/4 in [-4, 4], weights in multiples of 1/2 in [-2, 2], key BYTES the integers -4 .. 4, one
scale of 1/8, 1/4 or 1/2 per key.  A dot product is a multiple of 1/4 below 2^11, a weighted term a multiple of 1/8 below 2^12, a
sum over 64 heads stays below 2^18 at a granularity of 2^-3: 21 bits, exact in fp32 in any order, and the power-of-two scale is
exact.  So logits and indices EQUAL the oracle's; the keys are drawn from six prototypes, which makes ties at the cut the rule."""
import pytest
import torch
from test_index_topk_gpu import _tie_at_the_cut, _visible  # (the 16-bit indexer's tests: n(b, i), and a tie at some row's cut)

from flash_attention_annotated_amd import _lib, hopper_interface as H

pytestmark = pytest.mark.gpu
DEV, BF, FP, F8, EPS, SENTINEL, BYTE = "cuda", torch.bfloat16, torch.float16, torch.float8_e4m3fn, 2.0 ** -24, 77, 0x7B


def _layout(b, cap, d, form, spare=2):
    """A sentinel-filled cache on the CPU and where the logical position (e, s) lies in it: (bytes (entries, rows, d) uint8, scales
    (entries, rows), entry (b, cap), row (b, cap), page_table or None, the call's cache_batch_idx / page_table on the device); dense
    behind a shuffled cache_batch_idx, or pages of int(form[1:]) rows behind a shuffled table."""
    g, pos = torch.Generator().manual_seed(0), torch.arange(cap).expand(b, cap)
    if form == "dense":
        shape, table, batch_idx = (b + spare, cap), None, torch.randperm(b + spare, generator=g)[:b].to(torch.int32)
        entry, row, kw = batch_idx.long()[:, None].expand(b, cap), pos, dict(cache_batch_idx=batch_idx.to(DEV), page_table=None)
    else:
        page = int(form[1:])
        table = torch.randperm(b * cap // page + spare, generator=g)[:b * cap // page].to(torch.int32).view(b, cap // page)
        shape, entry, row = (b * cap // page + spare, page), table.long()[torch.arange(b)[:, None], pos // page], pos % page
        kw = dict(cache_batch_idx=None, page_table=table.to(DEV))
    return torch.full((*shape, d), BYTE, dtype=torch.uint8), torch.full(shape, float(SENTINEL)), entry, row, table, kw


def _quantise_ref(x):
    """The append's rule on rows (n, d) of a 16-bit CPU tensor: (bytes uint8, scales)."""
    xf = x.float()
    amax = xf.abs().amax(-1)
    m, ex = torch.frexp(amax)  # amax = m 2^ex, m in [0.5, 1); 448 = 0.875 * 2^9
    e = torch.where(amax == 0, 0, (ex - 9 + (m > 0.875)).clamp(-126, 127))
    scale = torch.ldexp(torch.ones_like(amax), e)
    return (xf / scale[:, None]).to(F8).view(torch.uint8), scale


@pytest.mark.parametrize("form", ["dense", "p16", "p64"])
@pytest.mark.parametrize("s_q", [1, 7])
@pytest.mark.parametrize("d_i,h_i", [(64, 16), (128, 64)])
def test_index_topk8_exact(d_i, h_i, s_q, form):
    """Capacity 768 = 3 chunks of 256; fill levels up to capacity + 5 (clamped); buffers sentinel-filled and wider than needed."""
    cap, causal = 768, form != "p16"  # (pages of 16 run without the causal edge)
    fills = torch.tensor([0, 1, 63, 64, 65, 513, 773], dtype=torch.int32)
    b, g = len(fills), torch.Generator().manual_seed(d_i + s_q)
    q = (torch.randint(-16, 17, (b, s_q, h_i, d_i), generator=g).float() / 4).to(BF)
    w = torch.randint(-4, 5, (b, s_q, h_i), generator=g).float() / 2
    proto, proto_scale = torch.randint(-4, 5, (b, 6, d_i), generator=g).float(), 2.0 ** -torch.randint(1, 4, (b, 6), generator=g).float()
    pick = torch.randint(0, 6, (b, cap), generator=g)
    k8, scale = torch.gather(proto, 1, pick[..., None].expand(b, cap, d_i)).to(F8), torch.gather(proto_scale, 1, pick)
    store, scales, entry, row, _, kw = _layout(b, cap, d_i, form)
    store[entry, row], scales[entry, row] = k8.view(torch.uint8), scale
    args = (q.to(DEV), store.to(DEV).view(F8), scales.to(DEV), w.to(DEV), fills.to(DEV))
    ties = []
    for topk in (1, 64, 100):
        ref = H.index_topk_ref(q, k8.float() * scale[..., None], w, fills, topk, causal=causal)
        idx = torch.full((b, s_q, 1, topk + 3), SENTINEL, dtype=torch.int32, device=DEV)
        logits = torch.full((b, s_q, cap + 5), float(SENTINEL), dtype=torch.float32, device=DEV)
        H.kvcache_index_topk(args[0], args[1], *args[3:], topk, k_index_scale=args[2], causal=causal, indices=idx, logits=logits, **kw)
        plan = _lib.binding().kvcache_index_topk_fp8_plan(*args, topk, *kw.values(), causal, idx, logits)
        assert plan == f"index_logits8_kernel d={d_i} heads={h_i} sq={s_q} chunk=256 grid=(3,7) | index_select_kernel threads=256 passes=4"
        idx, logits = idx.cpu(), logits.cpu()
        assert torch.all(idx[..., topk:] == SENTINEL) and torch.all(logits[..., cap:] == SENTINEL), "written outside [0, topk) / [0, capacity)"
        assert torch.equal(logits[..., :cap].double(), ref.logits) and torch.equal(idx[..., :topk], ref.indices), topk
        ties.append(_tie_at_the_cut(ref, fills, topk, causal))
    assert any(ties), "ties at the cut are the rule here by construction"


@pytest.mark.parametrize("dtype", [BF, FP])
def test_index_topk8_normal_data_through_both_kernels(dtype):
    """randn keys go through kvcache_index_append_fp8 into a p64 cache in two appends (ragged, then dense), then are indexed.  Every
    logit within (d_i + h_i + 1) 2^-24 A of the fp64 logit on the dequantised cache contents (A from the oracle; + 1: the multiply
    by the scale), and the chosen set valid under that slack, as test_index_topk_normal_data checks it.
    The bound is derived, not measured; the worst ratio printed below was 0.001 on MI355X, both dtypes."""
    torch.manual_seed(3)
    b, s_q, h_i, d_i, cap, topk = 3, 2, 64, 128, 1024, 128
    q, k, w = torch.randn(b, s_q, h_i, d_i).to(dtype), torch.randn(b, cap, d_i).to(dtype), torch.randn(b, s_q, h_i) * h_i ** -0.5
    fills = torch.tensor([cap, 517, 90], dtype=torch.int32)
    store, scales, _, _, table, _ = _layout(b, cap, d_i, "p64")
    store, scales = store.to(DEV), scales.to(DEV)
    first = fills // 2 - 1  # the ragged append; the dense one brings the rest, 513 / 260 / 46 rows, padded to 513 an entry
    cu = torch.cat([torch.zeros(1, dtype=torch.int32), first.cumsum(0).int()])
    level = H.kvcache_index_append_fp8(store.view(F8), scales, torch.cat([k[e, :first[e]] for e in range(b)]).to(DEV),
                                       torch.zeros(b, dtype=torch.int32, device=DEV), cu_seqlens_k_new=cu.to(DEV), page_table=table.to(DEV))
    assert level.cpu().tolist() == first.tolist()
    rest = torch.stack([torch.cat([k[e, first[e]:fills[e]], k[e, :513 - int(fills[e] - first[e])]]) for e in range(b)])
    H.kvcache_index_append_fp8(store.view(F8), scales, rest.to(DEV), level, page_table=table.to(DEV))
    keys = store.cpu().view(F8).float() * scales.cpu()[..., None]  # (what the cache holds: the rows behind a fill level are not read)
    ref = H.index_topk_ref(q, keys, w, fills, topk, page_table=table)
    idx, logits = H.kvcache_index_topk(q.to(DEV), store.view(F8), w.to(DEV), fills.to(DEV), topk, k_index_scale=scales, page_table=table.to(DEV),
                                       return_logits=True)
    idx, logits, worst = idx.cpu(), logits.cpu(), 0.0
    for e, i in ((e, i) for e in range(b) for i in range(s_q)):
        n = _visible(fills[e], cap, s_q, i)
        assert torch.all(logits[e, i, n:] == float("-inf"))
        l32, l64, bound = logits[e, i, :n].double(), ref.logits[e, i, :n], (d_i + h_i + 1) * EPS * ref.A[e, i, :n]
        worst = max(worst, float(((l32 - l64).abs() / bound).max()))
        K = min(topk, n)
        got = idx[e, i, 0, :K].tolist()
        assert got == sorted(set(got)) and all(0 <= j < n for j in got) and torch.all(idx[e, i, 0, K:] == -1)
        if K < n:
            cut, slack = torch.sort(l64, descending=True).values[K - 1], 2 * bound.amax()
            assert torch.all(l64[got] >= cut - slack) and torch.all(l64[sorted(set(range(n)) - set(got))] <= cut + slack)
    print(f"index logits8 {dtype}: worst |l32 - l64| / ((d_i + h_i + 1) 2^-24 A) = {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("ragged", [False, True], ids=["dense_rows", "ragged_rows"])
@pytest.mark.parametrize("form", ["dense", "p16", "p64"])
@pytest.mark.parametrize("d_i", [64, 128])
def test_index_append8_bit_for_bit(d_i, form, ragged):
    """fp16 rows into a capacity of 64 at fill levels 0 / 37 / 60: 6 rows each, or 6 / 1 / 9 ragged -- the last entry loses rows.
    Entry 0 carries an all-zero row, a row whose amax is exactly 448 * 2^-3, one an ulp above it and a row of fp16 subnormals."""
    b, cap, g = 3, 64, torch.Generator().manual_seed(d_i)
    fills, lens = torch.tensor([0, 37, 60], dtype=torch.int32), [6, 1, 9] if ragged else [6, 6, 6]
    rows = [(torch.randn(n, d_i, generator=g) * 3).to(FP) for n in lens]
    rows[0][0] = 0
    rows[0][1:3] = rows[0][1:3].clamp(-50, 50)
    rows[0][1, 5], rows[0][2, 7] = 56.0, -56.03125  # 448 / 8, and the next fp16 above it
    rows[0][3] = (torch.randint(-1023, 1024, (d_i,), generator=g).float() * 2.0 ** -24).to(FP)
    store, scales, entry, row, _, kw = _layout(b, cap, d_i, form)
    want_store, want_scales = store.clone(), scales.clone()
    for e in range(b):
        kept = min(lens[e], cap - int(fills[e]))
        at = slice(int(fills[e]), int(fills[e]) + kept)
        want_store[entry[e, at], row[e, at]], want_scales[entry[e, at], row[e, at]] = _quantise_ref(rows[e][:kept])
    assert want_scales[entry[0, :4], row[0, :4]].tolist()[:3] == [1.0, 0.125, 0.25] and kept < lens[2]
    store, scales, lens_dev = store.to(DEV), scales.to(DEV), fills.to(DEV)
    new = dict(k_index_new=torch.cat(rows).to(DEV), cu_seqlens_k_new=torch.tensor([0, 6, 7, 16], dtype=torch.int32, device=DEV),
               max_seqlen_k_new=9) if ragged else dict(k_index_new=torch.stack(rows).to(DEV))
    level = H.kvcache_index_append_fp8(store.view(F8), scales, cache_seqlens=lens_dev, **kw, **new)
    assert level.dtype == torch.int32 and level.cpu().tolist() == [min(int(f) + n, cap) for f, n in zip(fills, lens)]
    assert torch.equal(lens_dev.cpu(), fills), "cache_seqlens is not modified"
    assert torch.equal(store.cpu(), want_store) and torch.equal(scales.cpu(), want_scales)


def test_append_and_index_replay_in_one_graph():
    """append -> index on one stream, captured; replayed after the new row and the fill level changed, it gives the oracle's list
    for the new state.  Integer rows in [-4, 4] quantise exactly (scale 2^-6, bytes up to 256), so the lists are equal."""
    b, h_i, d_i, cap, topk = 3, 16, 64, 512, 96
    g = torch.Generator().manual_seed(5)
    q = (torch.randint(-16, 17, (b, 1, h_i, d_i), generator=g).float() / 4).to(BF)
    w = torch.randint(-4, 5, (b, 1, h_i), generator=g).float() / 2
    k = torch.randint(-4, 5, (b, cap, d_i), generator=g).float().to(BF)
    fills = torch.tensor([130, 384, 509], dtype=torch.int32)
    store, scales, _, _, table, _ = _layout(b, cap, d_i, "p64", spare=0)
    store, scales = store.to(DEV), scales.to(DEV)
    table_dev, q_dev, w_dev = table.to(DEV), q.to(DEV), w.to(DEV)
    H.kvcache_index_append_fp8(store.view(F8), scales, k[:, :509].to(DEV), torch.zeros(b, dtype=torch.int32, device=DEV), page_table=table_dev)
    lens, k_new = fills.to(DEV), torch.stack([k[e, fills[e]:fills[e] + 1] for e in range(b)]).to(DEV)
    idx = torch.empty((b, 1, 1, topk), dtype=torch.int32, device=DEV)
    logits = torch.empty((b, 1, cap), dtype=torch.float32, device=DEV)

    def step():
        level = H.kvcache_index_append_fp8(store.view(F8), scales, k_new, lens, page_table=table_dev)
        H.kvcache_index_topk(q_dev, store.view(F8), w_dev, level, topk, k_index_scale=scales, page_table=table_dev, indices=idx, logits=logits)

    def oracle(levels):
        keys = store.cpu().view(F8).float() * scales.cpu()[..., None]
        return H.index_topk_ref(q, keys, w, levels, topk, page_table=table).indices

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()  # (warm-up outside the capture: allocator and lazy initialisation)
    torch.cuda.current_stream().wait_stream(side)
    before = idx.cpu()
    assert torch.equal(before, oracle(fills + 1))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    k_new.copy_(torch.stack([k[e, fills[e] + 1:fills[e] + 2] + 1 for e in range(b)]))
    lens.add_(1)
    for _ in range(3):
        graph.replay()
        replayed = idx.clone()
        step()
        assert torch.equal(replayed, idx)
    assert torch.equal(idx.cpu(), oracle(fills + 2)) and not torch.equal(idx.cpu(), before)
    new_rows = (store.cpu().view(F8).float() * scales.cpu()[..., None])[table.long()].view(b, cap, d_i)[torch.arange(b), (fills + 1).long()]
    assert torch.equal(new_rows, k_new.cpu().float()[:, 0]), "the captured append wrote the new row"
