"""GPU parity of the block-sparse backward on the cute surface (cute_interface.flash_attn_func with mask_block_* / full_block_*
and the key-major q_block_cnt / q_block_idx -> fa_bwd_block_sparse, include/fa_bwd.h, csrc/fa_bwd_kernel_bs.h) against autograd
through tests/block_sparse_bwd_oracle.py.

Bounds, the rule of tests/test_sink_gpu.py (_bound), for dX in dq, dk, dv:
    global     |dX - dX_ref|max <= 3 |dX_pt - dX_ref|max + atol + 1e-5,   atol = 2 |(dX_ref + 0.3 - 0.3) - dX_ref|max
    per block  the same inequality with every maximum taken over one block: dq per (batch, head, 128-row query block), dk / dv
               per (batch, kv head, 128-key block) -- a wrong block where gradients are small, or one that must be zero, fails here.
dX_ref: the oracle in fp32, dX_pt: the same math in the inputs' precision.  dsink: the global bound.  Every case asserts that
the plan of the backward names the bs_bwd_* kernels with the expected head-dim tile and SOFTCAP.

Base shape: the forward suite's -- b2, h4 / hk2, sq 300 (the last query block has 44 rows), sk 715 (the last key block one full
64-key tile and 11 keys), sq != sk for the bottom-right alignment.  Lists from block_sparse_oracle.random_lists: distinct per
batch and per query head inside a GQA group, shuffled, unvisited indices in the tails.  The key-major lists come from the
definition (block_sparse_bwd_oracle.key_major_lists), their entries shuffled; one case takes them from
cute_interface.block_sparse_bwd_lists on the device."""
import functools

import pytest
import torch

import block_sparse_bwd_oracle as bwo
import block_sparse_oracle as bso
from parity_helpers import record_bwd_plan

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
B, H, HK, SQ, SK = 2, 4, 2, 300, 715
NM, NK = 3, 6


def _cute():
    from flash_attention_annotated_amd import cute_interface
    return cute_interface


@functools.lru_cache(maxsize=None)
def _inputs(d, dt, seed=0):
    g = torch.Generator().manual_seed(seed)
    dtype = DTYPES[dt]
    return (torch.randn(B, SQ, H, d, generator=g).to(dtype), torch.randn(B, SK, HK, d, generator=g).to(dtype),
            torch.randn(B, SK, HK, d, generator=g).to(dtype), torch.randn(B, SQ, H, d, generator=g).to(dtype))


def _shuffled(cnt, idx, seed):
    """The first cnt entries of every row in a random order (the tails stay 0)."""
    g = torch.Generator().manual_seed(seed)
    out = idx.clone()
    flat, c = out.view(-1, idx.shape[-1]), cnt.reshape(-1).tolist()
    for i, n in enumerate(c):
        flat[i, :n] = flat[i, :n][torch.randperm(n, generator=g)]
    return cnt, out


def _key_lists(lists, b=B, h=H, seed=0):
    return _shuffled(*bwo.key_major_lists(lists, b, h), seed)


def _dev(ts):
    return tuple(None if t is None else t.to(DEV) for t in ts)


def _plan(tile, softcap):
    sc = " SOFTCAP" if softcap else ""
    return f"bwd_dot LPR={tile // 8} | bs_bwd_dkdv D={tile}{sc} | bs_bwd_dq D={tile}{sc}"


def _run(t, lists, key_lists, sink=None, **kw):
    """Forward + backward on the GPU -> [dq, dk, dv(, dsink)] on the CPU; asserts the plan of the backward."""
    q, k, v, g = t
    fc, fi, mc, mi = _dev(lists)
    qc, qi = _dev(key_lists)
    leaves = [x.to(DEV).requires_grad_(True) for x in (q, k, v)] + ([sink.to(DEV).requires_grad_(True)] if sink is not None else [])
    out, _ = _cute().flash_attn_func(*leaves[:3], learnable_sink=leaves[3] if sink is not None else None, full_block_cnt=fc,
                                     full_block_idx=fi, mask_block_cnt=mc, mask_block_idx=mi, q_block_cnt=qc, q_block_idx=qi, **kw)
    plans = record_bwd_plan(out)
    got = torch.autograd.grad(out, leaves, g.to(DEV))
    torch.cuda.synchronize()
    tile = 64 if q.shape[-1] <= 64 else 128
    assert plans == [_plan(tile, kw.get("softcap", 0) > 0)], plans
    return [x.detach().cpu() for x in got]


def _oracle(t, lists, sink=None, **kw):
    q, k, v, g = t
    leaves = [q, k, v] + ([sink] if sink is not None else [])
    fn = lambda a, b, c, *z, **o: bwo.attention_block_sparse_grad_ref(a, b, c, lists, learnable_sink=z[0] if z else None, **kw, **o)[0]  # noqa: E731
    return bwo.grads(fn, leaves, g)


def _blocks(x):
    """(b, s, heads, d) -> (b, ceil(s / 128), 128, heads, d), zero padded."""
    b, s, h, d = x.shape
    n = (s + 127) // 128
    pad = torch.zeros(b, n * 128, h, d)
    pad[:, :s] = x.float()
    return pad.view(b, n, 128, h, d)


def _check(got, ref, pt, what):
    worst = 0.0
    for name, g, r, p in zip(("dq", "dk", "dv", "dsink"), got, ref, pt):
        g, r, p = g.float(), r.float(), p.float()
        assert torch.isfinite(g).all(), f"{what} {name}: non-finite"
        atol = 2 * (r + 0.3 - 0.3 - r).abs().max().item()
        err, bound = (g - r).abs().max().item(), 3 * (p - r).abs().max().item() + atol + 1e-5
        print(f"{what} {name}: err {err:.3e} (bound {bound:.3e})")
        assert err <= bound, f"{what} {name}: max err {err:.3e} > bound {bound:.3e}"
        if name == "dsink":
            continue
        amax = lambda x: _blocks(x).abs().amax(dim=(2, 4))  # noqa: E731  (b, blocks, heads)
        berr = amax(g - r)
        bbound = 3 * amax(p - r) + 2 * amax(r + 0.3 - 0.3 - r) + 1e-5
        ratio = (berr / bbound).max().item()
        worst = max(worst, ratio)
        print(f"{what} {name}: worst per-block err / bound {ratio:.3f}")
        bad = torch.nonzero(berr > bbound)
        assert bad.numel() == 0, f"{what} {name}: (batch, block, head) {bad[0].tolist()} err {berr[tuple(bad[0])]:.3e} > {bbound[tuple(bad[0])]:.3e}"
    return worst


def _case(lists, d=128, dt="bf16", seed=0, sink=None, what="", **kw):
    t = _inputs(d, dt, seed)
    got = _run(t, lists, _key_lists(lists, seed=seed), sink=sink, **kw)
    ref, pt = _oracle(t, lists, sink=sink, **kw)
    _check(got, ref, pt, what or f"d{d} {dt} {kw}")
    return got, ref


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("d", [64, 128])
def test_random_subsets(d, dt):
    lists, visited = bso.random_lists(d, B, H, NM, NK, min_visited=1, max_visited=NK - 1)
    assert not torch.equal(visited[:, 0], visited[:, 1]) and not torch.equal(visited[0], visited[1])
    _case(lists, d=d, dt=dt)


@pytest.mark.parametrize("kw,seed", [(dict(causal=True), 2), (dict(window_size=(200, 50)), 1), (dict(softcap=5.0, causal=True), 13),
                                     (dict(softcap=5.0), 3)], ids=["causal", "window_200_50", "softcap_causal", "softcap"])
def test_call_masks_and_softcap(kw, seed):
    """Random subsets under the call's own mask (bottom-right aligned, sq != sk): rows that lose all their keys, dead listed
    tiles, the diagonal inside listed blocks; softcap on both kernels."""
    lists, _ = bso.random_lists(seed, B, H, NM, NK, min_visited=1, max_visited=NK - 1)
    _case(lists, d=128, **kw)
    if "softcap" in kw and "causal" in kw:
        _case(lists, d=64, dt="fp16", **kw)


def test_learnable_sink_and_dsink():
    sink = torch.linspace(-4, 4, H).to(torch.bfloat16)  # distinct per head
    lists, _ = bso.random_lists(11, B, H, NM, NK, min_visited=1, max_visited=NK - 1)
    lists[0][:, :, 1] = 0
    lists[2][:, :, 1] = 0    # query block 1 visits nothing: LSE = z there, all of its weight on the sink
    got, _ = _case(lists, sink=sink, causal=True, what="sink")
    assert got[3].dtype == torch.bfloat16 and got[3].shape == (H,)
    assert (got[0][:, 128:256] == 0).all()


def test_every_block_listed_descending_is_the_dense_backward():
    cnt = torch.full((B, H, NM), NK, dtype=torch.int32)
    idx = torch.arange(NK, dtype=torch.int32).flip(0).view(1, 1, 1, NK).expand(B, H, NM, NK).contiguous()
    lists = (None, None, cnt, idx)
    qc = torch.full((B, H, NK), NM, dtype=torch.int32)
    qi = torch.arange(NM, dtype=torch.int32).flip(0).view(1, 1, 1, NM).expand(B, H, NK, NM).contiguous()
    t = _inputs(128, "bf16")
    for kw in (dict(), dict(causal=True)):
        got = _run(t, lists, (qc, qi), **kw)
        ref, pt = _oracle(t, lists, **kw)
        _check(got, ref, pt, f"all blocks {kw}")
        leaves = [x.to(DEV).requires_grad_(True) for x in t[:3]]
        out, _ = _cute().flash_attn_func(*leaves, **kw)
        plans = record_bwd_plan(out)
        dense = [x.cpu() for x in torch.autograd.grad(out, leaves, t[3].to(DEV))]
        assert len(plans) == 1 and "bs_bwd" not in plans[0] and "bwd_dkdv D=128" in plans[0]
        _check(dense, ref, pt, f"dense call {kw}")
        # the two backwards against each other, under the same bound (the dense gradients as the reference)
        shifted = [d_.float() + (p.float() - r.float()) for d_, p, r in zip(dense, pt, ref)]  # |pt - ref| around the dense result
        _check(got, [d_.float() for d_ in dense], shifted, f"block-sparse vs dense {kw}")


def _through_mask_list(visited):
    """Everything through the mask list: visited blocks first, the unvisited ones behind the count."""
    mi = torch.sort((~visited).to(torch.int8), dim=-1, stable=True).indices.to(torch.int32)
    return None, None, visited.sum(-1, dtype=torch.int32), mi


def test_query_block_with_both_counts_zero():
    _, visited = bso.random_lists(7, B, H, NM, NK, min_visited=1, max_visited=NK - 1)
    visited[:, :, 1] = False     # query block 1 of every (batch, head)
    visited[0, 3, 2] = False     # and the ragged last block of one head
    got, _ = _case(_through_mask_list(visited), what="empty query block")
    dq = got[0]
    assert (dq[:, 128:256] == 0).all() and (dq[0, 256:, 3] == 0).all()
    assert dq[:, :128].abs().max() > 0 and dq[1, 256:, 3].abs().max() > 0


def test_key_block_no_head_visits():
    _, visited = bso.random_lists(9, B, H, NM, NK, min_visited=2, max_visited=NK - 1)
    visited[..., 2] = False      # key block 2: nobody
    visited[:, :2, :, 5] = False  # the ragged last key block: no head of kv head 0 (heads 2, 3 of kv head 1 may)
    visited[:, 2, 0, 5] = True
    got, _ = _case(_through_mask_list(visited), what="unvisited key block")
    for x in got[1:3]:
        assert (x[:, 256:384] == 0).all() and (x[:, 640:, 0] == 0).all()
        assert x[:, :256].abs().max() > 0 and x[:, 640:, 1].abs().max() > 0


def test_broadcast_lists_equal_expanded_lists():
    """All six lists of shape (1, 1, ..) are read through stride 0: bit-equal to the call with expanded copies."""
    lists, _ = bso.random_lists(17, 1, 1, NM, NK, min_visited=1, max_visited=NK - 1)
    kl = _key_lists(lists, 1, 1, seed=17)
    t = _inputs(128, "bf16")
    got = _run(t, lists, kl, causal=True)
    wide = tuple(x.expand(B, H, *x.shape[2:]).contiguous() for x in lists)
    wide_kl = tuple(x.expand(B, H, *x.shape[2:]).contiguous() for x in kl)
    again = _run(t, wide, wide_kl, causal=True)
    assert all(torch.equal(a, b) for a, b in zip(got, again))
    mixed = _run(t, tuple(x[:1] for x in wide), tuple(x[:, :1] for x in wide_kl), causal=True)  # views: stride != 0 on a size-1 dim
    assert all(torch.equal(a, b) for a, b in zip(got, mixed))
    ref, pt = _oracle(t, lists, causal=True)
    _check(got, ref, pt, "broadcast")


def test_entry_dead_under_the_causal_mask_changes_nothing():
    """Query block 0 (rows 0..127) sees keys up to 127 + 415 under the causal mask: key block 5 (keys 640..) is dead for it.
    Listed or not -- in the forward list and in the key-major list -- the gradients are the same bits, and nothing faults."""
    _, visited = bso.random_lists(19, B, H, NM, NK, min_visited=2, max_visited=NK - 1)
    visited[:, :, 0, 5] = False
    t = _inputs(128, "bf16")
    without = _through_mask_list(visited)
    got = _run(t, without, _key_lists(without, seed=19), causal=True)
    ref, pt = _oracle(t, without, causal=True)
    _check(got, ref, pt, "without the dead entry")
    # the dead entry in front of the live ones, in both directions
    fc, fi, mc, mi = without
    mi2, mc2 = mi.clone(), mc.clone()
    mi2[:, :, 0, 1:] = mi[:, :, 0, :-1]
    mi2[:, :, 0, 0] = 5
    mc2[:, :, 0] += 1
    qc, qi = _key_lists(without, seed=19)
    qi2, qc2 = qi.clone(), qc.clone()
    qi2[:, :, 5, 1:] = qi[:, :, 5, :-1]
    qi2[:, :, 5, 0] = 0
    qc2[:, :, 5] += 1
    again = _run(t, (fc, fi, mc2, mi2), (qc2, qi2), causal=True)
    assert all(torch.equal(a, b) for a, b in zip(got, again))


def test_two_runs_are_bit_equal_and_the_device_helper_gives_the_lists():
    lists, _ = bso.random_lists(29, B, H, NM, NK, min_visited=1, max_visited=NK - 1)
    t = _inputs(128, "fp16")
    kl = tuple(x.cpu() for x in _cute().block_sparse_bwd_lists(*_dev(lists)))   # ascending order, made on the device
    want = bwo.key_major_lists(lists, B, H)
    assert torch.equal(kl[0], want[0]) and torch.equal(kl[1], want[1])
    a = _run(t, lists, kl, window_size=(200, 50))
    b = _run(t, lists, kl, window_size=(200, 50))
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    ref, pt = _oracle(t, lists, window_size=(200, 50))
    _check(a, ref, pt, "fp16 window, lists from block_sparse_bwd_lists")


def test_graph_capture_of_forward_and_backward_with_rewritten_lists():
    """Nothing of the six lists is read on the host: forward + backward captured once, replayed after all six were rewritten
    in place, the new gradients match the oracle of the new lists."""
    t = _inputs(128, "bf16")
    qd, kd, vd, gd = (x.to(DEV) for x in t)
    first, _ = bso.random_lists(31, B, H, NM, NK, min_visited=1, max_visited=NK - 1)
    second, _ = bso.random_lists(37, B, H, NM, NK, min_visited=0, max_visited=NK - 1)
    static = _dev(first) + _dev(_key_lists(first, seed=31))
    leaves = [x.requires_grad_(True) for x in (qd, kd, vd)]

    def step():
        out, _ = _cute().flash_attn_func(*leaves, causal=True, full_block_cnt=static[0], full_block_idx=static[1], mask_block_cnt=static[2],
                                         mask_block_idx=static[3], q_block_cnt=static[4], q_block_idx=static[5])
        return torch.autograd.grad(out, leaves, gd)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        grads = step()
    for lists, seed in ((first, 31), (second, 37)):
        for dst, src in zip(static, tuple(lists) + _key_lists(lists, seed=seed)):
            dst.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        ref, pt = _oracle(t, lists, causal=True)
        _check([x.cpu() for x in grads], ref, pt, f"graph replay {seed}")


def test_surface():
    f = _cute().flash_attn_func
    q, k, v, g = (x.to(DEV) for x in _inputs(64, "bf16"))
    lists, _ = bso.random_lists(41, B, H, NM, NK, min_visited=1)
    fc, fi, mc, mi = _dev(lists)
    qc, qi = _dev(_key_lists(lists))
    sparse = dict(full_block_cnt=fc, full_block_idx=fi, mask_block_cnt=mc, mask_block_idx=mi)
    # without the key-major lists the backward still raises
    out, _ = f(q.clone().requires_grad_(True), k, v, **sparse)
    with pytest.raises(NotImplementedError, match="block-sparse backward"):
        out.sum().backward()
    with pytest.raises(ValueError, match="specified together"):
        f(q, k, v, q_block_cnt=qc, **sparse)
    with pytest.raises(ValueError, match="specified together"):
        f(q, k, v, q_block_idx=qi, **sparse)
    with pytest.raises(ValueError, match="only valid with mask_block"):
        f(q, k, v, q_block_cnt=qc, q_block_idx=qi)
    with pytest.raises(ValueError, match="int32"):
        f(q, k, v, q_block_cnt=qc.long(), q_block_idx=qi, **sparse)
    with pytest.raises(ValueError, match="device of q"):
        f(q, k, v, q_block_cnt=qc.cpu(), q_block_idx=qi, **sparse)
    with pytest.raises(ValueError, match="q_block_idx must have shape"):
        f(q, k, v, q_block_cnt=qc, q_block_idx=qi.transpose(-1, -2).contiguous(), **sparse)
    with pytest.raises(ValueError, match="q_block_cnt must have shape"):
        f(q, k, v, q_block_cnt=qc[..., :NM], q_block_idx=qi, **sparse)
    # head dim 192: the forward runs, the backward names the limit
    g192 = torch.Generator().manual_seed(5)
    q2, k2, v2 = (torch.randn(B, s, h, 192, generator=g192).to(torch.bfloat16).to(DEV) for s, h in ((SQ, H), (SK, HK), (SK, HK)))
    out, _ = f(q2.requires_grad_(True), k2, v2, q_block_cnt=qc, q_block_idx=qi, **sparse)
    with pytest.raises(NotImplementedError, match="head dims up to 128"):
        out.sum().backward()
