"""GPU parity of the block-sparse forward on the cute surface (cute_interface.flash_attn_func with mask_block_* / full_block_*
-> fa_fwd_block_sparse, include/fa_fwd.h, csrc/fa_fwd_kernel_bs.h) against tests/block_sparse_oracle.py.

The rule of tests/test_sink_gpu.py (_check):  |O - O_ref|max <= 2 |O_pt - O_ref|max + 1e-5  (O_ref: the oracle in fp32, O_pt:
the same math in the inputs' precision), LSE within 2e-3 with the same inf pattern.  Every case asserts that the plan of the
call names bs_fwd_kernel.

Base shape: b2, h4 / hk2, sq 300 (3 query blocks, the last of 44 rows), sk 715 (6 key blocks, the last of 75 keys: one full
64-key tile and 11 keys).  Lists come from a seeded generator on the CPU (block_sparse_oracle.random_lists): distinct per
batch and per query head -- they differ inside a GQA group, so indexing by the KV head shows --, shuffled, split at random
between the two lists, the tails behind the counts filled with in-range indices that are not visited (ignoring a count gives
wrong numbers, not a fault)."""
import math

import pytest
import torch

import block_sparse_oracle as bso
from parity_helpers import last_plan

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
B, H, HK, SQ, SK = 2, 4, 2, 300, 715
NM, NK = 3, 6


def _cute():
    from flash_attention_annotated_amd import cute_interface
    return cute_interface


def _qkv(d, dtype, dv=None, seed=0, b=B, sq=SQ, sk=SK, h=H, hk=HK):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(b, sq, h, d, generator=g).to(dtype), torch.randn(b, sk, hk, d, generator=g).to(dtype),
            torch.randn(b, sk, hk, dv or d, generator=g).to(dtype))


def _check(out, lse, ref, pt, lse_ref, what):
    err = (out.float().cpu() - ref.float()).abs().max().item()
    bound = 2 * (pt.float() - ref.float()).abs().max().item() + 1e-5
    lse = lse.float().cpu()
    fin = torch.isfinite(lse_ref)
    lerr = (lse[fin] - lse_ref[fin]).abs().max().item() if fin.any() else 0.0
    print(f"{what}: out err {err:.3e} (bound {bound:.3e}), lse err {lerr:.3e}")
    assert math.isfinite(err) and err <= bound, f"{what}: max err {err:.3e} > bound {bound:.3e}"
    assert torch.equal(torch.isfinite(lse), fin), f"{what}: lse inf pattern"
    assert lerr <= 2e-3, f"{what}: lse err {lerr:.3e}"
    return bound


def _dev(lists):
    return tuple(None if t is None else t.to(DEV) for t in lists)


def _run(q, k, v, lists, tile, softcap_form=False, **kw):
    """The block-sparse call on the GPU; asserts the plan.  lists: (full_cnt, full_idx, mask_cnt, mask_idx) on the CPU."""
    fc, fi, mc, mi = _dev(lists)
    sink = kw.pop("learnable_sink", None)
    out, lse = _cute().flash_attn_func(q.to(DEV), k.to(DEV), v.to(DEV), full_block_cnt=fc, full_block_idx=fi, mask_block_cnt=mc,
                                       mask_block_idx=mi, learnable_sink=None if sink is None else sink.to(DEV), **kw)
    plan = last_plan()
    torch.cuda.synchronize()
    want = f"bs_fwd_kernel D={tile} waves=4{' SOFTCAP' if softcap_form else ''} block_m=128 splits=1"
    assert plan == want, f"{plan!r} is not {want!r}"
    assert out.shape == (*q.shape[:3], v.shape[-1]) and out.dtype == q.dtype
    assert lse.shape == (q.shape[0], q.shape[2], q.shape[1]) and lse.dtype == torch.float32
    return out, lse


def _oracle(q, k, v, lists, **kw):
    ref, lse_ref = bso.attention_block_sparse_ref(q, k, v, *lists, **kw)
    pt, _ = bso.attention_block_sparse_ref(q, k, v, *lists, upcast=False, reorder_ops=True, **kw)
    return ref, pt, lse_ref


def _case(lists, d=128, dtype=torch.bfloat16, dv=None, what="", **kw):
    q, k, v = _qkv(d, dtype, dv)
    tile = 64 if max(d, dv or d) <= 64 else 128 if max(d, dv or d) <= 128 else 256
    out, lse = _run(q, k, v, lists, tile, softcap_form=kw.get("softcap", 0) > 0, **kw)
    ref, pt, lse_ref = _oracle(q, k, v, lists, **kw)
    _check(out, lse, ref, pt, lse_ref, what or f"d{d} {dtype}")
    return out, lse, lse_ref


def _all_blocks(in_full):
    cnt = torch.full((B, H, NM), NK, dtype=torch.int32)
    idx = torch.arange(NK, dtype=torch.int32).flip(0).view(1, 1, 1, NK).expand(B, H, NM, NK).contiguous()  # descending order
    if in_full:
        return cnt, idx, torch.zeros_like(cnt), torch.full_like(idx, 3)
    return None, None, cnt, idx


@pytest.mark.parametrize("in_full", [False, True], ids=["mask_list", "full_list"])
@pytest.mark.parametrize("kw", [dict(), dict(causal=True)], ids=str)
def test_every_block_listed_is_the_dense_call(in_full, kw):
    """Every block in the mask list, or every block in the full list -- a causal diagonal among them: the oracle, and the plain
    dense call of the same inputs under the same tolerance."""
    lists = _all_blocks(in_full)
    q, k, v = _qkv(128, torch.bfloat16)
    out, lse = _run(q, k, v, lists, 128, **kw)
    ref, pt, lse_ref = _oracle(q, k, v, lists, **kw)
    bound = _check(out, lse, ref, pt, lse_ref, "all blocks")
    dense, dense_lse = _cute().flash_attn_func(q.to(DEV), k.to(DEV), v.to(DEV), **kw)
    assert last_plan().startswith("fwd_kernel")
    _check(dense, dense_lse, ref, pt, lse_ref, "dense call")
    diff = (out.float() - dense.float()).abs().max().item()
    print(f"block-sparse vs dense: {diff:.3e} (bound {bound:.3e})")
    assert diff <= bound
    assert (lse - dense_lse).abs().max().item() <= 2e-3


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("d,dv", [(64, None), (128, None), (256, None), (192, 128)])
def test_random_subsets(d, dv, dt):
    lists, visited = bso.random_lists(d, B, H, NM, NK, min_visited=1, max_visited=NK - 1)
    assert visited.any(-1).all() and not visited.all(-1).any()       # >= 1 visited, >= 1 unvisited block per query block
    assert not torch.equal(visited[:, 0], visited[:, 1])             # the two query heads of one KV head differ
    assert not torch.equal(visited[0], visited[1])
    _, lse, lse_ref = _case(lists, d=d, dv=dv, dtype=DTYPES[dt])
    assert torch.isfinite(lse_ref).all()


def _call_mask(causal=False, window_size=(None, None)):
    i, j = torch.arange(SQ).view(-1, 1) + SK - SQ, torch.arange(SK).view(1, -1)
    left, right = window_size
    right = 0 if causal else right
    ok = torch.ones(SQ, SK, dtype=torch.bool)
    if right is not None:
        ok &= j <= i + right
    if left is not None:
        ok &= j >= i - left
    return ok


def _block_view(mask):
    """(SQ, SK) bool -> (any, all) per 128 x 128 block, (NM, NK) each (the ragged last blocks count their own cells)."""
    pad = torch.zeros(NM * 128, NK * 128, dtype=torch.bool)
    pad[:SQ, :SK] = mask
    real = torch.zeros_like(pad)
    real[:SQ, :SK] = True
    blk = lambda t: t.view(NM, 128, NK, 128).permute(0, 2, 1, 3).reshape(NM, NK, -1)  # noqa: E731
    return blk(pad).any(-1), (blk(pad) | ~blk(real)).all(-1)


@pytest.mark.parametrize("kw,seed", [(dict(causal=True), 2), (dict(window_size=(200, 50)), 1)], ids=["causal", "window_200_50"])
def test_causal_and_window_with_diagonal_blocks_in_the_full_list(kw, seed):
    """Random subsets under the call's own mask; every visited block the mask cuts through -- the diagonal, the window's
    edges -- is placed in the full list on purpose: the kernel must mask inside full blocks.  The seed is chosen so that
    some rows lose all their keys (visited blocks, all of them masked for the row) and some query block has a live diagonal."""
    call = _call_mask(**kw)
    some, every = _block_view(call)
    diagonal = some & ~every
    lists, visited = bso.random_lists(seed, B, H, NM, NK, min_visited=1, max_visited=NK - 1, to_full=diagonal)
    in_full = bso.block_mask_from_lists(None, None, lists[0], lists[1], B, H)
    assert (in_full & diagonal).any(), "no live diagonal block in the full list"
    assert not (visited & diagonal & ~in_full).any()
    allowed = bso.dense_mask(visited, SQ, SK) & call
    keyless = ~allowed.any(-1)                                        # (b, h, sq)
    assert keyless.any() and not keyless.all(), "the seed gives no row that loses all its keys"
    out, lse, lse_ref = _case(lists, what=str(kw), **kw)
    assert torch.equal(torch.isinf(lse_ref), keyless)
    assert (out.cpu().transpose(1, 2)[keyless] == 0).all()


def test_query_block_without_blocks_and_no_full_list():
    """Both counts 0 is legal: O == 0 exactly, LSE = +inf on those rows, finite elsewhere.  full_block_* = None."""
    (_, _, mc, mi), visited = bso.random_lists(7, B, H, NM, NK, min_visited=1, max_visited=NK - 1)
    # everything through the mask list: visited blocks first (shuffled), unvisited ones behind the count
    mi = torch.sort((~visited).to(torch.int8), dim=-1, stable=True).indices.to(torch.int32)
    mc = visited.sum(-1, dtype=torch.int32)
    mc[:, :, 1] = 0          # query block 1 of every (batch, head)
    mc[0, 3, 2] = 0          # and the ragged last block of one head
    lists = (None, None, mc, mi)
    out, lse, _ = _case(lists)
    out, lse = out.cpu(), lse.cpu()
    empty = torch.zeros(B, H, SQ, dtype=torch.bool)
    empty[:, :, 128:256] = True
    empty[0, 3, 256:] = True
    assert (out.transpose(1, 2)[empty] == 0).all()
    assert torch.isposinf(lse[empty]).all() and torch.isfinite(lse[~empty]).all()


def test_learnable_sink():
    """Parity with a sink distinct per head; rows without a visible key give O = 0 and LSE == z."""
    sink = torch.linspace(-4, 4, H).to(torch.bfloat16)
    lists, _ = bso.random_lists(11, B, H, NM, NK, min_visited=1, max_visited=NK - 1)
    lists[0][:, :, 1] = 0
    lists[2][:, :, 1] = 0    # query block 1 visits nothing
    out, lse, lse_ref = _case(lists, learnable_sink=sink, causal=True)
    assert torch.isfinite(lse_ref).all()
    want = sink.float().view(1, H, 1).expand(B, H, 128)
    assert torch.equal(lse.cpu()[:, :, 128:256], want)
    assert (out.cpu()[:, 128:256] == 0).all()


def test_softcap():
    lists, _ = bso.random_lists(13, B, H, NM, NK, min_visited=1, max_visited=NK - 1)
    _case(lists, softcap=5.0, causal=True)


def test_broadcast_lists_equal_expanded_lists():
    """Lists of shape (1, 1, nm) / (1, 1, nm, nk) are read through stride 0: the result is bit-equal to the call with the
    lists expanded, and the caller makes no expanded copy."""
    lists, _ = bso.random_lists(17, 1, 1, NM, NK, min_visited=1, max_visited=NK - 1)
    q, k, v = _qkv(128, torch.bfloat16)
    out, lse = _run(q, k, v, lists, 128, causal=True)
    wide = tuple(t.expand(B, H, *t.shape[2:]).contiguous() for t in lists)
    out2, lse2 = _run(q, k, v, wide, 128, causal=True)
    assert torch.equal(out, out2) and torch.equal(lse, lse2)
    ref, pt, lse_ref = _oracle(q, k, v, lists, causal=True)
    _check(out, lse, ref, pt, lse_ref, "broadcast")
    # one dimension at a time, and as views of the wide tensors (stride != 0 on a size-1 dim)
    for sl in ((slice(0, 1), slice(None)), (slice(None), slice(0, 1))):
        part = tuple(t[sl] for t in wide)
        out3, lse3 = _run(q, k, v, part, 128, causal=True)
        assert torch.equal(out, out3) and torch.equal(lse, lse3)


def test_packed_qkv_view_and_single_block():
    """Non-contiguous q / k / v (views of one packed (b, s, 3, h, d) tensor, MHA), and sq = sk = 128: one block each."""
    g = torch.Generator().manual_seed(19)
    for s, seed in ((300, 19), (128, 23)):
        qkv = torch.randn(B, s, 3, H, 128, generator=g).to(torch.bfloat16)
        n = (s + 127) // 128
        lists, _ = bso.random_lists(seed, B, H, n, n, min_visited=1)
        qkv_d = qkv.to(DEV)
        qd, kd, vd = qkv_d.unbind(2)
        assert not qd.is_contiguous()
        out, lse = _cute().flash_attn_func(qd, kd, vd, causal=True, full_block_cnt=lists[0].to(DEV), full_block_idx=lists[1].to(DEV),
                                           mask_block_cnt=lists[2].to(DEV), mask_block_idx=lists[3].to(DEV))
        assert last_plan() == "bs_fwd_kernel D=128 waves=4 block_m=128 splits=1"
        q, k, v = qkv.unbind(2)
        ref, pt, lse_ref = _oracle(q, k, v, lists, causal=True)
        _check(out, lse, ref, pt, lse_ref, f"packed s{s}")


def test_two_calls_are_bit_equal():
    lists, _ = bso.random_lists(29, B, H, NM, NK, min_visited=1, max_visited=NK - 1)
    q, k, v = _qkv(128, torch.float16)
    a = _run(q, k, v, lists, 128, window_size=(200, 50))
    b = _run(q, k, v, lists, 128, window_size=(200, 50))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_graph_capture_and_replay_with_rewritten_lists():
    """The call reads nothing on the host: captured once, replayed after the lists were rewritten in place, the new result
    matches the oracle of the new lists."""
    q, k, v = _qkv(128, torch.bfloat16)
    qd, kd, vd = q.to(DEV), k.to(DEV), v.to(DEV)
    first, _ = bso.random_lists(31, B, H, NM, NK, min_visited=1, max_visited=NK - 1)
    second, _ = bso.random_lists(37, B, H, NM, NK, min_visited=0, max_visited=NK - 1)
    static = _dev(first)
    f = lambda: _cute().flash_attn_func(qd, kd, vd, causal=True, full_block_cnt=static[0], full_block_idx=static[1],  # noqa: E731
                                        mask_block_cnt=static[2], mask_block_idx=static[3])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        f()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, lse = f()
    assert last_plan() == "bs_fwd_kernel D=128 waves=4 block_m=128 splits=1"
    for lists in (first, second):
        for dst, src in zip(static, lists):
            dst.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        ref, pt, lse_ref = _oracle(q, k, v, lists, causal=True)
        _check(out, lse, ref, pt, lse_ref, "graph replay")


def test_surface():
    f = _cute().flash_attn_func
    q, k, v = (t.to(DEV) for t in _qkv(64, torch.bfloat16))
    lists, _ = bso.random_lists(41, B, H, NM, NK, min_visited=1)
    fc, fi, mc, mi = _dev(lists)
    sparse = dict(full_block_cnt=fc, full_block_idx=fi, mask_block_cnt=mc, mask_block_idx=mi)
    with pytest.raises(NotImplementedError, match="mask_mod"):
        f(q, k, v, mask_mod=lambda *a: True, **sparse)
    with pytest.raises(NotImplementedError, match="full_block_cnt, full_block_idx"):
        f(q, k, v, full_block_cnt=fc, full_block_idx=fi)
    with pytest.raises(NotImplementedError, match="num_splits"):
        f(q, k, v, num_splits=2, **sparse)
    with pytest.raises(NotImplementedError, match="head dim of V"):
        f(q, k, torch.zeros(B, SK, HK, 512, dtype=torch.bfloat16, device=DEV), **sparse)
    with pytest.raises(ValueError, match="specified together"):
        f(q, k, v, mask_block_cnt=mc)
    with pytest.raises(ValueError, match="specified together"):
        f(q, k, v, full_block_cnt=fc, mask_block_cnt=mc, mask_block_idx=mi)
    with pytest.raises(ValueError, match="int32"):
        f(q, k, v, mask_block_cnt=mc.long(), mask_block_idx=mi)
    with pytest.raises(ValueError, match="device of q"):
        f(q, k, v, mask_block_cnt=mc.cpu(), mask_block_idx=mi)
    with pytest.raises(ValueError, match="mask_block_idx must have shape"):
        f(q, k, v, mask_block_cnt=mc, mask_block_idx=mi[..., :5])
    with pytest.raises(ValueError, match="mask_block_cnt must have shape"):
        f(q, k, v, mask_block_cnt=mc[:, :2], mask_block_idx=mi)
    with pytest.raises(ValueError, match="full_block_idx must have shape"):
        f(q, k, v, full_block_cnt=fc, full_block_idx=fi[:, :, :2], mask_block_cnt=mc, mask_block_idx=mi)
    # the varlen function has no block-sparse arguments (the reference refuses the combination)
    with pytest.raises(TypeError):
        _cute().flash_attn_varlen_func(q, k, v, mask_block_cnt=mc, mask_block_idx=mi)
    # accepted and ignored / no split: num_splits 0 and 1, pack_gqa
    out, lse = f(q, k, v, num_splits=0, pack_gqa=True, **sparse)
    assert last_plan() == "bs_fwd_kernel D=64 waves=4 block_m=128 splits=1"
    # forward only
    qg = q.clone().requires_grad_(True)
    out, _ = f(qg, k, v, **sparse)
    with pytest.raises(NotImplementedError, match="block-sparse backward"):
        out.sum().backward()
