"""GPU tests of the top-k token-sparse MLA decode: hopper_interface.flash_attn_with_kvcache_topk / torch.ops.flash_attn_3.fwd_kvcache_topk,
i.e. fa_fwd_topk_kv and tk_fwd_kernel (csrc/fa_fwd_kernel_tk.h), against an fp64 restatement of the definition.  The bound is
parity_helpers._check_rows': twice the error of the same math in the input precision + 1e-5 for out, 2e-3 for lse."""
import math

import pytest
import torch

from oracle import attention_ref as oracle
from parity_helpers import last_plan

pytestmark = pytest.mark.gpu
DEV, IMAX = "cuda", 2 ** 31 - 1


def _fa3():
    from flash_attention_annotated_amd import hopper_interface
    return hopper_interface


def _reference(q, qv, k, v, idx, sk):
    """fp64, one (batch, token, kv head): q (g, d), qv (g, dv) | None, k (cap, d), v (cap, dv), idx (topk,) -> out (g, dv), lse (g,)."""
    ok = (idx >= 0) & (idx < sk)
    rows = torch.where(ok, idx, 0).long()  # (a masked entry gathers row 0: valid whenever any entry is)
    kk, vv = k[rows].double(), v[rows].double()
    s = q.double() @ kk.T + (qv.double() @ vv.T if qv is not None else 0)
    s = (s * (q.shape[-1] + (v.shape[-1] if qv is not None else 0)) ** -0.5).masked_fill(~ok, -math.inf)
    return torch.softmax(s, -1) @ vv, torch.logsumexp(s, -1)


def _input_precision(q, qv, k, v, idx, sk):
    ok = (idx >= 0) & (idx < sk)
    rows = torch.where(ok, idx, 0).long()  # (a masked entry gathers row 0: valid whenever any entry is)
    bias = torch.zeros(1, 1, 1, len(idx)).masked_fill(~ok, -math.inf)
    return oracle.attention_ref(q[None, None], k[rows][None, :, None], v[rows][None, :, None], attn_bias=bias, upcast=False,
                                reorder_ops=True, qv=None if qv is None else qv[None, None])[0][0, 0]


def _lists(b, sq, nl, topk, sks, seed):
    g = torch.Generator().manual_seed(seed)
    idx = torch.full((b, sq, nl, topk), -1, dtype=torch.int32)
    for i in range(b):
        for t in range(sq):
            for l in range(nl):
                n = min(topk, sks[i])
                idx[i, t, l, :n] = torch.randperm(sks[i], generator=g)[:n].to(torch.int32)
    return idx


def _run(dtype=torch.bfloat16, sq=1, h=16, hk=1, d=64, dv=512, sks=(70, 200), cap=256, topk=65, page=None, batch_idx=False, qv=True,
         shared=False, splits=1, edit=None, nan_tail=False, check=True):
    """One call against the reference.  edit(idx, sks): changes the lists in place.  Returns (out, lse, call) for more checks."""
    b = len(sks)
    gen = torch.Generator().manual_seed(h + topk + d + sq)
    rnd = lambda *shape: torch.randn(*shape, generator=gen).to(dtype)
    q, qv_t = rnd(b, sq, h, d), rnd(b, sq, h, dv) if qv else None
    slots = b + 2 if batch_idx else b
    logical = rnd(slots, cap, hk, d + dv)
    slot = torch.tensor([slots - 1 - i for i in range(b)], dtype=torch.int32) if batch_idx else torch.arange(b, dtype=torch.int32)
    if nan_tail:
        for i in range(b):
            logical[slot[i], sks[i]:] = float("nan")
    idx = _lists(b, sq, 1 if shared else hk, topk, sks, seed=topk + h)
    if edit:
        edit(idx, sks)
    table, cache = None, logical
    if page:  # pages of the logical rows behind a shuffled table
        npg = -(-cap // page)
        table = torch.randperm(b * npg, generator=gen).view(b, npg).to(torch.int32)
        padded = torch.full((b, npg * page, hk, d + dv), float("nan") if nan_tail else 0.0, dtype=dtype)
        padded[:, :cap] = logical
        cache = torch.empty(b * npg, page, hk, d + dv, dtype=dtype)
        cache[table.flatten().long()] = padded.view(b * npg, page, hk, d + dv)
    cache, idx_dev = cache.to(DEV), idx.to(DEV)
    kw = dict(qv=None if qv_t is None else qv_t.to(DEV), cache_seqlens=torch.tensor(sks, dtype=torch.int32, device=DEV),
              cache_batch_idx=slot.to(DEV) if batch_idx else None, page_table=None if table is None else table.to(DEV),
              return_softmax_lse=True)
    tensors = (q.to(DEV), cache[..., :d], cache[..., d:])
    call = lambda **over: _fa3().flash_attn_with_kvcache_topk(*tensors, idx_dev, **{**kw, "num_splits": splits, **over})
    dense = lambda: _fa3().flash_attn_with_kvcache(*tensors, **kw, num_splits=1)[:2]
    out, lse = call()
    plan = last_plan()
    assert plan.startswith(f"tk_fwd_kernel DVT={256 if dv <= 256 else 512} waves=4 topk={topk} splits="), plan
    if splits:
        assert plan.endswith(f"splits={splits}"), plan
    assert out.shape == (b, sq, h, dv) and lse.shape == (b, h, sq)
    g = h // hk
    for i in range(b if check else 0):
        for t in range(sq):
            for kh in range(hk):
                hs = slice(kh * g, (kh + 1) * g)
                args = (q[i, t, hs], None if qv_t is None else qv_t[i, t, hs], logical[slot[i], :, kh, :d], logical[slot[i], :, kh, d:],
                        idx[i, t, 0 if shared else kh], sks[i])
                got, got_lse = out[i, t, hs].float().cpu(), lse[i, hs, t].cpu()
                if not ((args[4] >= 0) & (args[4] < sks[i])).any():
                    assert (got == 0).all() and (got_lse == math.inf).all(), f"an empty row of batch {i}"
                    continue
                ref, lse_ref = _reference(*args)
                err, err_pt = (got - ref).abs().max().item(), (_input_precision(*args).double() - ref).abs().max().item()
                print(f"batch {i} token {t} kv head {kh}: err {err:.3e}, input precision {err_pt:.3e}")
                assert math.isfinite(err) and err <= 2 * err_pt + 1e-5, f"max err {err:.3e} > bound {2 * err_pt + 1e-5:.3e}"
                assert (got_lse - lse_ref).abs().max().item() <= 2e-3
    return out, lse, call, idx_dev, dense


def _specials(idx, sks):
    """-1, sk, the capacity and INT32_MAX between valid entries of the same tile, and a duplicated entry."""
    for i, sk in enumerate(sks):
        idx[i, ..., 1::7] = torch.tensor([-1, sk, 256, IMAX, -2 ** 31, sk + 1], dtype=torch.int32).repeat(4)[:idx[i, ..., 1::7].shape[-1]]
        idx[i, ..., 2] = idx[i, ..., 0]


def _fillers(idx, sks):
    idx[0] = -1
    idx[1, ..., ::2] = IMAX


CASES = dict(
    **{f"topk{k}": dict(topk=k) for k in (1, 63, 64, 65, 130)},                       # ragged last tile, one entry, topk > sk
    **{f"g{g}": dict(h=g) for g in (1, 40, 128)},                                     # a partly empty / ragged second / four row blocks
    per_head_two_tokens=dict(sq=2, h=32, hk=2), shared_two_tokens=dict(sq=2, h=32, hk=2, shared=True),
    dv256_fp16=dict(dv=256, dtype=torch.float16), dv256_no_qv=dict(dv=256, qv=False), d24_dv264=dict(d=24, dv=264),
    d24_dv264_fp16_no_qv=dict(d=24, dv=264, dtype=torch.float16, qv=False), fp16_no_qv=dict(dtype=torch.float16, qv=False),
    batch_idx=dict(batch_idx=True), page16=dict(page=16, topk=130), page64_dv256=dict(page=64, dv=256, hk=2, h=4),
    specials_nan_tail=dict(edit=_specials, nan_tail=True, topk=130), specials_nan_tail_page16=dict(edit=_specials, nan_tail=True, page=16, dv=256),
    fillers_only=dict(edit=_fillers, nan_tail=True), fillers_only_split=dict(edit=_fillers, topk=130, splits=3),
    empty_cache=dict(sks=(0, 0), nan_tail=True), empty_cache_split=dict(sks=(0, 70), topk=130, splits=2, page=16),
    **{f"splits{n}": dict(topk=130, splits=n, sks=(70, 256)) for n in (3, 4, 0)},     # three tiles: one part of four is empty
    split_part_of_fillers=dict(topk=130, splits=3, edit=lambda idx, sks: idx[..., 64:128].fill_(-1)),
)


@pytest.mark.parametrize("case", CASES.values(), ids=CASES.keys())
def test_topk_kv(case):
    _run(**case)


def test_topk_kv_twice_and_listing_everything_is_the_dense_call():
    """The same call twice is bit-equal; with every position listed in order the unsplit result is bit-equal to
    flash_attn_with_kvcache(qv=) on the same cache: the same operations in the same order."""
    def everything(idx, sks):
        for i, sk in enumerate(sks):
            idx[i] = torch.where(torch.arange(256) < sk, torch.arange(256), -1).to(torch.int32)
    for page in (None, 64):
        out, lse, call, _, dense = _run(topk=256, sks=(200, 70), edit=everything, page=page)
        for other in (call(), dense()):
            assert torch.equal(out, other[0]) and torch.equal(lse, other[1])


def test_topk_kv_graph_replays_the_list_it_finds():
    """Captured once; a replay after indices was overwritten in place equals the eager call on the new list (several replays)."""
    out, lse, call, idx_dev, _ = _run(topk=130, splits=0, check=False)
    call()  # (warm: nothing allocates or compiles inside the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g_out, g_lse = call()
    for seed in (1, 2, 3):
        idx_dev.copy_(_lists(2, 1, 1, 130, (70, 200), seed).to(DEV))
        graph.replay()
        eager = call()
        assert torch.equal(g_out, eager[0]) and torch.equal(g_lse, eager[1])
        assert not torch.equal(g_out, out)
    _run(topk=130, splits=0, edit=lambda idx, sks: idx.copy_(_lists(2, 1, 1, 130, (70, 200), 3)))  # ... which the reference holds
