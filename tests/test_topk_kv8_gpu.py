"""GPU tests of the top-k token-sparse MLA decode over the fp8 (e4m3) latent cache: flash_attn_with_kvcache_topk(k_descale=,
v_descale=), i.e. fa_fwd_topk_kv8 and tk8_fwd_kernel (csrc/fa_fwd_kernel_tk8.h).  Structure: tests/test_topk_kv_gpu.py's _run;
cache values and descales: tests/test_qv8_kvcache_gpu.py's.  Reference: the fp64 restatement of the definition on the cache
dequantised exactly on the CPU (e4m3 -> fp32, times the descale).  Bound: |out - ref| <= 3 |pt - ref| + 1e-5, pt the oracle in
q's dtype on the dequantised rows; lse within 2e-3; empty rows exactly out = 0, lse = +inf."""
import math

import pytest
import torch

from parity_helpers import last_plan
from test_qv8_kvcache_gpu import _descales
from test_topk_kv_gpu import _fa3, _fillers, _input_precision, _lists, _reference, _specials

pytestmark = pytest.mark.gpu
DEV, F8 = "cuda", torch.float8_e4m3fn


def _run(dtype=torch.bfloat16, sq=1, h=16, hk=1, d=64, dv=512, sks=(70, 200), cap=256, topk=65, page=None, batch_idx=False, qv=True,
         shared=False, splits=1, edit=None, nan_rest=False, desc=None, check=True):
    """One call against the reference.  edit(idx, sks): changes the lists in place.  nan_rest: every cache row no valid entry
    names holds the NaN byte 0x7F.  Returns (out, lse, call, idx_dev, dense)."""
    b = len(sks)
    gen = torch.Generator().manual_seed(h + topk + d + sq)
    rnd = lambda *shape: torch.randn(*shape, generator=gen)
    q, qv_t = rnd(b, sq, h, d).to(dtype), rnd(b, sq, h, dv).to(dtype) if qv else None
    slots = b + 2 if batch_idx else b
    logical = rnd(slots, cap, hk, d + dv).to(F8)
    slot = torch.tensor([slots - 1 - i for i in range(b)], dtype=torch.int32) if batch_idx else torch.arange(b, dtype=torch.int32)
    kd, vd = (_descales(b, hk, 0), _descales(b, hk, 3)) if desc is None else (torch.full((b, hk), desc[0]), torch.full((b, hk), desc[1]))
    idx = _lists(b, sq, 1 if shared else hk, topk, sks, seed=topk + h)
    if edit:
        edit(idx, sks)
    if nan_rest:
        named = torch.zeros(slots, cap, hk, dtype=torch.bool)
        for i in range(b):
            for kh in range(hk):
                e = idx[i, :, 0 if shared else kh].flatten().long()
                named[int(slot[i]), e[(e >= 0) & (e < sks[i])], kh] = True
        logical.view(torch.uint8)[~named] = 0x7F
    table, cache = None, logical.view(torch.uint8)
    if page:  # pages of the logical rows behind a shuffled table
        npg = -(-cap // page)
        table = torch.randperm(b * npg, generator=gen).view(b, npg).to(torch.int32)
        padded = torch.full((b, npg * page, hk, d + dv), 0x7F if nan_rest else 0, dtype=torch.uint8)
        padded[:, :cap] = cache
        cache = torch.empty(b * npg, page, hk, d + dv, dtype=torch.uint8)
        cache[table.flatten().long()] = padded.view(b * npg, page, hk, d + dv)
    cache, idx_dev = cache.to(DEV).view(F8), idx.to(DEV)
    kw = dict(qv=None if qv_t is None else qv_t.to(DEV), cache_seqlens=torch.tensor(sks, dtype=torch.int32, device=DEV),
              cache_batch_idx=slot.to(DEV) if batch_idx else None, page_table=None if table is None else table.to(DEV),
              return_softmax_lse=True, k_descale=kd.to(DEV), v_descale=vd.to(DEV))
    tensors = (q.to(DEV), cache[..., :d], cache[..., d:])
    call = lambda **over: _fa3().flash_attn_with_kvcache_topk(*tensors, idx_dev, **{**kw, "num_splits": splits, **over})
    dense = lambda: _fa3().flash_attn_with_kvcache(*tensors, **kw, num_splits=1)[:2]
    out, lse = call()
    plan = last_plan()
    assert plan.startswith(f"tk8_fwd_kernel DVT={256 if dv <= 256 else 512} waves=4 topk={topk} splits="), plan
    if splits:
        assert plan.endswith(f"splits={splits}"), plan
    assert out.shape == (b, sq, h, dv) and lse.shape == (b, h, sq) and out.dtype == dtype
    _check(out, lse, q, qv_t, logical, slot, kd, vd, idx, sks, shared, d) if check else None
    return out, lse, call, idx_dev, dense


def _check(out, lse, q, qv_t, logical, slot, kd, vd, idx, sks, shared, d):
    (b, sq, h, _), hk = out.shape, logical.shape[2]
    g = h // hk
    for i in range(b):
        for t in range(sq):
            for kh in range(hk):
                hs = slice(kh * g, (kh + 1) * g)
                # exact: e4m3 -> fp32, times the descale.  (NaN rows become 0 for the reference alone: it gathers row 0 for a
                # masked entry; a NaN the kernel read would still show in `got`)
                k32 = torch.nan_to_num(logical[int(slot[i]), :, kh, :d].float() * kd[i, kh])
                v32 = torch.nan_to_num(logical[int(slot[i]), :, kh, d:].float() * vd[i, kh])
                e = idx[i, t, 0 if shared else kh]
                qs = (q[i, t, hs], None if qv_t is None else qv_t[i, t, hs])
                got, got_lse = out[i, t, hs].float().cpu(), lse[i, hs, t].cpu()
                if not ((e >= 0) & (e < sks[i])).any():
                    assert (got == 0).all() and (got_lse == math.inf).all(), f"an empty row of batch {i}"
                    continue
                ref, lse_ref = _reference(*qs, k32, v32, e, sks[i])
                pt = _input_precision(*qs, k32.to(q.dtype), v32.to(q.dtype), e, sks[i])
                err, err_pt = (got - ref).abs().max().item(), (pt.double() - ref).abs().max().item()
                print(f"batch {i} token {t} kv head {kh}: err {err:.3e}, input precision {err_pt:.3e}")
                assert math.isfinite(err) and err <= 3 * err_pt + 1e-5, f"max err {err:.3e} > bound {3 * err_pt + 1e-5:.3e}"
                assert (got_lse - lse_ref).abs().max().item() <= 2e-3


CASES = dict(
    **{f"topk{k}": dict(topk=k) for k in (1, 63, 64, 65, 130, 321)},                 # 321: six tiles, 385: an odd count (7)
    topk385=dict(topk=385, cap=512, sks=(70, 500)), g1=dict(h=1), g40=dict(h=40),
    per_head_two_tokens=dict(sq=2, h=32, hk=2), shared_two_tokens=dict(sq=2, h=32, hk=2, shared=True),
    dv256_fp16=dict(dv=256, dtype=torch.float16), d16_dv272_no_qv=dict(d=16, dv=272, qv=False),
    batch_idx=dict(batch_idx=True), page16=dict(page=16, topk=130), page64_dv256=dict(page=64, dv=256, hk=2, h=4),
    specials_nan_rest=dict(edit=_specials, nan_rest=True, topk=130), specials_nan_rest_page16=dict(edit=_specials, nan_rest=True, page=16, topk=130),
    fillers_only=dict(edit=_fillers, nan_rest=True), fillers_only_split=dict(edit=_fillers, topk=130, splits=3),
    empty_cache=dict(sks=(0, 0), nan_rest=True), empty_cache_split=dict(sks=(0, 70), topk=130, splits=2, page=16),
    **{f"splits{n}": dict(topk=130, splits=n, sks=(70, 256)) for n in (3, 4, 0)},     # three tiles: one part of four is empty
    split_part_of_fillers=dict(topk=130, splits=3, edit=lambda idx, sks: idx[..., 64:128].fill_(-1)),
    descales_not_powers_of_two=dict(desc=(0.3, 1.7), topk=130),
)


@pytest.mark.parametrize("case", CASES.values(), ids=CASES.keys())
def test_topk_kv8(case):
    _run(**case)


def test_topk_kv8_twice_and_listing_everything_is_the_dense_fp8_call():
    """The same call twice is bit-equal; with every position listed in order the unsplit result is bit-equal, out and lse, to
    flash_attn_with_kvcache(qv=, k_descale=, v_descale=, num_splits=1) on the same cache."""
    def everything(idx, sks):
        for i, sk in enumerate(sks):
            idx[i] = torch.where(torch.arange(256) < sk, torch.arange(256), -1).to(torch.int32)
    for page in (None, 64):
        out, lse, call, _, dense = _run(topk=256, sks=(200, 70), edit=everything, page=page)
        for other in (call(), dense()):
            assert torch.equal(out, other[0]) and torch.equal(lse, other[1])


def test_topk_kv8_reads_what_the_append_wrote_and_replays_the_list_it_finds():
    """kvcache_append_fp8 writes three rows per sequence; this call reads them on the returned fill levels and meets the
    reference on the cache as written; the pair, captured once, replayed after indices was overwritten equals the eager call."""
    b, cap, d, dv, topk, old = 2, 256, 64, 512, 130, (5, 70)
    gen = torch.Generator().manual_seed(7)
    rnd = lambda *shape: torch.randn(*shape, generator=gen)
    cache = rnd(b, cap, 1, d + dv).to(F8).to(DEV)
    kc, vc = cache[..., :d], cache[..., d:]
    q, qv = rnd(b, 1, 16, d).bfloat16(), rnd(b, 1, 16, dv).bfloat16()
    k_pe, latent = rnd(b, 3, 1, d).bfloat16().to(DEV), rnd(b, 3, 1, dv).bfloat16().to(DEV)
    kd, vd, lens = _descales(b, 1, 0), _descales(b, 1, 3), torch.tensor(old, dtype=torch.int32, device=DEV)
    sks = tuple(n + 3 for n in old)
    idx = _lists(b, 1, 1, topk, sks, 0)
    idx[:, ..., :3] = torch.tensor([[n, n + 1, n + 2] for n in old], dtype=torch.int32).view(b, 1, 1, 3)  # the appended rows
    idx_dev, q_dev, qv_dev, kd_dev, vd_dev = idx.to(DEV), q.to(DEV), qv.to(DEV), kd.to(DEV), vd.to(DEV)

    def pair():
        new = _fa3().kvcache_append_fp8(kc, vc, k_pe, latent, lens, kd_dev, vd_dev)
        return (*_fa3().flash_attn_with_kvcache_topk(q_dev, kc, vc, idx_dev, qv=qv_dev, cache_seqlens=new, num_splits=0,
                                                     return_softmax_lse=True, k_descale=kd_dev, v_descale=vd_dev), new)
    out, lse, new = pair()
    assert new.tolist() == list(sks) and last_plan().startswith("tk8_fwd_kernel DVT=512 waves=4 topk=130")
    _check(out, lse, q, qv, cache.cpu(), torch.arange(b), kd, vd, idx, sks, False, d)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g_out, g_lse, _ = pair()
    for seed in (1, 2, 3):
        idx_dev.copy_(_lists(b, 1, 1, topk, sks, seed).to(DEV))
        graph.replay()
        eager = pair()
        assert torch.equal(g_out, eager[0]) and torch.equal(g_lse, eager[1]) and not torch.equal(g_out, out)
