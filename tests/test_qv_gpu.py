"""GPU tests of the FA3 qv argument (MLA absorbed attention, hopper/flash_api.cpp:1028-1048) and of d <= 64 beside a V head
dim in [256, 512] on paged caches / split-KV -- the qv kernel (csrc/fa_fwd_kernel_qv.h).

The oracle is oracle.attention_ref(q, k, v, qv=qv): scores += (qv * scale) @ v^T with the default scale 1 / sqrt(d + d_v),
pinned to the reference's FA3 oracle (hopper/test_util.py:287-293) by oracle/make_golden.py and tests/golden/attention_qv_golden.pt;
tests/test_oracle.py keeps the identity  Q.K^T + Qv.V^T = [Q | Qv].[K | V]^T  beside it.  Every call also asserts which kernel ran
(fa_fwd_last_plan_name).
Contract as in hopper/test_flash_attn.py:193-194,223:
    |out - out_ref|max <= 2 |out_pt - out_ref|max + fwd_atol,  fwd_atol = 2 |(out_ref + 0.3 - 0.3) - out_ref|max."""
import math

import pytest
import torch

from oracle import attention_ref as oracle
from parity_helpers import last_plan

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _fa3():
    from flash_attention_annotated_amd import hopper_interface
    return hopper_interface


def _check(out, out_ref, out_pt, rtol=2):
    err = (out.float().cpu() - out_ref.float()).abs().max().item()
    fwd_atol = 2 * (out_ref.float() + 0.3 - 0.3 - out_ref.float()).abs().max().item()
    bound = rtol * (out_pt.float() - out_ref.float()).abs().max().item() + fwd_atol
    assert math.isfinite(err) and err <= bound, f"max err {err:.3e} > bound {bound:.3e}"


def _check_lse(lse, lse_ref):
    lse, lse_ref = lse.float().cpu(), lse_ref.float()
    fin = torch.isfinite(lse_ref)
    assert torch.equal(fin, torch.isfinite(lse))
    assert (lse[fin] - lse_ref[fin]).abs().max().item() < 2e-3 if fin.any() else True


def _refs(q, k, v, qv, **kw):
    """(out_ref, out_pt, lse_ref) of qv attention (CPU); the oracle's default scale is the kernel's (1 / sqrt(d + d_v) with qv,
    1 / sqrt(d) without)."""
    out_ref, _, lse_ref = oracle.attention_ref(q, k, v, qv=qv, return_lse=True, **kw)
    out_pt, _ = oracle.attention_ref(q, k, v, qv=qv, upcast=False, reorder_ops=True, **kw)
    return out_ref, out_pt, lse_ref


def _ran(dvt, softcap=False, splits=None):
    """The call just made launched fwd_kernel_qv with this V tile (and split count, when given)."""
    plan = last_plan()
    assert plan.startswith(f"fwd_kernel_qv DVT={dvt} waves=4{' SOFTCAP' if softcap else ''} block_m="), plan
    if splits is not None:
        assert f" splits={splits}" in plan, plan


DENSE = [  # (dtype, b, sq, sk, h, hk, d, dv, causal, window, softcap, chunk)
    (torch.bfloat16, 2, 37, 113, 4, 4, 64, 512, False, (-1, -1), 0.0, 0),
    (torch.float16, 2, 65, 200, 8, 2, 64, 256, True, (-1, -1), 0.0, 0),
    (torch.bfloat16, 1, 129, 91, 6, 1, 32, 384, True, (-1, -1), 0.0, 0),   # seqlen_q > seqlen_k
    (torch.bfloat16, 2, 50, 300, 4, 2, 64, 512, False, (40, 7), 0.0, 0),
    (torch.float16, 1, 80, 257, 4, 1, 32, 512, False, (-1, -1), 15.0, 0),
    (torch.bfloat16, 2, 61, 190, 8, 8, 64, 384, True, (-1, -1), 0.0, 48),
    (torch.bfloat16, 1, 3, 1000, 16, 1, 64, 512, True, (-1, -1), 0.0, 0),
]


@pytest.mark.parametrize("case", DENSE, ids=[f"c{i}" for i in range(len(DENSE))])
def test_qv_dense(case):
    dtype, b, sq, sk, h, hk, d, dv, causal, window, softcap, chunk = case
    torch.manual_seed(sum(case[1:8]))
    q = torch.randn(b, sq, h, d, dtype=dtype)
    qv = torch.randn(b, sq, h, dv, dtype=dtype)
    k = torch.randn(b, sk, hk, d, dtype=dtype)
    v = torch.randn(b, sk, hk, dv, dtype=dtype)
    out, lse = _fa3().flash_attn_func(q.to(DEV), k.to(DEV), v.to(DEV), qv=qv.to(DEV), causal=causal, window_size=window,
                                      softcap=softcap, attention_chunk=chunk, return_attn_probs=True)
    _ran(256 if dv <= 256 else 512, softcap > 0)
    out_ref, out_pt, lse_ref = _refs(q, k, v, qv, causal=causal, window_size=window, softcap=softcap, attention_chunk=chunk)
    assert out.shape == (b, sq, h, dv)
    _check(out, out_ref, out_pt)
    _check_lse(lse, lse_ref)


def test_qv_varlen_with_empty_sequence():
    torch.manual_seed(3)
    lens_q, lens_k = [17, 0, 40], [50, 9, 130]
    h, hk, d, dv = 8, 2, 64, 512
    cu_q = torch.tensor([0] + list(torch.tensor(lens_q).cumsum(0)), dtype=torch.int32)
    cu_k = torch.tensor([0] + list(torch.tensor(lens_k).cumsum(0)), dtype=torch.int32)
    q = torch.randn(sum(lens_q), h, d, dtype=torch.bfloat16)
    qv = torch.randn(sum(lens_q), h, dv, dtype=torch.bfloat16)
    k = torch.randn(sum(lens_k), hk, d, dtype=torch.bfloat16)
    v = torch.randn(sum(lens_k), hk, dv, dtype=torch.bfloat16)
    out, lse = _fa3().flash_attn_varlen_func(q.to(DEV), k.to(DEV), v.to(DEV), cu_q.to(DEV), cu_k.to(DEV), max(lens_q),
                                             max(lens_k), qv=qv.to(DEV), causal=True, return_attn_probs=True)
    _ran(512, splits=1)
    for i in range(3):
        if lens_q[i] == 0:
            continue
        sl_q, sl_k = slice(cu_q[i], cu_q[i + 1]), slice(cu_k[i], cu_k[i + 1])
        ref, pt, lse_ref = _refs(q[sl_q][None], k[sl_k][None], v[sl_k][None], qv[sl_q][None], causal=True)
        _check(out[sl_q][None], ref, pt)
        _check_lse(lse[:, sl_q][None], lse_ref)


def _mla_cache(b, sk_max, hk, d, dv, dtype, page=None, seed=0):
    """One (…, d + dv) cache tensor; K and V are its column views.  page: paged layout with a shuffled block table."""
    g = torch.Generator().manual_seed(seed)
    logical = torch.randn(b, sk_max, hk, d + dv, generator=g).to(dtype)
    if page is None:
        cache = logical.to(DEV)
        return logical, cache, None
    npg = -(-sk_max // page)
    perm = torch.randperm(b * npg, generator=g)
    table = perm.view(b, npg).to(torch.int32)
    paged = torch.zeros(b * npg, page, hk, d + dv, dtype=dtype)
    padded = torch.zeros(b, npg * page, hk, d + dv, dtype=dtype)
    padded[:, :sk_max] = logical
    for i in range(b):
        for j in range(npg):
            paged[table[i, j]] = padded[i, j * page:(j + 1) * page]
    return logical, paged.to(DEV), table.to(DEV)


def _kv_ref(logical, i, lo, hi, d):
    kk = logical[i:i + 1, lo:hi]
    return kk[..., :d], kk[..., d:]


KV = [  # (h, hk, sq, page, num_splits, causal)
    (16, 1, 1, None, 1, False),
    (16, 1, 2, 64, 0, True),
    (128, 1, 1, 16, 3, False),
    (128, 1, 4, 1, 0, True),
    (16, 4, 2, None, 3, True),   # GQA
    (16, 1, 1, 64, 1, False),
]


@pytest.mark.parametrize("case", KV, ids=[f"h{c[0]}hk{c[1]}sq{c[2]}p{c[3]}s{c[4]}" for c in KV])
def test_qv_kvcache_mla(case):
    h, hk, sq, page, splits, causal = case
    b, d, dv, sk_max, dtype = 3, 64, 512, 700, torch.bfloat16
    logical, cache, table = _mla_cache(b, sk_max, hk, d, dv, dtype, page, seed=h + sq)
    torch.manual_seed(h * 7 + sq)
    seqlens = torch.tensor([sk_max, 333, 65], dtype=torch.int32)
    q = torch.randn(b, sq, h, d, dtype=dtype)
    qv = torch.randn(b, sq, h, dv, dtype=dtype)
    out, lse, *_ = _fa3().flash_attn_with_kvcache(
        q.to(DEV), cache[..., :d], cache[..., d:], qv=qv.to(DEV), cache_seqlens=seqlens.to(DEV), page_table=table,
        causal=causal, num_splits=splits, return_softmax_lse=True)
    _ran(512, splits=splits or None)  # (0: the heuristic's count)
    for i in range(b):
        k_i, v_i = _kv_ref(logical, i, 0, int(seqlens[i]), d)
        ref, pt, lse_ref = _refs(q[i:i + 1], k_i, v_i, qv[i:i + 1], causal=causal)
        _check(out[i:i + 1], ref, pt)
        _check_lse(lse[i:i + 1], lse_ref)


@pytest.mark.parametrize("rotary", [False, True])
def test_qv_kvcache_append(rotary):
    """k / v appended in place land in both column views of the one cache tensor; rotary touches q and the keys only."""
    b, hk, h, d, dv, sk_max, sn, dtype = 2, 1, 16, 64, 512, 300, 2, torch.bfloat16
    logical, cache, _ = _mla_cache(b, sk_max, hk, d, dv, dtype, None, seed=11)
    torch.manual_seed(12)
    seqlens = torch.tensor([100, 250], dtype=torch.int32)
    q = torch.randn(b, sn, h, d, dtype=dtype)
    qv = torch.randn(b, sn, h, dv, dtype=dtype)
    k_new = torch.randn(b, sn, hk, d, dtype=dtype)
    v_new = torch.randn(b, sn, hk, dv, dtype=dtype)
    cos = sin = None
    if rotary:
        ang = torch.rand(sk_max, 16) * 2 * math.pi
        cos, sin = torch.cos(ang).to(dtype), torch.sin(ang).to(dtype)
    out = _fa3().flash_attn_with_kvcache(
        q.to(DEV), cache[..., :d], cache[..., d:], k=k_new.to(DEV), v=v_new.to(DEV), qv=qv.to(DEV),
        rotary_cos=None if cos is None else cos.to(DEV), rotary_sin=None if sin is None else sin.to(DEV),
        cache_seqlens=seqlens.to(DEV), causal=True, rotary_interleaved=False, num_splits=1)
    _ran(512, splits=1)
    k_app = k_new if not rotary else oracle.apply_rotary_emb_ref(k_new, cos, sin, seqlens, interleaved=False)
    q_use = q if not rotary else oracle.apply_rotary_emb_ref(q, cos, sin, seqlens, interleaved=False)
    exp = logical.clone()
    for i in range(b):
        s0 = int(seqlens[i])
        exp[i, s0:s0 + sn, :, :d] = k_app[i]
        exp[i, s0:s0 + sn, :, d:] = v_new[i]
    got = cache.cpu()
    assert torch.equal(got[..., d:], exp[..., d:])
    assert (got[..., :d].float() - exp[..., :d].float()).abs().max().item() <= (0.02 if rotary else 0.0)
    for i in range(b):
        k_i, v_i = _kv_ref(got, i, 0, int(seqlens[i]) + sn, d)
        ref, pt, _ = _refs(q_use[i:i + 1], k_i, v_i, qv[i:i + 1], causal=True)
        _check(out[i:i + 1], ref, pt)


def test_qv_kvcache_batch_idx_and_leftpad():
    b, hk, h, d, dv, dtype = 3, 1, 16, 64, 512, torch.bfloat16
    logical, cache, _ = _mla_cache(5, 400, hk, d, dv, dtype, None, seed=21)
    torch.manual_seed(22)
    q = torch.randn(b, 2, h, d, dtype=dtype)
    qv = torch.randn(b, 2, h, dv, dtype=dtype)
    idx = torch.tensor([4, 0, 2], dtype=torch.int32)
    seqlens = torch.tensor([400, 123, 301], dtype=torch.int32)
    out = _fa3().flash_attn_with_kvcache(q.to(DEV), cache[..., :d], cache[..., d:], qv=qv.to(DEV),
                                         cache_seqlens=seqlens.to(DEV), cache_batch_idx=idx.to(DEV), num_splits=0)
    _ran(512)
    for i in range(b):
        k_i, v_i = _kv_ref(logical, int(idx[i]), 0, int(seqlens[i]), d)
        ref, pt, _ = _refs(q[i:i + 1], k_i, v_i, qv[i:i + 1])
        _check(out[i:i + 1], ref, pt)
    lp = torch.tensor([0, 50, 300], dtype=torch.int32)
    out = _fa3().flash_attn_with_kvcache(q.to(DEV), cache[:b, ..., :d], cache[:b, ..., d:], qv=qv.to(DEV),
                                         cache_seqlens=seqlens.to(DEV), cache_leftpad=lp.to(DEV), num_splits=3, causal=True)
    _ran(512, splits=3)
    for i in range(b):
        k_i, v_i = _kv_ref(logical, i, int(lp[i]), int(seqlens[i]), d)
        ref, pt, _ = _refs(q[i:i + 1], k_i, v_i, qv[i:i + 1], causal=True)
        _check(out[i:i + 1], ref, pt)


@pytest.mark.parametrize("page,splits", [(64, 1), (16, 1), (None, 3)])
def test_wide_v_without_qv_paged_and_split(page, splits):
    """d 64 / d_v 512 without qv on a paged cache or with split-KV (rejected before): plain attention with the wide V."""
    b, hk, h, d, dv, dtype = 2, 2, 8, 64, 512, torch.float16
    logical, cache, table = _mla_cache(b, 333, hk, d, dv, dtype, page, seed=31)
    torch.manual_seed(32)
    q = torch.randn(b, 3, h, d, dtype=dtype)
    seqlens = torch.tensor([333, 200], dtype=torch.int32)
    out = _fa3().flash_attn_with_kvcache(q.to(DEV), cache[..., :d], cache[..., d:], cache_seqlens=seqlens.to(DEV),
                                         page_table=table, num_splits=splits, causal=True)
    _ran(512, splits=splits)
    for i in range(b):
        k_i, v_i = _kv_ref(logical, i, 0, int(seqlens[i]), d)
        ref, pt, _ = _refs(q[i:i + 1], k_i, v_i, None, causal=True)
        _check(out[i:i + 1], ref, pt)


@pytest.mark.parametrize("splits", [1, 0])
def test_qv_deterministic_and_graph(splits):
    b, hk, h, d, dv, dtype = 4, 1, 128, 64, 512, torch.bfloat16
    _, cache, table = _mla_cache(b, 2048, hk, d, dv, dtype, 64, seed=41)
    torch.manual_seed(42)
    q = torch.randn(b, 1, h, d, dtype=dtype, device=DEV)
    qv = torch.randn(b, 1, h, dv, dtype=dtype, device=DEV)
    seqlens = torch.tensor([2048, 1000, 1500, 7], dtype=torch.int32, device=DEV)
    fa3 = _fa3()

    def step():
        return fa3.flash_attn_with_kvcache(q, cache[..., :d], cache[..., d:], qv=qv, cache_seqlens=seqlens, page_table=table,
                                           num_splits=splits)
    first = step()
    _ran(512, splits=1 if splits == 1 else None)
    for _ in range(19):
        assert torch.equal(step(), first)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out_g = step()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out_g, first)


def test_qv_backward_raises_and_bad_shapes_rejected():
    fa3 = _fa3()
    q = torch.randn(1, 8, 4, 64, dtype=torch.bfloat16, device=DEV, requires_grad=True)
    k = torch.randn(1, 8, 1, 64, dtype=torch.bfloat16, device=DEV)
    v = torch.randn(1, 8, 1, 512, dtype=torch.bfloat16, device=DEV)
    qv = torch.randn(1, 8, 4, 512, dtype=torch.bfloat16, device=DEV)
    out = fa3.flash_attn_func(q, k, v, qv=qv)
    _ran(512, splits=1)
    with pytest.raises(AssertionError, match="does not support qv"):
        out.sum().backward()
    with pytest.raises(RuntimeError, match="does not support qv"):
        fa3.flash_attn_func(q.detach(), k, v[..., :128].contiguous(), qv=qv[..., :128].contiguous())
    with pytest.raises(RuntimeError, match="does not support cu_seqlens_k_new"):
        fa3.flash_attn_with_kvcache(q.detach(), k, v, k=k, v=v, qv=qv, cache_seqlens=0,
                                    cu_seqlens_k_new=torch.zeros(2, dtype=torch.int32, device=DEV))

# ---- the kernel's edges: head dims that are multiples of 8 only, GQA packs that cross query rows inside a 32-row block,
#      clamped loads, empty splits.  Every case asserts the kernel that ran.
EDGE = [  # (dtype, b, sq, sk, h, hk, d, dv, causal, window, softcap, chunk)
    (torch.bfloat16, 1, 70, 300, 4, 2, 8, 264, True, (-1, -1), 0.0, 0),
    (torch.float16, 2, 45, 257, 6, 2, 24, 328, False, (30, 9), 0.0, 0),
    (torch.bfloat16, 1, 90, 200, 3, 1, 40, 504, True, (-1, -1), 0.0, 0),
    (torch.float16, 1, 33, 130, 5, 1, 56, 264, False, (-1, -1), 0.0, 0),
    (torch.float16, 1, 40, 333, 2, 2, 24, 504, False, (-1, -1), 12.0, 0),
    (torch.bfloat16, 1, 50, 200, 4, 2, 64, 256, False, (-1, -1), 15.0, 0),   # DVT = 256 with softcap
    (torch.bfloat16, 1, 43, 120, 3, 1, 64, 256, True, (-1, -1), 0.0, 0),     # g = 3: a 32-row block starts mid query row
    (torch.float16, 2, 29, 150, 5, 1, 32, 384, False, (20, 5), 0.0, 0),      # g = 5 under a two-sided window
    (torch.bfloat16, 1, 37, 190, 7, 1, 64, 512, True, (-1, -1), 0.0, 48),    # g = 7 under attention_chunk
]


@pytest.mark.parametrize("case", EDGE, ids=[f"d{c[6]}dv{c[7]}g{c[4] // c[5]}c{i}" for i, c in enumerate(EDGE)])
def test_qv_edges_dense(case):
    test_qv_dense(case)


@pytest.mark.parametrize("dv", [256, 512])
@pytest.mark.parametrize("page,splits", [(16, 1), (None, 3), (16, 3)])
def test_wide_v_tiles_without_qv(dv, page, splits):
    """Both V tiles of the qv kernel without qv: a paged cache of 16-key pages, and three splits."""
    b, hk, h, d, dtype = 2, 2, 6, 64, torch.bfloat16
    logical, cache, table = _mla_cache(b, 333, hk, d, dv, dtype, page, seed=51 + dv)
    torch.manual_seed(52)
    q = torch.randn(b, 3, h, d, dtype=dtype)
    seqlens = torch.tensor([333, 200], dtype=torch.int32)
    out, lse, *_ = _fa3().flash_attn_with_kvcache(q.to(DEV), cache[..., :d], cache[..., d:], cache_seqlens=seqlens.to(DEV),
                                                  page_table=table, num_splits=splits, causal=True, return_softmax_lse=True)
    _ran(dv, splits=splits)
    for i in range(b):
        k_i, v_i = _kv_ref(logical, i, 0, int(seqlens[i]), d)
        ref, pt, lse_ref = _refs(q[i:i + 1], k_i, v_i, None, causal=True)
        _check(out[i:i + 1], ref, pt)
        _check_lse(lse[i:i + 1], lse_ref)


@pytest.mark.parametrize("page", [None, 16])
def test_qv_clamped_loads_never_leak(page):
    """Cache rows past cache_seqlens hold NaN (the kernel clamps rows to seqlen - 1: a wrong clamp shows as NaN); the dense
    cache is a padded row layout -- row stride wider than d + d_v -- with NaN in the gap, next to head dims (24 / 328) whose
    last column chunks are clamped duplicates."""
    b, hk, h, d, dv, sk_max, dtype = 2, 1, 6, 24, 328, 300, torch.float16
    logical, cache, table = _mla_cache(b, sk_max, hk, d, dv, dtype, page, seed=61)
    seqlens = torch.tensor([211, 77], dtype=torch.int32)
    if page is None:
        wide = torch.full((b, sk_max, hk, d + dv + 40), float("nan"), dtype=dtype)
        wide[..., :d + dv] = logical
        for i in range(b):
            wide[i, int(seqlens[i]):] = float("nan")
        cache = wide.to(DEV)
    else:
        pages = cache.cpu()
        for i in range(b):
            for r in range(int(seqlens[i]), table.shape[1] * page):
                pages[int(table[i, r // page]), r % page] = float("nan")
        cache = pages.to(DEV)
    torch.manual_seed(62)
    q = torch.randn(b, 5, h, d, dtype=dtype)
    qv = torch.randn(b, 5, h, dv, dtype=dtype)
    out, lse, *_ = _fa3().flash_attn_with_kvcache(q.to(DEV), cache[..., :d], cache[..., d:d + dv], qv=qv.to(DEV),
                                                  cache_seqlens=seqlens.to(DEV), page_table=table, causal=True, num_splits=1,
                                                  return_softmax_lse=True)
    _ran(512, splits=1)
    assert torch.isfinite(out.float()).all() and torch.isfinite(lse).all()
    for i in range(b):
        k_i, v_i = _kv_ref(logical, i, 0, int(seqlens[i]), d)
        ref, pt, lse_ref = _refs(q[i:i + 1], k_i, v_i, qv[i:i + 1], causal=True)
        _check(out[i:i + 1], ref, pt)
        _check_lse(lse[i:i + 1], lse_ref)


def test_qv_split_with_empty_splits():
    """Three splits over a 700-key cache of which one batch entry uses 40 keys: its later splits see no key at all and hand
    LSE = +inf partials to the merge; out and LSE against the oracle."""
    b, hk, h, d, dv, dtype = 2, 1, 16, 64, 512, torch.bfloat16
    logical, cache, _ = _mla_cache(b, 700, hk, d, dv, dtype, None, seed=71)
    torch.manual_seed(72)
    q = torch.randn(b, 2, h, d, dtype=dtype)
    qv = torch.randn(b, 2, h, dv, dtype=dtype)
    seqlens = torch.tensor([700, 40], dtype=torch.int32)
    out, lse, *_ = _fa3().flash_attn_with_kvcache(q.to(DEV), cache[..., :d], cache[..., d:], qv=qv.to(DEV),
                                                  cache_seqlens=seqlens.to(DEV), num_splits=3, causal=True, return_softmax_lse=True)
    _ran(512, splits=3)
    for i in range(b):
        k_i, v_i = _kv_ref(logical, i, 0, int(seqlens[i]), d)
        ref, pt, lse_ref = _refs(q[i:i + 1], k_i, v_i, qv[i:i + 1], causal=True)
        _check(out[i:i + 1], ref, pt)
        _check_lse(lse[i:i + 1], lse_ref)


@pytest.mark.parametrize("window", [(-1, -1), (25, 6)])
def test_qv_varlen_seqused_and_empty_last_sequence(window):
    """Packed batch, non-causal and windowed, with seqused_q / seqused_k shorter than the cu_seqlens spans and an empty last
    sequence: the used rows see the used keys only."""
    torch.manual_seed(81)
    span_q, span_k, used_q, used_k = [30, 41, 0], [90, 140, 20], [21, 41, 0], [70, 133, 20]
    h, hk, d, dv = 6, 2, 40, 264
    cu_q = torch.tensor([0, 30, 71, 71], dtype=torch.int32)
    cu_k = torch.tensor([0, 90, 230, 250], dtype=torch.int32)
    q = torch.randn(71, h, d, dtype=torch.bfloat16)
    qv = torch.randn(71, h, dv, dtype=torch.bfloat16)
    k = torch.randn(250, hk, d, dtype=torch.bfloat16)
    v = torch.randn(250, hk, dv, dtype=torch.bfloat16)
    out, lse = _fa3().flash_attn_varlen_func(
        q.to(DEV), k.to(DEV), v.to(DEV), cu_q.to(DEV), cu_k.to(DEV), max(span_q), max(span_k),
        seqused_q=torch.tensor(used_q, dtype=torch.int32, device=DEV), seqused_k=torch.tensor(used_k, dtype=torch.int32, device=DEV),
        qv=qv.to(DEV), window_size=window, return_attn_probs=True)
    _ran(512, splits=1)
    for i in range(2):
        sl_q = slice(int(cu_q[i]), int(cu_q[i]) + used_q[i])
        sl_k = slice(int(cu_k[i]), int(cu_k[i]) + used_k[i])
        ref, pt, lse_ref = _refs(q[sl_q][None], k[sl_k][None], v[sl_k][None], qv[sl_q][None], window_size=window)
        _check(out[sl_q][None], ref, pt)
        _check_lse(lse[:, sl_q][None], lse_ref)


@pytest.mark.parametrize("d,dv", [(24, 264), (56, 504)])
def test_qv_split_at_odd_head_dims(d, dv):
    """Three splits at V head dims that are no multiple of 32: the fp32 split epilogue's column clamp and the merge over
    d_v / 8 chunks, out and LSE against the oracle."""
    b, hk, h, dtype = 2, 1, 6, torch.float16
    logical, cache, _ = _mla_cache(b, 500, hk, d, dv, dtype, None, seed=91 + d)
    torch.manual_seed(92)
    q = torch.randn(b, 3, h, d, dtype=dtype)
    qv = torch.randn(b, 3, h, dv, dtype=dtype)
    seqlens = torch.tensor([500, 301], dtype=torch.int32)
    out, lse, *_ = _fa3().flash_attn_with_kvcache(q.to(DEV), cache[..., :d], cache[..., d:], qv=qv.to(DEV),
                                                  cache_seqlens=seqlens.to(DEV), num_splits=3, causal=True, return_softmax_lse=True)
    _ran(512, splits=3)
    for i in range(b):
        k_i, v_i = _kv_ref(logical, i, 0, int(seqlens[i]), d)
        ref, pt, lse_ref = _refs(q[i:i + 1], k_i, v_i, qv[i:i + 1], causal=True)
        _check(out[i:i + 1], ref, pt)
        _check_lse(lse[i:i + 1], lse_ref)
