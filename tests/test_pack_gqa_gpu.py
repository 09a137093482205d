"""GPU parity of PackGQA (`pack_gqa=True` on the FA3 and cute surfaces -> FA_FLAG_PACK_GQA -> fa::pk_fwd_kernel,
csrc/fa_fwd_kernel_pk.h): the h / h_k query heads of a kv head are packed into the rows of a tile, packed row pr = query row
pr / g of head kv_head * g + pr % g.

Every honoured case asserts that the plan that ran (parity_helpers.last_plan) is a `pk_fwd_kernel ...` one, and compares out
and LSE with the oracle under the project's forward rule (parity_helpers._check_rows):
    |O - O_ref|max <= 2 |O_pt - O_ref|max + 1e-5,   LSE within 2e-3 on the finite entries, the same +inf pattern
(O_ref: the oracle in fp32, O_pt: the same math in the inputs' precision).  Gradients: the 3 x rule of tests/test_sink_gpu.py.
Shapes are the smallest at which the row mapping can go wrong: groups of 3 that straddle 32-row wave slices and 128-row blocks,
a one-row tail block, MQA, rows without keys, empty sequences, ragged batches, every cache form, split-KV with empty parts."""
import math

import pytest
import torch

import sink_oracle
from oracle import attention_ref as oracle
from parity_helpers import last_plan

pytestmark = pytest.mark.gpu
DEV = "cuda"
I32 = torch.int32
BF16, FP16 = torch.bfloat16, torch.float16


def _fa3():
    from flash_attention_annotated_amd import hopper_interface
    return hopper_interface


def _cute():
    from flash_attention_annotated_amd import cute_interface
    return cute_interface


def _rand(*shape, dtype=BF16, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(dtype)


def _qkv(b, sq, sk, h, hk, d, dtype=BF16, seed=0):
    g = torch.Generator().manual_seed(seed)
    return tuple(torch.randn(*s, generator=g).to(dtype) for s in ((b, sq, h, d), (b, sk, hk, d), (b, sk, hk, d)))


def _cu(lens):
    return torch.tensor([sum(lens[:i]) for i in range(len(lens) + 1)], dtype=I32)


def _packed(plan, tile, splits=None, softcap=False):
    want = f"pk_fwd_kernel D={tile} waves=4{' SOFTCAP' if softcap else ''} block_m=128 splits="
    assert plan.startswith(want), f"{plan!r} is not a {want!r} plan"
    if splits is not None:
        assert plan == want + str(splits), plan


def _check(out, lse, ref, pt, lse_ref, what):
    err = (out.float().cpu() - ref.float()).abs().max().item()
    bound = 2 * (pt.float() - ref.float()).abs().max().item() + 1e-5
    lse, lse_ref = lse.float().cpu(), lse_ref.float()
    fin = torch.isfinite(lse_ref)
    lerr = (lse[fin] - lse_ref[fin]).abs().max().item() if fin.any() else 0.0
    print(f"{what}: out err {err:.3e} (bound {bound:.3e}), lse err {lerr:.3e}")
    assert math.isfinite(err) and err <= bound, f"{what}: max err {err:.3e} > bound {bound:.3e}"
    assert torch.equal(torch.isfinite(lse), fin), f"{what}: lse inf pattern"
    assert lerr <= 2e-3, f"{what}: lse err {lerr:.3e}"


def _oracle(q, k, v, **kw):
    ref, _, lse_ref = oracle.attention_ref(q, k, v, return_lse=True, **kw)
    pt, _ = oracle.attention_ref(q, k, v, upcast=False, reorder_ops=True, **kw)
    return ref, pt, lse_ref


def _fa3_dense(q, k, v, pack_gqa=True, **kw):
    out, lse = _fa3().flash_attn_func(q.to(DEV), k.to(DEV), v.to(DEV), pack_gqa=pack_gqa, return_attn_probs=True, **kw)
    plan = last_plan()
    torch.cuda.synchronize()
    return out, lse, plan


# ---- 1. g = 3 straddling blocks ---------------------------------------------------------------------------------------------

def test_g3_straddles_wave_slices_and_blocks():
    """43 rows x 3 heads = 129 packed rows: a tail block of one row, and edges of 32-row slices and of the 128-row block that
    cut a head group (32 = 10 * 3 + 2)."""
    q, k, v = _qkv(2, 43, 107, 6, 2, 64, BF16, seed=1)
    out, lse, plan = _fa3_dense(q, k, v, causal=True)
    _packed(plan, 64, splits=1)
    assert out.shape == q.shape and lse.shape == (2, 6, 43)
    _check(out, lse, *_oracle(q, k, v, causal=True), plan)


# ---- 2. MQA g = 8 -------------------------------------------------------------------------------------------------------------

MQA = dict(b=2, sq=5, sk=300, h=8, hk=1, d=128, dtype=FP16, seed=2)


@pytest.mark.parametrize("kw", [dict(), dict(window_size=(17, 0)), dict(softcap=30.0)], ids=["full", "window", "softcap"])
def test_mqa_fa3_surface(kw):
    q, k, v = _qkv(**MQA)
    out, lse, plan = _fa3_dense(q, k, v, **kw)  # (FA_FLAG_FA3_WINDOW: the FA3 window rule)
    _packed(plan, 128, splits=1, softcap="softcap" in kw)
    _check(out, lse, *_oracle(q, k, v, **kw), plan)


def test_mqa_window_under_the_fa2_rule():
    """The same window through the KV-cache route (any cache argument takes it: here an identity cache_batch_idx), whose launch
    leaves FA_FLAG_FA3_WINDOW unset (the FA2 window rule)."""
    q, k, v = _qkv(**MQA)
    lens = torch.full((2,), 300, dtype=I32, device=DEV)
    out, lse, *_ = _fa3().flash_attn_with_kvcache(q.to(DEV), k.to(DEV), v.to(DEV), cache_seqlens=lens, window_size=(17, 0),
                                                  cache_batch_idx=torch.arange(2, dtype=I32, device=DEV), num_splits=1,
                                                  pack_gqa=True, return_softmax_lse=True)
    plan = last_plan()
    _packed(plan, 128, splits=1)
    _check(out, lse, *_oracle(q, k, v, window_size=(17, 0)), plan)


# ---- 3. rows without keys ------------------------------------------------------------------------------------------------------

def test_rows_without_keys_follow_the_unpacked_convention():
    """causal with seqlen_q 40 > seqlen_k 24: rows 0..15 see no key -- out 0 and LSE +inf, as the unpacked call writes them."""
    q, k, v = _qkv(2, 40, 24, 8, 2, 128, BF16, seed=3)
    out, lse, plan = _fa3_dense(q, k, v, causal=True)
    _packed(plan, 128, splits=1)
    out0, lse0, plan0 = _fa3_dense(q, k, v, pack_gqa=None, causal=True)
    assert not plan0.startswith("pk_fwd_kernel")
    _check(out, lse, *_oracle(q, k, v, causal=True), plan)
    assert torch.equal(out[:, :16], out0[:, :16]) and not out[:, :16].any()
    assert torch.equal(lse[:, :, :16], lse0[:, :, :16]) and torch.isposinf(lse[:, :, :16]).all()
    assert torch.isfinite(lse[:, :, 16:]).all() and torch.equal(torch.isfinite(lse), torch.isfinite(lse0))


# ---- 4. varlen -------------------------------------------------------------------------------------------------------------------

LENS_Q, LENS_K = [0, 1, 37, 3, 64], [5, 9, 0, 130, 64]


def _varlen_inputs():
    h, hk, d = 8, 2, 128
    q, k, v = _rand(sum(LENS_Q), h, d, seed=4), _rand(sum(LENS_K), hk, d, seed=5), _rand(sum(LENS_K), hk, d, seed=6)
    return q, k, v, _cu(LENS_Q), _cu(LENS_K)


@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
def test_varlen(causal):
    q, k, v, cq, ck = _varlen_inputs()
    out, lse = _fa3().flash_attn_varlen_func(q.to(DEV), k.to(DEV), v.to(DEV), cq.to(DEV), ck.to(DEV), max(LENS_Q), max(LENS_K),
                                             causal=causal, pack_gqa=True, return_attn_probs=True)
    plan = last_plan()
    _packed(plan, 128, splits=1)
    assert out.shape == q.shape and lse.shape == (8, sum(LENS_Q))  # the LSE layout is (h, total_q)
    ref, lse_ref = oracle.attention_varlen_ref(q, k, v, cq, ck, causal=causal)
    pt, _ = oracle.attention_varlen_ref(q, k, v, cq, ck, causal=causal, upcast=False, reorder_ops=True)
    _check(out, lse, ref, pt, lse_ref, plan)


@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
def test_varlen_seqused_q(causal):
    """seqused_q shorter than the cu_seqlens slots: the rows of a slot past seqused_q keep what the unpacked call leaves there
    (nothing is written: the caller's `out` shows through)."""
    q, k, v, cq, ck = _varlen_inputs()
    used_q, used_k = [0, 1, 20, 2, 33], [5, 4, 0, 100, 64]
    qd, kd, vd, cqd, ckd = (t.to(DEV) for t in (q, k, v, cq, ck))
    uq, uk = torch.tensor(used_q, dtype=I32, device=DEV), torch.tensor(used_k, dtype=I32, device=DEV)

    def run(pack_gqa):
        out = torch.full(q.shape, 7.0, dtype=BF16, device=DEV)
        o, lse, *_ = torch.ops.flash_attn_3.fwd(qd, kd, vd, None, None, None, out, cqd, ckd, None, uq, uk, max(LENS_Q), max(LENS_K),
                                                None, None, None, None, None, None, None, None, None, None, causal, -1, -1, 0, 0.0,
                                                True, None, 1, pack_gqa, 0)
        plan = last_plan()
        torch.cuda.synchronize()
        return o, lse, plan
    out, lse, plan = run(True)
    out0, lse0, plan0 = run(None)
    _packed(plan, 128, splits=1)
    assert not plan0.startswith("pk_fwd_kernel") and lse.shape == (8, sum(LENS_Q))
    inside = torch.zeros(sum(LENS_Q), dtype=torch.bool)
    ref, pt = torch.zeros_like(q), torch.zeros_like(q)
    lse_ref = torch.full((8, sum(LENS_Q)), float("inf"))
    for i, (nq, nk) in enumerate(zip(used_q, used_k)):
        q0, k0 = int(cq[i]), int(ck[i])
        inside[q0:q0 + nq] = True
        if nq and nk:
            args = (q[q0:q0 + nq][None], k[k0:k0 + nk][None], v[k0:k0 + nk][None])
            r, p, l = _oracle(*args, causal=causal)
            ref[q0:q0 + nq], pt[q0:q0 + nq], lse_ref[:, q0:q0 + nq] = r[0], p[0], l[0]
    _check(out[inside.to(DEV)], lse[:, inside.to(DEV)], ref[inside], pt[inside], lse_ref[:, inside], plan)
    outside = (~inside).to(DEV)
    assert outside.any() and torch.equal(out[outside], out0[outside]) and (out[outside] == 7.0).all()


# ---- 5. KV cache -----------------------------------------------------------------------------------------------------------------

CACHE = dict(b=4, sq=6, h=8, hk=2, d=128, cap=192)
FILLS = [0, 17, 100, 64]  # ragged, one empty


def _pages(kc, vc, page, seed):
    """(b, cap, hk, d) caches -> a shuffled pool of pages + the page table."""
    b, cap, hk, d = kc.shape
    per = cap // page
    table = torch.randperm(b * per, generator=torch.Generator().manual_seed(seed)).to(I32).view(b, per)
    flat = table.flatten().long()
    kp, vp = torch.empty(b * per, page, hk, d, dtype=kc.dtype), torch.empty(b * per, page, hk, d, dtype=kc.dtype)
    kp[flat], vp[flat] = kc.reshape(-1, page, hk, d), vc.reshape(-1, page, hk, d)
    return kp, vp, table


def _cache_oracle(q, kc, vc, fills, leftpad=None, **kw):
    j = torch.arange(kc.shape[1]).view(1, -1)
    kmask = j < torch.tensor(fills).view(-1, 1)
    if leftpad is not None:
        kmask &= j >= leftpad.view(-1, 1)
    kw = dict(key_padding_mask=kmask, key_leftpad=leftpad, **kw)
    return _oracle(q, kc, vc, **kw)


@pytest.mark.parametrize("layout", ["page16", "page48", "page16_append", "batch_idx", "leftpad"])
def test_kvcache(layout):
    c = CACHE
    q = _rand(c["b"], c["sq"], c["h"], c["d"], seed=7)
    bc = c["b"] + 2 if layout == "batch_idx" else c["b"]
    kc, vc = _rand(bc, c["cap"], c["hk"], c["d"], seed=8), _rand(bc, c["cap"], c["hk"], c["d"], seed=9)
    fills, kw, leftpad = list(FILLS), {}, None
    idx = torch.arange(c["b"])
    k_ref, v_ref = kc, vc
    if layout == "batch_idx":
        idx = torch.tensor([4, 0, 5, 2])
        kw["cache_batch_idx"] = idx.to(I32).to(DEV)
        k_ref, v_ref = kc[idx], vc[idx]
    if layout == "leftpad":
        leftpad = torch.tensor([0, 3, 20, 64], dtype=I32)  # (the last one pads the whole fill away)
        kw["cache_leftpad"] = leftpad.to(DEV)
    kd, vd = kc.to(DEV), vc.to(DEV)
    if layout.startswith("page"):
        kp, vp, table = _pages(kc, vc, int(layout[4:6]), seed=10)
        kd, vd, kw["page_table"] = kp.to(DEV), vp.to(DEV), table.to(DEV)
    if layout.endswith("append"):
        kn, vn = _rand(c["b"], c["sq"], c["hk"], c["d"], seed=11), _rand(c["b"], c["sq"], c["hk"], c["d"], seed=12)
        kw.update(k=kn.to(DEV), v=vn.to(DEV))
        k_ref, v_ref = kc.clone(), vc.clone()
        for i, f in enumerate(fills):
            k_ref[i, f:f + c["sq"]], v_ref[i, f:f + c["sq"]] = kn[i], vn[i]
        after = [f + c["sq"] for f in fills]
    else:
        after = fills
    out, lse, *_ = _fa3().flash_attn_with_kvcache(q.to(DEV), kd, vd, cache_seqlens=torch.tensor(fills, dtype=I32, device=DEV),
                                                  causal=True, num_splits=1, pack_gqa=True, return_softmax_lse=True, **kw)
    plan = last_plan()
    torch.cuda.synchronize()
    _packed(plan, 128, splits=1)
    assert out.shape == q.shape and lse.shape == (c["b"], c["h"], c["sq"])
    _check(out, lse, *_cache_oracle(q, k_ref, v_ref, after, leftpad, causal=True), f"{layout}: {plan}")
    if layout.endswith("append"):  # the appended rows landed in their pages
        flat = kw["page_table"].flatten().long()
        assert torch.equal(kd[flat].reshape(kc.shape).cpu(), k_ref) and torch.equal(vd[flat].reshape(vc.shape).cpu(), v_ref)


def test_single_token_decode_keeps_its_gqa_swap():
    """seqlen_q 1: the binding folds the GQA group into the rows (h == h_k afterwards), the hint has nothing left to pack --
    the plan and the bits of the flagged call are the unflagged call's."""
    c = CACHE
    q = _rand(c["b"], 1, c["h"], c["d"], seed=13).to(DEV)
    kc, vc = _rand(c["b"], c["cap"], c["hk"], c["d"], seed=8), _rand(c["b"], c["cap"], c["hk"], c["d"], seed=9)
    kp, vp, table = (t.to(DEV) for t in _pages(kc, vc, 16, seed=10))
    lens = torch.tensor([1, 17, 100, 192], dtype=I32, device=DEV)
    res = {}
    for hint in (True, None):
        out, lse, *_ = _fa3().flash_attn_with_kvcache(q, kp, vp, cache_seqlens=lens, page_table=table, causal=True, num_splits=1,
                                                      pack_gqa=hint, return_softmax_lse=True)
        res[hint] = (out, lse, last_plan())
    assert res[True][2] == res[None][2] and not res[True][2].startswith("pk_fwd_kernel")
    assert torch.equal(res[True][0], res[None][0]) and torch.equal(res[True][1], res[None][1])


# ---- 6. ragged queries over a paged cache ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("num_splits", [1, 3])
def test_ragged_over_paged_cache(num_splits):
    lens_q, fills, cap, h, hk, d, page = [1, 1, 17, 1, 130], [100, 517, 64, 300, 411], 768, 8, 2, 128, 64
    b, tq = len(lens_q), sum(lens_q)
    q = _rand(tq, h, d, seed=14)
    kc, vc = _rand(b, cap, hk, d, seed=15), _rand(b, cap, hk, d, seed=16)
    kp, vp, table = _pages(kc, vc, page, seed=17)
    cq = _cu(lens_q)
    out, lse, *_ = _fa3().flash_attn_with_kvcache(
        q.to(DEV), kp.to(DEV), vp.to(DEV), cache_seqlens=torch.tensor(fills, dtype=I32, device=DEV), page_table=table.to(DEV),
        cu_seqlens_q=cq.to(DEV), max_seqlen_q=max(lens_q), causal=True, num_splits=num_splits, pack_gqa=True, return_softmax_lse=True)
    plan = last_plan()
    torch.cuda.synchronize()
    _packed(plan, 128, splits=num_splits)
    assert out.shape == q.shape and lse.shape == (h, tq)
    ref, pt, lse_ref = torch.zeros_like(q), torch.zeros_like(q), torch.zeros(h, tq)
    for i, (n, f) in enumerate(zip(lens_q, fills)):
        q0 = int(cq[i])
        r, p, l = _oracle(q[q0:q0 + n][None], kc[i:i + 1, :f], vc[i:i + 1, :f], causal=True)
        ref[q0:q0 + n], pt[q0:q0 + n], lse_ref[:, q0:q0 + n] = r[0], p[0], l[0]
    _check(out, lse, ref, pt, lse_ref, plan)


# ---- 7. split-KV -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("num_splits,splits", [(4, 4), (0, 2)], ids=["four_parts", "heuristic"])
def test_split_kv(num_splits, splits):
    """seqlen_k 520 = 9 key blocks, causal with seqlen_q 200: the first row blocks end before the last key block, so parts of
    their 4-way split are empty (O = 0, LSE = +inf partials that the merge gives no weight).  num_splits = 0: 7 row blocks x 2
    kv heads = 14 groups, 9 key blocks -> min(ceil(1024 / 14), 9 / 4) = 2 parts."""
    q, k, v = _qkv(1, 200, 520, 8, 2, 128, BF16, seed=18)
    out, lse = _cute().flash_attn_func(q.to(DEV), k.to(DEV), v.to(DEV), causal=True, num_splits=num_splits, pack_gqa=True)
    plan = last_plan()
    torch.cuda.synchronize()
    _packed(plan, 128, splits=splits)
    _check(out, lse, *_oracle(q, k, v, causal=True), plan)


# ---- 8. learnable sink ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("num_splits", [1, 3], ids=["dense", "split"])
def test_learnable_sink_reads_the_lanes_own_head(num_splits):
    q, k, v = _qkv(2, 43, 300, 6, 2, 64, BF16, seed=19)
    sink = torch.linspace(-2, 3, 6).to(BF16)  # distinct per head: a wrong head lookup shows
    out, lse = _cute().flash_attn_func(q.to(DEV), k.to(DEV), v.to(DEV), causal=True, learnable_sink=sink.to(DEV),
                                       num_splits=num_splits, pack_gqa=True)
    plan = last_plan()
    torch.cuda.synchronize()
    _packed(plan, 64, splits=num_splits)
    ref, lse_ref = sink_oracle.attention_sink_ref(q, k, v, sink, causal=True)
    pt, _ = sink_oracle.attention_sink_ref(q, k, v, sink, causal=True, upcast=False, reorder_ops=True)
    _check(out, lse, ref, pt, lse_ref, plan)


# ---- 9. strides ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("view", ["head_dim_slice", "permuted"])
def test_q_strides(view):
    q, k, v = _qkv(2, 43, 107, 6, 2, 64, BF16, seed=20)
    if view == "head_dim_slice":  # the first 64 columns of 160-wide rows: head stride 160, row stride 6 * 160
        wide = torch.cat([q, _rand(2, 43, 6, 96, seed=21)], -1).to(DEV)
        qd = wide[..., :64]
    else:  # a (b, h, s, d) tensor seen as (b, s, h, d): row stride d, head stride s * d
        qd = q.permute(0, 2, 1, 3).contiguous().to(DEV).permute(0, 2, 1, 3)
    assert not qd.is_contiguous() and qd.stride(-1) == 1
    out, lse = _fa3().flash_attn_func(qd, k.to(DEV), v.to(DEV), causal=True, pack_gqa=True, return_attn_probs=True)
    plan = last_plan()
    _packed(plan, 64, splits=1)
    same, lse_same, _ = _fa3_dense(q, k, v, causal=True)
    assert torch.equal(out, same) and torch.equal(lse, lse_same)
    _check(out, lse, *_oracle(q, k, v, causal=True), plan)


# ---- 10. hint semantics -----------------------------------------------------------------------------------------------------------

def test_none_and_false_do_not_pack():
    q, k, v = _qkv(2, 8, 300, 8, 2, 128, BF16, seed=22)
    res = {hint: _fa3_dense(q, k, v, pack_gqa=hint, causal=True) for hint in (None, False, True)}
    assert res[None][2] == res[False][2] == "fwd_kernel D=128 waves=4 block_m=128 splits=1"  # today's route of this shape
    assert torch.equal(res[None][0], res[False][0]) and torch.equal(res[None][1], res[False][1])
    _packed(res[True][2], 128, splits=1)
    _check(res[True][0], res[True][1], *_oracle(q, k, v, causal=True), res[True][2])
    cute = {hint: _cute().flash_attn_func(q.to(DEV), k.to(DEV), v.to(DEV), causal=True, pack_gqa=hint) + (last_plan(),)
            for hint in (None, False)}
    assert cute[None][2] == cute[False][2] == res[None][2]
    assert torch.equal(cute[None][0], cute[False][0]) and torch.equal(cute[None][1], cute[False][1])


# ---- 11. HIP-graph capture, determinism ---------------------------------------------------------------------------------------------

def test_hip_graph_capture_of_a_packed_paged_verify_step():
    b, sq, h, hk, d, cap, page = 4, 4, 8, 2, 128, 256, 64
    q = _rand(b, sq, h, d, seed=23).to(DEV)
    kp, vp, table = (t.to(DEV) for t in _pages(_rand(b, cap, hk, d, seed=24), _rand(b, cap, hk, d, seed=25), page, seed=26))
    lens = torch.tensor([4, 77, 200, 256], dtype=I32, device=DEV)

    def step():
        return _fa3().flash_attn_with_kvcache(q, kp, vp, cache_seqlens=lens, page_table=table, causal=True, num_splits=1,
                                              pack_gqa=True, return_softmax_lse=True)[:2]
    side = torch.cuda.Stream()  # eager results and warm-up on a side stream, as torch's capture rules ask
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        want, want_lse = step()
        _packed(last_plan(), 128, splits=1)
        again, again_lse = step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert torch.equal(want, again) and torch.equal(want_lse, again_lse), "two eager runs differ"
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        got, got_lse = step()
    for _ in range(2):
        got.zero_(); got_lse.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(got, want) and torch.equal(got_lse, want_lse)


# ---- 12. autograd -----------------------------------------------------------------------------------------------------------------

def _grad_bound(ref, pt):
    ref = ref.float()
    atol = 2 * (ref + 0.3 - 0.3 - ref).abs().max().item()
    return 3 * (pt.float() - ref).abs().max().item() + atol + 1e-5


@pytest.mark.parametrize("surface", ["fa3", "cute"])
def test_autograd_through_a_packed_forward(surface):
    """The backward reads the packed forward's out and LSE like any other forward's."""
    q, k, v = _qkv(2, 96, 96, 8, 2, 64, BF16, seed=27)
    dout = _rand(*q.shape, seed=28)
    leaves = [t.to(DEV).requires_grad_(True) for t in (q, k, v)]
    if surface == "fa3":
        out = _fa3().flash_attn_func(*leaves, causal=True, pack_gqa=True)
    else:
        out, _ = _cute().flash_attn_func(*leaves, causal=True, pack_gqa=True)
    _packed(last_plan(), 64, splits=1)
    got = torch.autograd.grad(out, leaves, dout.to(DEV))

    def oracle_grads(**kw):
        ls = [t.clone().requires_grad_(True) for t in (q, k, v)]
        return torch.autograd.grad(oracle.attention_ref(*ls, causal=True, **kw)[0], ls, dout)
    ref, pt = oracle_grads(), oracle_grads(upcast=False, reorder_ops=True)
    for name, g, r, p in zip(("dq", "dk", "dv"), got, ref, pt):
        g = g.float().cpu()
        err, bound = (g - r.float()).abs().max().item(), _grad_bound(r, p)
        print(f"{surface} {name}: err {err:.3e} (bound {bound:.3e})")
        assert torch.isfinite(g).all() and err <= bound, f"{surface} {name}: max err {err:.3e} > bound {bound:.3e}"
