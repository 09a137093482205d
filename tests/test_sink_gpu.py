"""GPU parity of the learnable attention sink on the cute surface (flash_attention_annotated_amd/cute_interface.py ->
fa_fwd_sink / fa_sink_grad, include/fa_fwd.h, include/fa_bwd.h) against tests/sink_oracle.py.

Forward, the rule of parity_helpers._check_rows:  |O - O_ref|max <= 2 |O_pt - O_ref|max + 1e-5  (O_ref: the oracle in fp32,
O_pt: the same math in the inputs' precision), LSE within 2e-3 with the same inf pattern.  Every case also asserts that the
call with a sink launched the plan of the same call without one, and that the plan names the family the case is for.
Backward, the rule of tests/test_flash_attn_bwd_gpu.py:  |dX - dX_ref|max <= 3 |dX_pt - dX_ref|max + atol + 1e-5  for dq, dk,
dv and dsink (autograd through the oracle), and bit-equal repeats.
Shapes are those of tests/plan_universe.py: >= 3 full key tiles, a masked tile, a ragged last tile, seqlen_q no multiple of
block_m; sinks are distinct per head (linspace(-4, 4, h) in bf16) so that a wrong head index shows."""
import math

import pytest
import torch

import sink_oracle
from parity_helpers import last_plan

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}


def _cute():
    from flash_attention_annotated_amd import cute_interface
    return cute_interface


def _sinks(h, dtype=torch.bfloat16):
    return torch.linspace(-4, 4, h).to(torch.bfloat16).to(dtype)


def _qkv(b, sq, sk, h, hk, d, dtype, seed=0, dv=None):
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


def _oracle(q, k, v, sink, **kw):
    ref, lse_ref = sink_oracle.attention_sink_ref(q, k, v, sink, **kw)
    pt, _ = sink_oracle.attention_sink_ref(q, k, v, sink, upcast=False, reorder_ops=True, **kw)
    return ref, pt, lse_ref


def _both(fn, sink, family):
    """fn(sink) -> (out, lse): run without and with the sink, the plans must be the same text and name `family`."""
    fn(None)
    plan0 = last_plan()
    out, lse = fn(sink)
    plan = last_plan()
    torch.cuda.synchronize()
    assert plan == plan0, f"the sink changed the plan: {plan0!r} -> {plan!r}"
    assert plan.startswith(family + " "), f"{plan!r} is not {family!r}"
    return out, lse, plan


def _dense_case(family, b, h, hk, sq, sk, d, dtype, batches=None, sink_dtype=torch.bfloat16, **kw):
    q, k, v = _qkv(b, sq, sk, h, hk, d, dtype)
    sink = _sinks(h, sink_dtype)
    qd, kd, vd = q.to(DEV), k.to(DEV), v.to(DEV)
    out, lse, plan = _both(lambda s: _cute().flash_attn_func(qd, kd, vd, learnable_sink=None if s is None else s.to(DEV), **kw),
                           sink, family)
    assert out.shape == q.shape and lse.shape == (b, h, sq) and lse.dtype == torch.float32
    kw.pop("num_splits", None)
    bs = list(range(b)) if batches is None else batches  # (large batches: the oracle on some entries, all their rows)
    ref, pt, lse_ref = _oracle(q[bs], k[bs], v[bs], sink, **kw)
    _check(out[bs], lse[bs], ref, pt, lse_ref, plan)
    return out, lse


SMALL = dict(b=2, h=4, hk=2, sq=300, sk=715)


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("d,family,kw", [
    (128, "fwd_kernel_w64 D=128 DEFF=128 waves=4", dict(causal=True)),
    (96, "fwd_kernel_w64 D=128 DEFF=96 waves=4", dict(causal=True)),
    (64, "fwd_kernel_w64 D=64 DEFF=64 waves=4", dict(window_size=(400, 100))),
    (192, "fwd_kernel_d256 W=192 waves=4", dict(causal=True)),
    (256, "fwd_kernel_d256 W=256 waves=4", dict(causal=True)),
    (128, "fwd_kernel_d256 W=128 waves=4 SOFTCAP", dict(causal=True, softcap=5.0)),
], ids=lambda x: x if isinstance(x, int) else None)
def test_fwd_families(d, family, kw, dt):
    _dense_case(family, d=d, dtype=DTYPES[dt], **SMALL, **kw)


def test_fwd_fp32_sink():
    _dense_case("fwd_kernel_w64 D=128 DEFF=128 waves=4", d=128, dtype=torch.bfloat16, sink_dtype=torch.float32, causal=True, **SMALL)


def test_fwd_persistent():
    out, _ = _dense_case("fwd_kernel_w64 D=128 DEFF=128 waves=4 PERSIST", b=16, h=16, hk=4, sq=300, sk=1024, d=128,
                         dtype=torch.bfloat16, batches=[0, 7, 15], causal=True)


def test_fwd_kernel_short_q():
    _dense_case("fwd_kernel D=128 waves=4", b=2, h=4, hk=2, sq=100, sk=715, d=128, dtype=torch.bfloat16, causal=True)


def _paged(k, v, page, seed=1):
    """(b, sk, hk, d) caches -> pages in a shuffled pool + page table; sk is padded to whole pages with noise."""
    b, sk, hk, d = k.shape
    per = (sk + page - 1) // page
    g = torch.Generator().manual_seed(seed)
    pad = per * page - sk
    kp = torch.cat([k, torch.randn(b, pad, hk, d, generator=g).to(k.dtype)], 1).view(b * per, page, hk, d)
    vp = torch.cat([v, torch.randn(b, pad, hk, v.shape[-1], generator=g).to(v.dtype)], 1).view(b * per, page, hk, v.shape[-1])
    perm = torch.randperm(b * per, generator=g)
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(b * per)
    return kp[perm].contiguous(), vp[perm].contiguous(), inv.view(b, per).to(torch.int32)


def _paged_case(family, b, h, hk, sq, sk, d, dtype, lens=None, num_splits=1, causal=True):
    q, k, v = _qkv(b, sq, sk, h, hk, d, dtype, seed=2)
    sink = _sinks(h)
    kp, vp, table = _paged(k, v, 256)
    lens = [sk] * b if lens is None else lens
    used = torch.tensor(lens, dtype=torch.int32)
    qd, kpd, vpd, td, ud = q.to(DEV), kp.to(DEV), vp.to(DEV), table.to(DEV), used.to(DEV)
    fn = lambda s: _cute().flash_attn_varlen_func(qd, kpd, vpd, seqused_k=ud, page_table=td, causal=causal, num_splits=num_splits,  # noqa: E731
                                                   learnable_sink=None if s is None else s.to(DEV))
    out, lse, plan = _both(fn, sink, family)
    assert f"splits={num_splits}" in plan
    for i in range(b):
        ref, pt, lse_ref = _oracle(q[i:i + 1], k[i:i + 1, :lens[i]], v[i:i + 1, :lens[i]], sink, causal=causal)
        _check(out[i:i + 1], lse[i:i + 1], ref, pt, lse_ref, f"{plan} batch {i}")
    return (qd, kpd, vpd, td, ud), out, lse, plan


def test_fwd_kernel_paged():
    _paged_case("fwd_kernel D=128 waves=8", d=128, dtype=torch.bfloat16, **SMALL)


# ---- split-KV: the parts write sink-free partials, the merge adds the sink once ------------------------------------------------

def _close_to_unsplit(out, lse, out1, lse1):
    """the merge's tolerance (tests/test_combine_gpu.py): lse allclose(1e-5, 1e-5) -- here through two __logf, 1e-4 as its
    kernel-against-kernel test -- and O within the 16-bit rounding of the two results"""
    assert torch.allclose(lse, lse1, atol=1e-4, rtol=1e-5), (lse - lse1).abs().max()
    assert (out.float() - out1.float()).abs().max().item() <= 2e-2


def test_split_w64():
    out1, lse1 = _dense_case("fwd_kernel_w64 D=128 DEFF=128 waves=4", d=128, dtype=torch.bfloat16, causal=True, **SMALL)
    out3, lse3 = _dense_case("fwd_kernel_w64 D=128 DEFF=128 waves=4", d=128, dtype=torch.bfloat16, causal=True, num_splits=3, **SMALL)
    assert "splits=3" in last_plan()
    _close_to_unsplit(out3, lse3, out1, lse1)


def test_split_paged():
    _, out1, lse1, _ = _paged_case("fwd_kernel D=128 waves=8", d=128, dtype=torch.bfloat16, **SMALL)
    _, out3, lse3, _ = _paged_case("fwd_kernel D=128 waves=8", d=128, dtype=torch.bfloat16, num_splits=3, **SMALL)
    _close_to_unsplit(out3, lse3, out1, lse1)


# ---- decode: one row per sequence, the GQA group folded into the rows ----------------------------------------------------------

DECODE_LENS = [1000, 1, 257, 715]


@pytest.mark.parametrize("num_splits", [1, 3])
@pytest.mark.parametrize("d", [64, 128])
def test_decode(d, num_splits):
    from flash_attention_annotated_amd import hopper_interface
    family = f"fwd_kernel D={d} waves=8"
    args, out, lse, plan = _paged_case(family, b=4, h=16, hk=2, sq=1, sk=1000, d=d, dtype=torch.bfloat16, lens=DECODE_LENS,
                                       num_splits=num_splits, causal=False)
    qd, kpd, vpd, td, ud = args
    hopper_interface.flash_attn_with_kvcache(qd, kpd, vpd, cache_seqlens=ud, page_table=td, num_splits=num_splits)
    assert last_plan() == plan, "the decode step with a sink left the route of flash_attn_with_kvcache (the GQA swap)"
    assert "block_m=256" in plan or "block_m=" in plan
    # -inf: the call without a sink, bit for bit
    neg = torch.full((16,), float("-inf"), dtype=torch.bfloat16, device=DEV)
    out_n, lse_n = _cute().flash_attn_varlen_func(qd, kpd, vpd, seqused_k=ud, page_table=td, num_splits=num_splits, learnable_sink=neg)
    out_0, lse_0 = _cute().flash_attn_varlen_func(qd, kpd, vpd, seqused_k=ud, page_table=td, num_splits=num_splits)
    assert torch.equal(out_n, out_0) and torch.equal(lse_n, lse_0)


def test_decode_graph_capture():
    """One decode step with a sink (paged, split) is captured and replays to the same bits."""
    q, k, v = _qkv(4, 1, 1000, 16, 2, 64, torch.bfloat16, seed=3)
    kp, vp, table = _paged(k, v, 256)
    qd, kpd, vpd, td = q.to(DEV), kp.to(DEV), vp.to(DEV), table.to(DEV)
    ud = torch.tensor(DECODE_LENS, dtype=torch.int32, device=DEV)
    sink = _sinks(16).to(DEV)
    run = lambda: _cute().flash_attn_varlen_func(qd, kpd, vpd, seqused_k=ud, page_table=td, num_splits=3, learnable_sink=sink)  # noqa: E731
    want_out, want_lse = run()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got_out, got_lse = run()
    got_out.zero_(); got_lse.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(got_out, want_out) and torch.equal(got_lse, want_lse)


# ---- varlen ----------------------------------------------------------------------------------------------------------------------

def _cu(lens):
    return torch.tensor([0] + list(torch.tensor(lens).cumsum(0)), dtype=torch.int32)


def test_varlen_with_an_empty_sequence():
    lens_q, lens_k = [300, 0, 77, 130], [715, 0, 200, 70]  # (the last one: causal rows without keys)
    h, hk, d = 4, 2, 128
    g = torch.Generator().manual_seed(4)
    q = torch.randn(sum(lens_q), h, d, generator=g).to(torch.bfloat16)
    k = torch.randn(sum(lens_k), hk, d, generator=g).to(torch.bfloat16)
    v = torch.randn(sum(lens_k), hk, d, generator=g).to(torch.bfloat16)
    cq, ck, sink = _cu(lens_q), _cu(lens_k), _sinks(h)
    qd, kd, vd, cqd, ckd = (t.to(DEV) for t in (q, k, v, cq, ck))
    out, lse, plan = _both(lambda s: _cute().flash_attn_varlen_func(qd, kd, vd, cqd, ckd, causal=True,
                                                                    learnable_sink=None if s is None else s.to(DEV)),
                           sink, "fwd_kernel_w64 D=128 DEFF=128 waves=4")
    assert lse.shape == (h, sum(lens_q))
    ref, lse_ref = sink_oracle.attention_sink_varlen_ref(q, k, v, cq, ck, sink, causal=True)
    pt, _ = sink_oracle.attention_sink_varlen_ref(q, k, v, cq, ck, sink, causal=True, upcast=False, reorder_ops=True)
    _check(out, lse, ref, pt, lse_ref, plan)


def test_ragged_queries_over_a_cache():
    lens_q, fills, cap = [300, 1, 77], [715, 400, 77], 768
    b, h, hk, d = 3, 4, 2, 128
    g = torch.Generator().manual_seed(5)
    q = torch.randn(sum(lens_q), h, d, generator=g).to(torch.bfloat16)
    k = torch.randn(b, cap, hk, d, generator=g).to(torch.bfloat16)
    v = torch.randn(b, cap, hk, d, generator=g).to(torch.bfloat16)
    cq, sink = _cu(lens_q), _sinks(h)
    used = torch.tensor(fills, dtype=torch.int32)
    qd, kd, vd, cqd, ud = (t.to(DEV) for t in (q, k, v, cq, used))
    out, lse, plan = _both(lambda s: _cute().flash_attn_varlen_func(qd, kd, vd, cqd, seqused_k=ud, causal=True,
                                                                    learnable_sink=None if s is None else s.to(DEV)),
                           sink, "fwd_kernel_w64 D=128 DEFF=128 waves=4")
    for i in range(b):
        r0, r1 = int(cq[i]), int(cq[i + 1])
        ref, pt, lse_ref = _oracle(q[r0:r1][None], k[i:i + 1, :fills[i]], v[i:i + 1, :fills[i]], sink, causal=True)
        _check(out[r0:r1][None], lse[:, r0:r1][None], ref, pt, lse_ref, f"{plan} sequence {i}")


# ---- edge rows -------------------------------------------------------------------------------------------------------------------

def test_keyless_rows_are_zero_with_the_sink_as_lse():
    b, h, hk, sq, sk, d = 2, 4, 2, 130, 70, 128
    q, k, v = _qkv(b, sq, sk, h, hk, d, torch.bfloat16, seed=6)
    sink = _sinks(h)
    out, lse = _cute().flash_attn_func(q.to(DEV), k.to(DEV), v.to(DEV), causal=True, learnable_sink=sink.to(DEV))
    ref, pt, lse_ref = _oracle(q, k, v, sink, causal=True)
    _check(out, lse, ref, pt, lse_ref, last_plan())
    assert (out[:, :sq - sk] == 0).all()
    assert torch.equal(lse[:, :, :sq - sk].cpu(), sink.float().view(1, h, 1).expand(b, h, sq - sk))


def test_sink_neg_inf_is_bit_identical_w64():
    q, k, v = (t.to(DEV) for t in _qkv(d=128, dtype=torch.bfloat16, seed=7, **SMALL))
    neg = torch.full((4,), float("-inf"), dtype=torch.bfloat16, device=DEV)
    out_n, lse_n = _cute().flash_attn_func(q, k, v, causal=True, learnable_sink=neg)
    assert last_plan().startswith("fwd_kernel_w64 ")
    out_0, lse_0 = _cute().flash_attn_func(q, k, v, causal=True)
    assert torch.equal(out_n, out_0) and torch.equal(lse_n, lse_0)


def test_sink_far_above_the_scores():
    """q = 3, k = -3, d = 64 with scale 1/8: every score is -72; the sink is +60.  exp(60 + 72) overflows fp32: the sink has to
    be the offset.  LSE = 60 + log1p(sk e^-132) = 60."""
    b, h, hk, sq, sk, d = 1, 4, 2, 300, 715, 64
    q, k = torch.full((b, sq, h, d), 3.0).to(torch.bfloat16), torch.full((b, sk, hk, d), -3.0).to(torch.bfloat16)
    v = _qkv(b, sq, sk, h, hk, d, torch.bfloat16)[2]
    sink = torch.full((h,), 60.0).to(torch.bfloat16)
    out, lse = _cute().flash_attn_func(q.to(DEV), k.to(DEV), v.to(DEV), learnable_sink=sink.to(DEV))
    ref, pt, lse_ref = _oracle(q, k, v, sink)
    assert torch.isfinite(lse).all()
    _check(out, lse, ref, pt, lse_ref, last_plan())


# ---- the surface -----------------------------------------------------------------------------------------------------------------

def test_surface_checks():
    q, k, v = (t.to(DEV) for t in _qkv(1, 64, 64, 4, 2, 64, torch.bfloat16))
    f = _cute().flash_attn_func
    with pytest.raises(NotImplementedError, match="mask_mod"):
        f(q, k, v, mask_mod=lambda *a: True)
    with pytest.raises(NotImplementedError, match="full_block_cnt"):
        f(q, k, v, full_block_cnt=torch.zeros(1, device=DEV))
    with pytest.raises(AssertionError, match="num_head"):
        f(q, k, v, learnable_sink=torch.zeros(3, dtype=torch.bfloat16, device=DEV))
    with pytest.raises(AssertionError, match="bfloat16"):
        f(q, k, v, learnable_sink=torch.zeros(4, dtype=torch.float16, device=DEV))
    with pytest.raises(AssertionError, match="CUDA"):
        f(q, k, v, learnable_sink=torch.zeros(4, dtype=torch.bfloat16))
    out, lse = f(q, k, v, pack_gqa=True)  # accepted and ignored
    assert out.shape == q.shape and lse.shape == (1, 4, 64)


# ---- backward --------------------------------------------------------------------------------------------------------------------

def _bound(ref, pt):
    ref = ref.float()
    atol = 2 * (ref + 0.3 - 0.3 - ref).abs().max().item()
    return 3 * (pt.float() - ref).abs().max().item() + atol + 1e-5


def _check_grads(got, ref, pt, what):
    for name, g, r, p in zip(("dq", "dk", "dv", "dsink"), got, ref, pt):
        g = g.float().cpu()
        assert torch.isfinite(g).all(), f"{what} {name}: non-finite"
        err, bound = (g - r.float()).abs().max().item(), _bound(r, p)
        print(f"{what} {name}: err {err:.3e} (bound {bound:.3e})")
        assert err <= bound, f"{what} {name}: max err {err:.3e} > bound {bound:.3e}"


def _oracle_grads(fn, q, k, v, sink, g):
    """fn(q, k, v, sink, **order) -> out.  fp32 path: the sink as an fp32 leaf (its bf16 values are exact there); the
    low-precision path: the sink as it is."""
    def run(s, **order):
        leaves = [t.clone().requires_grad_(True) for t in (q, k, v, s)]
        return torch.autograd.grad(fn(*leaves, **order), leaves, g)
    return run(sink.float()), run(sink, upcast=False, reorder_ops=True)


@pytest.mark.parametrize("d", [64, 128])
def test_bwd_dense(d):
    q, k, v = _qkv(d=d, dtype=torch.bfloat16, seed=8, **SMALL)
    sink = _sinks(4)
    g = torch.randn(q.shape, generator=torch.Generator().manual_seed(9)).to(torch.bfloat16)

    def run():
        leaves = [t.to(DEV).requires_grad_(True) for t in (q, k, v, sink)]
        out, _ = _cute().flash_attn_func(*leaves[:3], causal=True, learnable_sink=leaves[3])
        return torch.autograd.grad(out, leaves, g.to(DEV))
    got, again = run(), run()
    assert got[3].dtype == torch.bfloat16 and got[3].shape == (4,)
    ref, pt = _oracle_grads(lambda a, b_, c, s, **o: sink_oracle.attention_sink_ref(a, b_, c, s, causal=True, **o)[0], q, k, v, sink, g)
    _check_grads(got, ref, pt, f"dense d{d}")
    for a, b_ in zip(got, again):
        assert torch.equal(a, b_), "the backward with a sink is not bit-reproducible"


def test_bwd_varlen_fp32_sink():
    lens_q, lens_k = [300, 77, 128], [715, 200, 128]
    h, hk, d = 4, 2, 64
    gen = torch.Generator().manual_seed(10)
    q = torch.randn(sum(lens_q), h, d, generator=gen).to(torch.bfloat16)
    k = torch.randn(sum(lens_k), hk, d, generator=gen).to(torch.bfloat16)
    v = torch.randn(sum(lens_k), hk, d, generator=gen).to(torch.bfloat16)
    g = torch.randn(q.shape, generator=gen).to(torch.bfloat16)
    cq, ck = _cu(lens_q), _cu(lens_k)
    sink = _sinks(h, torch.float32)

    def run():
        leaves = [t.to(DEV).requires_grad_(True) for t in (q, k, v, sink)]
        out, _ = _cute().flash_attn_varlen_func(*leaves[:3], cq.to(DEV), ck.to(DEV), causal=True, learnable_sink=leaves[3])
        return torch.autograd.grad(out, leaves, g.to(DEV))
    got, again = run(), run()
    assert got[3].dtype == torch.float32
    ref, pt = _oracle_grads(lambda a, b_, c, s, **o: sink_oracle.attention_sink_varlen_ref(a, b_, c, cq, ck, s, causal=True, **o)[0],
                            q, k, v, sink.to(torch.bfloat16), g)
    _check_grads(got, ref, pt, "varlen")
    for a, b_ in zip(got, again):
        assert torch.equal(a, b_)
