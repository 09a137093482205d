"""Plan-keyed gradient parity: every case of tests/bwd_plan_universe.py, in bf16 and fp16, through the public entry point its row
names.  A hook on the backward node reads fa_bwd_last_plan_name() right behind the node's fa_bwd (on the autograd thread that
ran it: parity_helpers.record_bwd_plan) and the case asserts that exactly the plan of its row ran -- a routing change that
moves the case to other kernels fails here and asks for a case for the ones it left -- then
compares dq / dk / dv with the oracle's autograd: `ref` differentiates the oracle in fp32, `pt` the same math in the inputs'
precision (reorder_ops), as tests/test_flash_attn_bwd_gpu.py::_oracle_grads; dropout cases hand the oracle the kernel's
keep-mask (the sign of S_dmask).

Bounds, for dX in dq, dk, dv:
    global    |dX - dX_ref|max <= 3 |dX_pt - dX_ref|max + atol + 1e-5,  atol = 2 |(dX_ref + 0.3 - 0.3) - dX_ref|max
    per tile  the same inequality with every maximum taken over one tile: dq per (batch, head, 64-row block), dk / dv per
              (batch, kv head, 128-key block).  A wrong tile where gradients are small -- the last key block of a causal
              problem, a ragged tail -- passes the global bound and fails this one.
Factor 3 is the reference's own; the per-tile form keeps it.  Every case prints its worst per-tile ratio
err / (3 pt_err + atol + 1e-5); with FA_BWD_PARITY_JSONL=<path> the ratios are appended to that file as JSON lines.
Exact: non-finite values fail; query rows without a visible key have dq == 0, keys no query sees have dk == dv == 0 (the
sequences without keys / without queries of the varlen cases).  Varlen cases are compared sequence by sequence, so rows outside
every sequence are not compared.  The sink case also compares dsink (global bound, as tests/test_sink_gpu.py).
The last test asserts that the kernels seen in the session are the whole universe."""
import itertools
import json
import math
import os

import pytest
import torch

import sink_oracle
from bwd_plan_universe import CASES, DTYPES, SINK_KEY, UNIVERSE, case_id, segments
from oracle import attention_ref as oracle
from parity_helpers import record_bwd_plan

pytestmark = pytest.mark.gpu
DEV = "cuda"
TORCH_DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
FACTOR = 3
SEEN = set()  # kernel keys launched by the cases of this session

PARAMS = [(name, dt) for name in CASES for dt in DTYPES]


def _cu(lens):
    return torch.tensor([0] + list(itertools.accumulate(lens)), dtype=torch.int32)


def _inputs(case, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    h, hk, d = case["h"], case["hk"], case["d"]
    dv = case.get("dv", d)
    lead_q, lead_k = ((sum(case["lens_q"]),), (sum(case["lens_k"]),)) if "lens_q" in case else \
        ((case["b"], case["sq"]), (case["b"], case["sk"]))
    t = {"q": torch.randn(*lead_q, h, d, generator=g).to(dtype), "k": torch.randn(*lead_k, hk, d, generator=g).to(dtype),
         "v": torch.randn(*lead_k, hk, dv, generator=g).to(dtype), "g": torch.randn(*lead_q, h, dv, generator=g).to(dtype)}
    if case.get("alibi"):
        t["slopes"] = torch.rand(case["b"], h, generator=g) * 0.3
    if case.get("sink"):
        t["sink"] = torch.linspace(-4, 4, h).to(torch.bfloat16)  # distinct per head: a wrong head index shows
    return t


def _run(case, t):
    """-> (gradients on the CPU, plan text, oracle keyword arguments the run adds: the dropout keep-mask)."""
    import flash_attention_annotated_amd as fa
    from flash_attention_annotated_amd import cute_interface as cute
    from flash_attention_annotated_amd import hopper_interface as fa3
    leaves = [t[n].to(DEV).requires_grad_(True) for n in ("q", "k", "v")]
    mask = dict(causal=case.get("causal", False), window_size=case.get("window", (-1, -1)))
    okw = {}
    if case["api"] == "fa3":
        out = fa3.flash_attn_func(*leaves, **mask)
    elif case["api"] == "cute":
        leaves.append(t["sink"].to(DEV).requires_grad_(True))
        out, _ = cute.flash_attn_func(*leaves[:3], causal=mask["causal"], learnable_sink=leaves[3])
    elif case["api"] == "fa2_varlen":
        cq, ck = _cu(case["lens_q"]), _cu(case["lens_k"])
        out = fa.flash_attn_varlen_func(*leaves, cq.to(DEV), ck.to(DEV), max(case["lens_q"]), max(case["lens_k"]), **mask)
    else:
        p_drop = case.get("dropout", 0.0)
        slopes = t["slopes"].to(DEV) if "slopes" in t else None
        out, _, S = fa.flash_attn_func(*leaves, p_drop, softcap=case.get("softcap", 0.0), alibi_slopes=slopes,
                                       return_attn_probs=True, **mask)
        if p_drop:
            keep = ~torch.signbit(S[:, :, :case["sq"], :case["sk"]].float().cpu())
            okw = dict(dropout_p=p_drop, dropout_mask=keep)
    plans = record_bwd_plan(out)
    got = torch.autograd.grad(out, leaves, t["g"].to(DEV))
    assert len(plans) == 1, f"one backward node, one fa_bwd: {plans}"
    return [x.detach().cpu() for x in got], plans[0], okw


def _autograd(fn, leaves, g):
    """fn(*leaves, **order) -> out; -> (ref gradients, pt gradients)."""
    def run(cast, **order):
        ls = [cast(x).clone().requires_grad_(True) for x in leaves]
        return torch.autograd.grad(fn(*ls, **order), ls, g)
    sink_fp32 = lambda x: x.float() if x.dim() == 1 else x  # noqa: E731  (the sink as an fp32 leaf: its bf16 values are exact)
    return run(sink_fp32), run(lambda x: x, upcast=False, reorder_ops=True)


def _problems(case, t, got, okw):
    """[(label, got (dq, dk, dv[, dsink]), ref, pt, sq, sk)] with tensors (b, s, heads, d): the dense batch, or one sequence each."""
    kw = dict(causal=case.get("causal", False), window_size=case.get("window", (-1, -1)), softcap=case.get("softcap", 0.0), **okw)
    if "lens_q" in case:
        cq, ck = _cu(case["lens_q"]).tolist(), _cu(case["lens_k"]).tolist()
        out = []
        for i in range(len(cq) - 1):
            (q0, q1), (k0, k1) = cq[i:i + 2], ck[i:i + 2]
            sl = [got[0][q0:q1][None], got[1][k0:k1][None], got[2][k0:k1][None]]
            if q1 == q0 or k1 == k0:  # no attention at all: every gradient of the sequence is exactly zero
                out.append((f"sequence {i}", sl, None, None, q1 - q0, k1 - k0))
                continue
            leaves = [t["q"][q0:q1][None], t["k"][k0:k1][None], t["v"][k0:k1][None]]
            ref, pt = _autograd(lambda a, b, c, **o: oracle.attention_ref(a, b, c, **kw, **o)[0], leaves, t["g"][q0:q1][None])
            out.append((f"sequence {i}", sl, ref, pt, q1 - q0, k1 - k0))
        return out
    if case.get("sink"):
        fn = lambda a, b, c, s, **o: sink_oracle.attention_sink_ref(a, b, c, s, causal=kw["causal"], **o)[0]  # noqa: E731
        ref, pt = _autograd(fn, [t["q"], t["k"], t["v"], t["sink"]], t["g"])
    else:
        if "slopes" in t:
            kw["attn_bias"] = oracle.attn_bias_from_alibi_slopes(t["slopes"], case["sq"], case["sk"], causal=kw["causal"])
        ref, pt = _autograd(lambda a, b, c, **o: oracle.attention_ref(a, b, c, **kw, **o)[0], [t["q"], t["k"], t["v"]], t["g"])
    return [("batch", got, ref, pt, case["sq"], case["sk"])]


def _tile_max(x, rows):
    """(b, s, heads, d) -> (b, ceil(s / rows), heads): the maximum of every (batch, head, `rows`-row block)."""
    b, s, h, d = x.shape
    pad = -s % rows
    x = torch.nn.functional.pad(x, (0, 0, 0, 0, 0, pad))
    return x.view(b, (s + pad) // rows, rows, h, d).amax(dim=(2, 4))


def _atol_term(ref):
    return 2 * (ref + 0.3 - 0.3 - ref).abs()


def _check_problem(what, got, ref, pt, sq, sk, case):
    """-> {name: (global err, global pt err, global atol, worst per-tile ratio)}; asserts the exact checks and the per-tile bound."""
    stats = {}
    for name, g in zip(("dq", "dk", "dv"), got):
        assert torch.isfinite(g.float()).all(), f"{what} {name}: non-finite"
    if ref is None:
        for name, g in zip(("dq", "dk", "dv"), got):
            assert not g.float().abs().sum().item(), f"{what} {name}: not exactly zero in a sequence without queries / keys"
        return stats
    wl, wr = case.get("window", (-1, -1))
    hidden = oracle.local_mask(sq, sk, (wl, 0 if case.get("causal") else wr)).view(sq, sk) if (case.get("causal") or wl >= 0 or wr >= 0) \
        else torch.zeros(sq, sk, dtype=torch.bool)
    rows_blind, keys_unseen = hidden.all(dim=1), hidden.all(dim=0)
    assert not got[0][:, rows_blind].float().abs().sum().item(), f"{what} dq: rows without a visible key are not exactly zero"
    assert not got[1][:, keys_unseen].float().abs().sum().item(), f"{what} dk: keys no query sees are not exactly zero"
    assert not got[2][:, keys_unseen].float().abs().sum().item(), f"{what} dv: keys no query sees are not exactly zero"
    for name, g, r, p, rows in zip(("dq", "dk", "dv"), got, ref, pt, (64, 128, 128)):
        g, r, p = g.float(), r.float(), p.float()
        err, pt_err, atol = _tile_max((g - r).abs(), rows), _tile_max((p - r).abs(), rows), _tile_max(_atol_term(r), rows)
        ratio = err / (FACTOR * pt_err + atol + 1e-5)
        worst = ratio.max().item()
        stats[name] = (err.max().item(), pt_err.max().item(), atol.max().item(), worst)
        if worst > 1:
            bi, ti, hi = (int(x) for x in (ratio == ratio.max()).nonzero()[0])
            raise AssertionError(f"{what} {name}: tile (batch {bi}, block {ti}, head {hi}) err {err[bi, ti, hi]:.3e} > "
                                 f"{FACTOR} x {pt_err[bi, ti, hi]:.3e} + {atol[bi, ti, hi]:.3e} + 1e-5 (ratio {worst:.2f})")
    return stats


@pytest.mark.parametrize("name,dt", PARAMS, ids=[case_id(n, dt) for n, dt in PARAMS])
def test_bwd_plan_parity(name, dt):
    want_plan, case = CASES[name]
    seed = sum(ord(c) for c in name + dt)
    t = _inputs(case, TORCH_DTYPES[dt], seed)
    got, plan, okw = _run(case, t)
    keys = {(dt, seg) for seg in segments(plan)}
    if case.get("sink"):
        assert got[3] is not None and got[3].shape == t["sink"].shape
        keys.add(SINK_KEY)  # inferred, not read from a plan: the binding launches it behind fa_bwd whenever a sink is given, and the
        #                    plan text has no segment for it; the dsink comparison below is what observes its result
    SEEN.update(keys)
    assert plan == want_plan, f"planned {plan!r}: the case no longer reaches {want_plan!r} -- add a case for the kernels it left"

    glob = {}
    worst = {"dq": 0.0, "dk": 0.0, "dv": 0.0}
    for label, gp, ref, pt, sq, sk in _problems(case, t, got, okw):
        for n, (err, pt_err, atol, ratio) in _check_problem(f"{name} {dt} {label}", gp, ref, pt, sq, sk, case).items():
            e0, p0, a0 = glob.get(n, (0.0, 0.0, 0.0))
            glob[n] = (max(e0, err), max(p0, pt_err), max(a0, atol))
            worst[n] = max(worst[n], ratio)
        if case.get("sink"):
            r, p = ref[3].float(), pt[3].float()
            err, bound = (gp[3].float() - r).abs().max().item(), FACTOR * (p - r).abs().max().item() + _atol_term(r).max().item() + 1e-5
            print(f"{name} {dt} dsink: err {err:.3e} bound {bound:.3e}")
            assert math.isfinite(err) and err <= bound, f"{name} {dt} dsink: err {err:.3e} > bound {bound:.3e}"
    record = dict(case=case_id(name, dt), plan=plan, worst_tile_ratio={n: round(v, 4) for n, v in worst.items()})
    print(json.dumps(record))
    if os.environ.get("FA_BWD_PARITY_JSONL"):
        with open(os.environ["FA_BWD_PARITY_JSONL"], "a") as f:
            f.write(json.dumps(record) + "\n")
    for n, (err, pt_err, atol) in glob.items():  # the global inequality (implied by the per-tile one; stated for the record)
        bound = FACTOR * pt_err + atol + 1e-5
        assert err <= bound, f"{name} {dt} {n}: max err {err:.3e} > bound {bound:.3e}"


def test_every_backward_kernel_ran(request):
    """The kernel keys the cases above launched are the universe (tests/test_bwd_plan.py ties it to the compiled symbols)."""
    if request.config.option.keyword or any("::" in a for a in request.config.args):
        pytest.skip("a subset of the cases was selected: the coverage assertion needs the whole file")
    want = set(UNIVERSE)
    assert SEEN == want, f"never launched: {sorted(want - SEEN)}; outside the universe: {sorted(SEEN - want)}"
