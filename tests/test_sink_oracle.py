"""CPU: the learnable-sink oracle (tests/sink_oracle.py) replays the frozen reference results of
tests/golden/attention_sink_golden.pt (tools/make_sink_golden.py: the reference's flash_attn/cute/testing.py attention_ref,
both operation orders, bit-equal when frozen), and the dsink formula the sink-gradient kernel implements
(include/fa_bwd.h) is checked against autograd through the oracle in float64 and by finite differences -- the yardstick of
the GPU gradient tests is guarded here."""
import os

import pytest
import torch

import sink_oracle

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "attention_sink_golden.pt")
CASES = ["bf16_gqa_causal", "fp16_mqa_decode", "bf16_left_window", "fp16_softcap_causal", "bf16_keyless_rows",
         "bf16_sink_far_above", "bf16_sink_neg_inf", "fp16_d128_right_window"]


@pytest.fixture(scope="module")
def gold():
    return torch.load(GOLDEN)


def test_golden_covers_the_cases(gold):
    assert sorted(gold) == sorted(CASES)
    assert os.path.getsize(GOLDEN) < (1 << 20)
    assert {c["q"].dtype for c in gold.values()} == {torch.bfloat16, torch.float16}


@pytest.mark.parametrize("name", CASES)
def test_oracle_replays_the_reference(gold, name):
    c = gold[name]
    out, lse = sink_oracle.attention_sink_ref(c["q"], c["k"], c["v"], c["sink"], **c["kwargs"])
    out_pt, _ = sink_oracle.attention_sink_ref(c["q"], c["k"], c["v"], c["sink"], upcast=False, reorder_ops=True, **c["kwargs"])
    assert torch.equal(out, c["out_ref"]), (out.float() - c["out_ref"].float()).abs().max()
    assert torch.equal(out_pt, c["out_pt"]), (out_pt.float() - c["out_pt"].float()).abs().max()
    assert torch.equal(lse, c["lse"])


def test_keyless_rows_give_zero_and_the_sink(gold):
    c = gold["bf16_keyless_rows"]  # causal, sq 130 over sk 70: rows 0..59 see no key
    out, lse = sink_oracle.attention_sink_ref(c["q"], c["k"], c["v"], c["sink"], **c["kwargs"])
    assert (out[:, :60] == 0).all()
    assert torch.equal(lse[:, :, :60], c["sink"].float().view(1, -1, 1).expand(1, -1, 60))
    assert torch.isfinite(lse).all()


def test_sink_far_above_the_scores_is_finite(gold):
    c = gold["bf16_sink_far_above"]  # scores -72 (q = 3, k = -3, d = 64), sink +60
    _, lse = sink_oracle.attention_sink_ref(c["q"], c["k"], c["v"], c["sink"], **c["kwargs"])
    assert torch.isfinite(lse).all() and (lse - 60.0).abs().max() < 1e-6


def test_sink_neg_inf_is_the_call_without_a_sink(gold):
    c = gold["bf16_sink_neg_inf"]
    out, lse = sink_oracle.attention_sink_ref(c["q"], c["k"], c["v"], c["sink"], **c["kwargs"])
    out0, lse0 = sink_oracle.attention_sink_ref(c["q"], c["k"], c["v"], None, **c["kwargs"])
    assert torch.equal(out, out0)
    assert torch.allclose(lse, lse0, atol=1e-6, rtol=0)


def _dsink_formula(lse, out, dout, sink):
    """dsink[h] = - sum_{b, i} exp(z_h - LSE[b, h, i]) * D[b, h, i],  D = rowsum(dO * O)  (include/fa_bwd.h)"""
    dsum = (dout * out).sum(-1).transpose(1, 2)  # (b, h, sq)
    return -(torch.exp(sink.view(1, -1, 1) - lse) * dsum).sum((0, 2))


@pytest.mark.parametrize("kw", [dict(causal=True), dict(window_size=(7, 3)), dict(causal=True, softcap=5.0)], ids=str)
@pytest.mark.parametrize("sq,sk", [(9, 21), (21, 9)])  # (21, 9) causal: rows without keys, LSE = z there
def test_dsink_formula_float64(sq, sk, kw):
    torch.manual_seed(5)
    b, h, hk, d = 2, 4, 2, 16
    q, k, v, dout = (torch.randn(b, s, n, d, dtype=torch.float64) for s, n in ((sq, h), (sk, hk), (sk, hk), (sq, h)))
    sink = torch.linspace(-2, 3, h, dtype=torch.float64).requires_grad_(True)
    out, lse = sink_oracle.attention_sink_ref(q, k, v, sink, upcast=False, **kw)
    assert out.dtype == torch.float64
    (auto,) = torch.autograd.grad(out, sink, dout)
    formula = _dsink_formula(lse.double(), out.detach(), dout, sink.detach())
    # lse is returned in fp32 (~1e-7 relative): the formula sees it through exp()
    assert torch.allclose(formula, auto, rtol=1e-5, atol=1e-6), (formula, auto)
    # central differences on the scalar loss sum(out * dout)
    eps = 1e-5
    for i in range(h):
        e = torch.zeros(h, dtype=torch.float64)
        e[i] = eps
        lp = (sink_oracle.attention_sink_ref(q, k, v, sink.detach() + e, upcast=False, **kw)[0] * dout).sum()
        lm = (sink_oracle.attention_sink_ref(q, k, v, sink.detach() - e, upcast=False, **kw)[0] * dout).sum()
        assert abs(((lp - lm) / (2 * eps)).item() - auto[i].item()) < 1e-6 * max(1.0, abs(auto[i].item()))
