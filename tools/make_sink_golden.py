"""Freeze the learnable-sink oracle against the reference (build container only: needs the reference checkout).

Loads the reference's flash_attn/cute/testing.py BY FILE PATH (the file imports torch and einops only; the package __init__
needs cutlass), asserts tests/sink_oracle.py equals its `attention_ref(..., learnable_sink=)` bit for bit on the cases below --
on the fp32 path and on the `upcast=False, reorder_ops=True` path -- and writes inputs and reference outputs, data only, to
tests/golden/attention_sink_golden.pt.  The LSE (which the reference's oracle does not return) is frozen from the
restatement after a float64 evaluation of its definition has confirmed it.

    python tools/make_sink_golden.py [--reference /path/to/reference]
"""
import argparse
import importlib.util
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sink_oracle  # noqa: E402

INF = float("inf")
# name, dtype, (b, h, hk, sq, sk, d), kwargs, sink ("lin" = distinct per head, or one value for every head), constant q/k
CASES = [
    ("bf16_gqa_causal", torch.bfloat16, (1, 4, 2, 33, 70, 64), dict(causal=True), "lin", None),
    ("fp16_mqa_decode", torch.float16, (1, 8, 1, 1, 130, 64), dict(), "lin", None),
    ("bf16_left_window", torch.bfloat16, (1, 4, 4, 50, 50, 64), dict(window_size=(16, 0)), "lin", None),
    ("fp16_softcap_causal", torch.float16, (1, 4, 2, 40, 90, 64), dict(causal=True, softcap=5.0), "lin", None),
    ("bf16_keyless_rows", torch.bfloat16, (1, 2, 1, 130, 70, 64), dict(causal=True), "lin", None),
    ("bf16_sink_far_above", torch.bfloat16, (1, 2, 2, 16, 32, 64), dict(), 60.0, (3.0, -3.0)),
    ("bf16_sink_neg_inf", torch.bfloat16, (1, 4, 2, 33, 70, 64), dict(causal=True), -INF, None),
    ("fp16_d128_right_window", torch.float16, (1, 2, 1, 20, 40, 128), dict(window_size=(None, 10)), "lin", None),
]


def lse_float64(q, k, v, sink, causal=False, window_size=(None, None), softcap=0.0):
    """The definition of include/fa_fwd.h in float64, for the frozen LSE."""
    from oracle import attention_ref as oracle
    w = tuple(-1 if x is None else x for x in window_size)
    if causal:
        w = (w[0], 0)
    g = q.shape[2] // k.shape[2]
    s = torch.einsum("bthd,bshd->bhts", q.double() / math.sqrt(q.shape[-1]), k.double().repeat_interleave(g, dim=2))
    if softcap > 0:
        s = torch.tanh(s / softcap) * softcap
    if w[0] >= 0 or w[1] >= 0:
        s = s.masked_fill(oracle.local_mask(q.shape[1], k.shape[1], w), -INF)
    z = sink.double().view(1, -1, 1, 1).expand(s.shape[0], -1, s.shape[2], 1)
    return torch.logsumexp(torch.cat([s, z], dim=-1), dim=-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("FA_REFERENCE", "/root/reference"))
    args = ap.parse_args()
    spec = importlib.util.spec_from_file_location("cute_testing", os.path.join(args.reference, "flash_attn", "cute", "testing.py"))
    ct = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ct)
    gold = {}
    for i, (name, dtype, (b, h, hk, sq, sk, d), kw, sink_kind, const) in enumerate(CASES):
        gen = torch.Generator().manual_seed(100 + i)
        if const is None:
            q = torch.randn(b, sq, h, d, generator=gen).to(dtype)
            k = torch.randn(b, sk, hk, d, generator=gen).to(dtype)
        else:
            q = torch.full((b, sq, h, d), const[0]).to(dtype)
            k = torch.full((b, sk, hk, d), const[1]).to(dtype)
        v = torch.randn(b, sk, hk, d, generator=gen).to(dtype)
        sink = (torch.linspace(-4, 4, h) if sink_kind == "lin" else torch.full((h,), sink_kind)).to(torch.bfloat16)
        neg_inf = bool(torch.isneginf(sink).all())
        # the reference divides by a normaliser of 0 + exp(-inf - -inf) = nan on rows without keys when the sink is -inf: that
        # case has no such rows (sq <= sk), and there its function is the plain softmax
        out_ref, _ = ct.attention_ref(q, k, v, learnable_sink=sink, **kw)
        out_pt, _ = ct.attention_ref(q, k, v, learnable_sink=sink, upcast=False, reorder_ops=True, **kw)
        mine_ref, lse = sink_oracle.attention_sink_ref(q, k, v, sink, **kw)
        mine_pt, _ = sink_oracle.attention_sink_ref(q, k, v, sink, upcast=False, reorder_ops=True, **kw)
        for what, a, r in (("fp32 path", mine_ref, out_ref), ("low-precision path", mine_pt, out_pt)):
            delta = (a.float() - r.float()).abs().max().item()
            assert torch.equal(a, r), f"{name}: restatement differs from the reference on the {what}: max |delta| {delta:.3e}"
        lse64 = lse_float64(q, k, v, sink, **kw)
        fin = torch.isfinite(lse64)
        assert torch.equal(torch.isfinite(lse), fin), name
        assert (lse[fin].double() - lse64[fin]).abs().max().item() < 2e-5, name
        if neg_inf:
            plain, _ = ct.attention_ref(q, k, v, **kw)
            assert torch.equal(plain, out_ref), name
        gold[name] = dict(q=q, k=k, v=v, sink=sink, kwargs=kw, out_ref=out_ref, out_pt=out_pt, lse=lse)
        print(f"{name}: bit-equal on both paths; |out_pt - out_ref|max {(out_pt.float() - out_ref.float()).abs().max().item():.3e}")
    path = os.path.join(ROOT, "tests", "golden", "attention_sink_golden.pt")
    torch.save(gold, path)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
