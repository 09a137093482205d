"""Developer aid: what the fused MLP activations cost.  One process, bf16, random data; plain shapes M x N (bias + gelu, tanh
form, fp32-free: the bias is bf16) and gated shapes M x H (SwiGLU from one packed (M, 2H) tensor).  Hip-event timings of
single calls after warm-up: the median of --iters (>= 30) calls, with the fastest and the slowest beside it.

Each row: us and TB/s of algorithmic bytes (every tensor once: plain forward 4 B per element, backward 6, with recompute 8;
gated forward 6 B per element of H, backward 10, with recompute 12; the bias and dbias rows are counted too), and the time
ratio to the eager sequence it replaces on the same device in the same run -- F.gelu(pre + bias, approximate="tanh") and its
autograd (whose bias gradient is the separate pass), chunk + F.silu * up and its autograd for the gated form.  Eager has no
recompute variant: those rows are compared with eager backward + eager forward.  A ratio below 1 is a finding.

Usage: python tools/act_bench.py [--warmup W] [--iters N] [--out profiles/act.jsonl]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

DEV = "cuda"
PLAIN = ((8192, 16384), (32768, 16384), (64, 16384))
GATED = ((8192, 11008), (8192, 14336), (32768, 14336), (64, 14336))


def timed(run, iters):
    """(median, fastest, slowest) ms of `iters` single calls"""
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, e in ev:
        a.record(); run(); e.record()
    torch.cuda.synchronize()
    ms = sorted(a.elapsed_time(e) for a, e in ev)
    return ms[iters // 2], ms[0], ms[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "act.jsonl"))
    args = ap.parse_args()
    assert args.iters >= 30
    assert torch.cuda.is_available(), "act_bench needs a GPU"
    from flash_attention_annotated_amd.ops import activations as A
    torch.manual_seed(0)
    rows = []

    def record(form, shape, direction, fused, eager, nbytes, plan):
        for run in (fused, eager):
            for _ in range(args.warmup):
                run()
        ms, lo, hi = timed(fused, args.iters)
        e_ms = timed(eager, args.iters)[0]
        row = dict(form=form, shape=shape, dtype="bf16", direction=direction, cw=plan["cw"], us=round(ms * 1e3, 2),
                   us_min=round(lo * 1e3, 2), us_max=round(hi * 1e3, 2), algorithmic_bytes=nbytes, tb_per_s=round(nbytes / ms / 1e9, 3),
                   eager_us=round(e_ms * 1e3, 2), eager_over_fused=round(e_ms / ms, 2), warmup=args.warmup, iters=args.iters)
        rows.append(row)
        print(json.dumps(row), flush=True)

    for m, n in PLAIN:
        pre = torch.randn(m, n, dtype=torch.bfloat16, device=DEV)
        d = torch.randn(m, n, dtype=torch.bfloat16, device=DEV)
        bias = torch.randn(n, dtype=torch.bfloat16, device=DEV)
        code, shape, e = A.GELU_TANH, f"M{m} N{n}", m * n * 2

        def eager_fwd():
            with torch.no_grad():
                return F.gelu(pre + bias, approximate="tanh")

        leaf, bleaf = pre.detach().requires_grad_(True), bias.detach().requires_grad_(True)
        held = F.gelu(leaf + bleaf, approximate="tanh")
        held_nobias = F.gelu(leaf, approximate="tanh")
        fplan, bplan = A._plan_forward(pre, None, bias, code), A._plan_backward(d, pre, None, bias, code, True, True, False)
        record("plain", shape, "forward", lambda: A._act_fwd(pre, None, bias, code), eager_fwd, 2 * e + 2 * n, fplan)
        record("plain", shape, "backward", lambda: A._act_bwd(d, pre, None, None, code, False, False, False),
               lambda: torch.autograd.grad(held_nobias, leaf, d, retain_graph=True), 3 * e, bplan)
        record("plain", shape, "backward_dbias", lambda: A._act_bwd(d, pre, None, bias, code, True, False, False),
               lambda: torch.autograd.grad(held, (leaf, bleaf), d, retain_graph=True), 3 * e + 4 * n, bplan)
        record("plain", shape, "backward_dbias_recompute", lambda: A._act_bwd(d, pre, None, bias, code, True, True, False),
               lambda: (torch.autograd.grad(held, (leaf, bleaf), d, retain_graph=True), eager_fwd()), 4 * e + 4 * n, bplan)
        del pre, d, held, held_nobias, leaf
        torch.cuda.empty_cache()

    for m, h in GATED:
        x12 = torch.randn(m, 2 * h, dtype=torch.bfloat16, device=DEV)
        d = torch.randn(m, h, dtype=torch.bfloat16, device=DEV)
        up, gate = x12[:, :h], x12[:, h:]
        code, shape, e = A.SILU, f"M{m} H{h}", m * h * 2

        def eager_gated(t):
            y, g = t.chunk(2, dim=-1)
            return y * F.silu(g)

        def eager_fwd():
            with torch.no_grad():
                return eager_gated(x12)

        leaf = x12.detach().requires_grad_(True)
        held = eager_gated(leaf)
        fplan, bplan = A._plan_forward(gate, up, None, code), A._plan_backward(d, gate, up, None, code, False, True, True)
        record("gated", shape, "forward", lambda: A._act_fwd(gate, up, None, code), eager_fwd, 3 * e, fplan)
        record("gated", shape, "backward", lambda: A._act_bwd(d, gate, up, None, code, False, False, True),
               lambda: torch.autograd.grad(held, leaf, d, retain_graph=True), 5 * e, bplan)
        record("gated", shape, "backward_recompute", lambda: A._act_bwd(d, gate, up, None, code, False, True, True),
               lambda: (torch.autograd.grad(held, leaf, d, retain_graph=True), eager_fwd()), 6 * e, bplan)
        del x12, d, held, leaf, up, gate
        torch.cuda.empty_cache()

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
