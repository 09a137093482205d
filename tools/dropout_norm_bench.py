"""Developer aid: what fusing the dropout into the residual add and the norm saves.  One process, M = 16384 rows, N in
{2048, 4096, 8192}, bf16 x0, fp32 residual, prenorm, p = 0.1, LayerNorm, random data.  Two arms, interleaved call by call so
that clocks and cache state drift over both alike:

    fused    ops.layer_norm.dropout_add_layer_norm(x0, residual, ..., prenorm=True)        (csrc/fa_dropout_norm.hip)
    parent   F.dropout(x0, p) followed by ops.triton.layer_norm.layer_norm_fn(residual=..., prenorm=True,
             residual_in_fp32=True): what a training block pays without this layer            (csrc/fa_norm.hip)

each forward alone and forward + backward (autograd of either arm, gradients of x0, the residual, weight and bias).  Hip-event
timings of single calls after warm-up; per row the median of --iters (>= 30) calls of each arm, the spread (min .. max) of
each, and parent / fused.  A ratio below 1 is a finding and is reported as it is.

Usage: python tools/dropout_norm_bench.py [--warmup W] [--iters N] [--out profiles/dropout_norm.jsonl]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

DEV = "cuda"
M, NS, P, EPS = 16384, (2048, 4096, 8192), 0.1, 1e-5


def interleaved(arms, warmup, iters):
    """{name: sorted ms of `iters` single calls}, the arms taking turns"""
    for _ in range(warmup):
        for run in arms.values():
            run()
    ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)] for k in arms}
    for i in range(iters):
        for k, run in arms.items():
            a, e = ev[k][i]
            a.record(); run(); e.record()
    torch.cuda.synchronize()
    return {k: sorted(a.elapsed_time(e) for a, e in v) for k, v in ev.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dropout_norm.jsonl"))
    args = ap.parse_args()
    assert args.iters >= 30
    assert torch.cuda.is_available(), "dropout_norm_bench needs a GPU"
    from flash_attention_annotated_amd.ops.layer_norm import dropout_add_layer_norm
    from flash_attention_annotated_amd.ops.triton.layer_norm import layer_norm_fn
    torch.manual_seed(0)
    rows = []
    for n in NS:
        x0 = torch.randn(M, n, dtype=torch.bfloat16, device=DEV, requires_grad=True)
        res = torch.randn(M, n, dtype=torch.float32, device=DEV, requires_grad=True)
        w = torch.randn(n, dtype=torch.bfloat16, device=DEV, requires_grad=True)
        b = torch.randn(n, dtype=torch.bfloat16, device=DEV, requires_grad=True)
        gz = torch.randn(M, n, dtype=torch.bfloat16, device=DEV)
        gx = torch.randn(M, n, dtype=torch.float32, device=DEV)

        def fused():
            return dropout_add_layer_norm(x0, res, w, b, P, EPS, prenorm=True)

        def parent():
            return layer_norm_fn(F.dropout(x0, P), w, b, residual=res, eps=EPS, prenorm=True, residual_in_fp32=True)

        def step(fwd):
            def run():
                z, x = fwd()
                torch.autograd.backward((z, x), (gz, gx))
                x0.grad = res.grad = w.grad = b.grad = None
            return run

        def forward_only(fwd):
            def run():
                with torch.no_grad():
                    fwd()
            return run
        for direction, wrap in (("forward", forward_only), ("forward+backward", step)):
            ms = interleaved({"fused": wrap(fused), "parent": wrap(parent)}, args.warmup, args.iters)
            med = {k: v[len(v) // 2] for k, v in ms.items()}
            row = {"shape": f"M{M} N{n}", "x0": "bf16", "residual": "fp32", "prenorm": True, "p": P, "norm": "ln", "direction": direction,
                   "fused_us": round(med["fused"] * 1e3, 2), "fused_min_us": round(ms["fused"][0] * 1e3, 2),
                   "fused_max_us": round(ms["fused"][-1] * 1e3, 2), "parent_us": round(med["parent"] * 1e3, 2),
                   "parent_min_us": round(ms["parent"][0] * 1e3, 2), "parent_max_us": round(ms["parent"][-1] * 1e3, 2),
                   "parent_over_fused": round(med["parent"] / med["fused"], 3), "warmup": args.warmup, "iters": args.iters}
            rows.append(row)
            print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
