"""Developer aid: what the fused residual-add + LayerNorm / RMSNorm costs.  One process, M = 65536 rows, N in {2048, 4096, 8192},
and M = 8192 rows of N = 32768 (the wide forms), bf16, random data.  Cases: RMS and LN, each with no residual, a bf16 residual,
and an fp32 residual under prenorm (not at N = 32768, where a row of the fp32 stream passes 64 KiB); forward and backward.
Hip-event timings of single calls after warm-up, the median of --iters (>= 30) calls.

Each row: us and TB/s of algorithmic bytes -- every tensor the case has to read or write, once (weight, bias, mean, rstd and
the fp32 dw / db partial rows left out: they are small) -- and the time ratio to two baselines on the same device in the same
run: `eager`, F.rms_norm / F.layer_norm plus the separate add and cast (autograd for the backward), and `ref`, this package's
layer_norm_ref / rms_norm_ref.  The yardstick for "fused pays" is eager: a ratio below 1 is a finding.

Usage: python tools/norm_bench.py [--warmup W] [--iters N] [--out profiles/norm.jsonl]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

DEV = "cuda"
SHAPES = ((65536, 2048), (65536, 4096), (65536, 8192), (8192, 32768))
EPS = 1e-5


def timed(run, iters):
    """median ms of `iters` single calls"""
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, e in ev:
        a.record(); run(); e.record()
    torch.cuda.synchronize()
    return sorted(a.elapsed_time(e) for a, e in ev)[iters // 2]


def eager_forward(x, w, b, res, rms, prenorm):
    """the passes a block pays without the fused kernel: the add (in the residual's dtype), the cast, the norm"""
    z = x if res is None else x.to(res.dtype) + res
    zn = z.to(x.dtype)
    y = F.rms_norm(zn, (x.shape[-1],), w, EPS) if rms else F.layer_norm(zn, (x.shape[-1],), w, b, EPS)
    return (y, z) if prenorm else y


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "norm.jsonl"))
    args = ap.parse_args()
    assert args.iters >= 30
    assert torch.cuda.is_available(), "norm_bench needs a GPU"
    from flash_attention_annotated_amd.ops import norm
    torch.manual_seed(0)
    rows = []
    for M, n in SHAPES:
        x = torch.randn(M, n, dtype=torch.bfloat16, device=DEV)
        w = torch.randn(n, dtype=torch.bfloat16, device=DEV)
        bias = torch.randn(n, dtype=torch.bfloat16, device=DEV)
        g = torch.randn(M, n, dtype=torch.bfloat16, device=DEV)
        for rms in (True, False):
            b = None if rms else bias
            ref_fn = norm.rms_norm_ref if rms else norm.layer_norm_ref
            for residual, prenorm in (("none", False), ("bf16", False), ("fp32", True)):
                if residual == "fp32" and n * 4 > 65536:
                    continue
                res = None if residual == "none" else torch.randn(M, n, device=DEV, dtype=torch.bfloat16 if residual == "bf16" else torch.float32)
                gres = torch.randn_like(res) if prenorm else None
                rb = 0 if res is None else res.element_size()
                # forward: x, residual in; y out; the new stream out where there is a residual
                fwd_bytes = M * n * (2 + rb + 2 + rb)
                # backward: the stream (or x), dy, dresidual in; dx out; dresidual_in out where it is not dx
                bwd_bytes = M * n * ((rb or 2) + 2 + (rb if prenorm else 0) + 2 + (rb if rb == 4 else 0))

                def leaves():
                    return [t.detach().requires_grad_(True) if t is not None else None for t in (x, w, b, res)]

                def forward(fn):
                    def run():
                        with torch.no_grad():
                            fn()
                    return run

                def backward(fn):
                    xl, wl, bl, rl = leaves()
                    out = fn(xl, wl, bl, rl)
                    outs, grads = ((out[0], out[1]), (g, gres)) if prenorm else ((out,), (g,))
                    ins = [t for t in (xl, wl, bl, rl) if t is not None]
                    return lambda: torch.autograd.grad(outs, ins, grads, retain_graph=True)

                fused = lambda xl, wl, bl, rl: norm.layer_norm_fn(xl, wl, bl, residual=rl, eps=EPS, prenorm=prenorm, is_rms_norm=rms)  # noqa: E731
                eager = lambda xl, wl, bl, rl: eager_forward(xl, wl, bl, rl, rms, prenorm)  # noqa: E731
                ref = lambda xl, wl, bl, rl: ref_fn(xl, wl, bl, residual=rl, eps=EPS, prenorm=prenorm)  # noqa: E731
                for direction, nbytes in (("forward", fwd_bytes), ("backward", bwd_bytes)):
                    runs = {}
                    for name, fn in (("fused", fused), ("eager", eager), ("ref", ref)):
                        runs[name] = forward(lambda fn=fn: fn(x, w, b, res)) if direction == "forward" else backward(fn)
                    for run in runs.values():
                        for _ in range(args.warmup):
                            run()
                    ms = {name: timed(run, args.iters) for name, run in runs.items()}
                    row = dict(shape=f"M{M} N{n}", dtype="bf16", norm="rms" if rms else "ln", residual=residual, prenorm=prenorm,
                               direction=direction, us=round(ms["fused"] * 1e3, 2), algorithmic_bytes=nbytes,
                               tb_per_s=round(nbytes / ms["fused"] / 1e9, 3), eager_us=round(ms["eager"] * 1e3, 2),
                               ref_us=round(ms["ref"] * 1e3, 2), eager_over_fused=round(ms["eager"] / ms["fused"], 2),
                               ref_over_fused=round(ms["ref"] / ms["fused"], 2), warmup=args.warmup, iters=args.iters)
                    rows.append(row)
                    print(json.dumps(row), flush=True)
                    del runs
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
