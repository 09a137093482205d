"""Developer aid: what the fused cross-entropy loss costs.  One process, bf16 logits, M in {64, 8192, 32768} rows of N in {32000,
50257, 128256} classes, int64 labels, random data, logit_scale 0.7 (so that eager pays its multiply), no smoothing, no z-loss.
Hip-event timings of single calls after warm-up: the median of --iters (>= 30) calls, with the fastest and the slowest beside it.

Each row: the forward, the backward into a new tensor and the backward in place, as us and TB/s of algorithmic bytes (2 B per
element forward: the logits read once; 4 B backward: read once, written once), the time ratio to eager on the same device in
the same run -- F.cross_entropy(logits.float() * s, labels, reduction="none"), autograd for the backward -- and the peak memory
either needs above the logits for a forward and a backward (ours: in place).  A ratio below 1 is a finding.  The in-place
backward is timed on a scratch copy that it overwrites call after call: its time does not depend on the values.

Usage: python tools/xent_bench.py [--warmup W] [--iters N] [--out profiles/xent.jsonl]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

DEV = "cuda"
MS = (64, 8192, 32768)
NS = (32000, 50257, 128256)
SCALE = 0.7


def timed(run, iters):
    """(median, fastest, slowest) ms of `iters` single calls"""
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, e in ev:
        a.record(); run(); e.record()
    torch.cuda.synchronize()
    ms = sorted(a.elapsed_time(e) for a, e in ev)
    return ms[iters // 2], ms[0], ms[-1]


def peak_above(run):
    """peak bytes allocated during run() above what was allocated before it"""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    run()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - before


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "xent.jsonl"))
    args = ap.parse_args()
    assert args.iters >= 30
    assert torch.cuda.is_available(), "xent_bench needs a GPU"
    from flash_attention_annotated_amd.ops.triton import cross_entropy as xent
    torch.manual_seed(0)
    rows = []
    for n in NS:
        for M in MS:
            x = torch.randn(M, n, dtype=torch.bfloat16, device=DEV)
            y = torch.randint(0, n, (M,), device=DEV)
            d = torch.randn(M, device=DEV)
            work = x.clone()
            consts = (0.0, SCALE, 0.0, -100, 0, n)
            lse = xent._xent_fwd(x, y, None, *consts, False)[1]

            def eager_loss(logits):
                return F.cross_entropy(logits.float() * SCALE, y, reduction="none")

            def eager_forward():
                with torch.no_grad():
                    eager_loss(x)

            xl = x.detach().requires_grad_(True)
            held = eager_loss(xl)

            def eager_step():
                leaf = x.detach().requires_grad_(True)
                torch.autograd.grad(eager_loss(leaf), leaf, d)

            def fused_step():
                leaf = work.detach().requires_grad_(True)
                losses, _ = xent.cross_entropy_loss(leaf, y, None, 0.0, SCALE, 0.0, -100, True)
                torch.autograd.grad(losses, leaf, d)

            runs = {
                "forward": (lambda: xent._xent_fwd(x, y, None, *consts, False), eager_forward, 2),
                "backward": (lambda: xent._xent_bwd(d, x, y, lse, *consts), lambda: torch.autograd.grad(held, xl, d, retain_graph=True), 4),
                "backward_inplace": (lambda: xent._xent_bwd_inplace(d, work, y, lse, *consts), None, 4),
            }
            eager_ms = {}
            for direction, (fused, eager, per_elem) in runs.items():
                for run in (fused, eager):
                    for _ in range(args.warmup if run else 0):
                        run()
                ms, lo, hi = timed(fused, args.iters)
                if eager:
                    eager_ms[direction] = timed(eager, args.iters)[0]
                e_ms = eager_ms["backward" if direction == "backward_inplace" else direction]
                nbytes = M * n * per_elem
                row = dict(shape=f"M{M} N{n}", dtype="bf16", direction=direction, us=round(ms * 1e3, 2), us_min=round(lo * 1e3, 2),
                           us_max=round(hi * 1e3, 2), algorithmic_bytes=nbytes, tb_per_s=round(nbytes / ms / 1e9, 3),
                           eager_us=round(e_ms * 1e3, 2), eager_over_fused=round(e_ms / ms, 2), warmup=args.warmup, iters=args.iters)
                rows.append(row)
                print(json.dumps(row), flush=True)
            del held, xl
            row = dict(shape=f"M{M} N{n}", dtype="bf16", direction="peak_memory", logits_bytes=M * n * 2,
                       fused_peak_bytes=peak_above(fused_step), eager_peak_bytes=peak_above(eager_step))
            rows.append(row)
            print(json.dumps(row), flush=True)
            del x, work, runs
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
