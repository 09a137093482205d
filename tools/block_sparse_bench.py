"""Developer aid: what block sparsity buys the forward.  One process, the C2 shape (b4 h16 s8192 d128 bf16: 64 x 64 blocks
per head), the block-sparse call of every pattern interleaved with the plain dense call of the same q / k / v (the manner of
tools/sink_bench.py: both sides see the same clocks and caches), medians of event timings.  Patterns: random block masks at
densities 1.0 / 0.5 / 0.25 / 0.125 (exactly density x nk blocks per query block, distinct per batch and head), block-causal,
and a local band of 8 blocks plus the first key block per query block.  Appends one JSON line per pattern to
profiles/block_sparse.jsonl: ms, t_sparse / t_dense (the dense default plan, which this kernel does not touch) and
t_sparse(rho) / (rho * t_sparse(1.0)) -- 1.0 = time proportional to the visited blocks.
Usage: python tools/block_sparse_bench.py [--rounds R] [--iters N] [--out profiles/block_sparse.jsonl]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

DEV = "cuda"
B, H, S, D = 4, 16, 8192, 128
N = S // 128


def random_mask(density, gen):
    keep = max(1, round(density * N))
    order = torch.rand(B, H, N, N, generator=gen).argsort(-1)
    return order < keep  # exactly `keep` blocks per query block


def block_causal(_gen):
    return torch.ones(N, N, dtype=torch.bool).tril().view(1, 1, N, N)


def band_plus_first(_gen):
    i, j = torch.arange(N).view(-1, 1), torch.arange(N).view(1, -1)
    return (((j <= i) & (j > i - 8)) | (j == 0)).view(1, 1, N, N)


PATTERNS = {
    "random_1.0": lambda g: random_mask(1.0, g),
    "random_0.5": lambda g: random_mask(0.5, g),
    "random_0.25": lambda g: random_mask(0.25, g),
    "random_0.125": lambda g: random_mask(0.125, g),
    "block_causal": block_causal,
    "band8_plus_first": band_plus_first,
}


def timed(run, iters):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, e in ev:
        a.record(); run(); e.record()
    torch.cuda.synchronize()
    return sorted(a.elapsed_time(e) for a, e in ev)[iters // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "block_sparse.jsonl"))
    ap.add_argument("--patterns", default=",".join(PATTERNS))
    args = ap.parse_args()
    from flash_attention_annotated_amd import cute_interface as cute
    from parity_helpers import last_plan
    torch.manual_seed(0)
    gen = torch.Generator().manual_seed(0)
    q, k, v = (torch.randn(B, S, H, D, device=DEV, dtype=torch.bfloat16) for _ in range(3))
    dense = lambda: cute.flash_attn_func(q, k, v)  # noqa: E731
    dense()
    dense_plan = last_plan()
    recs = []
    for name in args.patterns.split(","):
        mask = PATTERNS[name](gen)
        rho = mask.float().mean().item()
        fc, fi, mc, mi = (t.to(DEV) for t in cute.block_sparse_from_mask(mask))
        sparse = lambda: cute.flash_attn_func(q, k, v, full_block_cnt=fc, full_block_idx=fi, mask_block_cnt=mc,  # noqa: E731
                                              mask_block_idx=mi)
        for _ in range(3):  # warm up both sides
            dense(); sparse()
        plan = last_plan()
        td, ts = [], []
        for _ in range(args.rounds):
            td.append(timed(dense, args.iters))
            ts.append(timed(sparse, args.iters))
        a, b = sorted(td)[args.rounds // 2], sorted(ts)[args.rounds // 2]
        recs.append(dict(pattern=name, density=round(rho, 4), plan=plan, dense_plan=dense_plan, ms_sparse=round(b, 5),
                         ms_dense=round(a, 5), sparse_over_dense=round(b / a, 4), rounds=args.rounds, iters=args.iters,
                         device=torch.cuda.get_device_name(0)))
    full = next((r["ms_sparse"] for r in recs if r["pattern"] == "random_1.0"), None)
    with open(args.out, "a") as f:
        for r in recs:
            if full:  # time against the visited share of the all-blocks time: 1.0 = proportional
                r["proportionality"] = round(r["ms_sparse"] / (r["density"] * full), 4)
            print(json.dumps(r), flush=True)
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
