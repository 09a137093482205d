"""Developer aid: what block sparsity buys the backward -- the sibling of tools/block_sparse_bench.py.  One process, the C2 shape
(b4 h16 s8192 d128 bf16: 64 x 64 blocks per head) and the same patterns; for every pattern the block-sparse backward
(cute_bwd_block_sparse behind its own forward) interleaved with the dense backward (cute_bwd behind the dense forward) of the
same q / k / v / dout, so both sides see the same clocks and caches; medians of event timings over the three launches of a
backward (D, dK/dV, dQ).  Only the backward is inside the events: the forwards run once per pattern, outside.
Appends one JSON line per pattern to profiles/block_sparse_bwd.jsonl: ms, t_sparse / t_dense, t_sparse(rho) / (rho *
t_sparse(1.0)) -- 1.0 = time proportional to the visited blocks -- and a last line with the break-even density: where the
least-squares line through the random patterns' (rho, ms_sparse) meets the dense time.
Usage: python tools/block_sparse_bwd_bench.py [--rounds R] [--iters N] [--out profiles/block_sparse_bwd.jsonl]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

from block_sparse_bench import B, D, DEV, H, PATTERNS, S, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "block_sparse_bwd.jsonl"))
    ap.add_argument("--patterns", default=",".join(PATTERNS))
    args = ap.parse_args()
    from flash_attention_annotated_amd import _lib
    from flash_attention_annotated_amd import cute_interface as cute
    from parity_helpers import last_bwd_plan
    ext = _lib.binding()
    torch.manual_seed(0)
    gen = torch.Generator().manual_seed(0)
    q, k, v, g = (torch.randn(B, S, H, D, device=DEV, dtype=torch.bfloat16) for _ in range(4))
    scale = D ** -0.5
    out_d, lse_d = cute.flash_attn_func(q, k, v)
    dense = lambda: ext.cute_bwd(g, q, k, v, out_d, lse_d, None, None, None, None, scale, False, -1, -1, 0.0, None)  # noqa: E731
    dense()
    dense_plan = last_bwd_plan()
    recs = []
    for name in args.patterns.split(","):
        mask = PATTERNS[name](gen)
        rho = mask.float().mean().item()
        lists = tuple(t.to(DEV) for t in cute.block_sparse_from_mask(mask))
        key_lists = cute.block_sparse_bwd_lists(*lists)
        out_s, lse_s = cute.flash_attn_func(q, k, v, full_block_cnt=lists[0], full_block_idx=lists[1], mask_block_cnt=lists[2],
                                            mask_block_idx=lists[3])
        sparse = lambda: ext.cute_bwd_block_sparse(g, q, k, v, out_s, lse_s, scale, False, -1, -1, 0.0, None, *lists,  # noqa: E731
                                                   *key_lists)
        for _ in range(2):  # warm up both sides
            dense(); sparse()
        plan = last_bwd_plan()
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
        rnd = [r for r in recs if r["pattern"].startswith("random_")]
        if len(rnd) >= 2:  # ms_sparse = a + b rho over the random patterns; break-even where it meets the dense time
            xs, ys = [r["density"] for r in rnd], [r["ms_sparse"] for r in rnd]
            mx, my = sum(xs) / len(xs), sum(ys) / len(ys)
            slope = sum((x - mx) * (y - my) for x, y in zip(xs, ys)) / sum((x - mx) ** 2 for x in xs)
            icpt = my - slope * mx
            t_dense = sorted(r["ms_dense"] for r in rnd)[len(rnd) // 2]
            fit = dict(pattern="fit_random", ms_at_zero=round(icpt, 5), ms_per_density=round(slope, 5), ms_dense=round(t_dense, 5),
                       break_even_density=round((t_dense - icpt) / slope, 4))
            print(json.dumps(fit), flush=True)
            f.write(json.dumps(fit) + "\n")


if __name__ == "__main__":
    main()
