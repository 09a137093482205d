"""Developer aid: what producing the lists of a block-sparse prefill costs -- cute_interface.block_sparse_select
(csrc/fa_block_pattern.hip) -- against the torch composition a caller would write instead, and against the sparse forward the
lists feed.  hq 32 / hkv 8, d 128, bf16, causal, batch 1 / 4, s = sq = sk in 8192 / 32768 / 131072, num_blocks = nk / 8 (sink 1,
local 1), with and without the key-major lists of the backward.

Per shape, in one process, in alternating rounds (device events over warmed calls, median of --iters per round, median / min /
max over --rounds):
  select_us      block_sparse_select (two launches; three with the key-major lists)
  torch_us       the same rule composed of torch calls: pool q and k, an einsum over all (nm, nk) pairs, the causal block mask,
                 topk, a bool (b, h, nm, nk) mask, block_sparse_from_mask (and block_sparse_bwd_lists with the key-major lists).
                 The baseline: the code under test is never its own yardstick
  sparse_fwd_us  flash_attn_func on the producer's own lists
  select_over_torch, select_over_sparse_fwd   the two ratios
  qk_GBps_over_select   the bytes of q and k, which the pooling launch reads once, over select_us: a LOWER bound of the pooling's
                 rate.  The launches' own times come from a kernel trace, in a run of its own:
                 rocprofv3 --kernel-trace --stats -d DIR -- python tools/block_pattern_bench.py --profile B S
One JSON line per (shape, lists), printed and written to --out (profiles/block_pattern.jsonl).  GPU only.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from flash_attention_annotated_amd import _lib  # noqa: E402
from flash_attention_annotated_amd import cute_interface as cute  # noqa: E402

H, HK, D, BLOCK = 32, 8, 128, 128
BF = torch.bfloat16


def events(fn, iters):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, e in ev:
        a.record()
        fn()
        e.record()
    torch.cuda.synchronize()
    return sorted(a.elapsed_time(e) for a, e in ev)[iters // 2] * 1e-3


def torch_select(q, k, num_blocks, bwd, sink=1, local=1):
    """The rule of block_sparse_select (causal, sq = sk a multiple of 128) as a torch composition."""
    b, s, h, d = q.shape
    n = s // BLOCK
    qs = q.view(b, n, BLOCK, h, d).float().sum(2)
    km = k.view(b, n, BLOCK, k.shape[2], d).float().mean(2)
    u = torch.einsum("bmhc,bnhc->bhmn", qs, km.repeat_interleave(h // k.shape[2], dim=2))
    m, j = torch.arange(n, device=q.device)[:, None], torch.arange(n, device=q.device)[None, :]
    u = torch.where((j < sink) | (j > m - local), float("inf"), u)
    u = torch.where(j <= m, u, float("-inf"))
    idx = u.topk(num_blocks, -1).indices
    chosen = torch.zeros(b, h, n, n, dtype=torch.bool, device=q.device).scatter_(-1, idx, True) & (j <= m)
    lists = cute.block_sparse_from_mask(chosen, (j < m).expand(b, h, n, n))
    return lists + (cute.block_sparse_bwd_lists(*lists) if bwd else ())


def shape(b, s, bwd):
    q = torch.randn(b, s, H, D, dtype=BF, device="cuda")
    k = torch.randn(b, s, HK, D, dtype=BF, device="cuda")
    v = torch.randn(b, s, HK, D, dtype=BF, device="cuda")
    nk = s // BLOCK
    nb = max(2, nk // 8)
    select = lambda: cute.block_sparse_select(q, k, nb, causal=True, with_bwd_lists=bwd)  # noqa: E731
    sel = select()
    lists = {name: t for name, t in sel._asdict().items() if t is not None}
    calls = {"select": select, "torch": lambda: torch_select(q, k, nb, bwd),
             "sparse_fwd": lambda: cute.flash_attn_func(q, k, v, causal=True, **lists)}
    # the composition and the kernels choose the same blocks where fp32 sums in two orders rank alike: report the agreement
    t_lists = calls["torch"]()
    agree = [round((a == e).float().mean().item(), 4) for a, e in zip(t_lists, sel)]
    plan = _lib.binding().block_pattern_plan(q, k, *sel[:4], sel.q_block_cnt, sel.q_block_idx, None, None, nb, True, -1, -1, 1, 1)
    return dict(b=b, s=s, blocks=nk, num_blocks=nb, key_major_lists=bwd, plan=plan, torch_agreement=agree), calls


def measure(desc, calls, warmup, iters, rounds):
    for _ in range(warmup):
        for fn in calls.values():
            fn()
    t = {name: [] for name in calls}
    for _ in range(rounds):  # alternating rounds: drift of the clocks hits all of them
        for name, fn in calls.items():
            t[name].append(events(fn, iters))
    med = lambda x: sorted(x)[len(x) // 2]  # noqa: E731
    us = lambda x: round(x * 1e6, 1)  # noqa: E731
    m = {name: med(x) for name, x in t.items()}
    read_bytes = desc["b"] * desc["s"] * (H + HK) * D * 2
    return dict(desc, select_us=us(m["select"]), torch_us=us(m["torch"]), sparse_fwd_us=us(m["sparse_fwd"]),
                select_over_torch=round(m["select"] / m["torch"], 4), select_over_sparse_fwd=round(m["select"] / m["sparse_fwd"], 4),
                qk_bytes=read_bytes, qk_GBps_over_select=round(read_bytes / m["select"] / 1e9, 1),
                us_min_max={name: [us(min(x)), us(max(x))] for name, x in t.items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "block_pattern.jsonl"))
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="batch 1, s 8192 only")
    ap.add_argument("--profile", type=int, nargs=2, metavar=("B", "S"), help="20 calls with the key-major lists at this shape, for a kernel trace; nothing is written")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "block_pattern_bench needs a GPU"
    torch.manual_seed(0)
    if a.profile:
        q = torch.randn(a.profile[0], a.profile[1], H, D, dtype=BF, device="cuda")
        k = torch.randn(a.profile[0], a.profile[1], HK, D, dtype=BF, device="cuda")
        for _ in range(20):
            cute.block_sparse_select(q, k, max(2, a.profile[1] // BLOCK // 8), causal=True, with_bwd_lists=True)
        torch.cuda.synchronize()
        return
    grid = [(b, s, bwd) for s in (8192, 32768, 131072) for b in (1, 4) for bwd in (False, True)]
    if a.quick:
        grid = [(1, 8192, False), (1, 8192, True)]
    rows = []
    for b, s, bwd in grid:
        r = measure(*shape(b, s, bwd), a.warmup, a.iters if s < 131072 else max(3, a.iters // 3), a.rounds)
        print(json.dumps(r), flush=True)
        rows.append(r)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
