"""Developer aid: a decode step (seqlen_q = 1) that reads only listed key blocks of a KV cache -- sp_fwd_kernel,
csrc/fa_fwd_kernel_sp.h, through flash_attn_with_kvcache_sparse -- against the non-sparse call on the SAME cache
(flash_attn_with_kvcache: the GQA-folded decode of the 16-bit route, kv8_fwd_kernel over the fp8 cache), hq 32 / hkv 8, d 128,
bf16 queries, pages of 64 rows behind a shuffled table, num_splits = 0 on both sides (each route's own heuristic).

Grid: cache 8192 and 32768 (full), batch 1 / 8 / 64, a bf16 and an e4m3 cache, and 1, 1/2, 1/4, 1/8 of the blocks of B = 128
keys listed (a random subset per (batch, kv head), ascending).  The claim to test is time ~ fixed cost + listed bytes.  Per
shape the parent call and the four sparse calls are timed in the same process in alternating rounds (device events over warmed
calls, median of --iters per round, median / min / max over --rounds).  One JSON line per (shape, cache type), printed and
written to --out (profiles/sparse_kv_decode.jsonl):
  parent_us               the non-sparse step; sparse_us[f] the sparse step at listed fraction f
  ratio[f]                sparse_us[f] / parent_us; ratio["1"] is the price of the walk
  break_even              the listed fraction at which the line through the measured (fraction, time) points meets parent_us
                          (least squares: time = fixed_us + per_fraction_us * f), i.e. below which the sparse call wins
  listed_TBps[f]          listed K and V bytes of the step per second
GPU only.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from flash_attention_annotated_amd import _lib  # noqa: E402
from flash_attention_annotated_amd import hopper_interface as fa3  # noqa: E402

H, HK, D, PAGE, BLOCK = 32, 8, 128, 64, 128
BF, F8 = torch.bfloat16, torch.float8_e4m3fn
FRACTIONS = (1.0, 0.5, 0.25, 0.125)


def events(fn, iters):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, e in ev:
        a.record()
        fn()
        e.record()
    torch.cuda.synchronize()
    return sorted(a.elapsed_time(e) for a, e in ev)[iters // 2] * 1e-3


def last_plan():
    return _lib.load().fa_fwd_last_plan_name().decode()


def shape(b, sk, fp8):
    """(description, parent call, {fraction: sparse call}, bytes of K + V per listed key row over all kv heads)."""
    rows = b * sk
    k = torch.randn(rows // PAGE, PAGE, HK, D, dtype=BF, device="cuda")
    v = torch.randn(rows // PAGE, PAGE, HK, D, dtype=BF, device="cuda")
    kw = dict(cache_seqlens=torch.full((b,), sk, dtype=torch.int32, device="cuda"), num_splits=0,
              page_table=torch.randperm(rows // PAGE, device="cuda", dtype=torch.int32).view(b, sk // PAGE))
    if fp8:
        k, v = k.to(F8), v.to(F8)
        kw.update(k_descale=torch.ones(b, HK, device="cuda"), v_descale=torch.ones(b, HK, device="cuda"))
    q = torch.randn(b, 1, H, D, dtype=BF, device="cuda")
    nb = sk // BLOCK
    order = torch.rand(b, HK, nb, device="cuda").argsort(-1)  # a random subset per (batch, kv head) ...
    sparse = {}
    for f in FRACTIONS:
        n = max(1, int(nb * f))
        idx = order[..., :n].sort(-1).values.to(torch.int32).contiguous()  # ... listed ascending
        cnt = torch.full((b, HK), n, dtype=torch.int32, device="cuda")
        sparse[f] = lambda cnt=cnt, idx=idx: fa3.flash_attn_with_kvcache_sparse(q, k, v, cnt, idx, kv_block_size=BLOCK, **kw)  # noqa: E731
    parent = lambda: fa3.flash_attn_with_kvcache(q, k, v, **kw)  # noqa: E731
    return dict(b=b, s_k=sk, cache="e4m3" if fp8 else "bf16", page=PAGE, block=BLOCK), parent, sparse, 2 * HK * D * (1 if fp8 else 2)


def measure(desc, parent, sparse, row_bytes, warmup, iters, rounds):
    out_p = parent()
    plan_p = last_plan()
    out_s = sparse[1.0]()
    plan_s = last_plan()
    torch.cuda.synchronize()
    diff = (out_p.float() - out_s.float()).abs().max().item()  # all blocks listed: the same attention
    calls = [("parent", parent)] + [(f, sparse[f]) for f in FRACTIONS]
    for _ in range(warmup):
        for _, fn in calls:
            fn()
    t = {name: [] for name, _ in calls}
    for _ in range(rounds):  # alternating rounds: drift of the clocks hits all of them
        for name, fn in calls:
            t[name].append(events(fn, iters))
    med = lambda x: sorted(x)[len(x) // 2]  # noqa: E731
    us = lambda x: round(x * 1e6, 1)  # noqa: E731
    tp = med(t["parent"])
    ts = {f: med(t[f]) for f in FRACTIONS}
    # least squares of time over the listed fraction
    n, sx, sy = len(FRACTIONS), sum(FRACTIONS), sum(ts.values())
    sxx, sxy = sum(f * f for f in FRACTIONS), sum(f * ts[f] for f in FRACTIONS)
    slope = (n * sxy - sx * sy) / (n * sxx - sx * sx)
    fixed = (sy - slope * sx) / n
    listed = lambda f: desc["b"] * max(1, int(desc["s_k"] // BLOCK * f)) * BLOCK * row_bytes  # noqa: E731
    return dict(desc, parent_us=us(tp), parent_us_min_max=[us(min(t["parent"])), us(max(t["parent"]))],
                sparse_us={str(f): us(ts[f]) for f in FRACTIONS},
                sparse_us_min_max={str(f): [us(min(t[f])), us(max(t[f]))] for f in FRACTIONS},
                ratio={str(f): round(ts[f] / tp, 3) for f in FRACTIONS},
                fixed_us=us(fixed), per_fraction_us=us(slope), break_even=round((tp - fixed) / slope, 3) if slope > 0 else None,
                listed_TBps={str(f): round(listed(f) / ts[f] / 1e12, 2) for f in FRACTIONS},
                max_abs_diff_all_listed=diff, parent_plan=plan_p, sparse_plan=plan_s)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "sparse_kv_decode.jsonl"))
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="batch 8, cache 8192 only")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "sparse_kv_decode_bench needs a GPU"
    torch.manual_seed(0)
    grid = [(b, sk, fp8) for sk in (8192, 32768) for fp8 in (False, True) for b in (1, 8, 64)]
    if a.quick:
        grid = [(8, 8192, False), (8, 8192, True)]
    rows = []
    for b, sk, fp8 in grid:
        r = measure(*shape(b, sk, fp8), a.warmup, a.iters, a.rounds)
        print(json.dumps(r), flush=True)
        rows.append(r)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
