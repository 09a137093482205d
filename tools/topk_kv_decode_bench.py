"""Developer aid: top-k token-sparse MLA decode -- tk_fwd_kernel, csrc/fa_fwd_kernel_tk.h, through flash_attn_with_kvcache_topk --
against the dense flash_attn_with_kvcache(qv=) of the parent commit (fwd_kernel_qv) on the SAME latent cache.  bf16, h_k 1, d 64 /
d_v 512, one query token per batch entry, pages of 64 rows behind a shuffled table, num_splits = 0 on both sides.

Grid: h 16 / 128, batch 1 / 8 / 64, cache 8192 / 32768 (full), topk 512 / 2048 random distinct positions per token, plus every
position listed in order at cache 8192 (the price of the gather walk itself).  Per shape the two calls are timed in the same
process in alternating rounds (device events over warmed calls, median of --iters per round, median / min / max over --rounds).
One JSON line per shape, printed and written to --out (profiles/topk_kv_decode.jsonl):
  dense_us, topk_us       the two calls;  ratio = topk_us / dense_us
  gathered_gbps           b * topk rows of 576 bf16 elements per topk_us (each row block of a token at h 128 gathers them again:
                          those reads are not counted)
  dense_gbps              b * cache rows of the same width per dense_us
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

D, DV, PAGE, BF = 64, 512, 64, torch.bfloat16


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


def shape(b, sk, h, topk):
    """(description, {name: call}); topk None = every position in order."""
    rows = b * sk
    cache = torch.randn(rows // PAGE, PAGE, 1, D + DV, dtype=BF, device="cuda")
    k, v = cache[..., :D], cache[..., D:]
    kw = dict(cache_seqlens=torch.full((b,), sk, dtype=torch.int32, device="cuda"), num_splits=0,
              page_table=torch.randperm(rows // PAGE, device="cuda", dtype=torch.int32).view(b, sk // PAGE))
    q = torch.randn(b, 1, h, D, dtype=BF, device="cuda")
    qv = torch.randn(b, 1, h, DV, dtype=BF, device="cuda")
    if topk is None:
        idx = torch.arange(sk, dtype=torch.int32, device="cuda").expand(b, 1, 1, sk).contiguous()
    else:
        idx = torch.rand(b, sk, device="cuda").argsort(-1)[:, :topk].to(torch.int32).view(b, 1, 1, topk).contiguous()
    calls = dict(dense=lambda: fa3.flash_attn_with_kvcache(q, k, v, qv=qv, **kw),
                 topk=lambda: fa3.flash_attn_with_kvcache_topk(q, k, v, idx, qv=qv, **kw))
    return dict(b=b, s_k=sk, h=h, topk=idx.shape[-1], listed="all" if topk is None else "random", page=PAGE), calls


def measure(desc, calls, warmup, iters, rounds):
    plans = {}
    for name, fn in calls.items():
        fn()
        plans[name] = last_plan()
    for _ in range(warmup):
        for fn in calls.values():
            fn()
    t = {name: [] for name in calls}
    for _ in range(rounds):  # alternating rounds: drift of the clocks hits both
        for name, fn in calls.items():
            t[name].append(events(fn, iters))
    med = lambda x: sorted(x)[len(x) // 2]  # noqa: E731
    us = lambda x: round(x * 1e6, 1)  # noqa: E731
    res = dict(desc)
    for name in calls:
        res[f"{name}_us"] = us(med(t[name]))
        res[f"{name}_us_min_max"] = [us(min(t[name])), us(max(t[name]))]
    row_bytes = (D + DV) * 2
    res.update(ratio=round(med(t["topk"]) / med(t["dense"]), 3),
               gathered_gbps=round(desc["b"] * desc["topk"] * row_bytes / med(t["topk"]) * 1e-9, 1),
               dense_gbps=round(desc["b"] * desc["s_k"] * row_bytes / med(t["dense"]) * 1e-9, 1),
               dense_plan=plans["dense"], topk_plan=plans["topk"])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "topk_kv_decode.jsonl"))
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="batch 8, h 16 only")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "topk_kv_decode_bench needs a GPU"
    torch.manual_seed(0)
    grid = [(b, sk, h, topk) for h in (16, 128) for sk in (8192, 32768) for b in (1, 8, 64)
            for topk in (512, 2048) + ((None,) if sk == 8192 else ())]
    if a.quick:
        grid = [g for g in grid if g[0] == 8 and g[2] == 16]
    rows = []
    for b, sk, h, topk in grid:
        r = measure(*shape(b, sk, h, topk), a.warmup, a.iters, a.rounds)
        print(json.dumps(r), flush=True)
        rows.append(r)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
