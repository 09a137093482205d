"""Developer aid: top-k token-sparse MLA decode over the fp8 (e4m3) latent cache -- tk8_fwd_kernel, csrc/fa_fwd_kernel_tk8.h,
through flash_attn_with_kvcache_topk(k_descale=, v_descale=) -- against two baselines of the parent commit on the SAME values:
  topk16   the 16-bit flash_attn_with_kvcache_topk (tk_fwd_kernel) on the cache expanded to bf16 with the descales multiplied in;
  dense8   the dense fp8 flash_attn_with_kvcache(qv=, k_descale=, v_descale=) (qv8_fwd_kernel) on the same e4m3 cache.
bf16 q, h_k 1, d 64 / d_v 512, one query token per batch entry, pages of 64 rows behind a shuffled table, num_splits = 0.

Grid (tools/topk_kv_decode_bench.py's): h 16 / 128, batch 1 / 8 / 64, cache 8192 / 32768 (full), topk 512 / 2048 random distinct
positions per token, plus every position listed in order at cache 8192.  Per shape the three calls are timed in the same process in
alternating rounds (device events over warmed calls, median of --iters per round, median / min / max over --rounds).  One JSON
line per shape, printed and written to --out (profiles/topk_kv8_decode.jsonl):
  topk8_us, topk16_us, dense8_us    the three calls;  vs_topk16 = topk8_us / topk16_us, vs_dense8 = topk8_us / dense8_us
  rows_per_us_8 / rows_per_us_16    b * topk gathered rows per microsecond of the fp8 / the 16-bit top-k call
GPU only.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from flash_attention_annotated_amd import hopper_interface as fa3  # noqa: E402
from tools.topk_kv_decode_bench import D, DV, PAGE, BF, events, last_plan  # noqa: E402


def shape(b, sk, h, topk):
    """(description, {name: call}); topk None = every position in order."""
    rows = b * sk
    cache8 = torch.randn(rows // PAGE, PAGE, 1, D + DV, device="cuda").to(torch.float8_e4m3fn)
    kd, vd = torch.full((b, 1), 0.5, device="cuda"), torch.full((b, 1), 2.0, device="cuda")
    cache16 = cache8.to(BF)  # the same values: e4m3 is exact in bf16, the descales are powers of two
    cache16[..., :D] *= 0.5
    cache16[..., D:] *= 2.0
    kw = dict(cache_seqlens=torch.full((b,), sk, dtype=torch.int32, device="cuda"), num_splits=0,
              page_table=torch.randperm(rows // PAGE, device="cuda", dtype=torch.int32).view(b, sk // PAGE))
    q = torch.randn(b, 1, h, D, dtype=BF, device="cuda")
    qv = torch.randn(b, 1, h, DV, dtype=BF, device="cuda")
    if topk is None:
        idx = torch.arange(sk, dtype=torch.int32, device="cuda").expand(b, 1, 1, sk).contiguous()
    else:
        idx = torch.rand(b, sk, device="cuda").argsort(-1)[:, :topk].to(torch.int32).view(b, 1, 1, topk).contiguous()
    k8, v8, k16, v16 = cache8[..., :D], cache8[..., D:], cache16[..., :D], cache16[..., D:]
    calls = dict(topk8=lambda: fa3.flash_attn_with_kvcache_topk(q, k8, v8, idx, qv=qv, k_descale=kd, v_descale=vd, **kw),
                 topk16=lambda: fa3.flash_attn_with_kvcache_topk(q, k16, v16, idx, qv=qv, **kw),
                 dense8=lambda: fa3.flash_attn_with_kvcache(q, k8, v8, qv=qv, k_descale=kd, v_descale=vd, **kw))
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
    for _ in range(rounds):  # alternating rounds: drift of the clocks hits all three
        for name, fn in calls.items():
            t[name].append(events(fn, iters))
    med = lambda x: sorted(x)[len(x) // 2]  # noqa: E731
    us = lambda x: round(x * 1e6, 1)  # noqa: E731
    res = dict(desc)
    for name in calls:
        res[f"{name}_us"] = us(med(t[name]))
        res[f"{name}_us_min_max"] = [us(min(t[name])), us(max(t[name]))]
    n = desc["b"] * desc["topk"]
    res.update(vs_topk16=round(med(t["topk8"]) / med(t["topk16"]), 3), vs_dense8=round(med(t["topk8"]) / med(t["dense8"]), 3),
               rows_per_us_8=round(n / med(t["topk8"]) * 1e-6, 1), rows_per_us_16=round(n / med(t["topk16"]) * 1e-6, 1),
               **{f"{name}_plan": plan for name, plan in plans.items()})
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "topk_kv8_decode.jsonl"))
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="batch 8, h 16 only")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "topk_kv8_decode_bench needs a GPU"
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
