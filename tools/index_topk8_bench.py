"""Developer aid: what the lightning indexer costs over an e4m3 index-key cache with one scale per token --
kvcache_index_topk(k_index_scale=) (csrc/fa_index_topk8.hip) -- against the 16-bit kvcache_index_topk on the SAME values (the
dequantised cache in bf16, which holds them exactly), and what the quantising append kvcache_index_append_fp8 costs per row.
Shapes: index heads 64, index dim 128, bf16 queries, pages of 64 rows behind a shuffled table, one token per batch entry, batch
1 / 8 / 64, cache 8192 / 32768 / 131072 (full), topk 2048.

Per shape, in one process, in alternating rounds (device events over warmed calls, median of --iters per round, median / min /
max over --rounds):
  call8_us / call16_us      both launches, e4m3 / 16-bit cache; call_ratio = call8 / call16
  logits8_us / logits16_us  the call with topk = capacity: its selection launch only writes 0 .. n - 1, so this is the logits
                            launch (+ a near-empty launch); logits_ratio = logits8 / logits16
  key8_GBps / key16_GBps    the key bytes (b * sk * (128 + 4), b * sk * 256) over the logits time
  append_us                 one new row per batch entry (a decode step's append)
  fill_ns_per_row           the append of the whole cache, b * sk rows in one call, per row
  lists_equal               the share of list entries the two calls agree on (the fp8 call rounds once more, by the scale)
One JSON line per shape, printed and written to --out (profiles/index_topk8.jsonl).  GPU only.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from flash_attention_annotated_amd import _lib  # noqa: E402
from flash_attention_annotated_amd import hopper_interface as fa3  # noqa: E402

HI, DI, PAGE, TOPK = 64, 128, 64, 2048
BF, F8 = torch.bfloat16, torch.float8_e4m3fn


def events(fn, iters):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, e in ev:
        a.record()
        fn()
        e.record()
    torch.cuda.synchronize()
    return sorted(a.elapsed_time(e) for a, e in ev)[iters // 2] * 1e-3


def shape(b, sk):
    pages = b * sk // PAGE
    table = torch.randperm(pages, device="cuda", dtype=torch.int32).view(b, sk // PAGE)
    k8 = torch.empty(pages, PAGE, DI, dtype=F8, device="cuda")
    scale = torch.empty(pages, PAGE, dtype=torch.float32, device="cuda")
    rows = torch.randn(b, sk, DI, dtype=BF, device="cuda")
    zero, fills = torch.zeros(b, dtype=torch.int32, device="cuda"), torch.full((b,), sk, dtype=torch.int32, device="cuda")
    last = fills - 1
    fill = lambda: fa3.kvcache_index_append_fp8(k8, scale, rows, zero, page_table=table)  # noqa: E731
    fill()
    k16 = (k8.float() * scale[..., None]).to(BF)  # the same values: 4 significant bits times a power of two
    q_i = torch.randn(b, 1, HI, DI, dtype=BF, device="cuda")
    w = torch.randn(b, 1, HI, device="cuda") * HI ** -0.5
    idx8, idx16 = (torch.empty(b, 1, 1, TOPK, dtype=torch.int32, device="cuda") for _ in range(2))
    every = torch.empty(b, 1, 1, sk, dtype=torch.int32, device="cuda")
    logits = torch.empty(b, 1, sk, dtype=torch.float32, device="cuda")
    kw = dict(page_table=table, logits=logits)
    calls = {"call8": lambda: fa3.kvcache_index_topk(q_i, k8, w, fills, TOPK, k_index_scale=scale, indices=idx8, **kw),
             "call16": lambda: fa3.kvcache_index_topk(q_i, k16, w, fills, TOPK, indices=idx16, **kw),
             "logits8": lambda: fa3.kvcache_index_topk(q_i, k8, w, fills, sk, k_index_scale=scale, indices=every, **kw),
             "logits16": lambda: fa3.kvcache_index_topk(q_i, k16, w, fills, sk, indices=every, **kw),
             # (the last row again: the cache keeps its values)
             "append": lambda: fa3.kvcache_index_append_fp8(k8, scale, rows[:, sk - 1:], last, page_table=table),
             "fill": fill}
    calls["call8"](), calls["call16"]()
    desc = dict(b=b, s_k=sk, h_i=HI, d_i=DI, page=PAGE, topk=TOPK, lists_equal=round((idx8 == idx16).float().mean().item(), 4),
                plan=_lib.binding().kvcache_index_topk_fp8_plan(q_i, k8, scale, w, fills, TOPK, None, table, True, idx8, logits))
    return desc, calls


def measure(desc, calls, warmup, iters, rounds):
    for _ in range(warmup):
        for fn in calls.values():
            fn()
    t = {name: [] for name in calls}
    for _ in range(rounds):  # alternating rounds: drift of the clocks hits all of them
        for name, fn in calls.items():
            t[name].append(events(fn, iters if name != "fill" else max(iters // 5, 3)))
    med = lambda x: sorted(x)[len(x) // 2]  # noqa: E731
    us = lambda x: round(x * 1e6, 1)  # noqa: E731
    m = {name: med(x) for name, x in t.items()}
    keys = desc["b"] * desc["s_k"]
    return dict(desc, call8_us=us(m["call8"]), call16_us=us(m["call16"]), call_ratio=round(m["call8"] / m["call16"], 3),
                logits8_us=us(m["logits8"]), logits16_us=us(m["logits16"]), logits_ratio=round(m["logits8"] / m["logits16"], 3),
                key8_GBps=round(keys * (DI + 4) / m["logits8"] / 1e9, 1), key16_GBps=round(keys * DI * 2 / m["logits16"] / 1e9, 1),
                append_us=us(m["append"]), fill_ns_per_row=round(m["fill"] / keys * 1e9, 3),
                us_min_max={name: [us(min(x)), us(max(x))] for name, x in t.items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "index_topk8.jsonl"))
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="batch 8, cache 8192 only")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "index_topk8_bench needs a GPU"
    torch.manual_seed(0)
    grid = [(8, 8192)] if a.quick else [(b, sk) for sk in (8192, 32768, 131072) for b in (1, 8, 64)]
    rows = []
    for b, sk in grid:
        r = measure(*shape(b, sk), a.warmup, a.iters, a.rounds)
        print(json.dumps(r), flush=True)
        rows.append(r)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
