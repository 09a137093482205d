"""Developer aid: what producing the lists of a token-sparse decode step costs -- kvcache_index_topk (csrc/fa_index_topk.hip) --
against the same rule composed of torch calls, and whether the whole sparse step (indexer + flash_attn_with_kvcache_topk) beats
the dense flash_attn_with_kvcache(qv=) on the SAME cache.  Shapes: index heads 64, index dim 128, bf16, pages of 64 rows behind a
shuffled table, one token per batch entry, batch 1 / 8 / 64, cache 8192 / 32768 / 131072 (full), topk 2048; the attention is the
MLA shape of tools/topk_kv_decode_bench.py (h 16, h_k 1, d 64, d_v 512) on the same page table.

Per shape, in one process, in alternating rounds (device events over warmed calls, median of --iters per round, median / min /
max over --rounds):
  call_us       kvcache_index_topk, both launches
  logits_us     the call with topk = capacity: its selection launch only writes 0 .. n - 1, so this is the logits launch (+ a
                near-empty launch); select_us = call_us - logits_us is the selection launch by difference
  key_GBps      the key bytes (b * sk * 128 * 2) over logits_us
  torch_us      einsum, relu, weighted sum, topk, sort on the GPU; torch_over_call = torch_us / call_us
  step_us       indexer + flash_attn_with_kvcache_topk on its list; dense_us the dense call; step_ratio = step_us / dense_us
One JSON line per shape, printed and written to --out (profiles/index_topk.jsonl).  GPU only.
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
H, D, DV = 16, 64, 512
BF = torch.bfloat16


def events(fn, iters):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, e in ev:
        a.record()
        fn()
        e.record()
    torch.cuda.synchronize()
    return sorted(a.elapsed_time(e) for a, e in ev)[iters // 2] * 1e-3


def torch_index_topk(q_i, keys, w, topk):
    """The rule of kvcache_index_topk on a full cache as a torch composition (keys: the logical rows (b, sk, d_i))."""
    logits = (torch.einsum("bhc,bsc->bhs", q_i[:, 0], keys).float().relu_() * w[:, 0, :, None]).sum(1)
    return logits.topk(topk, -1).indices.sort(-1).values.to(torch.int32)


def shape(b, sk):
    pages = b * sk // PAGE
    k_i = torch.randn(pages, PAGE, DI, dtype=BF, device="cuda")
    cache = torch.randn(pages, PAGE, 1, D + DV, dtype=BF, device="cuda")
    table = torch.randperm(pages, device="cuda", dtype=torch.int32).view(b, sk // PAGE)
    fills = torch.full((b,), sk, dtype=torch.int32, device="cuda")
    q_i = torch.randn(b, 1, HI, DI, dtype=BF, device="cuda")
    w = torch.randn(b, 1, HI, device="cuda") * HI ** -0.5
    q, qv = torch.randn(b, 1, H, D, dtype=BF, device="cuda"), torch.randn(b, 1, H, DV, dtype=BF, device="cuda")
    idx = torch.empty(b, 1, 1, TOPK, dtype=torch.int32, device="cuda")
    every = torch.empty(b, 1, 1, sk, dtype=torch.int32, device="cuda")
    logits = torch.empty(b, 1, sk, dtype=torch.float32, device="cuda")
    keys = k_i[table.long()].view(b, sk, DI)  # the logical rows, for the composition only
    kw = dict(cache_seqlens=fills, page_table=table)
    call = lambda: fa3.kvcache_index_topk(q_i, k_i, w, fills, TOPK, page_table=table, indices=idx, logits=logits)  # noqa: E731

    def step():
        call()
        return fa3.flash_attn_with_kvcache_topk(q, cache[..., :D], cache[..., D:], idx, qv=qv, num_splits=0, **kw)

    calls = {"call": call,
             "logits": lambda: fa3.kvcache_index_topk(q_i, k_i, w, fills, sk, page_table=table, indices=every, logits=logits),
             "torch": lambda: torch_index_topk(q_i, keys, w, TOPK), "step": step,
             "dense": lambda: fa3.flash_attn_with_kvcache(q, cache[..., :D], cache[..., D:], qv=qv, num_splits=0, **kw)}
    # the composition and the kernels choose the same positions where fp32 sums in two orders rank alike: report the agreement
    agree = (calls["torch"]()[:, None, None] == call()).float().mean().item()
    desc = dict(b=b, s_k=sk, h_i=HI, d_i=DI, page=PAGE, topk=TOPK, torch_agreement=round(agree, 4),
                plan=_lib.binding().kvcache_index_topk_plan(q_i, k_i, w, fills, TOPK, None, table, True, idx, logits))
    return desc, calls


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
    key_bytes = desc["b"] * desc["s_k"] * DI * 2
    return dict(desc, call_us=us(m["call"]), logits_us=us(m["logits"]), select_us=us(m["call"] - m["logits"]),
                key_GBps=round(key_bytes / m["logits"] / 1e9, 1), torch_us=us(m["torch"]),
                torch_over_call=round(m["torch"] / m["call"], 2), step_us=us(m["step"]), dense_us=us(m["dense"]),
                step_ratio=round(m["step"] / m["dense"], 3), us_min_max={name: [us(min(x)), us(max(x))] for name, x in t.items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "index_topk.jsonl"))
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="batch 8, cache 8192 only")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "index_topk_bench needs a GPU"
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
