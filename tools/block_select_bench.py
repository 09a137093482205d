"""Developer aid: what producing the lists of a block-sparse decode step costs -- kvcache_block_summary_update and
kvcache_select_blocks (csrc/fa_block_select.hip) -- and whether the whole sparse step (update, selection, sparse attention) still
beats the non-sparse flash_attn_with_kvcache on the SAME cache.  The shapes of tools/sparse_kv_decode_bench.py: hq 32 / hkv 8,
d 128, bf16 queries, pages of 64 rows behind a shuffled table, B = 128, cache 8192 / 32768 (full), batch 1 / 8 / 64, a bf16 and
an e4m3 cache.

Per shape, in one process, in alternating rounds (device events over warmed calls, median of --iters per round, median / min /
max over --rounds):
  parent_us        flash_attn_with_kvcache on the cache (num_splits = 0)
  update_us        the summary update for one new row per sequence (max_seqlen_new = 1)
  select_us[f]     the selection of num_blocks = n * f blocks, f = 1/8 and 1/4 (sink 1, local 1, "max")
  step_us[f]       update + selection + flash_attn_with_kvcache_sparse on the selection's own lists
  step_ratio[f]    step_us[f] / parent_us: below 1 the sparse step wins
  torch_select_us  the same rule at f = 1/8 composed of torch calls on the GPU (products, maximum, sum, amax, topk, sort, count)
  summary_GBps     the summary bytes the scoring streams, over select_us["0.125"]
One JSON line per (shape, cache type), printed and written to --out (profiles/block_select.jsonl).  GPU only.
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
FRACTIONS = (0.125, 0.25)


def events(fn, iters):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, e in ev:
        a.record()
        fn()
        e.record()
    torch.cuda.synchronize()
    return sorted(a.elapsed_time(e) for a, e in ev)[iters // 2] * 1e-3


def torch_select(q, summary, fills, num_blocks, sink=1, local=1):
    """The rule of kvcache_select_blocks ("max") as a torch composition; returns (cnt, idx ascending, -1 behind the count)."""
    b, nb = q.shape[0], summary.shape[1]
    rows = q.view(b, HK, H // HK, 1, D).float()
    lo, hi = (summary[:, :, side].permute(0, 2, 1, 3)[:, :, None].float() for side in (0, 1))  # (b, HK, 1, nb, D)
    u = torch.maximum(rows * lo, rows * hi).sum(-1).amax(2)  # (b, HK, nb)
    n = ((fills + BLOCK - 1) // BLOCK)[:, None, None]
    j = torch.arange(nb, device=q.device)[None, None]
    u = torch.where((j < sink) | (j >= n - local), float("inf"), u)
    u = torch.where(j < n, u, float("-inf"))
    cnt = torch.clamp(n[:, :, 0], max=num_blocks).expand(b, HK).to(torch.int32)
    idx = u.topk(num_blocks, -1).indices
    idx = torch.where(torch.arange(num_blocks, device=q.device) < cnt[..., None], idx, nb).sort(-1).values
    return cnt, torch.where(idx < nb, idx, -1).to(torch.int32)


def shape(b, sk, fp8):
    rows = b * sk
    k = torch.randn(rows // PAGE, PAGE, HK, D, dtype=BF, device="cuda")
    v = torch.randn(rows // PAGE, PAGE, HK, D, dtype=BF, device="cuda")
    table = torch.randperm(rows // PAGE, device="cuda", dtype=torch.int32).view(b, sk // PAGE)
    fills = torch.full((b,), sk, dtype=torch.int32, device="cuda")
    kw = dict(cache_seqlens=fills, page_table=table)
    if fp8:
        k, v = k.to(F8), v.to(F8)
        kw.update(k_descale=torch.ones(b, HK, device="cuda"), v_descale=torch.ones(b, HK, device="cuda"))
    q = torch.randn(b, 1, H, D, dtype=BF, device="cuda")
    nb = sk // BLOCK
    summary = torch.zeros(b, nb, 2, HK, D, dtype=BF, device="cuda")
    fa3.kvcache_block_summary_update(summary, k, None, fills, kv_block_size=BLOCK, page_table=table)
    old = fills - 1
    update = lambda: fa3.kvcache_block_summary_update(summary, k, old, fills, kv_block_size=BLOCK, max_seqlen_new=1, page_table=table)  # noqa: E731
    calls = {"parent": lambda: fa3.flash_attn_with_kvcache(q, k, v, num_splits=0, **kw), "update": update}
    for f in FRACTIONS:
        n = max(2, int(nb * f))
        cnt = torch.zeros(b, HK, dtype=torch.int32, device="cuda")
        idx = torch.zeros(b, HK, n, dtype=torch.int32, device="cuda")
        select = lambda n=n, cnt=cnt, idx=idx: fa3.kvcache_select_blocks(q, summary, fills, n, kv_block_size=BLOCK, kv_block_cnt=cnt,  # noqa: E731
                                                                         kv_block_idx=idx)

        def step(select=select, cnt=cnt, idx=idx):
            update()
            select()
            return fa3.flash_attn_with_kvcache_sparse(q, k, v, cnt, idx, kv_block_size=BLOCK, num_splits=0, **kw)

        calls[f"select_{f}"], calls[f"step_{f}"] = select, step
    n8 = max(2, int(nb * FRACTIONS[0]))
    calls["torch_select"] = lambda: torch_select(q, summary, fills, n8)
    # the composition and the kernels choose the same blocks where fp32 sums in two orders rank alike: report the agreement
    cnt_t, idx_t = calls["torch_select"]()
    cnt_k, idx_k = calls[f"select_{FRACTIONS[0]}"]()
    agree = (idx_t == idx_k).float().mean().item()
    desc = dict(b=b, s_k=sk, cache="e4m3" if fp8 else "bf16", page=PAGE, block=BLOCK, blocks=nb,
                select_plan=_lib.binding().kvcache_select_blocks_plan(q, summary, fills, n8, BLOCK, 1, 1, "max", None, cnt_k, idx_k,
                                                                      torch.empty(b, HK, nb, device="cuda")),
                torch_agreement=round(agree, 4), counts_equal=bool(torch.equal(cnt_t, cnt_k)))
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
    summary_bytes = desc["b"] * desc["blocks"] * 2 * HK * D * 2
    return dict(desc, parent_us=us(m["parent"]), update_us=us(m["update"]),
                select_us={str(f): us(m[f"select_{f}"]) for f in FRACTIONS},
                step_us={str(f): us(m[f"step_{f}"]) for f in FRACTIONS},
                step_ratio={str(f): round(m[f"step_{f}"] / m["parent"], 3) for f in FRACTIONS},
                torch_select_us=us(m["torch_select"]), torch_over_select=round(m["torch_select"] / m[f"select_{FRACTIONS[0]}"], 2),
                summary_GBps=round(summary_bytes / m[f"select_{FRACTIONS[0]}"] / 1e9, 1),
                us_min_max={name: [us(min(x)), us(max(x))] for name, x in t.items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "block_select.jsonl"))
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="batch 8, cache 8192 only")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "block_select_bench needs a GPU"
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
