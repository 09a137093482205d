"""Developer aid: the verify step of speculative decoding over a token tree -- tr_fwd_kernel, csrc/fa_fwd_kernel_tr.h, through
flash_attn_with_kvcache_tree -- against the closest route of the parent commit on the SAME cache and queries with a chain as the
draft: flash_attn_with_kvcache(causal=True, pack_gqa=True), i.e. pk_fwd_kernel over a bf16 cache and kv8_fwd_kernel over an e4m3
cache, which run the same packed-row body with RangeMask.  hq 32 / hkv 8, d 128, bf16 queries, pages of 64 rows behind a
shuffled table, num_splits = 0 on both sides (the same shape-only heuristic).

Grid: cache 8192 and 32768 (full, the T draft rows included), batch 1 / 8 / 64, T = 16 / 64, a bf16 and an e4m3 cache.  The tree
call is timed twice: with the chain's words (the same attention as the causal call: the two differ only in which of the last
one or two tiles take the element mask and in the causal route's shorter key range for early rows) and with the words of a
random forest.  Per shape the three calls are timed in the same process in alternating rounds (device events over warmed calls,
median of --iters per round, median / min / max over --rounds).  One JSON line per shape, printed and written to --out
(profiles/tree_verify.jsonl):
  causal_us               the chain through the causal PackGQA / kv8 route
  tree_chain_us           the chain through the tree route;  ratio_chain = tree_chain_us / causal_us
  tree_forest_us          a random forest through the tree route;  ratio_forest = tree_forest_us / causal_us
  max_abs_diff_chain      |out_tree - out_causal| of the chain (the same attention)
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

H, HK, D, PAGE = 32, 8, 128, 64
BF, F8 = torch.bfloat16, torch.float8_e4m3fn


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


def shape(b, sk, T, fp8):
    """(description, {name: call})."""
    rows = b * sk
    k = torch.randn(rows // PAGE, PAGE, HK, D, dtype=BF, device="cuda")
    v = torch.randn(rows // PAGE, PAGE, HK, D, dtype=BF, device="cuda")
    kw = dict(cache_seqlens=torch.full((b,), sk, dtype=torch.int32, device="cuda"), num_splits=0,
              page_table=torch.randperm(rows // PAGE, device="cuda", dtype=torch.int32).view(b, sk // PAGE))
    causal_kw = dict(pack_gqa=True)
    if fp8:
        k, v = k.to(F8), v.to(F8)
        kw.update(k_descale=torch.ones(b, HK, device="cuda"), v_descale=torch.ones(b, HK, device="cuda"))
        causal_kw = {}  # (kv8_fwd_kernel packs the group itself)
    q = torch.randn(b, T, H, D, dtype=BF, device="cuda")
    chain = fa3.tree_mask_from_parents((torch.arange(T, device="cuda") - 1).expand(b, T))
    parents = (torch.rand(b, T, device="cuda") * torch.arange(T, device="cuda")).long() - (torch.rand(b, T, device="cuda") < 0.1).long() * T
    forest = fa3.tree_mask_from_parents(parents.clamp(min=-1))  # parents[i] in [-1, i): about one root in ten nodes
    calls = dict(causal=lambda: fa3.flash_attn_with_kvcache(q, k, v, causal=True, **causal_kw, **kw),
                 tree_chain=lambda: fa3.flash_attn_with_kvcache_tree(q, k, v, chain, **kw),
                 tree_forest=lambda: fa3.flash_attn_with_kvcache_tree(q, k, v, forest, **kw))
    return dict(b=b, s_k=sk, T=T, cache="e4m3" if fp8 else "bf16", page=PAGE), calls


def measure(desc, calls, warmup, iters, rounds):
    out_c = calls["causal"]()
    plan_c = last_plan()
    out_t = calls["tree_chain"]()
    plan_t = last_plan()
    torch.cuda.synchronize()
    diff = (out_c.float() - out_t.float()).abs().max().item()
    for _ in range(warmup):
        for fn in calls.values():
            fn()
    t = {name: [] for name in calls}
    for _ in range(rounds):  # alternating rounds: drift of the clocks hits all of them
        for name, fn in calls.items():
            t[name].append(events(fn, iters))
    med = lambda x: sorted(x)[len(x) // 2]  # noqa: E731
    us = lambda x: round(x * 1e6, 1)  # noqa: E731
    res = dict(desc)
    for name in calls:
        res[f"{name}_us"] = us(med(t[name]))
        res[f"{name}_us_min_max"] = [us(min(t[name])), us(max(t[name]))]
    res.update(ratio_chain=round(med(t["tree_chain"]) / med(t["causal"]), 3), ratio_forest=round(med(t["tree_forest"]) / med(t["causal"]), 3),
               max_abs_diff_chain=diff, causal_plan=plan_c, tree_plan=plan_t)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "tree_verify.jsonl"))
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="batch 8, cache 8192 only")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "tree_verify_bench needs a GPU"
    torch.manual_seed(0)
    grid = [(b, sk, T, fp8) for sk in (8192, 32768) for fp8 in (False, True) for b in (1, 8, 64) for T in (16, 64)]
    if a.quick:
        grid = [(8, 8192, T, fp8) for fp8 in (False, True) for T in (16, 64)]
    rows = []
    for b, sk, T, fp8 in grid:
        r = measure(*shape(b, sk, T, fp8), a.warmup, a.iters, a.rounds)
        print(json.dumps(r), flush=True)
        rows.append(r)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
