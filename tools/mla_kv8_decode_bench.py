"""Developer aid: an MLA decode step (absorbed attention, qv) over an fp8 (e4m3) KV cache -- qv8_fwd_kernel,
csrc/fa_fwd_kernel_qv8.h -- against the 16-bit qv route (fwd_kernel_qv) on the SAME values (the cache expanded to bf16), h_k 1,
d 64 / d_v 512, bf16 queries, through the FA3 surface (flash_attn_with_kvcache, num_splits = 0: the qv kernel's split heuristic
on both routes).

Shapes: h 16 and h 128, cache 8192 (full), batch 1 / 32 / 128, seqlen_q 1 / 2, a dense cache and pages of 64 rows behind a
shuffled table.  Per shape both routes are timed in the same process in alternating rounds (device events over warmed calls,
median of --iters per round, median / min / max over --rounds); their plans are recorded and their outputs compared (same values
in: the largest |out_fp8 - out_16bit| is reported).  One JSON line per shape, printed and written to --out
(profiles/mla_kv8_decode.jsonl):
  kv8_us / bf16_us        time of a step; ratio = kv8_us / bf16_us (< 1: the fp8 cache wins; the cache bytes halve, q / qv / out /
                          the merge launch do not)
  kv8_TBps / bf16_TBps    K and V bytes of the step per second (576 bytes per key against 1152)
h 128 is bound by issue, not by HBM: no gain is expected there.  GPU only.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from flash_attention_annotated_amd import _lib  # noqa: E402
from flash_attention_annotated_amd import hopper_interface as fa3  # noqa: E402

HK, D, DV, PAGE = 1, 64, 512, 64
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


def shape(h, b, sq, sk, paged):
    """(description, fp8 call, 16-bit call, K + V elements read by a step)."""
    rows = b * sk
    k8 = torch.randn(rows, HK, D, device="cuda").to(F8)
    v8 = torch.randn(rows, HK, DV, device="cuda").to(F8)
    k16, v16 = k8.to(BF), v8.to(BF)  # the same values
    q = torch.randn(b, sq, h, D, dtype=BF, device="cuda")
    qv = torch.randn(b, sq, h, DV, dtype=BF, device="cuda")
    fills = torch.full((b,), sk, dtype=torch.int32, device="cuda")
    kw = dict(qv=qv, cache_seqlens=fills, num_splits=0, causal=True)
    if paged:
        view = lambda x: x.view(rows // PAGE, PAGE, HK, x.shape[-1])  # noqa: E731
        kw["page_table"] = torch.randperm(rows // PAGE, device="cuda", dtype=torch.int32).view(b, sk // PAGE)
    else:
        view = lambda x: x.view(b, sk, HK, x.shape[-1])  # noqa: E731
    k8, v8, k16, v16 = view(k8), view(v8), view(k16), view(v16)
    call8 = lambda: fa3.flash_attn_with_kvcache(q, k8, v8, **kw)  # noqa: E731
    call16 = lambda: fa3.flash_attn_with_kvcache(q, k16, v16, **kw)  # noqa: E731
    return dict(h=h, b=b, s_q=sq, s_k=sk, cache="page64" if paged else "dense"), call8, call16, rows * HK * (D + DV)


def measure(desc, call8, call16, elems, warmup, iters, rounds):
    out8 = call8()
    plan8 = last_plan()
    out16 = call16()
    plan16 = last_plan()
    torch.cuda.synchronize()
    diff = (out8.float() - out16.float()).abs().max().item()
    for _ in range(warmup):
        call8(), call16()
    t8, t16 = [], []
    for _ in range(rounds):  # alternating rounds: drift of the clocks hits both
        t8.append(events(call8, iters))
        t16.append(events(call16, iters))
    med = lambda x: sorted(x)[len(x) // 2]  # noqa: E731
    us = lambda x: round(x * 1e6, 1)  # noqa: E731
    return dict(desc, kv8_us=us(med(t8)), bf16_us=us(med(t16)), ratio=round(med(t8) / med(t16), 3),
                kv8_us_min_max=[us(min(t8)), us(max(t8))], bf16_us_min_max=[us(min(t16)), us(max(t16))],
                kv8_TBps=round(elems / med(t8) / 1e12, 2), bf16_TBps=round(2 * elems / med(t16) / 1e12, 2),
                max_abs_diff=diff, kv8_plan=plan8, bf16_plan=plan16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "mla_kv8_decode.jsonl"))
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="h 16 / h 128, batch 128, seqlen_q 1, dense and paged only")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "mla_kv8_decode_bench needs a GPU"
    torch.manual_seed(0)
    grid = [(h, b, sq, 8192, paged) for h in (16, 128) for paged in (False, True) for sq in (1, 2) for b in (1, 32, 128)]
    if a.quick:
        grid = [(h, 128, 1, 8192, paged) for h in (16, 128) for paged in (False, True)]
    rows = []
    for g in grid:
        r = measure(*shape(*g), a.warmup, a.iters, a.rounds)
        print(json.dumps(r), flush=True)
        rows.append(r)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
