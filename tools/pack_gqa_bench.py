"""Developer aid: what PackGQA (`pack_gqa=True` -> pk_fwd_kernel, csrc/fa_fwd_kernel_pk.h) buys or costs against the unpacked
route of the same call, hq 32 / hkv 8, d 128, bf16, through the FA3 surface.

Per shape both forms are timed in the same process in alternating rounds (device events over warmed calls, median of --iters
per round, median / min / max over --rounds), their plans are recorded, and their outputs are compared (a hint must not change
what is computed: the largest |out_packed - out_unpacked| is reported beside the ratio).  One JSON line per shape, printed and
written to --out (profiles/pack_gqa.jsonl):
  mixed          the continuous-batching step of tools/ragged_decode_bench.py: 4 prefill chunks of 512 beside 60 single-token
                 decodes, b 64, pages of 64 rows, cache 4096, appended raggedly, causal, num_splits 0;
  verify4/8      a speculative-decode verify step: 4 / 8 query tokens per sequence over a paged cache of 8192, b 32, causal,
                 num_splits 0;
  varlen_short   256 sequences of 64 .. 512 tokens (tools/varlen_short_bench.py), causal and not;
  chunk128       chunked prefill: 128 query tokens per sequence over a paged cache of 4096, b 16, causal, num_splits 0;
  c4             BASELINE config 4 (8 sequences of 8192 .. 1024 tokens, non-causal): the control -- every tile is full without
                 packing, so packing should not help.
speedup = unpacked time / packed time (> 1: packing wins).  GPU only.
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
BF = torch.bfloat16


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


def paged_cache(b, cap):
    npg = cap // PAGE
    kc = torch.randn(b * npg, PAGE, HK, D, dtype=BF, device="cuda")
    vc = torch.randn(b * npg, PAGE, HK, D, dtype=BF, device="cuda")
    table = torch.randperm(b * npg, device="cuda", dtype=torch.int32).view(b, npg)
    return kc, vc, table


def cu_of(lens):
    return torch.tensor([sum(lens[:i]) for i in range(len(lens) + 1)], dtype=torch.int32, device="cuda")


def mixed(b=64, sk=4096, chunks=4, chunk=512):
    kc, vc, table = paged_cache(b, sk)
    lens = [chunk] * chunks + [1] * (b - chunks)
    total = sum(lens)
    fills = torch.tensor([sk - n for n in lens], dtype=torch.int32, device="cuda")
    cu = cu_of(lens)
    q = torch.randn(total, H, D, dtype=BF, device="cuda")
    kn, vn = (torch.randn(total, HK, D, dtype=BF, device="cuda") for _ in range(2))
    pairs = sum(n * sk - n * (n - 1) // 2 for n in lens)
    call = lambda hint: fa3.flash_attn_with_kvcache(q, kc, vc, k=kn, v=vn, cache_seqlens=fills, page_table=table, cu_seqlens_q=cu,  # noqa: E731
                                                    cu_seqlens_k_new=cu, max_seqlen_q=chunk, causal=True, num_splits=0, pack_gqa=hint)
    return dict(shape="mixed", b=b, s_k=sk, total_q=total), call, 4 * D * H * pairs


def over_cache(name, b, sq, sk):
    kc, vc, table = paged_cache(b, sk)
    fills = torch.full((b,), sk, dtype=torch.int32, device="cuda")
    q = torch.randn(b, sq, H, D, dtype=BF, device="cuda")
    pairs = b * (sq * sk - sq * (sq - 1) // 2)
    call = lambda hint: fa3.flash_attn_with_kvcache(q, kc, vc, cache_seqlens=fills, page_table=table, causal=True, num_splits=0,  # noqa: E731
                                                    pack_gqa=hint)
    return dict(shape=name, b=b, s_q=sq, s_k=sk), call, 4 * D * H * pairs


def varlen(name, lens, causal):
    cu = cu_of(lens)
    tot = sum(lens)
    q = torch.randn(tot, H, D, dtype=BF, device="cuda")
    k, v = (torch.randn(tot, HK, D, dtype=BF, device="cuda") for _ in range(2))
    flop = sum(4 * H * D * n * n for n in lens) // (2 if causal else 1)
    call = lambda hint: fa3.flash_attn_varlen_func(q, k, v, cu, cu, max(lens), max(lens), causal=causal, pack_gqa=hint)  # noqa: E731
    return dict(shape=name, sequences=len(lens), total_q=tot, causal=causal), call, flop


def measure(desc, call, flop, warmup, iters, rounds):
    out_p = call(True)
    plan_p = last_plan()
    out_u = call(None)
    plan_u = last_plan()
    torch.cuda.synchronize()
    diff = (out_p.float() - out_u.float()).abs().max().item()
    for _ in range(warmup):
        call(True), call(None)
    t_p, t_u = [], []
    for _ in range(rounds):  # alternating rounds: drift of the clocks hits both
        t_p.append(events(lambda: call(True), iters))
        t_u.append(events(lambda: call(None), iters))
    med = lambda x: sorted(x)[len(x) // 2]  # noqa: E731
    us = lambda x: round(x * 1e6, 1)  # noqa: E731
    return dict(desc, packed_us=us(med(t_p)), unpacked_us=us(med(t_u)), speedup=round(med(t_u) / med(t_p), 3),
                packed_us_min_max=[us(min(t_p)), us(max(t_p))], unpacked_us_min_max=[us(min(t_u)), us(max(t_u))],
                packed_TFLOPs=round(flop / med(t_p) / 1e12, 1), unpacked_TFLOPs=round(flop / med(t_u) / 1e12, 1),
                max_abs_diff=diff, packed_plan=plan_p, unpacked_plan=plan_u)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "pack_gqa.jsonl"))
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="the first shape only")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "pack_gqa_bench needs a GPU"
    torch.manual_seed(0)
    short = torch.randint(64, 513, (256,), generator=torch.Generator().manual_seed(0)).tolist()
    c4 = [8192, 7168, 6144, 5120, 4096, 3072, 2048, 1024]
    shapes = [lambda: mixed(), lambda: over_cache("verify4", 32, 4, 8192), lambda: over_cache("verify8", 32, 8, 8192),
              lambda: varlen("varlen_short", short, False), lambda: varlen("varlen_short", short, True),
              lambda: over_cache("chunk128", 16, 128, 4096), lambda: varlen("c4", c4, False)]
    rows = []
    for make in shapes[:1] if a.quick else shapes:
        r = measure(*make(), a.warmup, a.iters, a.rounds)
        print(json.dumps(r), flush=True)
        rows.append(r)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
