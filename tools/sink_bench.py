"""Developer aid: what a learnable sink costs the forward.  One process, the same call with and without `learnable_sink`,
interleaved rounds (the manner of tools/ab_interleaved.py: both sides see the same clocks and caches), medians of event
timings.  Cases: C2 (b4 h16 d128 s8192), C3 (causal, s16384), a gpt-oss-like decode step (hq64 / hkv8, d64, paged cache with
fill levels 4096..8192, batch 1 and 64, window 128 and none) and one split-KV case.  Appends one JSON line per case to
profiles/sink.jsonl.
Usage: python tools/sink_bench.py [--rounds R] [--iters N] [--out profiles/sink.jsonl]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

DEV = "cuda"


def dense(b, s, h, d, causal, num_splits=1, hk=None, sq=None):
    from flash_attention_annotated_amd import cute_interface as cute
    q = torch.randn(b, sq or s, h, d, device=DEV, dtype=torch.bfloat16)
    k, v = (torch.randn(b, s, hk or h, d, device=DEV, dtype=torch.bfloat16) for _ in range(2))
    return lambda sink: cute.flash_attn_func(q, k, v, causal=causal, learnable_sink=sink, num_splits=num_splits), h


def decode(b, window, hq=64, hkv=8, d=64, page=256, cap=8192, num_splits=0):
    from flash_attention_annotated_amd import cute_interface as cute
    per = cap // page
    q = torch.randn(b, 1, hq, d, device=DEV, dtype=torch.bfloat16)
    kp, vp = (torch.randn(b * per, page, hkv, d, device=DEV, dtype=torch.bfloat16) for _ in range(2))
    table = torch.randperm(b * per, device=DEV).to(torch.int32).view(b, per)
    used = torch.linspace(4096, cap, b, device=DEV).to(torch.int32)
    return lambda sink: cute.flash_attn_varlen_func(q, kp, vp, seqused_k=used, page_table=table, window_size=window,
                                                    learnable_sink=sink, num_splits=num_splits), hq


CASES = {
    "c2": lambda: dense(4, 8192, 16, 128, False),
    "c3_causal": lambda: dense(4, 16384, 16, 128, True),
    "decode_b1": lambda: decode(1, (None, None)),
    "decode_b64": lambda: decode(64, (None, None)),
    "decode_b1_window128": lambda: decode(1, (128, 0)),
    "decode_b64_window128": lambda: decode(64, (128, 0)),
    "split4_sq300_sk8192": lambda: dense(2, 8192, 8, 128, True, num_splits=4, hk=2, sq=300),
}


def timed(run, sink, iters):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, e in ev:
        a.record(); run(sink); e.record()
    torch.cuda.synchronize()
    return sorted(a.elapsed_time(e) for a, e in ev)[iters // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sink.jsonl"))
    ap.add_argument("--cases", default=",".join(CASES))
    args = ap.parse_args()
    from parity_helpers import last_plan
    torch.manual_seed(0)
    with open(args.out, "a") as f:
        for name in args.cases.split(","):
            run, h = CASES[name]()
            sink = torch.linspace(-4, 4, h, device=DEV).to(torch.bfloat16)
            for s in (None, sink) * 3:  # warm up both sides
                run(s)
            plan = last_plan()
            without, with_ = [], []
            for _ in range(args.rounds):
                without.append(timed(run, None, args.iters))
                with_.append(timed(run, sink, args.iters))
            a, b = sorted(without)[args.rounds // 2], sorted(with_)[args.rounds // 2]
            rec = dict(case=name, plan=plan, ms_without=round(a, 5), ms_with=round(b, 5), ratio=round(b / a, 4),
                       rounds=args.rounds, iters=args.iters, device=torch.cuda.get_device_name(0))
            print(json.dumps(rec), flush=True)
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
