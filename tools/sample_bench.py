"""Developer aid: what the fused token sampling costs beside the torch composition it replaces.  One process, bf16 logits of a
peaked distribution (a bulk of N(0, 1), 12 columns raised by N(25, 4)), (B, V) in {(1, 32000), (16, 128256), (64, 128256),
(256, 152064)} and (top_k, top_p) in {(50, 0.9), (0, 0.9), (0, 0)} at temperature 0.8.

Three arms, interleaved round by round in the same process: `ours` is utils.generation.sample as a user calls it ((seed, offset)
drawn on the device by a torch.randint, then one launch); `ours_u` the same with uniforms given, the one launch alone; `eager` is
the reference's algorithm written out in torch here (topk -> divide -> sort, softmax, cumsum, scatter, masked_fill -> softmax
-> multinomial).  A round times --inner back-to-back calls of one arm between two events; per arm the median, the fastest
and the slowest round are reported, in us per call.  A ratio eager / ours below 1 is a finding.

Usage: python tools/sample_bench.py [--warmup W] [--rounds R] [--inner I] [--out profiles/sample.jsonl]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

DEV = "cuda"
SHAPES = ((1, 32000), (16, 128256), (64, 128256), (256, 152064))
SETTINGS = ((50, 0.9), (0, 0.9), (0, 0.0))
TEMPERATURE = 0.8


def eager_top_p_(logits, top_p):
    if top_p <= 0.0 or top_p >= 1.0:
        return
    srt, idx = torch.sort(logits, descending=False)
    remove = srt.softmax(dim=-1).cumsum(dim=-1) <= (1 - top_p)
    logits.masked_fill_(remove.scatter(1, idx, remove), float("-inf"))


def eager_sample(logits, top_k, top_p, temperature):
    if top_k > 0:
        top, idx = torch.topk(logits, min(top_k, logits.size(-1)), dim=-1)
        top = top / temperature
        eager_top_p_(top, top_p)
        pick = torch.multinomial(torch.softmax(top, dim=-1), num_samples=1).squeeze(dim=-1)
        return idx[torch.arange(idx.shape[0], device=idx.device), pick]
    top = logits / temperature
    eager_top_p_(top, top_p)
    return torch.multinomial(torch.softmax(top, dim=-1), num_samples=1).squeeze(dim=-1)


def one_round(run, inner):
    a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        run()
    e.record()
    torch.cuda.synchronize()
    return a.elapsed_time(e) * 1e3 / inner


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample.jsonl"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "sample_bench needs a GPU"
    from flash_attention_annotated_amd.utils import generation
    torch.manual_seed(0)
    rows = []
    for b, v in SHAPES:
        x = torch.randn(b, v, device=DEV)
        cols = torch.stack([torch.randperm(v, device=DEV)[:12] for _ in range(b)])
        x.scatter_add_(1, cols, 25.0 + 4.0 * torch.randn(b, 12, device=DEV))
        x = x.to(torch.bfloat16)
        u = torch.rand(b, device=DEV)
        for top_k, top_p in SETTINGS:
            arms = {"ours": lambda: generation.sample(x, top_k, top_p, TEMPERATURE),
                    "ours_u": lambda: generation.sample(x, top_k, top_p, TEMPERATURE, u=u),
                    "eager": lambda: eager_sample(x, top_k, top_p, TEMPERATURE)}
            for run in arms.values():
                for _ in range(args.warmup):
                    run()
            torch.cuda.synchronize()
            us = {name: [] for name in arms}
            for _ in range(args.rounds):  # the arms in turn: what drifts, drifts for all
                for name, run in arms.items():
                    us[name].append(one_round(run, args.inner))
            row = dict(shape=f"B{b} V{v}", dtype="bf16", top_k=top_k, top_p=top_p, temperature=TEMPERATURE, rounds=args.rounds,
                       inner=args.inner, warmup=args.warmup)
            for name, t in us.items():
                t = sorted(t)
                row.update({f"{name}_us": round(t[len(t) // 2], 2), f"{name}_us_min": round(t[0], 2), f"{name}_us_max": round(t[-1], 2)})
            row["eager_over_ours"] = round(row["eager_us"] / row["ours_us"], 2)
            rows.append(row)
            print(json.dumps(row), flush=True)
        del x
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
