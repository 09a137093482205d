"""Developer aid: what the fused verification of speculative sampling costs beside a torch composition of the same rule.  One
process, bf16 logits of a peaked distribution (a bulk of N(0, 1), 12 columns raised by N(25, 4)); the draft's logits are the
target's + N(0, 1) and its tokens are drawn from its own filtered distribution.  B in {1, 8, 64}, S in {4, 8}, V in {32000,
128256}, (top_k, top_p, temperature) in {(50, 0.9, 0.7), (0, 0.9, 1)}.

Three arms, interleaved round by round in the same process: `ours` is utils.generation.sample_speculative as a user calls it
((seed, offset) drawn on the device by a torch.randint, then the two launches); `ours_u` the same with uniforms given, the two
launches alone; `eager` is the rule written out in torch here: divide, a top-k threshold by topk, a top-p mask by sort, softmax,
cumsum and scatter, two softmaxes, the gathers, the acceptance, the clamped difference at the first rejection and a multinomial,
with the per-row write.  A round times back-to-back calls of one arm between two events, as many as fill --window-ms (from a
probe of 5 calls; `inner` in the output); per arm the median, the fastest and the slowest round are reported, in us per call.
A ratio eager / ours below 1 is a finding.  The output file is written anew.

Usage: python tools/sample_spec_bench.py [--warmup W] [--rounds R] [--window-ms MS] [--out profiles/sample_spec.jsonl]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

DEV = "cuda"
BS, SS, VS = (1, 8, 64), (4, 8), (32000, 128256)
SETTINGS = ((50, 0.9, 0.7), (0, 0.9, 1.0))


def eager_probs(logits, top_k, top_p, temperature):
    """softmax over what top-k (ties stay) and top-p leave of logits / temperature, (..., V) fp32"""
    x = logits.float() / temperature
    if 0 < top_k < x.shape[-1]:
        x = x.masked_fill(x < torch.topk(x, top_k, dim=-1).values[..., -1:], float("-inf"))
    if 0.0 < top_p < 1.0:
        srt, idx = torch.sort(x, dim=-1, descending=False)
        remove = srt.softmax(dim=-1).cumsum(dim=-1) <= (1 - top_p)
        x = x.masked_fill(remove.scatter(-1, idx, remove), float("-inf"))
    return torch.softmax(x, dim=-1)


def eager_speculative(logits, logits_draft, tokens_draft, top_k, top_p, temperature):
    """the rule of include/fa_spec_sample.h as a user would compose it from torch calls; seqlen >= 1"""
    b, s = tokens_draft.shape
    rows = torch.arange(b, device=logits.device)
    p, q = eager_probs(logits, top_k, top_p, temperature), eager_probs(logits_draft, top_k, top_p, temperature)
    at = tokens_draft.unsqueeze(2)
    p_tok, q_tok = torch.take_along_dim(p[:, :s], at, dim=2).squeeze(2), torch.take_along_dim(q, at, dim=2).squeeze(2)
    rejected = torch.rand_like(q_tok) * q_tok > p_tok
    n = (rejected.cumsum(dim=1) == 0).sum(dim=1)  # the length of the accepted prefix: the first rejected position, s if none
    p_n = p[rows, n]
    residual = (p_n - q[rows, n.clamp(max=s - 1)]).relu_()
    from_p = (n == s) | (residual.sum(dim=1) <= 0)
    weights = torch.where(from_p.unsqueeze(1), p_n, residual)
    tokens = torch.cat([tokens_draft, tokens_draft.new_zeros(b, 1)], dim=1)
    tokens[rows, n] = torch.multinomial(weights, num_samples=1).squeeze(1)  # per row
    return tokens, n + 1


def calls_per_round(run, window_ms):
    """how many back-to-back calls of `run` fill a timed window of about `window_ms`, from a probe of 5 calls"""
    return max(5, min(2000, int(window_ms * 1e3 / one_round(run, 5)) + 1))


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
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window-ms", type=float, default=60.0, help="a round times as many calls of an arm as fill this window")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample_spec.jsonl"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "sample_spec_bench needs a GPU"
    from flash_attention_annotated_amd.utils import generation
    torch.manual_seed(0)
    rows = []
    for v in VS:
        for b in BS:
            for s in SS:
                x = torch.randn(b * (s + 1), v, device=DEV)
                cols = torch.stack([torch.randperm(v, device=DEV)[:12] for _ in range(b * (s + 1))])
                x.scatter_add_(1, cols, 25.0 + 4.0 * torch.randn(b * (s + 1), 12, device=DEV))
                x = x.view(b, s + 1, v)
                d = (x[:, :s] + torch.randn(b, s, v, device=DEV)).to(torch.bfloat16)
                x = x.to(torch.bfloat16)
                u = (torch.rand(b, s, device=DEV), torch.rand(b, device=DEV))
                for top_k, top_p, t in SETTINGS:
                    tokens = torch.multinomial(eager_probs(d, top_k, top_p, t).view(b * s, v), num_samples=1).view(b, s)
                    arms = {"ours": lambda: generation.sample_speculative(x, d, tokens, top_k, top_p, t),
                            "ours_u": lambda: generation.sample_speculative(x, d, tokens, top_k, top_p, t, u=u),
                            "eager": lambda: eager_speculative(x, d, tokens, top_k, top_p, t)}
                    for run in arms.values():
                        for _ in range(args.warmup):
                            run()
                    torch.cuda.synchronize()
                    inner = {name: calls_per_round(run, args.window_ms) for name, run in arms.items()}
                    us = {name: [] for name in arms}
                    for _ in range(args.rounds):  # the arms in turn: what drifts, drifts for all
                        for name, run in arms.items():
                            us[name].append(one_round(run, inner[name]))
                    num = generation.sample_speculative(x, d, tokens, top_k, top_p, t, u=u)[1]
                    row = dict(shape=f"B{b} S{s} V{v}", dtype="bf16", top_k=top_k, top_p=top_p, temperature=t, rounds=args.rounds,
                               window_ms=args.window_ms, inner=inner, warmup=args.warmup, mean_generated=round(float(num.float().mean()), 2))
                    for name, ts in us.items():
                        ts = sorted(ts)
                        row.update({f"{name}_us": round(ts[len(ts) // 2], 2), f"{name}_us_min": round(ts[0], 2),
                                    f"{name}_us_max": round(ts[-1], 2)})
                    row["eager_over_ours"] = round(row["eager_us"] / row["ours_us"], 2)
                    rows.append(row)
                    print(json.dumps(row), flush=True)
                del x, d
                torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
