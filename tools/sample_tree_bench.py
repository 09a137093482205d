"""Developer aid: what the fused acceptance walk over a draft token tree costs beside a torch composition of the same rule, and
beside the chain verification on a chain-shaped tree.  One process, bf16 logits of a peaked distribution (a bulk of N(0, 1), 12
columns raised by N(25, 4)); the draft's logits are the target's + N(0, 1) and the token of a node is drawn from the filtered
draft distribution of its parent's row.  B in {1, 8, 64}, T in {16, 64}, V in {32000, 128256}, (top_k, top_p, temperature) =
(50, 0.9, 0.7), a binary tree, with draft rows (`draft`) and under the one-hot rule (`onehot`); and a chain of T nodes.

Arms, interleaved round by round in the same process: `ours` is utils.generation.sample_speculative_tree with uniforms given,
the two launches alone; `eager` is the rule written out in torch here: the filtered softmaxes of all rows (tools/
sample_spec_bench.py's eager_probs), then a host loop over the nodes in index order that carries (n, rounds, c, R) per sequence
in tensors, and a multinomial; on the chain, `chain` is utils.generation.sample_speculative on the same rows.  A round times
back-to-back calls of one arm between two events, as many as fill --window-ms; per arm the median, the fastest and the slowest
round are reported, in us per call.  A ratio below 1 is a finding.  The output file is written anew.

Usage: python tools/sample_tree_bench.py [--warmup W] [--rounds R] [--window-ms MS] [--out profiles/sample_tree.jsonl]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402
from sample_spec_bench import calls_per_round, eager_probs, one_round  # noqa: E402

DEV = "cuda"
BS, TS, VS = (1, 8, 64), (16, 64), (32000, 128256)
SETTING = (50, 0.9, 0.7)


def eager_tree(logits, logits_draft, tokens_draft, parents, top_k, top_p, temperature):
    """the rule of include/fa_tree_sample.h as a user would compose it from torch calls: -> (tokens, path, path_len)"""
    b, t, v = logits.shape
    dev = logits.device
    rows = torch.arange(b, device=dev)
    P = eager_probs(logits, top_k, top_p, temperature)
    Q = eager_probs(logits_draft, top_k, top_p, temperature) if logits_draft is not None else None
    u = torch.rand(b, t, device=dev)
    n, m = torch.zeros(b, dtype=torch.int64, device=dev), torch.zeros(b, dtype=torch.int64, device=dev)
    c = torch.zeros(b, device=dev)
    R = torch.zeros(b, device=dev) if Q is not None else P[:, 0].sum(dim=1)
    done = torch.zeros(b, dtype=torch.bool, device=dev)
    gone = torch.zeros(b, v, dtype=torch.bool, device=dev)
    path = torch.zeros(b, t, dtype=torch.int64, device=dev)
    length = torch.ones(b, dtype=torch.int64, device=dev)
    for i in range(1, t):
        run = (parents[:, i] == n) & ~done
        x = tokens_draft[:, i]
        p0 = P[rows, n, x]
        if Q is not None:
            q0 = Q[rows, n, x]
            first = m == 0
            ok = torch.where(first, u[:, i] * q0 <= p0, u[:, i] * q0 * R <= (p0 - c * q0).relu())
            c_next = torch.where(first, torch.ones_like(c), c + R)
            R_next = (P[rows, n] - c_next[:, None] * Q[rows, n]).relu_().sum(dim=1)
        else:
            w = torch.where(gone[rows, x], torch.zeros_like(p0), p0)
            ok = (w > 0) & (u[:, i] * R <= w)
            c_next, R_next = c, R - w
            gone[rows, x] |= run & ~ok
        yes, no = run & ok, run & ~ok
        c, R, m = torch.where(no, c_next, c), torch.where(no, R_next, R), torch.where(no, m + 1, m)
        done |= no & (R <= 0)
        path[rows, length] = torch.where(yes, i, path[rows, length])
        length = length + yes
        n = torch.where(yes, i, n)
        m, c = m.masked_fill(yes, 0), c.masked_fill(yes, 0.0)
        if Q is not None:
            R = R.masked_fill(yes, 0.0)
        else:
            R = torch.where(yes, P[:, i].sum(dim=1), R)
            gone &= ~yes[:, None]
    Pn = P[rows, n]
    if Q is not None:
        residual = (Pn - c[:, None] * Q[rows, n]).relu_()
        weights = torch.where(((m == 0) | (residual.sum(dim=1) <= 0))[:, None], Pn, residual)
    else:
        weights = Pn.masked_fill(gone, 0.0)
        weights = torch.where((weights.sum(dim=1) > 0)[:, None], weights, torch.ones_like(weights))
    token = torch.multinomial(weights, num_samples=1).squeeze(1)
    tokens = tokens_draft.gather(1, torch.cat([path[:, 1:], path[:, :1]], dim=1))
    tokens[rows, length - 1] = token
    return tokens, path, length


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window-ms", type=float, default=60.0, help="a round times as many calls of an arm as fill this window")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample_tree.jsonl"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "sample_tree_bench needs a GPU"
    from flash_attention_annotated_amd.utils import generation
    torch.manual_seed(0)
    top_k, top_p, t = SETTING
    rows = []
    for v in VS:
        for b in BS:
            for nodes in TS:
                x = torch.randn(b * nodes, v, device=DEV)
                cols = torch.stack([torch.randperm(v, device=DEV)[:12] for _ in range(b * nodes)])
                x.scatter_add_(1, cols, 25.0 + 4.0 * torch.randn(b * nodes, 12, device=DEV))
                x = x.view(b, nodes, v)
                d = (x + torch.randn(b, nodes, v, device=DEV)).to(torch.bfloat16)
                x = x.to(torch.bfloat16)
                u = (torch.rand(b, nodes, device=DEV), torch.rand(b, device=DEV))
                i = torch.arange(nodes, device=DEV)
                for shape, par in (("binary", (i - 1) // 2), ("chain", i - 1)):
                    parents = torch.where(i > 0, par, -1).int().expand(b, nodes).contiguous()
                    q = eager_probs(d, top_k, top_p, t)[torch.arange(b, device=DEV)[:, None], parents.long().clamp_min(0)]
                    tokens = torch.multinomial(q.view(b * nodes, v), num_samples=1).view(b, nodes)
                    del q
                    for mode in ("draft", "onehot") if shape == "binary" else ("draft",):
                        dr = d if mode == "draft" else None
                        arms = {"ours": lambda: generation.sample_speculative_tree(x, dr, tokens, parents, top_k, top_p, t, u=u)}
                        if shape == "chain":
                            arms["chain"] = lambda: generation.sample_speculative(x, d[:, :-1], tokens[:, 1:], top_k, top_p, t,
                                                                                  u=(u[0][:, 1:].contiguous(), u[1]))
                        else:
                            arms["eager"] = lambda: eager_tree(x, dr, tokens, parents.long(), top_k, top_p, t)
                        for run in arms.values():
                            for _ in range(args.warmup):
                                run()
                        torch.cuda.synchronize()
                        inner = {name: calls_per_round(run, args.window_ms) for name, run in arms.items()}
                        us = {name: [] for name in arms}
                        for _ in range(args.rounds):  # the arms in turn: what drifts, drifts for all
                            for name, run in arms.items():
                                us[name].append(one_round(run, inner[name]))
                        out = generation.sample_speculative_tree(x, dr, tokens, parents, top_k, top_p, t, u=u, stats=True)
                        row = dict(shape=f"B{b} T{nodes} V{v}", tree=shape, mode=mode, dtype="bf16", top_k=top_k, top_p=top_p, temperature=t,
                                   rounds=args.rounds, window_ms=args.window_ms, inner=inner, warmup=args.warmup,
                                   mean_generated=round(float(out[1].float().mean()), 2),
                                   mean_rejections=round(float((out[6] - out[7]).sum(dim=1).float().mean()), 2))
                        for name, ts in us.items():
                            ts = sorted(ts)
                            row.update({f"{name}_us": round(ts[len(ts) // 2], 2), f"{name}_us_min": round(ts[0], 2),
                                        f"{name}_us_max": round(ts[-1], 2)})
                        other = "chain" if shape == "chain" else "eager"
                        row[f"{other}_over_ours"] = round(row[f"{other}_us"] / row["ours_us"], 2)
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
