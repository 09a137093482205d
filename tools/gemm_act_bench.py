"""Developer aid: what the GEMM with a fused bias + activation epilogue (csrc/fa_gemm_act.hip) costs against the sequence it
replaces.  One process, bf16, random operands (x ~ N(0, 1), W ~ N(0, 1) / sqrt(K)), squared ReLU, the fc1 of an MLP:
M in {4096, 16384} x (in, hidden) in {(2048, 8192), (4096, 16384)}.  The arms of a group alternate within every round
(interleaved A/B); a round times --inner back-to-back calls of an arm between two hip events; per arm the median over --rounds
(>= 10) rounds, with the fastest and the slowest round beside it.

    forward    ours    triton_linear_act(x, W1, b1, "squared_relu", save_act_input=True)
               parent  torch.mm(x, W1.T) + _act_fwd(pre, bias)             (what FusedMLPFunc.forward runs)
               mm      torch.mm(x, W1.T) alone                              (where the GEMM itself stands against hipBLASLt)
    dgrad      ours    gemm_act_dgrad(g, W2, "squared_relu", act_input, want_dbias=True)
               parent  torch.mm(g, W2) + _act_bwd(..., want_dbias=True)     (what FusedMLPFunc.backward runs)
               mm      torch.mm(g, W2) alone
    layer      ours    FusedDenseSqreluDense forward + backward
               parent  FusedMLP(activation="sqrelu") forward + backward

TFLOP/s are 2 M N K of the one GEMM (forward, dgrad) and 6 x that for the layer's six GEMMs of the same size.  A ratio
parent / ours above 1 means the fused call is faster.

Usage: python tools/gemm_act_bench.py [--rounds R] [--inner I] [--out profiles/gemm_act.jsonl] [--shapes small]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

DEV = "cuda"
SHAPES = tuple((m, i, h) for m in (4096, 16384) for i, h in ((2048, 8192), (4096, 16384)))


def rounds_of(arms, rounds, inner, warmup=2):
    """{arm: sorted ms per call, one figure per round}; the arms alternate within a round"""
    for run in arms.values():
        for _ in range(warmup):
            run()
    torch.cuda.synchronize()
    ms = {name: [] for name in arms}
    for _ in range(rounds):
        for name, run in arms.items():
            a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner):
                run()
            e.record()
            torch.cuda.synchronize()
            ms[name].append(a.elapsed_time(e) / inner)
    return {name: sorted(v) for name, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--shapes", default="all", choices=("all", "small"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gemm_act.jsonl"))
    args = ap.parse_args()
    assert args.rounds >= 10
    assert torch.cuda.is_available(), "gemm_act_bench needs a GPU"
    from flash_attention_annotated_amd.ops import activations as A
    from flash_attention_annotated_amd.ops.fused_dense import FusedMLP
    from flash_attention_annotated_amd.ops.triton import linear as L
    from flash_attention_annotated_amd.ops.triton.mlp import FusedDenseSqreluDense
    torch.manual_seed(0)
    rows = []

    def record(group, shape, flops, arms):
        ms = rounds_of(arms, args.rounds, args.inner)
        med = {name: v[len(v) // 2] for name, v in ms.items()}
        row = dict(group=group, shape=shape, dtype="bf16", rounds=args.rounds, inner=args.inner)
        for name, v in ms.items():
            row[f"{name}_ms"] = round(med[name], 4)
            row[f"{name}_ms_min"], row[f"{name}_ms_max"] = round(v[0], 4), round(v[-1], 4)
            row[f"{name}_tflops"] = round(flops / med[name] / 1e9, 1)
        row["parent_over_ours"] = round(med["parent"] / med["ours"], 3)
        if "mm" in med:
            row["mm_over_ours"] = round(med["mm"] / med["ours"], 3)
        row["fused_beats_parent"] = bool(med["ours"] < med["parent"])
        rows.append(row)
        print(json.dumps(row), flush=True)

    for m, d_in, hidden in (SHAPES[:1] if args.shapes == "small" else SHAPES):
        shape = f"M{m} in{d_in} hidden{hidden}"
        flops = 2 * m * d_in * hidden
        x = torch.randn(m, d_in, device=DEV).to(torch.bfloat16)
        w1 = (torch.randn(hidden, d_in, device=DEV) / d_in ** 0.5).to(torch.bfloat16)
        b1 = torch.randn(hidden, device=DEV).to(torch.bfloat16)
        w1t = w1.t()
        record("forward", shape, flops, {
            "ours": lambda: L.triton_linear_act(x, w1, b1, "squared_relu", True),
            "parent": lambda: A._act_fwd(torch.mm(x, w1t), None, b1, A.SQRELU),
            "mm": lambda: torch.mm(x, w1t)})
        # dgrad: grad of the fc2 output (M, in) against W2 (in, hidden), act_input (M, hidden)
        g = torch.randn(m, d_in, device=DEV).to(torch.bfloat16)
        w2 = (torch.randn(d_in, hidden, device=DEV) / hidden ** 0.5).to(torch.bfloat16)
        act_input = torch.addmm(b1, x, w1t)
        record("dgrad", shape, flops, {
            "ours": lambda: L.gemm_act_dgrad(g, w2, "squared_relu", act_input, True),
            "parent": lambda: A._act_bwd(torch.mm(g, w2), act_input, None, b1, A.SQRELU, True, False, False),
            "mm": lambda: torch.mm(g, w2)})
        del act_input, w1t
        ours = FusedDenseSqreluDense(d_in, hidden, device=DEV, dtype=torch.bfloat16)
        parent = FusedMLP(d_in, hidden, activation="sqrelu", device=DEV, dtype=torch.bfloat16)
        parent.load_state_dict(ours.state_dict())
        xg = x.clone().requires_grad_(True)

        def layer(mod):
            def run():
                out = mod(xg)
                torch.autograd.grad(out, (xg, *mod.parameters()), g)
            return run

        record("layer", shape, 6 * flops, {"ours": layer(ours), "parent": layer(parent)})
        del x, w1, w2, g, xg, ours, parent
        torch.cuda.empty_cache()

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
