"""Developer aid: what producing the lists of a prompt costs over the e4m3 index-key cache -- kvcache_index_topk_prefill(
k_index_scale=) (csrc/fa_index_prefill8.hip) -- against the 16-bit prefill kernel on the same values and against what the decode
entry can do for the same tokens.  The grid is tools/index_prefill_bench.py's: index heads 64, index dim 128 and 64, bf16 queries,
pages of 64 rows behind a shuffled table, batch 1, s_q 512 / 4096 / 16384 over full caches of 8192 / 32768 / 131072 keys (where
s_q <= cache), causal, topk 2048.  The cache is written by kvcache_index_append_fp8 from randn rows.

Per shape, in one process, in alternating rounds (device events over warmed calls, median of --iters per round, median / min /
max over --rounds):
  call_us         (a) the call on the workspace it allocates by default (256 MiB at most): all rounds, both launches
  logits_us       (a) with topk = capacity into ONE list row shared by all tokens: the logits launches (+ near-empty selections),
                  as tools/index_prefill_bench.py isolates them; tflops = 2 * h_i * d_i flop per visible (token, key) pair over it
  bf16_us, bf16_logits_us   (b) the same two for the 16-bit kvcache_index_topk_prefill on the dequantised bf16 cache, which holds
                  the same values exactly (bf16_holds_the_values checks it)
  decode16_us     (c) kvcache_index_topk(k_index_scale=) once per 16 tokens with the fill level shifted to the tokens' causal edge
same_as_decode16: (a)'s lists equal (c)'s.  One JSON line per shape, printed and written to --out (profiles/index_prefill8.jsonl).
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
from tools.index_topk_bench import events  # noqa: E402

HI, PAGE, TOPK, STEP = 64, 64, 2048, 16
BF, F8 = torch.bfloat16, torch.float8_e4m3fn


def shape(s_q, sk, d_i):
    table = torch.randperm(sk // PAGE, device="cuda", dtype=torch.int32).view(1, sk // PAGE)
    k8, scale = torch.zeros(sk // PAGE, PAGE, d_i, device="cuda").to(F8), torch.zeros(sk // PAGE, PAGE, device="cuda")
    fills = fa3.kvcache_index_append_fp8(k8, scale, torch.randn(1, sk, d_i, dtype=BF, device="cuda"),
                                         torch.zeros(1, dtype=torch.int32, device="cuda"), page_table=table)
    k16 = (k8.float() * scale[..., None]).to(BF)
    q_i, w = torch.randn(1, s_q, HI, d_i, dtype=BF, device="cuda"), torch.randn(1, s_q, HI, device="cuda") * HI ** -0.5
    idx, idx_b, idx_d = (torch.empty(1, s_q, 1, TOPK, dtype=torch.int32, device="cuda") for _ in range(3))
    every = torch.empty(sk, dtype=torch.int32, device="cuda").expand(1, s_q, 1, sk)  # one row for all tokens (logits arms)
    rows = max(min(s_q, (fa3.INDEX_PREFILL_WORKSPACE_CAP // (4 * sk)) // 8 * 8), 8)
    work, logits16 = torch.empty(rows, sk, device="cuda"), torch.empty(1, STEP, sk, device="cuda")
    fills16 = [fills - (s_q - i0 - STEP) for i0 in range(0, s_q, STEP)]  # the fill level at the last token of each step

    def decode16():
        for j, i0 in enumerate(range(0, s_q, STEP)):
            fa3.kvcache_index_topk(q_i[:, i0:i0 + STEP], k8, w[:, i0:i0 + STEP], fills16[j], TOPK, page_table=table, k_index_scale=scale,
                                   indices=idx_d[:, i0:i0 + STEP], logits=logits16)

    bind = _lib.binding()
    calls = {"call": lambda: fa3.kvcache_index_topk_prefill(q_i, k8, w, fills, TOPK, page_table=table, indices=idx, workspace=work,
                                                            k_index_scale=scale),
             "logits": lambda: bind.kvcache_index_topk_prefill_fp8(q_i, k8, scale, w, fills, sk, None, table, True, every, work),
             "bf16": lambda: fa3.kvcache_index_topk_prefill(q_i, k16, w, fills, TOPK, page_table=table, indices=idx_b, workspace=work),
             "bf16_logits": lambda: bind.kvcache_index_topk_prefill(q_i, k16, w, fills, sk, None, table, True, every, work),
             "decode16": decode16}
    for fn in calls.values():
        fn()
    torch.cuda.synchronize()
    desc = dict(s_q=s_q, s_k=sk, h_i=HI, d_i=d_i, page=PAGE, topk=TOPK, workspace_rows=rows,
                bf16_holds_the_values=bool(torch.equal(k16.float(), k8.float() * scale[..., None])),
                same_as_decode16=bool(torch.equal(idx, idx_d)), bf16_agreement=round((idx == idx_b).float().mean().item(), 4),
                plan=bind.kvcache_index_topk_prefill_fp8_plan(q_i, k8, scale, w, fills, TOPK, None, table, True, idx, work))
    return desc, calls


def measure(desc, calls, iters, rounds):
    t = {name: [] for name in calls}
    for _ in range(rounds):  # alternating rounds: drift of the clocks hits all of them
        for name, fn in calls.items():
            t[name].append(events(fn, iters))
    med = lambda x: sorted(x)[len(x) // 2]  # noqa: E731
    us = lambda x: round(x * 1e6, 1)  # noqa: E731
    m = {name: med(x) for name, x in t.items()}
    s_q, sk = desc["s_q"], desc["s_k"]
    flop = 2 * HI * desc["d_i"] * (s_q * sk - s_q * (s_q - 1) // 2)
    return dict(desc, call_us=us(m["call"]), logits_us=us(m["logits"]), tflops=round(flop / m["logits"] / 1e12, 1),
                bf16_us=us(m["bf16"]), bf16_logits_us=us(m["bf16_logits"]), bf16_tflops=round(flop / m["bf16_logits"] / 1e12, 1),
                decode16_us=us(m["decode16"]), bf16_over_call=round(m["bf16"] / m["call"], 3),
                bf16_logits_over_logits=round(m["bf16_logits"] / m["logits"], 3), decode16_over_call=round(m["decode16"] / m["call"], 2),
                us_min_max={name: [us(min(x)), us(max(x))] for name, x in t.items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "index_prefill8.jsonl"))
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--quick", action="store_true", help="s_q 512 over 8192 keys only")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "index_prefill8_bench needs a GPU"
    torch.manual_seed(0)
    grid = [(512, 8192)] if a.quick else [(s_q, sk) for s_q in (512, 4096, 16384) for sk in (8192, 32768, 131072) if s_q <= sk]
    rows = []
    for d_i in (128, 64):
        for s_q, sk in grid:
            r = measure(*shape(s_q, sk, d_i), a.iters, a.rounds)
            print(json.dumps(r), flush=True)
            rows.append(r)
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
