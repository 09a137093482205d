"""Developer aid: what producing the lists of a prompt costs -- kvcache_index_topk_prefill (csrc/fa_index_prefill.hip) -- against
what the decode entry can do for the same tokens and against the rule composed of torch calls.  Shapes: index heads 64, index dim
128 and 64, bf16, pages of 64 rows behind a shuffled table, batch 1, s_q 512 / 4096 / 16384 over full caches of 8192 / 32768 /
131072 keys (where s_q <= cache), causal, topk 2048.

Per shape, in one process, in alternating rounds (device events over warmed calls, median of --iters per round, median / min /
max over --rounds):
  call_us       kvcache_index_topk_prefill on the workspace it allocates by default (256 MiB at most): all rounds, both launches
  logits_us     the call with topk = capacity into ONE list row shared by all tokens: its selection launches only write 0 .. n - 1
                (the tokens race on equal values, the row is discarded), so this is the logits launches (+ near-empty ones);
                select_us = call_us - logits_us and select_share = select_us / call_us are the selection by difference
  tflops        2 * h_i * d_i flop per visible (token, key) pair over logits_us; call_tflops the same over call_us
  decode16_us   kvcache_index_topk once per 16 tokens with the fill level shifted to the tokens' causal edge
  torch_us      einsum, relu, weighted sum, mask, topk, sort on the GPU in chunks of query tokens whose (chunk, h_i, keys) fp32
                tensor stays within 1 GiB
One JSON line per shape, printed and written to --out (profiles/index_prefill.jsonl).  GPU only.
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
BF = torch.bfloat16


def torch_index_topk(q_i, keys, w, sk, topk, out):
    """The rule on a full cache as a torch composition, a chunk of query tokens at a time (q_i (s_q, h, d), keys (sk, d))."""
    s_q, chunk = q_i.shape[0], max((1 << 28) // (HI * sk), 1)
    pos = torch.arange(sk, device=q_i.device)
    for i0 in range(0, s_q, chunk):
        qc = q_i[i0:i0 + chunk]
        logits = (torch.einsum("ihc,sc->ihs", qc, keys).float().relu_() * w[i0:i0 + chunk, :, None]).sum(1)
        n = sk - (s_q - 1 - torch.arange(i0, i0 + qc.shape[0], device=q_i.device))
        logits.masked_fill_(pos[None] >= n[:, None], float("-inf"))
        out[i0:i0 + chunk] = logits.topk(topk, -1).indices.sort(-1).values.to(torch.int32)


def shape(s_q, sk, d_i):
    k_i = torch.randn(sk // PAGE, PAGE, d_i, dtype=BF, device="cuda")
    table = torch.randperm(sk // PAGE, device="cuda", dtype=torch.int32).view(1, sk // PAGE)
    fills = torch.full((1,), sk, dtype=torch.int32, device="cuda")
    q_i, w = torch.randn(1, s_q, HI, d_i, dtype=BF, device="cuda"), torch.randn(1, s_q, HI, device="cuda") * HI ** -0.5
    idx, idx_d, idx_t = (torch.empty(1, s_q, 1, TOPK, dtype=torch.int32, device="cuda") for _ in range(3))
    every = torch.empty(sk, dtype=torch.int32, device="cuda").expand(1, s_q, 1, sk)  # one row for all tokens (logits arm)
    rows = max(min(s_q, (fa3.INDEX_PREFILL_WORKSPACE_CAP // (4 * sk)) // 8 * 8), 8)
    work, logits16 = torch.empty(rows, sk, device="cuda"), torch.empty(1, STEP, sk, device="cuda")
    keys = k_i[table[0].long()].view(sk, d_i)  # the logical rows, for the composition only
    fills16 = [fills - (s_q - i0 - STEP) for i0 in range(0, s_q, STEP)]  # the fill level at the last token of each step

    def decode16():
        for j, i0 in enumerate(range(0, s_q, STEP)):
            fa3.kvcache_index_topk(q_i[:, i0:i0 + STEP], k_i, w[:, i0:i0 + STEP], fills16[j], TOPK, page_table=table,
                                   indices=idx_d[:, i0:i0 + STEP], logits=logits16)

    calls = {"call": lambda: fa3.kvcache_index_topk_prefill(q_i, k_i, w, fills, TOPK, page_table=table, indices=idx, workspace=work),
             "logits": lambda: _lib.binding().kvcache_index_topk_prefill(q_i, k_i, w, fills, sk, None, table, True, every, work),
             "decode16": decode16, "torch": lambda: torch_index_topk(q_i[0], keys, w[0], sk, TOPK, idx_t[0, :, 0])}
    for fn in calls.values():
        fn()
    torch.cuda.synchronize()
    desc = dict(s_q=s_q, s_k=sk, h_i=HI, d_i=d_i, page=PAGE, topk=TOPK, workspace_rows=rows,
                same_as_decode16=bool(torch.equal(idx, idx_d)), torch_agreement=round((idx == idx_t).float().mean().item(), 4),
                plan=_lib.binding().kvcache_index_topk_prefill_plan(q_i, k_i, w, fills, TOPK, None, table, True, idx, work))
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
    return dict(desc, call_us=us(m["call"]), logits_us=us(m["logits"]), select_us=us(m["call"] - m["logits"]),
                select_share=round(1 - m["logits"] / m["call"], 3), tflops=round(flop / m["logits"] / 1e12, 1),
                call_tflops=round(flop / m["call"] / 1e12, 1), decode16_us=us(m["decode16"]), torch_us=us(m["torch"]),
                decode16_over_call=round(m["decode16"] / m["call"], 2), torch_over_call=round(m["torch"] / m["call"], 2),
                us_min_max={name: [us(min(x)), us(max(x))] for name, x in t.items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "index_prefill.jsonl"))
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--quick", action="store_true", help="s_q 512 over 8192 keys only")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "index_prefill_bench needs a GPU"
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
