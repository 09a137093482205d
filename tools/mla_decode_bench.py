"""Developer aid: MLA decode through FA3 qv (flash_attn_with_kvcache with qv; h_k 1, d 64, d_v 512, page 64, num_splits 0).

Times every shape with device events over warmed calls (median of --iters) and prints / writes one JSON line per shape:
cache bytes per second (b * s_k * (d + d_v) * 2) and FLOP/s (2 * b * h * s_q * s_k * (d + 2 d_v)), and the bound that applies
(HBM at 8 TB/s or bf16 MFMA at the 2.5 PF dense peak).  Kernel-only times come from a separate rocprofv3 --kernel-trace
--stats run of this script.  Also reports a qv prefill line (b 2, h 16 / h_k 1, s 4096, causal).  GPU only.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from flash_attention_annotated_amd import hopper_interface as fa3  # noqa: E402

HBM, MFMA = 8.0e12, 2.5e15


def timed(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, e in ev:
        a.record()
        fn()
        e.record()
    torch.cuda.synchronize()
    return sorted(a.elapsed_time(e) for a, e in ev)[iters // 2] * 1e-3


def decode(b, h, sk, sq, warmup, iters, d=64, dv=512, page=64):
    npg = sk // page
    cache = torch.randn(b * npg, page, 1, d + dv, dtype=torch.bfloat16, device="cuda")
    table = torch.randperm(b * npg, device="cuda", dtype=torch.int32).view(b, npg)
    q = torch.randn(b, sq, h, d, dtype=torch.bfloat16, device="cuda")
    qv = torch.randn(b, sq, h, dv, dtype=torch.bfloat16, device="cuda")
    seqlens = torch.full((b,), sk, dtype=torch.int32, device="cuda")
    fn = lambda: fa3.flash_attn_with_kvcache(q, cache[..., :d], cache[..., d:], qv=qv, cache_seqlens=seqlens,  # noqa: E731
                                             page_table=table, num_splits=0)
    t = timed(fn, warmup, iters)
    nbytes = b * sk * (d + dv) * 2
    flop = 2 * b * h * sq * sk * (d + 2 * dv)
    t_hbm, t_mfma = nbytes / HBM, flop / MFMA
    bound = "hbm" if t_hbm >= t_mfma else "mfma"
    return {"kind": "decode", "b": b, "h": h, "h_k": 1, "s_k": sk, "s_q": sq, "us": round(t * 1e6, 2),
            "cache_TBps": round(nbytes / t / 1e12, 3), "TFLOPs": round(flop / t / 1e12, 1), "bound": bound,
            "frac_of_bound": round(max(t_hbm, t_mfma) / t, 3)}


def prefill(warmup, iters, b=2, h=16, s=4096, d=64, dv=512):
    q = torch.randn(b, s, h, d, dtype=torch.bfloat16, device="cuda")
    qv = torch.randn(b, s, h, dv, dtype=torch.bfloat16, device="cuda")
    k = torch.randn(b, s, 1, d, dtype=torch.bfloat16, device="cuda")
    v = torch.randn(b, s, 1, dv, dtype=torch.bfloat16, device="cuda")
    t = timed(lambda: fa3.flash_attn_func(q, k, v, qv=qv, causal=True), warmup, iters)
    flop = 2 * b * h * s * s * (d + 2 * dv) / 2
    return {"kind": "prefill", "b": b, "h": h, "h_k": 1, "s": s, "causal": True, "us": round(t * 1e6, 1),
            "TFLOPs": round(flop / t / 1e12, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "mla_decode.jsonl"))
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--quick", action="store_true", help="one shape per head count (for a profiler run)")
    a = ap.parse_args()
    rows = []
    shapes = [(b, h, sk, sq) for h in (16, 128) for b in (1, 16, 64, 128) for sk in (4096, 8192) for sq in (1, 2)]
    if a.quick:
        shapes = [(128, 16, 8192, 1), (128, 128, 8192, 1)]
    for b, h, sk, sq in shapes:
        r = decode(b, h, sk, sq, a.warmup, a.iters)
        print(json.dumps(r), flush=True)
        rows.append(r)
    if not a.quick:
        r = prefill(a.warmup, max(5, a.iters // 3))
        print(json.dumps(r), flush=True)
        rows.append(r)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
