"""Developer aid: one continuous-batching step through the FA3 surface, flash_attn_with_kvcache(..., cu_seqlens_q=,
cu_seqlens_k_new=, max_seqlen_q=) -- hq 32 / hkv 8, d 128, bf16, pages of 64 rows, num_splits 0.

Per (cache length, batch) it times, with device events over warmed calls (median of --iters), and prints / writes one JSON
line each:
  decode   every sequence one token: the ragged call (q (b, h, d), cu_seqlens_q = arange) and the dense call (q (b, 1, h, d)),
           timed in alternating rounds on the same cache; both append one row per sequence.  The ragged form takes the dense
           route behind a view, so the two should sit inside each other's round-to-round spread.
  mixed    4 prefill chunks of 512 tokens beside b - 4 single-token decodes, appended raggedly and attended causally: cache
           bytes per second (the keys each sequence reads, K and V) and TFLOP/s (4 d per visible (query, key) pair and head).
  append   the ragged append launch alone (fa_kvcache_append_varlen through ctypes, max_seqlen_k_new given / not given)
           against the bytes it moves (new rows read + written, K and V).
GPU only.
"""
import argparse
import ctypes
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


def paged_cache(b, cap):
    npg = cap // PAGE
    kc = torch.randn(b * npg, PAGE, HK, D, dtype=BF, device="cuda")
    vc = torch.randn(b * npg, PAGE, HK, D, dtype=BF, device="cuda")
    table = torch.randperm(b * npg, device="cuda", dtype=torch.int32).view(b, npg)
    return kc, vc, table


def decode(b, sk, warmup, iters, rounds=5):
    kc, vc, table = paged_cache(b, sk)
    fills = torch.full((b,), sk - 1, dtype=torch.int32, device="cuda")
    q = torch.randn(b, H, D, dtype=BF, device="cuda")
    kn, vn = (torch.randn(b, 1, HK, D, dtype=BF, device="cuda") for _ in range(2))
    cu = torch.arange(b + 1, dtype=torch.int32, device="cuda")
    ragged = lambda: fa3.flash_attn_with_kvcache(q, kc, vc, k=kn, v=vn, cache_seqlens=fills, page_table=table, cu_seqlens_q=cu,  # noqa: E731
                                                 max_seqlen_q=1, causal=True, num_splits=0)
    dense = lambda: fa3.flash_attn_with_kvcache(q.view(b, 1, H, D), kc, vc, k=kn, v=vn, cache_seqlens=fills, page_table=table,  # noqa: E731
                                                causal=True, num_splits=0)
    assert torch.equal(ragged(), dense().view(b, H, D))
    for _ in range(warmup):
        ragged(), dense()
    t_r, t_d = [], []
    for _ in range(rounds):  # alternating rounds: drift of the clocks hits both
        t_r.append(events(ragged, iters))
        t_d.append(events(dense, iters))
    nbytes = 2 * b * sk * HK * D * 2
    med = lambda x: sorted(x)[len(x) // 2]  # noqa: E731
    return {"kind": "decode", "b": b, "s_k": sk, "ragged_us": round(med(t_r) * 1e6, 2), "dense_us": round(med(t_d) * 1e6, 2),
            "ragged_us_min_max": [round(min(t_r) * 1e6, 2), round(max(t_r) * 1e6, 2)],
            "dense_us_min_max": [round(min(t_d) * 1e6, 2), round(max(t_d) * 1e6, 2)],
            "ragged_cache_TBps": round(nbytes / med(t_r) / 1e12, 3), "dense_cache_TBps": round(nbytes / med(t_d) / 1e12, 3)}


def mixed(b, sk, warmup, iters, chunks=4, chunk=512):
    kc, vc, table = paged_cache(b, sk)
    lens = [chunk] * chunks + [1] * (b - chunks)
    total = sum(lens)
    fills = torch.tensor([sk - n for n in lens], dtype=torch.int32, device="cuda")
    cu = torch.tensor([sum(lens[:i]) for i in range(b + 1)], dtype=torch.int32, device="cuda")
    q = torch.randn(total, H, D, dtype=BF, device="cuda")
    kn, vn = (torch.randn(total, HK, D, dtype=BF, device="cuda") for _ in range(2))
    fn = lambda: fa3.flash_attn_with_kvcache(q, kc, vc, k=kn, v=vn, cache_seqlens=fills, page_table=table, cu_seqlens_q=cu,  # noqa: E731
                                             cu_seqlens_k_new=cu, max_seqlen_q=chunk, causal=True, num_splits=0)
    for _ in range(warmup):
        fn()
    t = events(fn, iters)
    nbytes = 2 * b * sk * HK * D * 2
    pairs = sum(n * sk - n * (n - 1) // 2 for n in lens)  # visible (query, key) pairs under the bottom-right aligned causal mask
    flop = 4 * D * H * pairs
    return {"kind": "mixed", "b": b, "s_k": sk, "prefill_chunks": chunks, "chunk": chunk, "decodes": b - chunks, "total_q": total,
            "us": round(t * 1e6, 1), "cache_TBps": round(nbytes / t / 1e12, 3), "TFLOPs": round(flop / t / 1e12, 1)}


def append(b, sk, warmup, iters, chunks=4, chunk=512):
    kc, vc, table = paged_cache(b, sk)
    lens = [chunk] * chunks + [1] * (b - chunks)
    total = sum(lens)
    keep = dict(fills=torch.tensor([sk - n for n in lens], dtype=torch.int32, device="cuda"),
                cu=torch.tensor([sum(lens[:i]) for i in range(b + 1)], dtype=torch.int32, device="cuda"),
                out=torch.empty(b, dtype=torch.int32, device="cuda"),
                kn=torch.randn(total, HK, D, dtype=BF, device="cuda"), vn=torch.randn(total, HK, D, dtype=BF, device="cuda"))
    p = _lib.FaKvcacheAppendVarlenParams()
    p.abi_version, p.struct_size = _lib.FA_ABI_VERSION, ctypes.sizeof(p)
    p.k_new, p.v_new, p.k_cache, p.v_cache = keep["kn"].data_ptr(), keep["vn"].data_ptr(), kc.data_ptr(), vc.data_ptr()
    p.knew_row_stride = p.vnew_row_stride = HK * D
    p.knew_head_stride = p.vnew_head_stride = p.kcache_head_stride = p.vcache_head_stride = D
    p.kcache_row_stride = p.vcache_row_stride = HK * D
    p.kcache_batch_stride = p.vcache_batch_stride = PAGE * HK * D
    p.b, p.total_k_new, p.seqlen_cache, p.h_k, p.d, p.dtype = b, total, sk, HK, D, _lib.FA_DTYPE_BF16
    p.cu_seqlens_k_new, p.cache_seqlens, p.seqused_out = keep["cu"].data_ptr(), keep["fills"].data_ptr(), keep["out"].data_ptr()
    p.block_table, p.block_table_batch_stride, p.page_block_size = table.data_ptr(), table.stride(0), PAGE
    lib = _lib.load()
    row = {"kind": "append", "b": b, "s_k": sk, "rows": total, "bytes": 2 * 2 * total * HK * D * 2}
    for name, bound in (("search", 0), ("grid2d", chunk)):
        p.max_seqlen_k_new = bound
        stream = torch.cuda.current_stream().cuda_stream

        def fn():
            st = lib.fa_kvcache_append_varlen(ctypes.byref(p), ctypes.c_void_p(stream))
            assert st == 0, st
        for _ in range(warmup):
            fn()
        t = events(fn, iters)
        row[f"{name}_us"] = round(t * 1e6, 2)
        row[f"{name}_TBps"] = round(row["bytes"] / t / 1e12, 3)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "ragged_decode.jsonl"))
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--quick", action="store_true", help="one shape only")
    a = ap.parse_args()
    shapes = [(b, sk) for sk in (4096, 8192) for b in (64, 128)]
    if a.quick:
        shapes = shapes[:1]
    rows = []
    for b, sk in shapes:
        for r in (decode(b, sk, a.warmup, a.iters), mixed(b, sk, a.warmup, a.iters), append(b, sk, a.warmup, a.iters)):
            print(json.dumps(r), flush=True)
            rows.append(r)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
