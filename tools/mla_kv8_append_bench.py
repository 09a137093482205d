"""Developer aid: the write half of the fp8 (e4m3) KV cache of the MLA shape -- kvcache_append_qv8_kernel,
csrc/fa_kvcache_append_qv8.hip -- against the 16-bit append on the same rows, bf16, h_k 1, d 64 (k_pe) / d_v 512 (latent).

(a) A prefill-sized append: 8192 new rows of one sequence into an empty cache, dense and pages of 64 rows behind a shuffled
    table, with and without rotary (interleaved, rotary_dim = d).  fp8: fa_kvcache_append_qv8 through the C-ABI, against the
    library's 16-bit fa_kvcache_append with d_v through the C-ABI on the same rows (one launch each, the same host path);
    `fp8_op_us` is the public op hopper_interface.kvcache_append_fp8 on the same rows (the launch behind the binding's checks
    and the dispatcher).  bytes moved per element: 2 read + 1 written against 2 + 2.
(b) One decode step: kvcache_append_fp8 of one new row per sequence, then flash_attn_with_kvcache with qv on the fill levels it
    returns (h 128, cache 8192, fill level 8191, batch 1 / 32 / 128), against that read alone on the same fill level, so the
    share of the append shows.
Both sides of a comparison are timed in the same process in alternating rounds (device events over warmed calls, median of
--iters per round, median / min / max over --rounds).  One JSON line per shape, printed and written to --out
(profiles/mla_kv8_append.jsonl).  GPU only.
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

H, HK, D, DV, PAGE = 128, 1, 64, 512, 64
BF, F8 = torch.bfloat16, torch.float8_e4m3fn


def events(fn, iters):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, e in ev:
        a.record()
        fn()
        e.record()
    torch.cuda.synchronize()
    return sorted(a.elapsed_time(e) for a, e in ev)[iters // 2] * 1e-3


def alternate(calls, warmup, iters, rounds):
    for _ in range(warmup):
        for c in calls:
            c()
    times = [[] for _ in calls]
    for _ in range(rounds):  # alternating rounds: drift of the clocks hits every side
        for t, c in zip(times, calls):
            t.append(events(c, iters))
    return times


def med(x):
    return sorted(x)[len(x) // 2]


def us(x):
    return round(x * 1e6, 1)


def append16_call(k_new, v_new, kc, vc, fills, table, cos, sin):
    """fa_kvcache_append on the current stream through the C-ABI (dense new rows)."""
    lib = _lib.load()
    p = _lib.FaKvcacheAppendParams()
    p.abi_version, p.struct_size = _lib.FA_ABI_VERSION, ctypes.sizeof(_lib.FaKvcacheAppendParams)
    p.k_new, p.v_new, p.k_cache, p.v_cache = k_new.data_ptr(), v_new.data_ptr(), kc.data_ptr(), vc.data_ptr()
    for t, x in (("knew", k_new), ("vnew", v_new), ("kcache", kc), ("vcache", vc)):
        for i, s in enumerate(("batch", "row", "head")):
            setattr(p, f"{t}_{s}_stride", x.stride(i))
    p.b, p.seqlen_new, p.h_k, p.d, p.d_v = k_new.shape[0], k_new.shape[1], HK, D, DV
    p.seqlen_cache = kc.shape[1] if table is None else table.shape[1] * PAGE
    p.cache_seqlens = fills.data_ptr()
    p.dtype = _lib.FA_DTYPE_BF16
    if table is not None:
        p.block_table, p.block_table_batch_stride, p.page_block_size = table.data_ptr(), table.stride(0), PAGE
    if cos is not None:
        p.rotary_cos, p.rotary_sin, p.rotary_dim, p.rotary_interleaved = cos.data_ptr(), sin.data_ptr(), D, 1
    stream = torch.cuda.current_stream().cuda_stream

    def call():
        st = lib.fa_kvcache_append(ctypes.byref(p), ctypes.c_void_p(stream))
        assert st == 0, st
    return call


def append8_call(k_new, v_new, kc, vc, fills, table, cos, sin, kd, vd):
    """fa_kvcache_append_qv8 on the current stream through the C-ABI (dense new rows): the launch without the op's host path."""
    lib = _lib.load()
    p = _lib.new_kvcache_append_kv8_params()
    p.k_new, p.v_new, p.k_cache, p.v_cache = k_new.data_ptr(), v_new.data_ptr(), kc.data_ptr(), vc.data_ptr()
    for t, x in (("knew", k_new), ("vnew", v_new), ("kcache", kc), ("vcache", vc)):
        for i, s in enumerate(("batch", "row", "head")):
            setattr(p, f"{t}_{s}_stride", x.stride(i))
    p.b, p.seqlen_new, p.h_k, p.d, p.d_v = k_new.shape[0], k_new.shape[1], HK, D, DV
    p.seqlen_cache = kc.shape[1] if table is None else table.shape[1] * PAGE
    p.cache_seqlens = fills.data_ptr()
    p.k_descale, p.v_descale = kd.data_ptr(), vd.data_ptr()
    p.k_descale_batch_stride, p.k_descale_head_stride = kd.stride(0), kd.stride(1)
    p.v_descale_batch_stride, p.v_descale_head_stride = vd.stride(0), vd.stride(1)
    if table is not None:
        p.block_table, p.block_table_batch_stride, p.page_block_size = table.data_ptr(), table.stride(0), PAGE
    if cos is not None:
        p.rotary_cos, p.rotary_sin, p.rotary_dim, p.rotary_interleaved = cos.data_ptr(), sin.data_ptr(), D, 1
    stream = torch.cuda.current_stream().cuda_stream

    def call():
        st = lib.fa_kvcache_append_qv8(ctypes.byref(p), ctypes.c_void_p(stream))
        assert st == 0, st
    return call


def prefill_append(paged, rotary, a):
    rows = 8192
    k_new = torch.randn(1, rows, HK, D, device="cuda").to(BF)
    v_new = torch.randn(1, rows, HK, DV, device="cuda").to(BF)
    fills = torch.zeros(1, dtype=torch.int32, device="cuda")
    kd = torch.full((1, HK), 0.37, device="cuda")
    vd = torch.full((1, HK), 1.5, device="cuda")
    lead = (rows // PAGE, PAGE, HK) if paged else (1, rows, HK)
    k8, v8 = torch.zeros(*lead, D, device="cuda").to(F8), torch.zeros(*lead, DV, device="cuda").to(F8)
    k16, v16 = torch.zeros(*lead, D, dtype=BF, device="cuda"), torch.zeros(*lead, DV, dtype=BF, device="cuda")
    table = torch.randperm(rows // PAGE, device="cuda", dtype=torch.int32).view(1, -1) if paged else None
    cos = sin = None
    if rotary:
        ang = torch.rand(rows, D // 2, device="cuda") * 6.283
        cos, sin = torch.cos(ang).to(BF), torch.sin(ang).to(BF)
    op8 = lambda: fa3.kvcache_append_fp8(k8, v8, k_new, v_new, fills, kd, vd, page_table=table, rotary_cos=cos,  # noqa: E731
                                           rotary_sin=sin, rotary_interleaved=True)
    call16 = append16_call(k_new, v_new, k16, v16, fills, table, cos, sin)
    call8 = append8_call(k_new, v_new, k8, v8, fills, table, cos, sin, kd, vd)
    t8, t16, top = alternate([call8, call16, op8], a.warmup, a.iters, a.rounds)
    elems = rows * HK * (D + DV)
    return dict(what="prefill_append", rows=rows, cache="page64" if paged else "dense", rotary=rotary,
                fp8_us=us(med(t8)), bf16_us=us(med(t16)), ratio=round(med(t8) / med(t16), 3), fp8_op_us=us(med(top)),
                fp8_us_min_max=[us(min(t8)), us(max(t8))], bf16_us_min_max=[us(min(t16)), us(max(t16))],
                fp8_GBps=round(3 * elems / med(t8) / 1e9, 1), bf16_GBps=round(4 * elems / med(t16) / 1e9, 1))


def decode_step(b, a):
    sk = 8192
    q = torch.randn(b, 1, H, D, dtype=BF, device="cuda")
    qv = torch.randn(b, 1, H, DV, dtype=BF, device="cuda")
    k_new = torch.randn(b, 1, HK, D, dtype=BF, device="cuda")
    v_new = torch.randn(b, 1, HK, DV, dtype=BF, device="cuda")
    k8 = torch.randn(b * sk, HK, D, device="cuda").to(F8).view(b, sk, HK, D)
    v8 = torch.randn(b * sk, HK, DV, device="cuda").to(F8).view(b, sk, HK, DV)
    fills = torch.full((b,), sk - 1, dtype=torch.int32, device="cuda")
    full = torch.full((b,), sk, dtype=torch.int32, device="cuda")
    one = torch.ones(b, HK, device="cuda")
    read = lambda fill: fa3.flash_attn_with_kvcache(q, k8, v8, qv=qv, cache_seqlens=fill, k_descale=one, v_descale=one,  # noqa: E731
                                                    num_splits=0)
    step = lambda: read(fa3.kvcache_append_fp8(k8, v8, k_new, v_new, fills, one, one))  # noqa: E731
    read_only = lambda: read(full)  # noqa: E731
    ts, tr = alternate([step, read_only], a.warmup, a.iters, a.rounds)
    return dict(what="decode_step", b=b, s_k=sk, h=H, step_us=us(med(ts)), read_only_us=us(med(tr)),
                append_share=round((med(ts) - med(tr)) / med(ts), 3),
                step_us_min_max=[us(min(ts)), us(max(ts))], read_only_us_min_max=[us(min(tr)), us(max(tr))])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "mla_kv8_append.jsonl"))
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "mla_kv8_append_bench needs a GPU"
    torch.manual_seed(0)
    rows = []
    for paged in (False, True):
        for rotary in (False, True):
            rows.append(prefill_append(paged, rotary, a))
            print(json.dumps(rows[-1]), flush=True)
            torch.cuda.empty_cache()
    for b in (1, 32, 128):
        rows.append(decode_step(b, a))
        print(json.dumps(rows[-1]), flush=True)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
