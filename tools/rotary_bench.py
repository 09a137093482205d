"""Developer aid: what the rotary embedding layer costs.  One process, b8 s8192 h32, d128 and d64, bf16, rotary_dim = d and d / 2,
both pair orders, random data.  Per shape four forms of the HIP launch (flash_attention_annotated_amd.layers.rotary):
out of place, in place, the packed-qkv call (q and k of a (b, s, 3, h, d) tensor in one launch) and the conjugate (backward)
launch.  Hip-event timings of single launches after warm-up, the median of --iters (>= 30) launches.

Each row: us and GB/s of algorithmic bytes -- the elements the form has to read, once, the elements it has to write, once, and
the two tables once (out of place: all of x and out; in place and packed: the rotary_dim columns of the rotated heads, read and
written).  Beside it: apply_rotary_emb_torch on the same tensors, and -- for the in-place form -- fa_rotary_apply (the
inference rotary pass of fa_fwd.h, called through the C-ABI) on the same values, the two timed in alternating rounds; the spread
of a side is max / min of its round medians.

Usage: python tools/rotary_bench.py [--warmup W] [--iters N] [--rounds R] [--out profiles/rotary.jsonl]"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

DEV = "cuda"
B, S, H = 8, 8192, 32


def timed(run, iters):
    """median ms of `iters` single launches"""
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, e in ev:
        a.record(); run(); e.record()
    torch.cuda.synchronize()
    return sorted(a.elapsed_time(e) for a, e in ev)[iters // 2]


def parent_launch(lib, _lib, x, cos, sin, offsets, interleaved):
    """fa_rotary_apply in place on x (b, s, h, d), one position per row"""
    p = _lib.FaRotaryParams()
    p.abi_version, p.struct_size = _lib.FA_ABI_VERSION, ctypes.sizeof(_lib.FaRotaryParams)
    p.src = p.dst = x.data_ptr()
    p.src_batch_stride = p.dst_batch_stride = x.stride(0)
    p.src_row_stride = p.dst_row_stride = x.stride(1)
    p.src_head_stride = p.dst_head_stride = x.stride(2)
    p.b, p.s, p.h, p.d = x.shape
    p.dtype, p.rotary_dim, p.rotary_interleaved, p.per_row_positions = _lib.FA_DTYPE_BF16, 2 * cos.shape[1], int(interleaved), 1
    p.rotary_cos, p.rotary_sin, p.seqlen_offsets = cos.data_ptr(), sin.data_ptr(), offsets.data_ptr()

    def run():
        st = lib.fa_rotary_apply(p, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert st == 0, st
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rotary.jsonl"))
    args = ap.parse_args()
    assert args.iters >= 30 and args.rounds >= 2
    assert torch.cuda.is_available(), "rotary_bench needs a GPU"
    from flash_attention_annotated_amd import _lib
    from flash_attention_annotated_amd.layers import rotary
    lib = _lib.load()
    torch.manual_seed(0)
    rows = []
    with torch.no_grad():
        for d in (128, 64):
            x = torch.randn(B, S, H, d, dtype=torch.bfloat16, device=DEV)
            qkv = torch.randn(B, S, 3, H, d, dtype=torch.bfloat16, device=DEV)
            offsets = torch.zeros(B, dtype=torch.int32, device=DEV)
            for rd in (d, d // 2):
                ang = torch.rand(S, rd // 2, device=DEV) * 6.2831853
                cos, sin = torch.cos(ang).bfloat16(), torch.sin(ang).bfloat16()
                table_bytes = 2 * cos.numel() * 2
                for il in (False, True):
                    xi, xp = x.clone(), x.clone()  # the in-place sides rotate buffers of their own, from the same values
                    forms = {
                        "out_of_place": (lambda: rotary.apply_rotary(x, cos, sin, interleaved=il), 2 * x.numel() * 2),
                        "in_place": (lambda: rotary.apply_rotary(xi, cos, sin, interleaved=il, inplace=True), 2 * B * S * H * rd * 2),
                        "packed_qkv": (lambda: rotary.apply_rotary_emb_qkv_(qkv, cos, sin, interleaved=il), 2 * B * S * 2 * H * rd * 2),
                        "conjugate": (lambda: rotary.apply_rotary(x, cos, sin, interleaved=il, conjugate=True), 2 * x.numel() * 2),
                    }
                    eager = {
                        "out_of_place": lambda: rotary.apply_rotary_emb_torch(x, cos, sin, il),
                        "in_place": lambda: xi.copy_(rotary.apply_rotary_emb_torch(xi, cos, sin, il)),
                        "packed_qkv": lambda: qkv[:, :, :2].copy_(rotary.apply_rotary_emb_torch(qkv[:, :, :2].reshape(B, S, 2 * H, d), cos, sin, il)
                                                                  .view(B, S, 2, H, d)),
                        "conjugate": lambda: rotary.apply_rotary_emb_torch(x, cos, -sin, il),
                    }
                    for form, (run, data_bytes) in forms.items():
                        for _ in range(args.warmup):
                            run(); eager[form]()
                        ms, ms_torch = timed(run, args.iters), timed(eager[form], args.iters)
                        nbytes = data_bytes + table_bytes
                        row = dict(shape=f"b{B} s{S} h{H} d{d}", dtype="bf16", rotary_dim=rd, interleaved=il, form=form,
                                   us=round(ms * 1e3, 2), algorithmic_bytes=nbytes, gb_per_s=round(nbytes / ms / 1e6, 1),
                                   torch_us=round(ms_torch * 1e3, 2), torch_over_hip=round(ms_torch / ms, 2),
                                   warmup=args.warmup, iters=args.iters)
                        if form == "in_place":
                            parent = parent_launch(lib, _lib, xp, cos, sin, offsets, il)
                            for _ in range(args.warmup):
                                parent()
                            ours_r, parent_r = [], []
                            for _ in range(args.rounds):
                                ours_r.append(timed(run, args.iters))
                                parent_r.append(timed(parent, args.iters))
                            ours_m, parent_m = sorted(ours_r)[args.rounds // 2], sorted(parent_r)[args.rounds // 2]
                            row.update(rounds=args.rounds, round_us=[round(t * 1e3, 2) for t in ours_r],
                                       fa_rotary_apply_round_us=[round(t * 1e3, 2) for t in parent_r],
                                       hip_over_fa_rotary_apply=round(ours_m / parent_m, 4),
                                       spread=round(max(ours_r) / min(ours_r), 4),
                                       fa_rotary_apply_spread=round(max(parent_r) / min(parent_r), 4))
                        rows.append(row)
                        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
