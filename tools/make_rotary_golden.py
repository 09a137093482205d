#!/usr/bin/env python
"""Freeze what the reference's pure-torch rotary code computes into tests/golden/rotary_golden.pt (tensors only).

    python tools/make_rotary_golden.py --reference /path/to/flash-attention

Runs on a CPU.  Reads two things of the reference's flash_attn/layers/rotary.py: apply_rotary_emb_torch and
RotaryEmbedding._update_cos_sin_cache (its Triton kernel is not imported: the module it comes from is replaced by an empty
stand-in while the file loads).  tests/test_rotary_ref.py asserts that this package's apply_rotary_emb_torch and tables equal
the frozen ones exactly.
"""
import argparse
import importlib.util
import os
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "rotary_golden.pt")


def load_reference(root):
    for name in ("flash_attn", "flash_attn.ops", "flash_attn.ops.triton"):
        sys.modules.setdefault(name, types.ModuleType(name))
    stand_in = types.ModuleType("flash_attn.ops.triton.rotary")
    stand_in.apply_rotary = None
    sys.modules["flash_attn.ops.triton.rotary"] = stand_in
    spec = importlib.util.spec_from_file_location("reference_rotary", os.path.join(root, "flash_attn", "layers", "rotary.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def tables(g, seqlen_ro, half):
    angle = torch.rand(seqlen_ro, half, generator=g) * 6.2831853
    return torch.cos(angle), torch.sin(angle)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference (the directory that holds flash_attn/)")
    args = ap.parse_args()
    ref = load_reference(args.reference)
    g = torch.Generator().manual_seed(20251019)
    cases = []

    def plain(name, b, s, h, d, rd, interleaved, offsets=None):
        """offsets None: tables of s rows; an int: rows [off, off + s) of longer tables; a list: one offset per batch entry,
        the tables gathered to (b, s, rd / 2)."""
        x = torch.randn(b, s, h, d, generator=g)
        cos, sin = tables(g, s + 11, rd // 2)
        case = dict(name=name, kind="plain", x=x, cos=cos, sin=sin, interleaved=interleaved, offsets=offsets)
        if offsets is None:
            c, sn = cos[:s], sin[:s]
        elif isinstance(offsets, int):
            c, sn = cos[offsets:offsets + s], sin[offsets:offsets + s]
        else:
            idx = torch.tensor(offsets)[:, None] + torch.arange(s)[None]
            c, sn = cos[idx], sin[idx]
        case["out"] = ref.apply_rotary_emb_torch(x, c, sn, interleaved)
        cases.append(case)

    for il in (False, True):
        tag = "il" if il else "half"
        plain(f"full_{tag}", 2, 7, 3, 16, 16, il)
        plain(f"partial_{tag}", 2, 7, 3, 16, 8, il)
        plain(f"odd_width_{tag}", 1, 5, 2, 24, 12, il)
        plain(f"int_offset_{tag}", 2, 6, 2, 16, 16, il, offsets=5)
        plain(f"batch_offsets_{tag}", 3, 4, 2, 16, 8, il, offsets=[0, 9, 3])
        plain(f"one_row_one_head_{tag}", 1, 1, 1, 8, 2, il)

    def packed(name, shape, num_heads_q, rd, interleaved, own_k_tables):
        """q and k of a packed qkv rotated, v passed on: (b, s, 3, h, d), or (b, s, hq + 2 hk, d) with num_heads_q."""
        qkv = torch.randn(*shape, generator=g)
        s = shape[1]
        cos, sin = tables(g, s, rd // 2)
        cos_k, sin_k = tables(g, s, rd // 2) if own_k_tables else (None, None)
        ck, sk = (cos_k, sin_k) if own_k_tables else (cos, sin)
        if qkv.dim() == 5:
            q, k, v = qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2]
            out = torch.stack([ref.apply_rotary_emb_torch(q, cos, sin, interleaved),
                               ref.apply_rotary_emb_torch(k, ck, sk, interleaved), v], dim=2)
        else:
            hk = (shape[2] - num_heads_q) // 2
            q, k, v = qkv[:, :, :num_heads_q], qkv[:, :, num_heads_q:num_heads_q + hk], qkv[:, :, num_heads_q + hk:]
            out = torch.cat([ref.apply_rotary_emb_torch(q, cos, sin, interleaved),
                             ref.apply_rotary_emb_torch(k, ck, sk, interleaved), v], dim=2)
        cases.append(dict(name=name, kind="qkv", qkv=qkv, cos=cos, sin=sin, cos_k=cos_k, sin_k=sin_k, interleaved=interleaved,
                          num_heads_q=num_heads_q, out=out))

    for il in (False, True):
        tag = "il" if il else "half"
        packed(f"qkv_{tag}", (2, 5, 3, 2, 16), None, 16, il, False)
        packed(f"qkv_gqa_{tag}", (2, 5, 6 + 2 * 2, 16), 6, 8, il, False)
        packed(f"qkv_own_k_tables_{tag}", (1, 5, 3, 2, 16), None, 16, il, True)
        packed(f"qkv_gqa_own_k_tables_{tag}", (1, 4, 4 + 2 * 1, 16), 4, 16, il, True)

    caches = []
    for dim, base, scale_base, seqlen, dtype in ((16, 10000.0, None, 33, torch.float32), (64, 10000.0, None, 50, torch.bfloat16),
                                                 (32, 500000.0, 512, 40, torch.float32), (16, 10000.0, 512, 9, torch.float16)):
        m = ref.RotaryEmbedding(dim, base=base, scale_base=scale_base)
        m._update_cos_sin_cache(seqlen, device=torch.device("cpu"), dtype=dtype)
        caches.append(dict(dim=dim, base=base, scale_base=scale_base, seqlen=seqlen, dtype=dtype, inv_freq=m.inv_freq, scale=m.scale,
                           cos=m._cos_cached, sin=m._sin_cached, cos_k=m._cos_k_cached, sin_k=m._sin_k_cached))
    torch.save(dict(cases=cases, caches=caches), OUT)
    print(f"{OUT}: {len(cases)} cases, {len(caches)} table sets, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
