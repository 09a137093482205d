#!/usr/bin/env python
"""Freeze what the reference's pure-torch norm code computes into tests/golden/norm_golden.pt (tensors only).

    python tools/make_norm_golden.py --reference /path/to/flash-attention

Runs on a CPU.  Reads two functions of the reference's flash_attn/ops/triton/layer_norm.py: layer_norm_ref and rms_norm_ref.
The file queries the device and decorates its Triton kernels while it loads, so it is loaded with stand-ins for
flash_attn.utils.torch, flash_attn.utils.library, triton.autotune and the two torch.cuda queries; none of its kernels runs.
tests/test_norm_ref.py asserts that this package's layer_norm_ref / rms_norm_ref give the frozen outputs and the frozen fp32
gradients exactly.
"""
import argparse
import importlib.util
import itertools
import os
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "norm_golden.pt")


def load_reference(root):
    import triton
    for name in ("flash_attn", "flash_attn.utils"):
        sys.modules.setdefault(name, types.ModuleType(name))
    passthrough = lambda fn=None, **kw: fn if fn is not None else (lambda f: f)  # noqa: E731
    utils_torch = types.ModuleType("flash_attn.utils.torch")
    utils_torch.custom_fwd = utils_torch.custom_bwd = passthrough
    utils_library = types.ModuleType("flash_attn.utils.library")
    utils_library.triton_op = lambda *a, **kw: (lambda f: f)
    sys.modules["flash_attn.utils.torch"], sys.modules["flash_attn.utils.library"] = utils_torch, utils_library
    saved = triton.autotune, torch.cuda.get_device_properties, torch.cuda.current_device
    triton.autotune = lambda *a, **kw: (lambda f: f)
    torch.cuda.get_device_properties = lambda *a, **kw: types.SimpleNamespace(warp_size=64, multi_processor_count=256)
    torch.cuda.current_device = lambda: 0
    try:
        spec = importlib.util.spec_from_file_location("reference_layer_norm",
                                                      os.path.join(root, "flash_attn", "ops", "triton", "layer_norm.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        triton.autotune, torch.cuda.get_device_properties, torch.cuda.current_device = saved
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference (the directory that holds flash_attn/)")
    args = ap.parse_args()
    ref = load_reference(args.reference)
    g = torch.Generator().manual_seed(20261019)
    cases = []

    def case(name, rms, dtype=torch.float32, wdtype=torch.float32, shape=(2, 5, 24), residual=False, res_dtype=None, prenorm=False,
             rowscale=False, zero_centered_weight=False, upcast=False, bias=True, dropout_p=0.0, grads=False):
        n = shape[-1]
        x = torch.randn(*shape, generator=g).to(dtype)
        w = torch.randn(n, generator=g).to(wdtype)
        b = torch.randn(n, generator=g).to(wdtype) if bias else None
        res = torch.randn(*shape, generator=g).to(res_dtype or dtype) if residual else None
        rs = torch.rand(*shape[:-1], generator=g).to(dtype) + 0.5 if rowscale else None
        mask = torch.rand(*shape, generator=g) > dropout_p if dropout_p > 0.0 else None
        fn = ref.rms_norm_ref if rms else ref.layer_norm_ref
        kw = dict(residual=res, eps=1e-5, dropout_p=dropout_p, rowscale=rs, prenorm=prenorm, zero_centered_weight=zero_centered_weight,
                  dropout_mask=mask, upcast=upcast)
        c = dict(name=name, rms=rms, x=x, weight=w, bias=b, residual=res, rowscale=rs, dropout_mask=mask, eps=1e-5, dropout_p=dropout_p,
                 prenorm=prenorm, zero_centered_weight=zero_centered_weight, upcast=upcast)
        out = fn(x, w, b, **kw)
        c["out"], c["residual_out"] = (out if prenorm else (out, None))
        if grads:  # fp32 leaves, the reference test's loss
            leaves = [t.clone().requires_grad_(True) if t is not None else None for t in (x, w, b, res)]
            xl, wl, bl, rl = leaves
            o = fn(xl, wl, bl, **{**kw, "residual": rl})
            go = torch.randn(*shape, generator=g)
            loss = o[0] * torch.sigmoid(o[1]) if prenorm else o
            got = torch.autograd.grad(loss, [t for t in leaves if t is not None], go)
            it = iter(got)
            c["g"] = go
            c["dx"], c["dw"], c["db"], c["dresidual"] = (next(it) if t is not None else None for t in leaves)
        cases.append(c)

    for rms in (False, True):
        tag = "rms" if rms else "ln"
        for residual, prenorm in itertools.product((False, True), (False, True)):
            case(f"{tag}_res{int(residual)}_pre{int(prenorm)}", rms, residual=residual, prenorm=prenorm, grads=True)
        case(f"{tag}_rowscale", rms, residual=True, prenorm=True, rowscale=True, grads=True)
        case(f"{tag}_zero_centered", rms, zero_centered_weight=True, grads=True)
        case(f"{tag}_no_bias", rms, bias=False, residual=True, grads=True)
        case(f"{tag}_dropout_mask", rms, residual=True, prenorm=True, dropout_p=0.27, grads=True)
        for dtype in (torch.bfloat16, torch.float16):
            short = str(dtype)[6:]
            for upcast in (False, True):
                case(f"{tag}_{short}_up{int(upcast)}", rms, dtype=dtype, wdtype=dtype, residual=True, prenorm=True, upcast=upcast)
            case(f"{tag}_{short}_fp32_weight_fp32_residual", rms, dtype=dtype, residual=True, res_dtype=torch.float32, prenorm=True,
                 rowscale=True, upcast=True)
        case(f"{tag}_odd_width", rms, shape=(3, 37), residual=True, grads=True)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    torch.save(dict(cases=cases), OUT)
    print(f"{OUT}: {len(cases)} cases, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
