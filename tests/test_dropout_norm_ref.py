"""CPU tests of flash_attention_annotated_amd.ops.layer_norm: the reference's surface (flash_attn/ops/layer_norm.py:311-800 and
the dropout_add_rms_norm forms of flash_attn/ops/rms_norm.py), signature by signature; the names that are not built are absent;
CPU tensors take the oracle of ops.norm; the return arity for prenorm x return_dropout_mask x parallel.  The signatures below
are restated from the reference: nothing here reads it."""
import importlib
import inspect
import itertools

import pytest
import torch

from flash_attention_annotated_amd.ops import layer_norm as L
from flash_attention_annotated_amd.ops import norm

E = inspect.Parameter.empty
ONE = [("x0", E), ("residual", E), ("weight", E), ("bias", E), ("dropout_p", E), ("epsilon", E), ("rowscale", None),
       ("layerscale", None), ("prenorm", False), ("residual_in_fp32", False), ("return_dropout_mask", False)]
PAR = [("x0", E), ("x1", E), ("residual", E), ("weight0", E), ("bias0", E), ("weight1", E), ("bias1", E), ("dropout_p", E),
       ("epsilon", E), ("prenorm", False), ("residual_in_fp32", False), ("return_dropout_mask", False)]
MODULE = [("self", E), ("hidden_size", E), ("prenorm", False), ("p", 0.0), ("eps", 1e-5), ("residual_in_fp32", False),
          ("device", None), ("dtype", None)]
SIGNATURES = {
    "layer_norm": [("x", E), ("weight", E), ("bias", E), ("epsilon", E)],
    "dropout_add_layer_norm": ONE,
    "dropout_add_rms_norm": ONE,
    "dropout_add_layer_norm_parallel_residual": PAR,
    "dropout_add_rms_norm_parallel_residual": PAR,
    "DropoutAddLayerNorm.__init__": MODULE,
    "DropoutAddRMSNorm.__init__": MODULE,
    "DropoutAddLayerNorm.forward": [("self", E), ("x0", E), ("residual", None)],
    "DropoutAddRMSNorm.forward": [("self", E), ("x0", E), ("residual", None)],
    "DropoutAddLayerNormFn.forward": [("ctx", E), ("x0", E), ("residual", E), ("gamma", E), ("beta", E), ("rowscale", E), ("colscale", E),
                                      ("dropout_p", E), ("epsilon", E), ("residual_in_fp32", False), ("prenorm", False),
                                      ("is_rms_norm", False), ("return_dmask", False)],
    "DropoutAddLayerNormParallelResidualFn.forward": [("ctx", E), ("x0", E), ("x1", E), ("residual", E), ("gamma0", E), ("beta0", E),
                                                      ("gamma1", E), ("beta1", E), ("dropout_p", E), ("epsilon", E),
                                                      ("residual_in_fp32", False), ("prenorm", False), ("is_rms_norm", False),
                                                      ("return_dmask", False)],
}


@pytest.mark.parametrize("name", sorted(SIGNATURES))
def test_signature_is_the_references(name):
    obj = L
    for part in name.split("."):
        obj = getattr(obj, part)
    got = [(p.name, p.default) for p in inspect.signature(obj).parameters.values()]
    assert got == SIGNATURES[name]


def test_surface():
    assert issubclass(L.DropoutAddLayerNormFn, torch.autograd.Function)
    assert issubclass(L.DropoutAddLayerNormParallelResidualFn, torch.autograd.Function)
    for name in ("dropout_add_layer_norm_subset", "dropout_add_rms_norm_subset", "DropoutAddLayerNormSubsetFn"):
        assert not hasattr(L, name)
        with pytest.raises(ImportError):
            exec(f"from flash_attention_annotated_amd.ops.layer_norm import {name}")
    for text in ("subset", "ops.rms_norm"):  # the docstring says what is not built, and where the RMS forms live
        assert text in L.__doc__
    # ops.rms_norm did not gain the RMS forms
    rms = importlib.import_module("flash_attention_annotated_amd.ops.rms_norm")
    assert not hasattr(rms, "dropout_add_rms_norm") and not hasattr(rms, "DropoutAddRMSNorm")
    mod = L.DropoutAddRMSNorm(8)
    assert mod.bias is None and [n for n, _ in mod.named_parameters()] == ["weight"]
    mod = L.DropoutAddLayerNorm(8, prenorm=True, p=0.1)
    assert sorted(n for n, _ in mod.named_parameters()) == ["bias", "weight"] and mod.prenorm and mod.p == 0.1
    assert bool((mod.weight == 1).all()) and bool((mod.bias == 0).all())


def _operands(parallel, dtype=torch.float32):
    torch.manual_seed(0)
    x0, x1, res = (torch.randn(2, 5, 24, dtype=dtype) for _ in range(3))
    w0, b0, w1, b1, cs = (torch.randn(24, dtype=dtype) for _ in range(5))
    rs = torch.rand(2, 5, dtype=dtype) + 0.5
    return x0, x1, res, w0, b0, w1, b1, rs, cs


@pytest.mark.parametrize("prenorm,mask,parallel", list(itertools.product((False, True), repeat=3)))
@pytest.mark.parametrize("p", [0.0, 0.3])
def test_cpu_arity_and_oracle(prenorm, mask, parallel, p):
    """z, then x with prenorm, then the mask(s) with return_dropout_mask; the parallel form has two of each.  Given the mask it
    returned, the CPU path is the oracle, bit for bit."""
    x0, x1, res, w0, b0, w1, b1, rs, cs = _operands(parallel)
    torch.manual_seed(1)
    if parallel:
        out = L.dropout_add_layer_norm_parallel_residual(x0, x1, res, w0, b0, w1, b1, p, 1e-5, prenorm=prenorm,
                                                         return_dropout_mask=True)
    else:
        out = L.dropout_add_rms_norm(x0, res, w0, b0, p, 1e-5, rowscale=rs, layerscale=cs, prenorm=prenorm, return_dropout_mask=True)
    n_z, n_m = (2, 2) if parallel else (1, 1)
    assert isinstance(out, tuple) and len(out) == n_z + int(prenorm) + n_m
    masks = out[-n_m:]
    for m in masks:
        assert m.dtype == torch.uint8 and m.shape == x0.shape
        assert bool(m.all()) if p == 0.0 else 0 < int(m.sum()) < m.numel()
    kw = dict(eps=1e-5, dropout_p=p, prenorm=prenorm, dropout_mask=masks[0].bool())
    if parallel:
        want = norm.layer_norm_ref(x0, w0, b0, residual=res, x1=x1, weight1=w1, bias1=b1, dropout_mask1=masks[1].bool(), **kw)
    else:
        want = norm.rms_norm_ref(x0 * cs, w0, b0, residual=res, rowscale=rs, **kw)
    want = want if isinstance(want, tuple) else (want,)
    for a, b in zip(out[:n_z + int(prenorm)], want):
        assert torch.equal(a, b)
    # without return_dropout_mask: the same without the masks; a lone z is no tuple
    torch.manual_seed(1)
    if parallel:
        short = L.dropout_add_layer_norm_parallel_residual(x0, x1, res, w0, b0, w1, b1, p, 1e-5, prenorm=prenorm)
    else:
        short = L.dropout_add_rms_norm(x0, res, w0, b0, p, 1e-5, rowscale=rs, layerscale=cs, prenorm=prenorm)
    if not mask:
        if not parallel and not prenorm:
            assert isinstance(short, torch.Tensor) and torch.equal(short, out[0])
        else:
            assert len(short) == n_z + int(prenorm) and all(torch.equal(a, b) for a, b in zip(short, out))


def test_cpu_conventions():
    x0, x1, res, w0, b0, w1, b1, rs, cs = _operands(True, torch.bfloat16)
    z0, z1, x = L.dropout_add_layer_norm_parallel_residual(x0, None, None, w0, b0, None, None, 0.0, 1e-5, prenorm=True,
                                                           residual_in_fp32=True)
    assert z1 is None and x.dtype == torch.float32 and z0.dtype == torch.bfloat16
    _, x = L.dropout_add_layer_norm(x0, res.float(), w0, b0, 0.0, 1e-5, prenorm=True)
    assert x.dtype == torch.float32  # the residual's dtype wins over residual_in_fp32=False
    assert torch.equal(L.layer_norm(x0, w0, b0, 1e-5), norm.layer_norm_ref(x0, w0, b0, eps=1e-5))
    mod = L.DropoutAddLayerNorm(24, p=0.5).eval()
    assert torch.equal(mod(x0.float()), norm.layer_norm_ref(x0.float(), mod.weight, mod.bias, eps=1e-5))
    x0g = x0.float().requires_grad_(True)
    L.dropout_add_layer_norm(x0g, None, w0.float(), None, 0.3, 1e-5).sum().backward()  # differentiable by torch itself
    assert x0g.grad is not None and x0g.grad.shape == x0.shape
    with pytest.raises(ValueError):
        L.dropout_add_layer_norm(x0, res[:1], w0, b0, 0.0, 1e-5)
