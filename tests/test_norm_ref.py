"""CPU tests of flash_attention_annotated_amd.ops: layer_norm_ref / rms_norm_ref against the reference's pure-torch functions,
frozen by tools/make_norm_golden.py into tests/golden/norm_golden.pt (outputs and fp32 autograd gradients, exactly), the public
names and signatures, the RMSNorm modules, the refusals and the return arities."""
import inspect
import os

import pytest
import torch

from flash_attention_annotated_amd.ops import norm, rms_norm
from flash_attention_annotated_amd.ops.triton import layer_norm

CASES = torch.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "norm_golden.pt"))["cases"]


def test_golden_covers_the_cases():
    for rms in (False, True):
        cs = [c for c in CASES if c["rms"] == rms]
        assert {(c["residual"] is not None, c["prenorm"]) for c in cs} == {(a, b) for a in (False, True) for b in (False, True)}
        assert any(c["rowscale"] is not None for c in cs) and any(c["zero_centered_weight"] for c in cs)
        assert any(c["upcast"] for c in cs) and any(c["bias"] is None for c in cs) and any(c["dropout_mask"] is not None for c in cs)
        assert {c["x"].dtype for c in cs} == {torch.float32, torch.float16, torch.bfloat16}
        assert any(c["residual"] is not None and c["residual"].dtype != c["x"].dtype for c in cs)
        assert sum("dx" in c for c in cs) >= 8


def _call(c, x, w, b, res):
    fn = norm.rms_norm_ref if c["rms"] else norm.layer_norm_ref
    return fn(x, w, b, residual=res, eps=c["eps"], dropout_p=c["dropout_p"], rowscale=c["rowscale"], prenorm=c["prenorm"],
              zero_centered_weight=c["zero_centered_weight"], dropout_mask=c["dropout_mask"], upcast=c["upcast"])


@pytest.mark.parametrize("c", CASES, ids=lambda c: c["name"])
def test_ref_equals_reference(c):
    out = _call(c, c["x"], c["weight"], c["bias"], c["residual"])
    out, residual_out = out if c["prenorm"] else (out, None)
    assert out.dtype == c["out"].dtype and torch.equal(out, c["out"])
    if c["prenorm"]:
        assert residual_out.dtype == c["residual_out"].dtype and torch.equal(residual_out, c["residual_out"])


@pytest.mark.parametrize("c", [c for c in CASES if "dx" in c], ids=lambda c: c["name"])
def test_ref_gradients_equal_reference(c):
    leaves = [t.clone().requires_grad_(True) if t is not None else None for t in (c["x"], c["weight"], c["bias"], c["residual"])]
    out = _call(c, *leaves)
    loss = out[0] * torch.sigmoid(out[1]) if c["prenorm"] else out
    got = iter(torch.autograd.grad(loss, [t for t in leaves if t is not None], c["g"]))
    for name, leaf in zip(("dx", "dw", "db", "dresidual"), leaves):
        if leaf is None:
            assert c[name] is None
        else:
            assert torch.equal(next(got), c[name]), name


def test_parallel_form_of_the_refs():
    """x1 / weight1 / bias1 are arguments of the oracle functions too: a second output, and x1 added before the norm."""
    g = torch.Generator().manual_seed(0)
    x, x1, w, w1, b1 = (torch.randn(*s, generator=g) for s in ((3, 8), (3, 8), (8,), (8,), (8,)))
    for fn in (norm.layer_norm_ref, norm.rms_norm_ref):
        out, out1, res = fn(x, w, None, x1=x1, weight1=w1, bias1=b1, prenorm=True)
        assert torch.equal(res, x + x1)
        assert torch.equal(out, fn(x + x1, w, None)) and torch.equal(out1, fn(x + x1, w1, b1))


# the reference's signatures, names and defaults in order
_FN = [("x", None), ("weight", None), ("bias", None), ("residual", None), ("x1", None), ("weight1", None), ("bias1", None),
       ("eps", 1e-6), ("dropout_p", 0.0), ("rowscale", None), ("prenorm", False), ("residual_in_fp32", False),
       ("zero_centered_weight", False), ("is_rms_norm", False), ("return_dropout_mask", False), ("out_dtype", None), ("out", None),
       ("residual_out", None)]
_REF = _FN[:11] + [("zero_centered_weight", False), ("dropout_mask", None), ("dropout_mask1", None), ("upcast", False)]
SIGNATURES = {
    "layer_norm_fn": _FN,
    "rms_norm_fn": [a for a in _FN if a[0] != "is_rms_norm"],
    "layer_norm_ref": _REF,
    "rms_norm_ref": _REF,
    "layer_norm_linear_fn": [("x", None), ("norm_weight", None), ("norm_bias", None), ("linear_weight", None), ("linear_bias", None),
                             ("residual", None), ("eps", 1e-6), ("prenorm", False), ("residual_in_fp32", False), ("is_rms_norm", False)],
}
REQUIRED = {"layer_norm_fn": 3, "rms_norm_fn": 3, "layer_norm_ref": 3, "rms_norm_ref": 3, "layer_norm_linear_fn": 5}


@pytest.mark.parametrize("name", sorted(SIGNATURES))
def test_signatures(name):
    params = inspect.signature(getattr(layer_norm, name)).parameters
    assert list(params) == [n for n, _ in SIGNATURES[name]]
    for i, (n, default) in enumerate(SIGNATURES[name]):
        if i < REQUIRED[name]:
            assert params[n].default is inspect.Parameter.empty, n
        else:
            assert params[n].default == default and type(params[n].default) is type(default), n


def test_exports_and_modules():
    assert set(layer_norm.__all__) == {"layer_norm_fn", "rms_norm_fn", "LayerNormFn", "RMSNorm", "layer_norm_ref", "rms_norm_ref",
                                       "LayerNormLinearFn", "layer_norm_linear_fn"}
    for name in layer_norm.__all__:
        assert getattr(layer_norm, name) is getattr(norm, name)
    assert issubclass(norm.LayerNormFn, torch.autograd.Function) and issubclass(norm.LayerNormLinearFn, torch.autograd.Function)
    assert not hasattr(rms_norm, "dropout_add_rms_norm")
    assert list(inspect.signature(rms_norm.rms_norm).parameters) == ["x", "weight", "epsilon"]
    init = inspect.signature(rms_norm.RMSNorm.__init__).parameters
    assert [(n, p.default) for n, p in init.items()][1:] == [("hidden_size", inspect.Parameter.empty), ("eps", 1e-5), ("device", None),
                                                             ("dtype", None)]
    init = inspect.signature(norm.RMSNorm.__init__).parameters
    assert [(n, p.default) for n, p in init.items()][1:] == [("hidden_size", inspect.Parameter.empty), ("eps", 1e-5), ("dropout_p", 0.0),
                                                             ("zero_centered_weight", False), ("device", None), ("dtype", None)]
    fwd = inspect.signature(norm.RMSNorm.forward).parameters
    assert [(n, p.default) for n, p in fwd.items()][1:] == [("x", inspect.Parameter.empty), ("residual", None), ("prenorm", False),
                                                            ("residual_in_fp32", False)]


def test_rms_norm_modules_initialise():
    m = norm.RMSNorm(12, dtype=torch.bfloat16)
    assert torch.equal(m.weight, torch.ones(12, dtype=torch.bfloat16)) and m.bias is None and m.eps == 1e-5 and m.dropout_p == 0.0
    z = norm.RMSNorm(12, zero_centered_weight=True)
    assert torch.equal(z.weight, torch.zeros(12))
    assert norm.RMSNorm(12, dropout_p=0.1).dropout_p == 0.1
    s = rms_norm.RMSNorm(7, eps=1e-3)
    assert torch.equal(s.weight, torch.ones(7)) and s.bias is None and s.eps == 1e-3
    assert set(dict(s.named_parameters())) == {"weight"}


def _cpu_args():
    return torch.randn(2, 3, 8), torch.ones(8), torch.zeros(8)


@pytest.mark.parametrize("kw,word", [(dict(dropout_p=0.1), "dropout_p"), (dict(x1=torch.zeros(2, 3, 8)), "x1"),
                                     (dict(weight1=torch.ones(8)), "weight1"), (dict(bias1=torch.zeros(8)), "bias1")])
def test_refusals_name_the_argument_before_any_device_call(kw, word):
    """On CPU tensors, without a device or the library: the refusal comes first."""
    x, w, b = _cpu_args()
    for fn in (norm.layer_norm_fn, norm.rms_norm_fn):
        with pytest.raises(NotImplementedError, match=word):
            fn(x, w, b, **kw)
    if "dropout_p" not in kw:
        return
    m = norm.RMSNorm(8, dropout_p=0.1)
    with pytest.raises(NotImplementedError, match="dropout_p"):
        m(x)


def test_feature_dim_above_64_kib_raises_the_references_error():
    x = torch.zeros(1, 32776, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="This layer norm doesn't support feature dim >= 64KB."):
        norm.layer_norm_fn(x, torch.ones(32776), None)
    with pytest.raises(RuntimeError, match="This layer norm doesn't support feature dim >= 64KB."):
        norm.rms_norm_fn(torch.zeros(1, 16385), torch.ones(16385), None)


@pytest.mark.parametrize("prenorm", [False, True])
@pytest.mark.parametrize("return_dropout_mask", [False, True])
def test_return_arity(monkeypatch, prenorm, return_dropout_mask):
    """The reference's LayerNormFn.forward :926-948 with weight1 None: y | (y, residual_out) | (y, None, None) |
    (y, residual_out, None, None).  The kernel entry is replaced by the oracle: this is about the wrapper."""
    def fake_fwd(x, weight, bias, residual, rowscale, out, residual_out, eps, zero_centered_weight, is_rms_norm):
        y, z = norm.layer_norm_ref(x, weight, bias, residual=residual, eps=eps, prenorm=True, upcast=True)
        out.copy_(y)
        if residual_out is not None:
            residual_out.copy_(z)
        return x.new_zeros(x.shape[0]), x.new_ones(x.shape[0])
    monkeypatch.setattr(norm, "_norm_fwd", fake_fwd)
    x, w, b = _cpu_args()
    res = torch.randn(2, 3, 8)
    ret = norm.layer_norm_fn(x, w, b, residual=res, prenorm=prenorm, return_dropout_mask=return_dropout_mask)
    if not prenorm and not return_dropout_mask:
        assert isinstance(ret, torch.Tensor) and ret.shape == x.shape
        return
    assert isinstance(ret, tuple) and len(ret) == 1 + int(prenorm) + 2 * int(return_dropout_mask)
    assert ret[0].shape == x.shape
    if prenorm:
        assert torch.equal(ret[1], x + res)
    if return_dropout_mask:
        assert ret[-2] is None and ret[-1] is None


def test_kernel_entries_are_custom_ops():
    ns = torch.ops.flash_attn_amd
    fwd = ns._norm_fwd.default._schema
    assert [a.name for a in fwd.arguments if a.alias_info is not None and a.alias_info.is_write] == ["out", "residual_out"]
    assert not ns._norm_bwd.default._schema.is_mutable
