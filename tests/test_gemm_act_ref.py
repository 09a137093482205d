"""CPU tests of the Python surface of the fused GEMM (ops.triton.linear, ops.triton.mlp): the reference's signatures, the pure
torch oracle against F.linear and torch's activations in fp64, and the CPU path of the functions and of the module."""
import inspect

import pytest
import torch
import torch.nn.functional as F

from flash_attention_annotated_amd.ops.triton import linear, mlp

ACTS = {"id": lambda t: t, "gelu": F.gelu, "gelu_approx": lambda t: F.gelu(t, approximate="tanh"),
        "squared_relu": lambda t: F.relu(t).square(), "relu": F.relu}


def _signature(fn):
    return [(n, p.default) for n, p in inspect.signature(fn).parameters.items()]


E = inspect.Parameter.empty


def test_signatures_are_the_references():
    assert _signature(linear.triton_linear_act) == [("x", E), ("weight", E), ("bias", None), ("activation", "id"), ("save_act_input", False)]
    assert _signature(linear.triton_dgrad_act) == [("grad_output", E), ("weight", E), ("activation", "id"), ("act_input", None)]
    assert _signature(linear.linear_act_ref) == _signature(linear.triton_linear_act)
    assert _signature(linear.dgrad_act_ref) == _signature(linear.triton_dgrad_act)
    assert _signature(linear.gemm_act_dgrad) == _signature(linear.triton_dgrad_act) + [("want_dbias", False)]
    assert _signature(mlp.FusedDenseSqreluDenseFunc.forward) == [("ctx", E), ("x", E), ("weight1", E), ("bias1", E), ("weight2", E),
                                                                 ("bias2", E), ("checkpoint_lvl", 0)]
    assert mlp.fused_dense_sqrelu_dense_function == mlp.FusedDenseSqreluDenseFunc.apply
    assert _signature(mlp.FusedDenseSqreluDense.__init__) == [("self", E), ("in_features", E), ("hidden_features", None),
                                                              ("out_features", None), ("bias1", True), ("bias2", True),
                                                              ("checkpoint_lvl", 0), ("device", None), ("dtype", None)]
    assert _signature(mlp.FusedDenseSqreluDense.forward) == [("self", E), ("x", E)]
    assert linear.__all__ == ["triton_linear_act", "triton_dgrad_act", "gemm_act_dgrad", "linear_act_ref", "dgrad_act_ref"]
    assert mlp.__all__ == ["FusedDenseSqreluDenseFunc", "fused_dense_sqrelu_dense_function", "FusedDenseSqreluDense"]


@pytest.mark.parametrize("activation", sorted(ACTS))
@pytest.mark.parametrize("with_bias", [False, True])
def test_oracle_agrees_with_torch_in_fp64(activation, with_bias):
    g = torch.Generator().manual_seed(3)
    x = torch.randn(3, 37, 24, dtype=torch.float64, generator=g)
    w = torch.randn(40, 24, dtype=torch.float64, generator=g) / 24 ** 0.5
    b = torch.randn(40, dtype=torch.float64, generator=g) if with_bias else None
    out, act_input = linear.linear_act_ref(x, w, b, activation, save_act_input=True)
    assert torch.equal(act_input, F.linear(x, w, b))
    torch.testing.assert_close(out, ACTS[activation](F.linear(x, w, b)), rtol=1e-12, atol=1e-12)
    assert torch.equal(linear.linear_act_ref(x, w, b, activation), out)
    # the closed-form derivative against autograd through torch's activation
    pre = act_input.detach().requires_grad_(True)
    go = torch.randn(3, 37, 56, dtype=torch.float64, generator=g)
    w2 = torch.randn(56, 40, dtype=torch.float64, generator=g)
    (want,) = torch.autograd.grad(ACTS[activation](pre), pre, go @ w2)
    got = linear.dgrad_act_ref(go, w2, activation, act_input)
    torch.testing.assert_close(got, want, rtol=1e-9, atol=1e-9)


def test_cpu_path_of_the_functions():
    g = torch.Generator().manual_seed(4)
    x = torch.randn(2, 5, 16, generator=g)
    w = torch.randn(24, 16, generator=g)
    b = torch.randn(24, generator=g)
    out, act_input = linear.triton_linear_act(x, w, b, activation="gelu", save_act_input=True)
    assert out.shape == act_input.shape == (2, 5, 24)
    torch.testing.assert_close(out, F.gelu(F.linear(x, w, b)))
    assert torch.equal(linear.triton_linear_act(x, w, b, activation="gelu"), out)
    go, w2 = torch.randn(2, 5, 8, generator=g), torch.randn(8, 24, generator=g)
    grad = linear.triton_dgrad_act(go, w2, "gelu", act_input)
    assert grad.shape == (2, 5, 24)
    grad2, dbias = linear.gemm_act_dgrad(go, w2, "gelu", act_input, want_dbias=True)
    assert torch.equal(grad, grad2)
    torch.testing.assert_close(dbias, grad.reshape(-1, 24).sum(0))
    assert torch.equal(linear.triton_dgrad_act(go, w2), go @ w2)
    with pytest.raises(AssertionError):
        linear.triton_dgrad_act(go, w2, "gelu")  # (act_input is required)
    with pytest.raises(AssertionError):
        linear.triton_linear_act(x, w, b, activation="tanh")
    with pytest.raises(AssertionError):
        linear.triton_linear_act(x, w.double(), b)


@pytest.mark.parametrize("checkpoint_lvl", [0, 1, 2])
def test_cpu_path_of_the_module(checkpoint_lvl):
    torch.manual_seed(5)
    m = mlp.FusedDenseSqreluDense(16, 40, checkpoint_lvl=checkpoint_lvl, dtype=torch.float64)
    x = torch.randn(2, 7, 16, dtype=torch.float64, requires_grad=True)
    go = torch.randn(2, 7, 16, dtype=torch.float64)
    out = m(x)
    grads = torch.autograd.grad(out, (x, *m.parameters()), go)
    xr = x.detach().clone().requires_grad_(True)
    ref = F.linear(F.relu(F.linear(xr, m.fc1.weight, m.fc1.bias)).square(), m.fc2.weight, m.fc2.bias)
    want = torch.autograd.grad(ref, (xr, *m.parameters()), go)
    torch.testing.assert_close(out, ref, rtol=1e-12, atol=1e-12)
    for a, b in zip(grads, want):
        torch.testing.assert_close(a, b, rtol=1e-10, atol=1e-10)
    with pytest.raises(AssertionError):
        mlp.FusedDenseSqreluDense(16, 40, bias1=False)
