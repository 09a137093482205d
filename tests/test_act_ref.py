"""CPU tests of the activation oracles (ops/activations.py: act_ref, gated_act_ref and the closed-form gradients), of the
public names and signatures of ops.activations, ops.fused_dense and modules.mlp, and of the modules on CPU tensors.  No
device; tests/test_act_gpu.py holds the kernels to these oracles."""
import inspect
from functools import partial

import pytest
import torch
import torch.nn.functional as F

from flash_attention_annotated_amd.modules import mlp
from flash_attention_annotated_amd.ops import activations as A
from flash_attention_annotated_amd.ops import fused_dense as D

F64 = torch.float64
NAMES = ("gelu_tanh", "gelu_erf", "relu", "sqrelu", "silu", "sigmoid", "identity")
TORCH = {"gelu_tanh": partial(F.gelu, approximate="tanh"), "gelu_erf": F.gelu, "relu": F.relu, "silu": F.silu}


def close(a, b):
    return torch.allclose(a, b, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("name", sorted(TORCH))
def test_oracle_matches_torch_in_fp64(name):
    torch.manual_seed(0)
    x, b = 3 * torch.randn(37, 203, dtype=F64), torch.randn(203, dtype=F64)
    assert close(A.act_ref(x, name), TORCH[name](x))
    assert close(A.act_ref(x, name, b), TORCH[name](x + b))


def test_gated_oracle_is_glu_in_fp64():
    torch.manual_seed(1)
    x12 = 3 * torch.randn(37, 2 * 203, dtype=F64)
    assert close(A.gated_act_ref(x12, "sigmoid"), F.glu(x12, dim=-1))
    up, gate = x12.chunk(2, dim=-1)
    assert close(A.gated_act_ref(x12, "silu"), up * F.silu(gate))
    assert close(A.gated_act_ref(x12, "sqrelu"), up * F.relu(gate) ** 2)


@pytest.mark.parametrize("name", NAMES)
def test_gradient_oracles_match_autograd_in_fp64(name):
    torch.manual_seed(2)
    x = (3 * torch.randn(37, 203, dtype=F64)).requires_grad_(True)
    b = torch.randn(203, dtype=F64, requires_grad=True)
    d = torch.randn(37, 203, dtype=F64)
    dx, db = torch.autograd.grad(A.act_ref(x, name, b), (x, b), d)
    dpre, dbias = A.act_grad_ref(d, x.detach(), name, b.detach())
    assert close(dpre, dx) and close(dbias, db)
    assert A.act_grad_ref(d, x.detach(), name)[1] is None
    x12 = (3 * torch.randn(37, 2 * 203, dtype=F64)).requires_grad_(True)
    (dx12,) = torch.autograd.grad(A.gated_act_ref(x12, name), x12, d)
    assert close(A.gated_act_grad_ref(d, x12.detach(), name), dx12)


def test_gradient_oracles_have_no_nan_at_saturation():
    big = torch.tensor([0.0, -0.0, 1e4, -1e4, 1e30, -1e30, torch.finfo(torch.float32).max, -torch.finfo(torch.float32).max])
    for name in NAMES:
        for x in (big, big.double()):
            assert not torch.isnan(A.act_grad_ref(torch.ones_like(x), x, name)[0]).any(), name  # (2 * max is inf: an overflow, no NaN)


def test_gradient_oracles_match_autograd_on_the_probes():
    """the closed forms select their limits (`w > 0`, sigmoid(-z) for 1 - sigmoid) as the kernels do; here they are held to
    torch's own fp64 autograd on the saturating values themselves, the largest finite values of every dtype included.
    Absolutely, to 1e-14: autograd forms 1 + tanh and 1 - tanh^2, which cancel in the tails, so it is exact there to an
    absolute 1e-16 and not relatively; a wrongly selected limit is an error of the order of the gradient itself"""
    vals = [0.0, -0.0]
    for v in (2.0 ** -20, 0.75, 1.278, 1.0, 5.0, 10.0, 40.0, 100.0, 1e4, 65504.0, 1.8e19, torch.finfo(torch.bfloat16).max, torch.finfo(torch.float32).max):
        vals += [v, -v]
    x = torch.tensor(vals, dtype=F64)
    d = torch.linspace(-3, 3, x.numel(), dtype=F64)
    for name in NAMES:
        leaf = x.clone().requires_grad_(True)
        (dx,) = torch.autograd.grad(A.act_ref(leaf, name), leaf, d)
        got = A.act_grad_ref(d, x, name)[0]
        assert torch.isfinite(dx).all() and torch.allclose(got, dx, rtol=1e-12, atol=1e-14), name
        x12 = torch.cat([x.flip(0), x])[None].clone().requires_grad_(True)
        (dx12,) = torch.autograd.grad(A.gated_act_ref(x12, name), x12, d[None])
        assert torch.allclose(A.gated_act_grad_ref(d[None], x12.detach(), name), dx12, rtol=1e-12, atol=1e-14 * x.abs().max().item()), name


# what the reference's modules define and with which parameters: written out from reading flash_attn/ops/activations.py,
# flash_attn/ops/fused_dense.py and flash_attn/modules/mlp.py; (name, default) pairs, REQUIRED where there is no default
REQUIRED = inspect.Parameter.empty
SIGNATURES = {
    (A, "bias_gelu"): [("y", REQUIRED), ("bias", REQUIRED)],
    (A, "bias_gelu_back"): [("g", REQUIRED), ("y", REQUIRED), ("bias", REQUIRED)],
    (A, "bias_gelu_impl"): [("input", REQUIRED), ("bias", REQUIRED)],
    (A, "gelu_fwd"): [("x", REQUIRED)],
    (A, "gelu_bwd"): [("g", REQUIRED), ("x", REQUIRED)],
    (A, "fast_gelu_impl"): [("input", REQUIRED)],
    (A, "relu_bwd"): [("g", REQUIRED), ("x", REQUIRED)],
    (A, "sqrelu_fwd"): [("x", REQUIRED)],
    (A, "sqrelu_bwd"): [("g", REQUIRED), ("x", REQUIRED)],
    (A, "swiglu_fwd"): [("x", REQUIRED), ("y", REQUIRED)],
    (A, "swiglu_bwd"): [("x", REQUIRED), ("y", REQUIRED), ("g", REQUIRED)],
    (A, "swiglu"): [("x", REQUIRED), ("y", REQUIRED)],
    (A, "gated_act"): [("x12", REQUIRED), ("activation", REQUIRED)],
    (D, "fused_dense_func"): [("x", REQUIRED), ("weight", REQUIRED), ("bias", None), ("return_residual", False), ("process_group", None),
                              ("sequence_parallel", True)],
    (D, "fused_mlp_func"): [("x", REQUIRED), ("weight1", REQUIRED), ("weight2", REQUIRED), ("bias1", None), ("bias2", None),
                            ("activation", "gelu_approx"), ("save_pre_act", True), ("return_residual", False), ("checkpoint_lvl", 0),
                            ("heuristic", 0), ("process_group", None), ("sequence_parallel", True)],
    (D, "FusedDense"): [("in_features", REQUIRED), ("out_features", REQUIRED), ("bias", True), ("return_residual", False), ("device", None),
                        ("dtype", None)],
    (D, "FusedMLP"): [("in_features", REQUIRED), ("hidden_features", None), ("out_features", None), ("bias1", True), ("bias2", True),
                      ("activation", "gelu_approx"), ("return_residual", False), ("checkpoint_lvl", 0), ("heuristic", "auto"),
                      ("device", None), ("dtype", None)],
    (mlp, "Mlp"): [("in_features", REQUIRED), ("hidden_features", None), ("out_features", None), ("activation", F.gelu), ("bias1", True),
                   ("bias2", True), ("return_residual", False), ("device", None), ("dtype", None)],
    (mlp, "GatedMlp"): [("in_features", REQUIRED), ("hidden_features", None), ("out_features", None), ("activation", F.sigmoid),
                        ("bias1", True), ("bias2", True), ("multiple_of", 128), ("return_residual", False), ("device", None),
                        ("dtype", None)],
}


@pytest.mark.parametrize("module,name", sorted(SIGNATURES, key=lambda k: (k[0].__name__, k[1])), ids=lambda v: getattr(v, "__name__", v))
def test_public_names_and_signatures(module, name):
    obj = getattr(module, name)
    assert name in module.__all__
    params = list(inspect.signature(obj).parameters.values())
    assert [(p.name, p.default) for p in params] == SIGNATURES[(module, name)]


def test_forward_signatures_of_the_modules():
    for cls in (D.FusedDense, D.FusedMLP):
        assert [(p.name, p.default) for p in inspect.signature(cls.forward).parameters.values()] == [("self", REQUIRED), ("x", REQUIRED),
                                                                                                     ("process_group", None)]


def test_parallel_classes_are_not_built():
    for module, names in ((D, ("ColumnParallelLinear", "RowParallelLinear", "ParallelFusedMLP")), (mlp, ("ParallelMLP", "ParallelGatedMlp"))):
        for name in names:
            assert not hasattr(module, name)
    with pytest.raises(ImportError):
        from flash_attention_annotated_amd.ops.fused_dense import ParallelFusedMLP  # noqa: F401


def test_process_group_is_refused_before_any_device_call():
    x, w = torch.randn(3, 8), torch.randn(16, 8)
    group = object()
    for call in (lambda: D.fused_dense_func(x, w, process_group=group),
                 lambda: D.fused_mlp_func(x, w, w.t().contiguous(), process_group=group),
                 lambda: D.FusedDense(8, 16)(x, process_group=group),
                 lambda: D.FusedMLP(8, 16)(x, process_group=group)):
        with pytest.raises(NotImplementedError, match="process_group"):
            call()


def test_gated_hidden_size():
    assert mlp.GatedMlp(512).fc1.out_features == 2 * 1408
    assert mlp.GatedMlp(64, hidden_features=130, multiple_of=64).fc2.in_features == 192
    assert mlp.Mlp(64).fc1.out_features == 256


def test_unknown_activation_name():
    with pytest.raises(ValueError, match="unknown activation"):
        A.act(torch.zeros(2, 2), "tanh")


@pytest.mark.parametrize("activation", [F.gelu, partial(F.gelu, approximate="tanh"), F.relu, F.silu, torch.tanh], ids=lambda a: getattr(a, "__name__", "gelu_tanh"))
def test_mlp_on_cpu_is_the_eager_composition(activation):
    torch.manual_seed(3)
    m = mlp.Mlp(16, 48, activation=activation, return_residual=True)
    x = torch.randn(2, 5, 16)
    y, res = m(x)
    assert res is x
    assert torch.equal(y, m.fc2(activation(m.fc1(x))))


@pytest.mark.parametrize("activation", [F.sigmoid, F.silu, F.gelu, F.relu, torch.tanh], ids=lambda a: a.__name__)
def test_gated_mlp_on_cpu_is_the_eager_composition(activation):
    torch.manual_seed(4)
    m = mlp.GatedMlp(16, 40, activation=activation, multiple_of=8)
    x = torch.randn(2, 5, 16)
    up, gate = m.fc1(x).chunk(2, dim=-1)
    assert torch.allclose(m(x), m.fc2(up * activation(gate)), rtol=1e-6, atol=1e-6)


def test_fused_mlp_and_reference_names_on_cpu():
    torch.manual_seed(5)
    m = D.FusedMLP(16, 48, return_residual=True)
    x = torch.randn(7, 16)
    y, res = m(x)
    assert res is x and torch.allclose(y, m.fc2(F.gelu(m.fc1(x), approximate="tanh")))
    g, b = torch.randn(7, 16), torch.randn(16)
    dy, db = A.bias_gelu_back(g, x, b)
    ry, rb = A.act_grad_ref(g, x, "gelu_tanh", b)
    assert torch.equal(dy, ry) and torch.allclose(db, rb)
    assert torch.equal(A.swiglu(x, g), F.silu(x) * g) and torch.equal(A.sqrelu_fwd(x), F.relu(x) ** 2)
    assert torch.equal(A.relu_bwd(g, x), torch.where(x > 0, g, torch.zeros_like(g)))
