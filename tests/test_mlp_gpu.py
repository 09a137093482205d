"""GPU tests of modules.mlp (Mlp, GatedMlp) and ops.fused_dense (FusedMLP, FusedDense): outputs and all parameter gradients
against the same weights run as the eager composition in a wider dtype, by the inequality of tests/test_norm_gpu.py with its
constants -- max|ours - ref| <= 2 max|eager_same_dtype - ref| + atol --, the three checkpoint levels among themselves bit
for bit, the residual, the eager path of an activation the kernels do not know, and the memory a checkpoint level saves."""
import copy
from functools import partial

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, FP32 = torch.bfloat16, torch.float32
EAGER = {"gelu_approx": partial(F.gelu, approximate="tanh"), "relu": F.relu, "sqrelu": lambda t: F.relu(t).square()}


def atol_of(dtype):
    return 5e-2 if dtype == BF16 else 1e-4


def accept(name, ours, pt, ref, atol):
    """max|ours - ref_upcast| <= 2 max|ref_in_dtype - ref_upcast| + atol"""
    err = (ours.double() - ref.double()).abs().max().item()
    base = (pt.double() - ref.double()).abs().max().item()
    print(f"{name}: err {err:.3e} bound 2 * {base:.3e} + {atol:g}")
    assert err <= 2 * base + atol, f"{name}: {err} > 2 * {base} + {atol}"


def step(module, x, d, forward=None):
    """(out, dx, parameter gradients by name) of one forward + backward"""
    x = x.detach().requires_grad_(True)
    module.zero_grad()
    out = (forward or module)(x)
    out = out[0] if isinstance(out, tuple) else out
    out.backward(d.to(out.dtype))
    return [out.detach(), x.grad] + [p.grad for _, p in sorted(module.named_parameters())]


def compare(module, eager_forward, dtype):
    """module in `dtype` against eager_forward(module_copy, x) in the same dtype and in the wider one"""
    torch.manual_seed(0)
    x = torch.randn(2, 19, 64, device=DEV, dtype=dtype)
    d = torch.randn(2, 19, 64, device=DEV, dtype=dtype)
    wide = FP32 if dtype == BF16 else torch.float64
    ref_module = copy.deepcopy(module).to(wide)
    ours = step(module, x, d)
    same = step(module, x, d, lambda t: eager_forward(module, t))
    ref = step(ref_module, x.to(wide), d.to(wide), lambda t: eager_forward(ref_module, t))
    names = ["out", "dx"] + [n for n, _ in sorted(module.named_parameters())]
    for n, o, s, r in zip(names, ours, same, ref):
        accept(n, o, s, r, atol_of(dtype))
    return ours


@pytest.mark.parametrize("dtype", [BF16, FP32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("biases", [True, False], ids=["biases", "nobias"])
@pytest.mark.parametrize("activation", sorted(EAGER))
def test_fused_mlp_at_every_checkpoint_level(activation, biases, dtype):
    from flash_attention_annotated_amd.ops.fused_dense import FusedMLP
    torch.manual_seed(1)
    base = FusedMLP(64, 256, bias1=biases, bias2=biases, activation=activation, device=DEV, dtype=dtype)
    eager = lambda m, t: m.fc2(EAGER[activation](m.fc1(t)))  # noqa: E731
    results = []
    for lvl in (0, 1, 2):
        m = copy.deepcopy(base)
        m.checkpoint_lvl = lvl
        results.append(compare(m, eager, dtype))
    for other in results[1:]:  # the three levels: the same bits
        for a, b in zip(results[0], other):
            assert torch.equal(a, b)


@pytest.mark.parametrize("dtype", [BF16, FP32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("activation", [F.gelu, partial(F.gelu, approximate="tanh"), F.relu, F.silu, torch.tanh],
                         ids=["gelu", "gelu_tanh", "relu", "silu", "tanh_eager"])
def test_mlp(activation, dtype):
    from flash_attention_annotated_amd.modules.mlp import Mlp
    torch.manual_seed(2)
    m = Mlp(64, 256, activation=activation, device=DEV, dtype=dtype)
    ours = compare(m, lambda mod, t: mod.fc2(activation(mod.fc1(t))), dtype)
    if activation is torch.tanh:  # the eager path: the composition itself
        x = torch.randn(2, 19, 64, device=DEV, dtype=dtype)
        assert torch.equal(m(x), m.fc2(torch.tanh(m.fc1(x))))
    assert ours[0].shape == (2, 19, 64)


@pytest.mark.parametrize("dtype", [BF16, FP32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("activation", [F.sigmoid, F.silu, F.gelu, F.relu, torch.tanh], ids=["sigmoid", "silu", "gelu", "relu", "tanh_eager"])
def test_gated_mlp(activation, dtype):
    from flash_attention_annotated_amd.modules.mlp import GatedMlp
    torch.manual_seed(3)
    m = GatedMlp(64, hidden_features=130, activation=activation, multiple_of=64, device=DEV, dtype=dtype)
    assert m.fc1.out_features == 2 * 192

    def eager(mod, t):  # the reference's half order: value first, gate second
        y, gate = mod.fc1(t).chunk(2, dim=-1)
        return mod.fc2(y * activation(gate))
    compare(m, eager, dtype)


def test_return_residual_is_x_itself():
    from flash_attention_annotated_amd.modules.mlp import GatedMlp, Mlp
    from flash_attention_annotated_amd.ops.fused_dense import FusedDense, FusedMLP
    x = torch.randn(2, 19, 64, device=DEV, dtype=BF16)
    for m in (Mlp(64, 256, return_residual=True, device=DEV, dtype=BF16), GatedMlp(64, return_residual=True, device=DEV, dtype=BF16),
              FusedMLP(64, 256, return_residual=True, device=DEV, dtype=BF16), FusedDense(64, 32, return_residual=True, device=DEV, dtype=BF16)):
        out, res = m(x)
        assert res is x and out.shape[:-1] == x.shape[:-1]
    dense = FusedDense(64, 32, device=DEV, dtype=BF16)
    assert torch.equal(dense(x), F.linear(x, dense.weight, dense.bias))


def test_checkpoint_level_1_saves_the_activation_output():
    """torch.cuda.max_memory_allocated over a forward + backward of FusedMLP at M = 4096, in = 256, hidden 1024 (bf16) is
    strictly lower at level 1 than at level 0, by at least M * hidden * 2 bytes: the one saved tensor, a derived figure.  The
    measure is taken on two FusedMLP layers in sequence.  In the backward of a single layer the one fa_act_bwd call has pre,
    dout, dpre and the activation output alive at either level, saved or recomputed, so a lone layer's peak is the same
    (69733376 bytes at both levels on an MI355X); what a level saves is the activation output of every other layer while
    one layer's backward runs, and the peak of two layers shows exactly one such tensor."""
    from flash_attention_annotated_amd.ops.fused_dense import FusedMLP
    torch.manual_seed(4)
    m_rows, hidden = 4096, 1024
    base = torch.nn.Sequential(FusedMLP(256, hidden, device=DEV, dtype=BF16), FusedMLP(256, hidden, device=DEV, dtype=BF16))
    x = torch.randn(m_rows, 256, device=DEV, dtype=BF16)
    d = torch.randn(m_rows, 256, device=DEV, dtype=BF16)
    peak = {}
    for lvl in (0, 1):
        m = copy.deepcopy(base)
        for layer in m:
            layer.checkpoint_lvl = lvl
        step(m, x, d)  # (warm: the GEMM workspaces exist)
        m.zero_grad()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        leaf = x.detach().requires_grad_(True)
        m(leaf).backward(d)
        torch.cuda.synchronize()
        peak[lvl] = torch.cuda.max_memory_allocated() - before
        print(f"level {lvl}: peak {peak[lvl]}")
        del leaf, m
    assert peak[0] - peak[1] >= m_rows * hidden * 2
