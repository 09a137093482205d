"""GPU tests of the GEMM with a fused bias + activation epilogue (csrc/fa_gemm_act.hip through ops/triton/linear.py and
ops/triton/mlp.py).

The parity contract, for out, act_input, grad_in and dbias, over every element:
    max|ours - ref64| <= 2 * max|eager - ref64| + 1e-5,   and max|eager - ref64| > 0
ref64 is the same computation in fp64 from the 16-bit inputs; eager is the same computation in torch in the 16-bit dtype on the
GPU (F.linear, the torch activation, autograd for the gradient).  Inputs are seeded: x ~ N(0, 1), W ~ N(0, 1) / sqrt(K),
bias ~ N(0, 1).  Every case of tests/gemm_act_plan_universe.py is launched in both directions and both dtypes, and checked
against the plan the binding reports, so every instantiation runs: {fwd, dgrad} x {fp16, bf16} x {64, 128}-row tile, and the
dbias reduce."""
import pytest
import torch
import torch.nn.functional as F

import gemm_act_plan_universe as U

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = (torch.bfloat16, torch.float16)
ACTS = {"id": lambda t: t, "gelu": F.gelu, "gelu_approx": lambda t: F.gelu(t, approximate="tanh"),
        "squared_relu": lambda t: F.relu(t).square(), "relu": F.relu}
NAMES = ("id", "gelu", "gelu_approx", "squared_relu", "relu")
ACT_CODE_NAME = {"id": "identity", "gelu": "gelu_erf", "gelu_approx": "gelu_tanh", "squared_relu": "sqrelu", "relu": "relu"}


def L():
    from flash_attention_annotated_amd.ops.triton import linear
    return linear


def hold(name, ours, eager, ref64):
    """the parity contract on every element"""
    assert ours.shape == ref64.shape == eager.shape, (name, ours.shape, ref64.shape)
    err = (ours.double() - ref64).abs().max().item()
    base = (eager.double() - ref64).abs().max().item()
    print(f"{name}: ours {err:.3e} eager {base:.3e}")
    assert base > 0, name
    assert err <= 2 * base + 1e-5, (name, err, base)


def inputs(m, n, k, dtype, seed, bias=True, x_pitch=None):
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn(m, x_pitch or k, device=DEV, generator=g).to(dtype)[:, :k]
    w = (torch.randn(n, k, device=DEV, generator=g) / k ** 0.5).to(dtype)
    b = torch.randn(n, device=DEV, generator=g).to(dtype) if bias else None
    return x, w, b


def check_forward(x, w, b, activation, save_act_input=True):
    lin = L()
    got = lin.triton_linear_act(x, w, b, activation, save_act_input)
    out, act_input = got if save_act_input else (got, None)
    s64 = F.linear(x.double(), w.double(), None if b is None else b.double())
    s16 = F.linear(x, w, b)
    hold(f"out[{activation}]", out, ACTS[activation](s16), ACTS[activation](s64))
    if save_act_input:
        hold("act_input", act_input, s16, s64)
    return out, act_input


def check_dgrad(go, w2, act_input, activation, want_dbias):
    """w2 (K, N); act_input (M, N) in the 16-bit dtype"""
    lin = L()
    grad_in, dbias = lin.gemm_act_dgrad(go, w2, activation, act_input, want_dbias)
    pre64 = act_input.double().requires_grad_(True)
    (ref,) = torch.autograd.grad(ACTS[activation](pre64), pre64, go.double() @ w2.double())
    pre16 = act_input.clone().requires_grad_(True)
    (eager,) = torch.autograd.grad(ACTS[activation](pre16), pre16, go @ w2)
    hold(f"grad_in[{activation}]", grad_in, eager, ref)
    if want_dbias:
        rows = eager.reshape(-1, eager.shape[-1])
        hold("dbias", dbias, rows.sum(dim=0), ref.reshape(-1, ref.shape[-1]).sum(dim=0))
    else:
        assert dbias is None
    return grad_in, dbias


# ---- the universe: every fused cell, both directions, both dtypes -----------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("case", list(enumerate(U.CASES)), ids=lambda c: "x".join(map(str, c[1])))
def test_universe_forward(case, dtype):
    i, (m, n, k) = case
    activation = NAMES[i % len(NAMES)]
    x, w, b = inputs(m, n, k, dtype, seed=100 + i)
    plan = L()._plan_linear_act(x, w, b, activation, True)
    assert plan.pop("form") == "fused" == U.form(m, n, k)
    assert plan.pop("dgrad") == 0 and plan.pop("dtype") == (1 if dtype == torch.bfloat16 else 0)
    assert U.Plan(**plan) == U.plan(m, n, k)
    check_forward(x, w, b, activation)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("case", list(enumerate(U.CASES)), ids=lambda c: "x".join(map(str, c[1])))
def test_universe_dgrad(case, dtype):
    """grad_out (M, K) @ weight (K, N): the case's N is the width of the result, its K the depth, as in the forward"""
    i, (m, n, k) = case
    # (the 8 elements of (1, 8, 8) get a gelu: with a relu form all of act_input may be negative, and the bound vacuous)
    activation = NAMES[(i + 1) % len(NAMES)]
    g = torch.Generator(device=DEV).manual_seed(200 + i)
    go = torch.randn(m, k, device=DEV, generator=g).to(dtype)
    w2 = (torch.randn(k, n, device=DEV, generator=g) / k ** 0.5).to(dtype)
    act_input = torch.randn(m, n, device=DEV, generator=g).to(dtype)
    plan = L()._plan_dgrad_act(go, w2, activation, act_input, True)
    assert plan.pop("form") == "fused"
    assert plan.pop("dgrad") == 1 and plan.pop("dtype") == (1 if dtype == torch.bfloat16 else 0)
    assert U.Plan(**plan) == U.plan(m, n, k, dbias=True)
    check_dgrad(go, w2, act_input, activation, True)


# ---- forward: activations, bias, save_act_input, layouts ---------------------------------------------------------------------------
@pytest.mark.parametrize("activation", NAMES)
@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
def test_forward_every_activation(activation, bias):
    x, w, b = inputs(129, 264, 72, torch.bfloat16, seed=7, bias=bias)
    out, _ = check_forward(x, w, b, activation, save_act_input=True)
    alone = L().triton_linear_act(x, w, b, activation)  # (save_act_input=False: a tensor, the same bits)
    assert isinstance(alone, torch.Tensor) and torch.equal(alone, out)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_forward_strided_and_batched(dtype):
    x, w, b = inputs(300, 128, 200, dtype, seed=8, x_pitch=208)  # row stride K + 8
    assert x.stride() == (208, 1)
    out, act_input = check_forward(x, w, b, "gelu_approx")
    same, same_in = L().triton_linear_act(x.contiguous(), w, b, "gelu_approx", True)
    assert torch.equal(out, same) and torch.equal(act_input, same_in)
    x3 = x.contiguous().reshape(3, 100, 200)  # leading dims are flattened and restored
    out3, act3 = L().triton_linear_act(x3, w, b, "gelu_approx", True)
    assert out3.shape == act3.shape == (3, 100, 128)
    assert torch.equal(out3.reshape(300, 128), out) and torch.equal(act3.reshape(300, 128), act_input)
    # a view whose base is not 16-byte aligned is copied, not refused
    xo = torch.randn(300 * 200 + 1, device=DEV).to(dtype)[1:].reshape(300, 200)
    assert xo.data_ptr() % 16
    assert L()._plan_linear_act(xo, w, b)["form"] == "fused"
    assert torch.equal(L().triton_linear_act(xo, w, b), L().triton_linear_act(xo.clone(), w, b))
    # a transposed weight (neither stride is 1 after the slice) is copied, as in the reference
    wt = torch.randn(200, 256, device=DEV).to(dtype).t()[::2]
    assert torch.equal(L().triton_linear_act(x, wt, b), L().triton_linear_act(x, wt.contiguous(), b))


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("activation", NAMES)
def test_activation_math_is_that_of_the_activation_kernels(activation, dtype):
    """W = I: the fp32 sum is x itself, so out must have the bits of the activation kernel on x."""
    from flash_attention_annotated_amd.ops import activations as A
    g = torch.Generator(device=DEV).manual_seed(9)
    x = (torch.randn(300, 128, device=DEV, generator=g) * 3).to(dtype)
    eye = torch.eye(128, device=DEV, dtype=dtype)
    out, act_input = L().triton_linear_act(x, eye, None, activation, True)
    assert torch.equal(act_input, x)
    assert torch.equal(out, A._act_fwd(x, None, None, A.ACTIVATIONS[ACT_CODE_NAME[activation]]))
    # ... and the derivative, through dgrad with the identity weight: (g · I) * act'(x)
    go = torch.randn(300, 128, device=DEV, generator=g).to(dtype)
    want = A._act_bwd(go, x, None, None, A.ACTIVATIONS[ACT_CODE_NAME[activation]], False, False, False)[0]
    assert torch.equal(L().triton_dgrad_act(go, eye, activation, x), want)


# ---- dgrad ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("activation", NAMES)
@pytest.mark.parametrize("want_dbias", [False, True], ids=["nodbias", "dbias"])
def test_dgrad_every_activation(activation, want_dbias):
    g = torch.Generator(device=DEV).manual_seed(11)
    go = torch.randn(300, 136, device=DEV, generator=g).to(torch.bfloat16)
    w2 = (torch.randn(136, 264, device=DEV, generator=g) / 136 ** 0.5).to(torch.bfloat16)
    act_input = torch.randn(300, 264, device=DEV, generator=g).to(torch.bfloat16)
    grad_in, dbias = check_dgrad(go, w2, act_input, activation, want_dbias)
    again, dbias2 = L().gemm_act_dgrad(go, w2, activation, act_input, want_dbias)
    assert torch.equal(grad_in, again)
    if want_dbias:
        assert torch.equal(dbias, dbias2)  # no atomics: the same bits
    assert torch.equal(L().triton_dgrad_act(go, w2, activation, act_input), grad_in)


def test_dgrad_identity_is_a_plain_mm():
    g = torch.Generator(device=DEV).manual_seed(12)
    go = torch.randn(2, 150, 200, device=DEV, generator=g).to(torch.float16)
    w2 = (torch.randn(200, 128, device=DEV, generator=g) / 200 ** 0.5).to(torch.float16)
    grad = L().triton_dgrad_act(go, w2)  # (no act_input)
    assert grad.shape == (2, 150, 128)
    hold("grad_in[id] vs mm", grad, go @ w2, go.double() @ w2.double())


# ---- a large extent: more than 2^31 elements, 64-bit row bases -----------------------------------------------------------------------
def test_large_extent():
    m, n, k = (1 << 28) + 128, 8, 8
    g = torch.Generator(device=DEV).manual_seed(13)
    x = torch.randn(m, k, device=DEV, generator=g, dtype=torch.bfloat16)
    w = (torch.randn(n, k, device=DEV, generator=g) / k ** 0.5).to(torch.bfloat16)
    b = torch.randn(n, device=DEV, generator=g).to(torch.bfloat16)
    assert x.numel() > 1 << 31
    plan = L()._plan_linear_act(x, w, b, "gelu", True)
    assert plan["form"] == "fused" and plan["tiles_m"] == (1 << 21) + 1 and plan["ragged_m"] == 0
    out, act_input = L().triton_linear_act(x, w, b, "gelu", True)
    rows = torch.cat([torch.arange(0, m, 65537, device=DEV), torch.arange(m - 128, m, device=DEV)])
    xs = x[rows]
    s64 = F.linear(xs.double(), w.double(), b.double())
    s16 = F.linear(xs, w, b)
    hold("large out", out[rows], F.gelu(s16), F.gelu(s64))
    hold("large act_input", act_input[rows], s16, s64)
    del out
    # dgrad at the same extent: grad_out = x, weight (K, N) = w
    grad_in = L().triton_dgrad_act(x, w, "gelu", act_input)
    pre64 = act_input[rows].double().requires_grad_(True)
    (ref,) = torch.autograd.grad(F.gelu(pre64), pre64, xs.double() @ w.double())
    pre16 = act_input[rows].clone().requires_grad_(True)
    (eager,) = torch.autograd.grad(F.gelu(pre16), pre16, xs @ w)
    hold("large grad_in", grad_in[rows], eager, ref)


# ---- the module ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_module(dtype):
    from flash_attention_annotated_amd.ops.triton.mlp import FusedDenseSqreluDense
    m, d_in, hidden = 300, 128, 264
    torch.manual_seed(14)
    mod = FusedDenseSqreluDense(d_in, hidden, device=DEV, dtype=dtype)
    with torch.no_grad():
        mod.fc1.bias.normal_()
        mod.fc2.bias.normal_()
    params = [mod.fc1.weight, mod.fc1.bias, mod.fc2.weight, mod.fc2.bias]
    x = torch.randn(m, d_in, device=DEV).to(dtype)
    go = torch.randn(m, d_in, device=DEV).to(dtype)

    def composition(cast):
        xr = cast(x).detach().requires_grad_(True)
        w1, b1, w2, b2 = (cast(p).detach().requires_grad_(True) for p in params)
        out = F.linear(F.relu(F.linear(xr, w1, b1)).square(), w2, b2)
        return (out, *torch.autograd.grad(out, (xr, w1, b1, w2, b2), cast(go)))

    ref, eager = composition(lambda t: t.float()), composition(lambda t: t)
    results = []
    for lvl in (0, 1, 2):
        mod.checkpoint_lvl = lvl
        xr = x.clone().requires_grad_(True)
        out = mod(xr)
        results.append((out, *torch.autograd.grad(out, (xr, *params), go)))
    for name, ours, e, r in zip(("out", "dx", "dw1", "db1", "dw2", "db2"), results[0], eager, ref):
        hold(f"module {name}", ours, e, r.double())
    for lvl in (1, 2):
        for a, b in zip(results[0], results[lvl]):
            assert torch.equal(a, b), lvl


# ---- the runtime ---------------------------------------------------------------------------------------------------------------
def test_no_rows():
    x, w, b = inputs(0, 128, 64, torch.bfloat16, seed=15)
    out, act_input = L().triton_linear_act(x, w, b, "gelu", True)
    assert out.shape == act_input.shape == (0, 128)
    go, w2 = torch.empty(0, 64, device=DEV, dtype=torch.bfloat16), w.t().contiguous()  # (K, N) = (64, 128)
    grad, dbias = L().gemm_act_dgrad(go, w2, "gelu", act_input, want_dbias=True)
    assert grad.shape == (0, 128) and dbias.shape == (128,) and not dbias.any()


def test_graph_capture_and_replay():
    lin = L()
    x, w, b = inputs(300, 264, 200, torch.bfloat16, seed=16)
    go = torch.randn(300, 200, device=DEV).to(torch.bfloat16)
    w2 = w.t().contiguous()  # (K, N) = (200, 264)

    def step():
        out, act_input = lin.triton_linear_act(x, w, b, "squared_relu", True)
        grad, dbias = lin.gemm_act_dgrad(go, w2, "squared_relu", act_input, True)
        return out, act_input, grad, dbias

    want = step()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = step()
    for t in got:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for g, wnt in zip(got, want):
        assert torch.equal(g, wnt)


def test_compile_fullgraph():
    lin = L()
    x, w, b = inputs(129, 264, 72, torch.float16, seed=17)

    def step(x, w, b):
        out, act_input = lin.triton_linear_act(x, w, b, "gelu_approx", True)
        return out, act_input, lin.triton_dgrad_act(out, w, "gelu_approx", x)  # ((129, 264) @ (264, 72), act_input (129, 72))

    got = torch.compile(step, fullgraph=True, backend="aot_eager")(x, w, b)
    for g, wnt in zip(got, step(x, w, b)):
        assert torch.equal(g, wnt)


@pytest.mark.parametrize("shape", U.FALLBACK_CASES, ids=lambda c: "x".join(map(str, c)))
def test_refused_shapes_take_the_fallback(shape):
    m, n, k = shape
    x, w, b = inputs(m, n, k, torch.bfloat16, seed=18)
    assert L()._plan_linear_act(x, w, b, "gelu", True) == {"form": "mm_act"} and U.form(m, n, k) == "mm_act"
    check_forward(x, w, b, "gelu")
    g = torch.Generator(device=DEV).manual_seed(19)
    go = torch.randn(m, k, device=DEV, generator=g).to(torch.bfloat16)
    w2 = (torch.randn(k, n, device=DEV, generator=g) / k ** 0.5).to(torch.bfloat16)
    act_input = torch.randn(m, n, device=DEV, generator=g).to(torch.bfloat16)
    assert L()._plan_dgrad_act(go, w2, "gelu", act_input, True) == {"form": "mm_act"}
    check_dgrad(go, w2, act_input, "gelu", True)
