"""GPU tests of the fused MLP activations (csrc/fa_act.hip through ops/activations.py): every element of every output against
the fp64 oracle, over a seeded grid in which every activation meets every dtype in both forms, then layouts, views, sizes and
the runtime (autograd, torch.compile, graphs).

The element rule.  |ours - ref64| <= ulp_dtype(ref64) + C * S + tiny, for every element of every output, the probe row
included; fp32 outputs have no ulp term.  S is the magnitude of the operands of the last multiply: forward |act(x)| * |up|, or
|x| in the plain form; dup |act(gate)| * |dout|; backward A(x) * |dout| * |up|, where A is the magnitude of act' as it is
formed -- |act'| for relu, sqrelu, sigmoid and identity, and the sum of the magnitudes of its two summands for silu and both
gelu forms (s + x s (1 - s) dz, Phi + x phi).  A is |act'| itself wherever the summands have one sign; it differs near the zero
of act' (x = -1.28 for silu, -0.75 for gelu), where the summands cancel and no fp32 evaluation, eager's included, is
accurate relative to |act'|: with |act'| there the rule would refuse every order of fp32 roundings, which the rule is meant to
admit.  A is at most 1.2, so a wrong constant or a dropped term (errors of 1e-2 A and more) is far outside.  dbias:
ulp + C_DBIAS * sum_r (A |dout|) + tiny.
tiny = 2^-126 (1 + |f|), f the other factor of the last multiply (up, dout or up * dout; for dbias their sum): below the smallest
normal fp32 an fp32 intermediate has no relative accuracy (silu(-100) = -3.7e-42 in fp64 is -0 in eager fp32), and that
absolute error is then multiplied by f.
C is a constant per activation and output.  It was measured with this file: on every case of the grid, what torch's eager fp32 evaluation of the same
expression, rounded once to the dtype, needs under this rule on the elements where eager is sound -- finite, and within 2^-10
of the oracle relative to it, i.e. not underflowed, saturated or cancelled against a nonzero oracle value as eager's
1 + tanh, 1 + erf and 1 - sigmoid are in their tails; there the oracle alone decides, with the same bound.  Figures (MI355X):
see the table C_EAGER, one constant per activation and output.  Ours is allowed twice the eager figure.  Where the fp64 result rounded to the dtype is
infinite (sqrelu of the largest finite value) ours must be that infinity.

Which case reaches which kernel: 16-bit contiguous cases with H in 8 / 4096 / 11008 run act_fwd_kernel<8> / act_bwd_kernel<8>,
fp32 ones <4>; H in 1 / 203 (pitches that are no multiple of 16 bytes) and the offset views run <1>; every plain backward with
a bias runs act_dbias_reduce_kernel.  tests/test_act_forms_gpu.py asserts the forms by the plan."""
import itertools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
M = 37
HS = (1, 8, 203, 4096, 11008)
DTYPES = (torch.bfloat16, torch.float16, torch.float32)
NAMES = ("gelu_tanh", "gelu_erf", "relu", "sqrelu", "silu", "sigmoid", "identity")
MANT = {torch.bfloat16: 7, torch.float16: 10}
TINY = 2.0 ** -126
# C_EAGER[activation][output]: what eager fp32 needs on its sound elements, the largest figure over the cases of the grid,
# rounded up to two digits and at least 6.0e-8 (2^-24, the one rounding any fp32 evaluation has); measured on an MI355X by
# running the grid with hold() printing, as it does in every run.  Beside each row: what ours needed on ALL elements, the
# probes included (out / dpre / dgate / dup).  Ours is allowed twice the eager figure.  The figures near 9.8e-4 are the
# soundness threshold 2^-10 itself: eager's 1 + tanh, 1 + erf and 1 - sigmoid lose accuracy steadily into their tails, so its
# figure is set by where it is cut off; ours stays at 1.7e-5 and below there (an fp32 exp of z has a relative error of
# |z| 2^-24, so no fp32 evaluation keeps 1e-7 in the tails).  sigmoid and sqrelu "out": S is |x| by the rule, which says
# little for sigmoid(x) at x = 2^-20 and x^2 at x = 1e4; eager and ours need the same there.
C_EAGER = {
    "gelu_tanh": {"out": 9.8e-04, "dpre": 9.1e-04, "dgate": 9.1e-04, "dup": 9.8e-04},  # ours 5.0e-06 / 1.7e-05 / 5.0e-06 / 5.0e-06
    "gelu_erf": {"out": 9.8e-04, "dpre": 9.2e-04, "dgate": 9.2e-04, "dup": 9.8e-04},  # ours 2.1e-06 / 7.1e-07 / 8.2e-07 / 2.1e-06
    "relu": {"out": 6.0e-08, "dpre": 6.0e-08, "dgate": 6.0e-08, "dup": 6.0e-08},  # ours 5.8e-08 / 0.0e+00 / 5.9e-08 / 5.9e-08
    "sqrelu": {"out": 1.2e-03, "dpre": 1.2e-07, "dgate": 1.2e-07, "dup": 1.2e-07},  # ours 1.2e-03 / 1.1e-07 / 1.1e-07 / 1.1e-07
    "silu": {"out": 2.0e-07, "dpre": 7.2e-07, "dgate": 7.3e-07, "dup": 2.0e-07},  # ours 2.4e-07 / 5.1e-07 / 3.0e-07 / 2.6e-07
    "sigmoid": {"out": 7.6e-04, "dpre": 9.8e-04, "dgate": 7.9e-04, "dup": 1.5e-07},  # ours 7.5e-04 / 7.4e-07 / 1.8e-07 / 9.7e-08
    "identity": {"out": 6.0e-08, "dpre": 6.0e-08, "dgate": 6.0e-08, "dup": 6.0e-08},  # ours 5.7e-08 / 0.0e+00 / 5.5e-08 / 5.9e-08
}
# dbias: a sum of M fp32 terms in any order is within (M - 1) 2^-24 of the sum of their magnitudes, each term within 2^-24 of
# it: M 2^-24 in all.  Eager's tree order needed 1.4e-7 on these cases where a sequential order, as valid, needed 3.1e-7.
C_DBIAS = M * 2.0 ** -24


def A():
    from flash_attention_annotated_amd.ops import activations
    return activations


def probes(dtype):
    big = torch.finfo(dtype).max
    vals = [0.0, -0.0]
    for v in (2.0 ** -20, 1.0, 10.0, 100.0, 1e4, big):
        vals += [v, -v]
    return torch.tensor(vals, dtype=torch.float64).to(dtype)


def make_input(h, dtype, gen):
    x = (3 * torch.randn(M, h, generator=gen, dtype=torch.float32)).to(dtype)
    p = probes(dtype)
    x[0] = p.repeat(-(-h // p.numel()))[:h]
    return x.to(DEV)


def ulp(ref, dtype):
    if dtype == torch.float32:
        return torch.zeros_like(ref)
    _, e = torch.frexp(ref.abs())
    fi = torch.finfo(dtype)
    return torch.clamp(torch.ldexp(torch.ones_like(ref), e - 1 - MANT[dtype]), min=fi.tiny * 2.0 ** -MANT[dtype])


def oracle(x, name):
    """(act(x), act'(x), A(x)) in fp64, written out here and not taken from the package: A is the magnitude of act' as it is
    formed (module docstring).  sigmoid(-z) stands for 1 - sigmoid(z) and erfc for 1 + erf, so that the tails keep their
    relative accuracy, which torch's own fp64 gelu and its autograd (1 + tanh, 1 - tanh^2) do not"""
    s, zero = torch.sigmoid, torch.zeros_like(x)
    if name == "gelu_tanh":
        k, c = math.sqrt(2.0 / math.pi), 0.044715
        z = 2 * k * x * (1 + c * x * x)
        w = s(z) * s(-z)
        t = torch.where(w > 0, x * w * 2 * k * (1 + 3 * c * x * x), zero)  # (0 * inf in the limit: the first factor decides)
        return x * s(z), s(z) + t, s(z) + t.abs()
    if name == "gelu_erf":
        phi, t = 0.5 * torch.erfc(-x / math.sqrt(2.0)), x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)
        return x * phi, phi + t, phi + t.abs()
    if name == "silu":
        t = x * (s(x) * s(-x))
        return x * s(x), s(x) + t, s(x) + t.abs()
    if name == "sigmoid":
        return s(x), s(x) * s(-x), s(x) * s(-x)
    if name == "relu":
        return torch.relu(x), (x > 0).double(), (x > 0).double()
    if name == "sqrelu":
        return torch.relu(x) ** 2, 2 * torch.relu(x), 2 * torch.relu(x)
    return x, torch.ones_like(x), torch.ones_like(x)


FIGURES = {}  # (activation, output) -> (eager's c on its sound elements, ours on all), the largest seen in this run


def hold(name, ours, eager32, ref, scale, dtype, factor, c=None):
    """the element rule of the module docstring on one output; name: `<activation> <output>`"""
    c = 2 * C_EAGER[name.split()[0]][name.split()[1]] if c is None else c
    assert not torch.isnan(ours).any(), f"{name}: NaN from finite inputs"
    rounded = ref.to(dtype)
    inf = torch.isinf(rounded)
    assert torch.equal(ours[inf], rounded[inf]), f"{name}: an overflow of the oracle is not the same infinity"
    fin = ~inf
    r, u, s = ref[fin], ulp(ref, dtype)[fin], scale[fin]
    tiny = TINY * (1 + (factor.expand_as(ref)[fin] if torch.is_tensor(factor) else factor))
    eager = eager32.to(dtype).double()[fin]
    e_err = (eager - r).abs()
    sound = torch.isfinite(eager) & (s > 0) & (e_err <= 2.0 ** -10 * r.abs() + u + tiny)
    need = ((e_err - u - tiny).clamp(min=0) / s.clamp(min=1e-300))[sound]
    c_eager = need.max().item() if need.numel() else 0.0
    err = (ours.double()[fin] - r).abs()
    c_ours = ((err - u - tiny).clamp(min=0) / s.clamp(min=1e-300))[s > 0]
    c_ours = c_ours.max().item() if c_ours.numel() else 0.0
    key = tuple(name.split())
    FIGURES[key] = tuple(max(a, b) for a, b in zip(FIGURES.get(key, (0.0, 0.0)), (c_eager, c_ours)))
    print(f"{name}: c eager (sound elements) {c_eager:.3e} ours (all elements) {c_ours:.3e} allowed {c:.3e}")
    bad = err > u + c * s + tiny
    assert not bad.any(), f"{name}: {int(bad.sum())} elements beyond ulp + {c:.3e} * S; worst c {c_ours:.3e}"


def run_case(name, dtype, h, form, bias_kind, recompute, gen):
    a = A()
    code = a.ACTIVATIONS[name]
    d = make_input(h, dtype, gen)
    d[0] = (3 * torch.randn(h, generator=gen)).to(dtype).to(DEV)  # (dout has no probes: a product with 0 is not an overflow)
    if form == "plain":
        x = make_input(h, dtype, gen)
        bias = None if bias_kind is None else torch.randn(h, generator=gen).to(bias_kind).to(DEV)
        out = a._act_fwd(x, None, bias, code)
        dpre, _, dbias, again = a._act_bwd(d, x, None, bias, code, bias is not None, recompute, False)
        x64 = x.double() if bias is None else x.double() + bias.double()
        x32 = (x.float() if bias is None else x.float() + bias.float()).requires_grad_(True)
        y32 = a._apply(x32, code)
        (g32,) = torch.autograd.grad(y32, x32, d.float())
        y64, der64, mag64 = oracle(x64, name)
        dref, s_bwd = der64 * d.double(), mag64 * d.double().abs()
        hold(f"{name} out", out, y32.detach(), y64, x64.abs(), dtype, 0.0)
        hold(f"{name} dpre", dpre, g32, dref, s_bwd, dtype, d.double().abs())
        if bias is not None:
            assert dbias.dtype == bias.dtype and dbias.shape == (h,)
            hold(f"{name} dbias", dbias, g32.sum(dim=0), dref.sum(dim=0), s_bwd.sum(dim=0), bias.dtype, d.double().abs().sum(dim=0), C_DBIAS)
    else:
        x12 = make_input(2 * h, dtype, gen)
        x12[0, :h] = x12[0, h:]  # (the probes meet themselves: max * max, not max * 2^-20)
        up, gate = x12[:, :h], x12[:, h:]
        if form == "two":
            up, gate = up.contiguous(), gate.contiguous()
        out = a._act_fwd(gate, up, None, code)
        dgate, dup, _, again = a._act_bwd(d, gate, up, None, code, False, recompute, False)
        g64, u64, d64 = gate.double(), up.double(), d.double()
        g32, u32 = gate.float().requires_grad_(True), up.float().requires_grad_(True)
        y32 = a._apply(g32, code) * u32
        dg32, du32 = torch.autograd.grad(y32, (g32, u32), d.float())
        act64, der64, mag64 = oracle(g64, name)
        dg64, du64 = der64 * (u64 * d64), act64 * d64
        hold(f"{name} out", out, y32.detach(), act64 * u64, (act64 * u64).abs(), dtype, u64.abs())
        hold(f"{name} dgate", dgate, dg32, dg64, mag64 * (u64 * d64).abs(), dtype, (u64 * d64).abs())
        hold(f"{name} dup", dup, du32, du64, (act64 * d64).abs(), dtype, d64.abs())
        if form == "packed":  # one gradient tensor, its halves the two gradients bit for bit
            dx12, none, _, _ = a._act_bwd(d, gate, up, None, code, False, False, True)
            assert dx12.shape == (M, 2 * h) and none.numel() == 0
            assert torch.equal(dx12[:, :h], dup) and torch.equal(dx12[:, h:], dgate)
    if recompute:
        assert torch.equal(again, out), "recompute_out is not the forward's bits"
    else:
        assert again.numel() == 0


def grid():
    """every activation in every dtype, in both forms; the other axes cycle so that every value of each occurs"""
    hs, plain, gated, rec = itertools.cycle(HS), itertools.cycle((None, "same", torch.float32, "same")), itertools.cycle(("packed", "two")), itertools.cycle((True, False, False, True, True))
    cases = []
    for name in NAMES:
        for dtype in DTYPES:
            b = next(plain)
            cases.append((name, dtype, next(hs), "plain", dtype if b == "same" else b, next(rec)))
            cases.append((name, dtype, next(hs), next(gated), None, next(rec)))
    return cases


GRID = grid()


def test_grid_covers_every_axis():
    assert {(c[0], c[1], c[3] == "plain") for c in GRID} == {(n, d, p) for n in NAMES for d in DTYPES for p in (True, False)}
    assert {c[2] for c in GRID} == set(HS) and {c[3] for c in GRID} == {"plain", "packed", "two"} and {c[5] for c in GRID} == {True, False}
    assert any(c[4] is None and c[3] == "plain" for c in GRID) and any(c[4] == torch.float32 and c[1] != torch.float32 for c in GRID)
    assert any(c[4] == c[1] and c[1] != torch.float32 for c in GRID)


@pytest.mark.parametrize("case", GRID, ids=[f"{c[0]}-{str(c[1])[6:]}-H{c[2]}-{c[3]}-{'nobias' if c[4] is None else 'bias_' + str(c[4])[6:]}-{'rec' if c[5] else 'norec'}" for c in GRID])
def test_elements_against_the_fp64_oracle(case):
    gen = torch.Generator().manual_seed(GRID.index(case))
    run_case(*case, gen)


def test_strided_views_and_mixed_phase():
    """inputs that are offset views of wider buffers: the columns around them are not touched, the plan says elements, and
    the results are those of the contiguous call bit for bit"""
    a = A()
    gen = torch.Generator().manual_seed(100)
    h, code = 203, a.SILU
    for dtype in (torch.bfloat16, torch.float32):
        wide = make_input(2 * h + 10, dtype, gen)
        keep = wide.clone()
        gate, up = wide[:, 3:3 + h], wide[:, 5 + h:5 + 2 * h]
        d = make_input(h + 8, dtype, gen)[:, 1:1 + h]
        assert a._plan_forward(gate, up, None, code)["cw"] == 1 and a._plan_backward(d, gate, up, None, code)["cw"] == 1
        out = a._act_fwd(gate, up, None, code)
        dgate, dup, _, again = a._act_bwd(d, gate, up, None, code, False, True, False)
        assert torch.equal(wide, keep)
        g, u, dc = gate.contiguous(), up.contiguous(), d.contiguous()
        assert torch.equal(out, a._act_fwd(g, u, None, code)) and torch.equal(again, out)
        rg, ru, _, _ = a._act_bwd(dc, g, u, None, code, False, False, False)
        assert torch.equal(dgate, rg) and torch.equal(dup, ru)
        # the plain form with its bias at another phase than pre: an aligned pre, a bias one element off
        x, bias = make_input(4096, dtype, gen), torch.randn(4097, generator=gen).to(dtype).to(DEV)[1:]
        assert a._plan_forward(x, None, bias, code)["cw"] == 1 and a._plan_forward(x, None, bias.clone(), code)["cw"] == 16 // x.element_size()
        assert torch.equal(a._act_fwd(x, None, bias, code), a._act_fwd(x, None, bias.clone(), code))


def test_one_row_and_no_rows():
    a = A()
    gen = torch.Generator().manual_seed(101)
    x, d, bias = make_input(203, torch.bfloat16, gen), make_input(203, torch.bfloat16, gen), torch.randn(203, device=DEV)
    full = a._act_fwd(x, None, bias, a.GELU_TANH)
    assert torch.equal(a._act_fwd(x[5:6], None, bias, a.GELU_TANH), full[5:6])
    dpre, _, dbias, _ = a._act_bwd(d[5:6], x[5:6], None, bias, a.GELU_TANH, True, False, False)
    assert torch.allclose(dbias, dpre[0].float(), rtol=2 ** -7, atol=1e-30)  # (one row: its unrounded dpre)
    out = a._act_fwd(x[:0], None, bias, a.GELU_TANH)
    dpre, dup, dbias, again = a._act_bwd(d[:0], x[:0], None, bias, a.GELU_TANH, True, True, False)
    assert out.shape == (0, 203) and dpre.shape == (0, 203) and again.shape == (0, 203) and dup.numel() == 0
    assert dbias.shape == (203,) and not dbias.any()
    x12 = make_input(406, torch.bfloat16, gen)
    assert a.gated_act(x12[:0], "silu").shape == (0, 203)


def test_rows_past_2_31_elements():
    """a packed (16400, 2 * 65536) bf16 call: the last rows lie beyond element 2^31 of the input and of the gradient"""
    a = A()
    m, h = 16400, 65536
    assert (m - 1) * 2 * h > 2 ** 31
    gen = torch.Generator(device=DEV).manual_seed(102)
    x12 = torch.empty(m, 2 * h, dtype=torch.bfloat16, device=DEV).normal_(generator=gen)
    d = torch.empty(m, h, dtype=torch.bfloat16, device=DEV).normal_(generator=gen)
    out = a._act_fwd(x12[:, h:], x12[:, :h], None, a.SILU)
    dx12, _, _, _ = a._act_bwd(d, x12[:, h:], x12[:, :h], None, a.SILU, False, False, True)
    tail = slice(m - 19, m)
    ref_out = a.gated_act_ref(x12[tail].double(), a.SILU)
    ref_dx = a.gated_act_grad_ref(d[tail].double(), x12[tail].double(), a.SILU)
    assert torch.allclose(out[tail].double(), ref_out, rtol=2 ** -7, atol=1e-30)
    assert torch.allclose(dx12[tail].double(), ref_dx, rtol=2 ** -7, atol=1e-30)
    del out, dx12, x12, d
    torch.cuda.empty_cache()


def test_dbias_is_deterministic():
    a = A()
    gen = torch.Generator().manual_seed(103)
    x = (3 * torch.randn(4099, 203, generator=gen)).to(torch.bfloat16).to(DEV)
    d = torch.randn(4099, 203, generator=gen).to(torch.bfloat16).to(DEV)
    bias = torch.randn(203, device=DEV)
    first = a._act_bwd(d, x, None, bias, a.GELU_TANH, True, False, False)[2]
    again = a._act_bwd(d, x, None, bias, a.GELU_TANH, True, False, False)[2]
    assert torch.equal(first, again)
    ref = a.act_grad_ref(d.double(), x.double(), a.GELU_TANH, bias.double())[1]
    assert torch.allclose(first.double(), ref, rtol=1e-4, atol=1e-3)


def test_public_functions_by_autograd():
    """the autograd of the public functions against the oracle on an fp64 copy (no gradcheck: the kernels round to 16 bits)"""
    a = A()
    gen = torch.Generator().manual_seed(104)
    x = make_input(203, torch.bfloat16, gen)[1:].reshape(4, 9, 203)
    y = make_input(203, torch.bfloat16, gen)[1:].reshape(4, 9, 203)
    d = make_input(203, torch.bfloat16, gen)[1:].reshape(4, 9, 203)
    bias = torch.randn(203, device=DEV).to(torch.bfloat16)
    x12 = torch.cat([y, x], dim=-1)

    def grads(fn, *leaves, double=False):
        leaves = [(t.double() if double else t).detach().requires_grad_(True) for t in leaves]
        out = fn(*leaves)
        return (out, *torch.autograd.grad(out, leaves, d.double() if double else d))

    def same(ours, ref):
        for o, r in zip(ours, ref):
            assert o.shape == r.shape and torch.allclose(o.double(), r, rtol=2 ** -6, atol=2 ** -6 * r.abs().max().item()), (o.double() - r).abs().max()

    same(grads(lambda t, b: a.bias_gelu_impl(t, b), x, bias), grads(lambda t, b: a.act_ref(t, "gelu_tanh", b), x, bias, double=True))
    same(grads(a.fast_gelu_impl, x), grads(lambda t: a.act_ref(t, "gelu_tanh"), x, double=True))
    same(grads(a.swiglu, x, y), grads(lambda g, u: a.gated_act_ref(torch.cat([u, g], dim=-1), "silu"), x, y, double=True))
    for name in NAMES:
        same(grads(lambda t: a.act(t, name), x), grads(lambda t: a.act_ref(t, name), x, double=True))
        same(grads(lambda t: a.gated_act(t, name), x12), grads(lambda t: a.gated_act_ref(t, name), x12, double=True))
    # the forward-only and backward-only names
    same((a.gelu_fwd(x), a.gelu_bwd(d, x), a.relu_bwd(d, x), a.sqrelu_fwd(x), a.sqrelu_bwd(d, x), a.swiglu_fwd(x, y), a.bias_gelu(x, bias)),
         (a.act_ref(x.double(), "gelu_tanh"), a.act_grad_ref(d.double(), x.double(), "gelu_tanh")[0],
          a.act_grad_ref(d.double(), x.double(), "relu")[0], a.act_ref(x.double(), "sqrelu"), a.act_grad_ref(d.double(), x.double(), "sqrelu")[0],
          a.gated_act_ref(x12.double(), "silu"), a.act_ref(x.double(), "gelu_tanh", bias.double())))
    dx, dy = a.swiglu_bwd(x, y, d)
    ref = a.gated_act_grad_ref(d.double(), x12.double(), "silu")
    same((dy, dx), (ref[..., :203], ref[..., 203:]))
    gy, gb = a.bias_gelu_back(d, x, bias)
    ry, rb = a.act_grad_ref(d.double(), x.double(), "gelu_tanh", bias.double())
    assert gb.dtype == bias.dtype
    same((gy, gb), (ry, rb))


def test_compile_traces_forward_and_backward():
    a = A()
    gen = torch.Generator().manual_seed(105)
    x12, bias = make_input(2 * 203, torch.bfloat16, gen)[1:], torch.randn(203, device=DEV)

    def step(t, b):
        y = a.gated_act(t, "silu")
        return a.act(y, "gelu_tanh", b).float().square().sum()

    def run(fn):
        t, b = x12.detach().requires_grad_(True), bias.detach().requires_grad_(True)
        loss = fn(t, b)
        return (loss, *torch.autograd.grad(loss, (t, b)))

    for o, r in zip(run(torch.compile(step, fullgraph=True, backend="aot_eager")), run(step)):
        assert torch.equal(o, r)


def test_graph_capture_and_replay():
    a = A()
    gen = torch.Generator().manual_seed(106)
    x, d, bias = make_input(4096, torch.bfloat16, gen), make_input(4096, torch.bfloat16, gen), torch.randn(4096, device=DEV)
    want = a._act_bwd(d, x, None, bias, a.GELU_TANH, True, True, False)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = a._act_bwd(d, x, None, bias, a.GELU_TANH, True, True, False)
    for t in got:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for g, w in zip(got, want):
        assert torch.equal(g, w)
