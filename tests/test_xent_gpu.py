"""GPU tests of the fused cross-entropy loss (ops/triton/cross_entropy.py and losses/cross_entropy.py over csrc/fa_xent.hip).

Shapes are M = 37 rows, 5 of them with the ignore label, and N from NS: one 16-byte chunk; head and tail only, in every phase;
a regular row; the reference test's vocabulary, whose odd pitch puts every row at another phase; and a row of several backward
slabs.  The oracle (`ref64`) is cross_entropy_ref / cross_entropy_grad_ref in fp64 on the same rounded logits; `eager32` is
torch's eager evaluation in fp32 of those logits, its gradient taken at the logits themselves and hence rounded once to their
dtype, as in the reference's test (tests/losses/test_cross_entropy.py:46-83).  Acceptance is the project's inequality
max|ours - ref64| <= 2 max|eager32 - ref64| + rtol max|ref64| + atol with that test's constants (:41, :78).
"""
import random

import pytest
import torch
import torch.nn.functional as F

from flash_attention_annotated_amd._lib import binding
from flash_attention_annotated_amd.losses.cross_entropy import CrossEntropyLoss
from flash_attention_annotated_amd.ops.triton import cross_entropy as xent
from flash_attention_annotated_amd.ops.triton.cross_entropy import cross_entropy_grad_ref, cross_entropy_loss, cross_entropy_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
M = 37
NS = (8, 203, 4096, 50257, 128256)
BF16, FP16, FP32 = torch.bfloat16, torch.float16, torch.float32
DTYPES = (BF16, FP16, FP32)
IGNORE = -100
TOL32, TOL16 = (1e-5, 1e-6), (1e-3, 1e-4)


def accept(name, ours, eager, ref, tol):
    """max|ours - ref64| <= 2 max|eager32 - ref64| + rtol max|ref64| + atol"""
    err = (ours.double() - ref).abs().max().item()
    base = (eager.double() - ref).abs().max().item()
    slack = tol[0] * ref.abs().max().item() + tol[1]
    print(f"{name}: err {err:.3e} bound 2 * {base:.3e} + {slack:.3e}")
    assert err <= 2 * base + slack, f"{name}: {err} > 2 * {base} + {slack}"


def problem(n, dtype, seed, m=M, label_dtype=torch.int64):
    """(logits, labels, dloss): seeded, 5 rows (of M = 37) with the ignore label."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = (torch.randn(m, n, device=DEV, generator=g) * 2).to(dtype)
    y = torch.randint(0, n, (m,), device=DEV, generator=g)
    if m >= 10:
        y[torch.randperm(m, device=DEV, generator=g)[:5]] = IGNORE
    return x, y.to(label_dtype), torch.randn(m, device=DEV, generator=g)


def eager32(x, y, d, s=0.0, scale=1.0, z=0.0):
    """(losses, z_losses, lse, dlogits) of torch's eager fp32 evaluation; dlogits arrives at x and has its dtype."""
    xl = x.detach().clone().requires_grad_(True)
    xs = xl.float() * scale
    lse = torch.logsumexp(xs, dim=-1)
    z_losses = (z * lse.square()).masked_fill(y == IGNORE, 0.0)
    losses = F.cross_entropy(xs, y.long(), label_smoothing=s, reduction="none", ignore_index=IGNORE) + z_losses
    (dx,) = torch.autograd.grad(losses, xl, d.expand(x.shape[0]))
    return losses.detach(), z_losses.detach(), lse.detach(), dx


def ref64(x, y, d, s=0.0, scale=1.0, z=0.0, **kw):
    losses, z_losses, lse = cross_entropy_ref(x.double(), y, label_smoothing=s, logit_scale=scale, lse_square_scale=z, **kw)
    return losses, z_losses, lse, cross_entropy_grad_ref(x.double(), y, lse, d, label_smoothing=s, logit_scale=scale, lse_square_scale=z)


def ours(x, y, d, s=0.0, scale=1.0, z=0.0, inplace=False, lse_given=None):
    """(losses, z_losses, dlogits, the logits the call was given) through the autograd function."""
    xl = x.detach().clone().requires_grad_(True)
    losses, z_losses = cross_entropy_loss(xl, y, lse_given, s, scale, z, IGNORE, inplace)
    assert not z_losses.requires_grad and losses.dtype == z_losses.dtype == FP32
    (dx,) = torch.autograd.grad(losses, xl, d.expand(x.shape[0]))
    return losses.detach(), z_losses, dx, xl


# ---- the grid: seeded cases for every N in every dtype; every value of every axis present ---------------------------------------
AXES = dict(s=(0.0, 0.1, 0.9), scale=(1.0, 0.7), z=(0.0, 1e-2), label_dtype=(torch.int64, torch.int32), inplace=(False, True),
            lse_given=(False, True))


def _grid():
    rng = random.Random(20261020)
    cases = []
    for n in NS:
        for dtype in DTYPES:
            for k in range(2):
                c = {a: rng.choice(v) for a, v in AXES.items()}
                if k == 1:  # one case of the two may be given its lse: the flag is valid only without smoothing and scale
                    c["lse_given"] = rng.choice((False, True))
                    if c["lse_given"]:
                        c["s"], c["scale"] = 0.0, 1.0
                else:
                    c["lse_given"] = False
                c.update(n=n, dtype=dtype)
                cases.append(c)
    return cases


GRID = _grid()


def _id(c):
    short = {BF16: "bf16", FP16: "fp16", FP32: "fp32"}
    return (f"n{c['n']}-{short[c['dtype']]}-s{c['s']}-k{c['scale']}-z{c['z']}-{'i32' if c['label_dtype'] == torch.int32 else 'i64'}"
            f"{'-inplace' if c['inplace'] else ''}{'-lse' if c['lse_given'] else ''}")


def test_grid_covers_every_axis_value_every_n_and_dtype():
    for axis, values in AXES.items():
        assert {c[axis] for c in GRID} == set(values), axis
    assert {(c["n"], c["dtype"]) for c in GRID} == {(n, t) for n in NS for t in DTYPES}
    assert all(not c["lse_given"] or (c["s"] == 0.0 and c["scale"] == 1.0) for c in GRID)


@pytest.mark.parametrize("c", GRID, ids=_id)
def test_acceptance(c):
    n, dtype, s, scale, z = c["n"], c["dtype"], c["s"], c["scale"], c["z"]
    x, y, d = problem(n, dtype, seed=n + len(_id(c)), label_dtype=c["label_dtype"])
    e_losses, e_z, e_lse, e_dx = eager32(x, y, d, s, scale, z)
    r_losses, r_z, r_lse, r_dx = ref64(x, y, d, s, scale, z)
    given = e_lse.clone() if c["lse_given"] else None
    losses, z_losses, dx, xl = ours(x, y, d, s, scale, z, c["inplace"], given)
    accept("losses", losses, e_losses, r_losses, TOL32)
    accept("z_losses", z_losses, e_z, r_z, TOL32)
    if not c["lse_given"]:
        _, lse, _ = xent._xent_fwd(x, y, None, s, scale, z, IGNORE, 0, n, False)
        accept("lse", lse, e_lse, r_lse, TOL32)
    assert dx.dtype == dtype and dx.shape == x.shape
    assert (dx.data_ptr() == xl.data_ptr()) == c["inplace"]
    accept("dlogits", dx, e_dx, r_dx, TOL32 if dtype == FP32 else TOL16)
    ignored = y == IGNORE
    assert not losses[ignored].any() and not z_losses[ignored].any() and not dx[ignored].any()


# ---- 16-bit rounding, element by element ---------------------------------------------------------------------------------------
# |dlogits - ref64| <= ulp16(ref64) + c |d logit_scale| (p (1 + 2 z |lse|) + [col == label]): one rounding to 16 bits, and an
# fp32 error in proportion to the terms that are added.  C_EAGER is what torch's eager fp32 gradient, rounded to 16 bits, needs
# as c over the cases below, measured on an MI355X: 6.08e-6 at the most, 0 in 18 of the 20 cases (ours: 1.49e-6).
# Ours is allowed twice the eager figure.
C_EAGER = 6.1e-6
ROUNDING_CASES = [(n, t, s, scale, z) for n in NS for t in (BF16, FP16) for s, scale, z in ((0.0, 1.0, 0.0), (0.1, 0.7, 1e-2))]


def ulp16(t, dtype):
    """the spacing of `dtype` at |t|, in fp64 (fp16: not below that of its subnormals)"""
    mant = 7 if dtype == BF16 else 10
    ulp = torch.exp2(torch.frexp(t.double()).exponent.double() - 1 - mant)
    return ulp.clamp_min(2.0 ** -24) if dtype == FP16 else ulp


def needed_c(dx, r_dx, terms, dtype):
    """the smallest c with |dx - ref64| <= ulp16(ref64) + c * terms"""
    over = ((dx.double() - r_dx).abs() - ulp16(r_dx, dtype)).clamp_min(0.0)
    return (over / terms).max().item()


@pytest.mark.parametrize("n,dtype,s,scale,z", ROUNDING_CASES)
def test_16_bit_gradient_is_rounded_once(n, dtype, s, scale, z):
    x, y, d = problem(n, dtype, seed=3 * n + 1)
    _, _, r_lse, r_dx = ref64(x, y, d, s, scale, z)
    p = torch.exp(x.double() * scale - r_lse[:, None])
    at_label = torch.arange(n, device=DEV)[None, :] == y[:, None]
    terms = (d.double().abs() * scale)[:, None] * (p * (1 + 2 * z * r_lse.abs())[:, None] + at_label.double())
    terms = terms.clamp_min(1e-300)  # (ignored rows: d is not read there, and both gradients are exact zeros)
    c_eager = needed_c(eager32(x, y, d, s, scale, z)[3], r_dx, terms, dtype)
    c_ours = needed_c(ours(x, y, d, s, scale, z)[2], r_dx, terms, dtype)
    print(f"c: eager {c_eager:.3e} ours {c_ours:.3e} (allowed {2 * C_EAGER:.3e})")
    assert c_ours <= 2 * C_EAGER


# ---- through the module ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reduction", ["mean", "sum"])
@pytest.mark.parametrize("n", [203, 50257])
def test_module_against_torch(n, reduction):
    """fp32 logits against torch.nn.CrossEntropyLoss; the gradient of a reduced loss is an expanded scalar, dloss_stride 0."""
    x, y, _ = problem(n, FP32, seed=n)

    def run(module, logits):
        xl = logits.detach().clone().requires_grad_(True)
        loss = module(xl, y)
        (dx,) = torch.autograd.grad(loss, xl)
        return loss.detach(), dx
    loss, dx = run(CrossEntropyLoss(reduction=reduction, label_smoothing=0.1), x)
    e_loss, e_dx = run(torch.nn.CrossEntropyLoss(reduction=reduction, label_smoothing=0.1), x)
    r_loss, r_dx = run(torch.nn.CrossEntropyLoss(reduction=reduction, label_smoothing=0.1), x.double())
    assert loss.shape == e_loss.shape and loss.dtype == FP32
    accept("loss", loss, e_loss, r_loss, TOL32)
    accept("dlogits", dx, e_dx, r_dx, TOL32)


@pytest.mark.parametrize("reduction", ["mean", "sum", "none"])
def test_module_returns_z_loss(reduction):
    n, z = 4096, 1e-2
    x, y, _ = problem(n, BF16, seed=5)
    loss, z_loss = CrossEntropyLoss(reduction=reduction, lse_square_scale=z, logit_scale=0.7, return_z_loss=True)(x, y)
    assert not z_loss.requires_grad and loss.shape == z_loss.shape == (() if reduction != "none" else (M,))
    r_losses, r_z, _ = cross_entropy_ref(x.double(), y, logit_scale=0.7, lse_square_scale=z)
    e_losses, e_z, _, _ = eager32(x, y, torch.ones(M, device=DEV), 0.0, 0.7, z)
    count = (y != IGNORE).sum()
    reduce = {"mean": lambda t: t.sum() / count, "sum": lambda t: t.sum(), "none": lambda t: t}[reduction]
    accept("loss", loss, reduce(e_losses), reduce(r_losses), TOL32)
    accept("z_loss", z_loss, reduce(e_z), reduce(r_z), TOL32)
    assert CrossEntropyLoss(reduction=reduction, lse_square_scale=z, logit_scale=0.7)(x, y).equal(loss)
    with pytest.raises(NotImplementedError):
        CrossEntropyLoss(reduction="max")


# ---- ignored rows, labels outside the columns --------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [203, 50257])
def test_ignored_rows_may_hold_nan(n, dtype):
    x, y, d = problem(n, dtype, seed=7)
    ignored = y == IGNORE
    clean = ours(x, y, d, 0.1, 0.7, 1e-2)
    x[ignored] = float("nan")
    for inplace in (False, True):
        losses, z_losses, dx, _ = ours(x, y, d, 0.1, 0.7, 1e-2, inplace)
        assert (losses[ignored] == 0).all() and (z_losses[ignored] == 0).all()
        assert (dx[ignored].view(torch.int16 if dtype != FP32 else torch.int32) == 0).all()  # exact zeros, no NaN and no -0
        assert torch.equal(losses[~ignored], clean[0][~ignored]) and torch.equal(dx[~ignored], clean[2][~ignored])


@pytest.mark.parametrize("s", [0.0, 0.1])
@pytest.mark.parametrize("dtype", [BF16, FP32])
def test_label_outside_the_columns_reads_nothing(s, dtype):
    """Labels >= N that are not the ignore label: the oracle's `lab outside` branch.  The logits end where a row of NaN begins,
    and the last row's label points into it: a kernel that read logits[r, lab] would return NaN there."""
    n, total = 203, 1000
    x, y, d = problem(n, dtype, seed=11)
    buf = torch.full((M + 1, n), float("nan"), device=DEV, dtype=dtype)
    buf[:M] = x
    logits = buf[:M]
    y[3], y[M - 1] = total - 1, n + 3
    losses, lse, z_losses = xent._xent_fwd(logits, y, None, s, 1.0, 0.0, IGNORE, 0, total, False)
    r_losses, _, r_lse = cross_entropy_ref(x.double(), y, label_smoothing=s, total_classes=total)
    e = cross_entropy_ref(x, y, label_smoothing=s, total_classes=total)  # (torch's own loss has no such labels)
    outside = torch.tensor([3, M - 1], device=DEV)
    assert (r_losses[outside] - s * (r_lse - x.double().sum(1) / total)[outside]).abs().max().item() < 1e-12
    accept("losses", losses, e[0], r_losses, TOL32)
    assert not losses.isnan().any()
    r_dx = cross_entropy_grad_ref(x.double(), y, r_lse, d, label_smoothing=s, total_classes=total)
    e_dx = cross_entropy_grad_ref(x, y, e[2], d, label_smoothing=s, total_classes=total).to(dtype)
    xent._xent_bwd_inplace(d, logits, y, lse, s, 1.0, 0.0, IGNORE, 0, total)
    accept("dlogits", logits, e_dx, r_dx, TOL32 if dtype == FP32 else TOL16)
    assert buf[M].isnan().all()


# ---- a vocabulary split, emulated in one process ---------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [BF16, FP32])
@pytest.mark.parametrize("n,cut", [(203, 96), (50257, 25000)])
def test_split_in_two_equals_unsplit(n, cut, dtype):
    s, scale, z = 0.1, 0.7, 1e-2
    x, y, d = problem(n, dtype, seed=13)
    e_losses, e_z, e_lse, e_dx = eager32(x, y, d, s, scale, z)
    r_losses, r_z, r_lse, r_dx = ref64(x, y, d, s, scale, z)
    halves = [(0, cut), (cut, n)]  # (column slices: a row stride of n, and every phase)
    parts = [xent._xent_fwd(x[:, a:b], y, None, s, scale, z, IGNORE, a, n, True) for a, b in halves]
    assert all(p[2].numel() == 0 for p in parts)
    losses, z_losses, lse = xent._finish_split(torch.stack([p[0] for p in parts]), torch.stack([p[1] for p in parts]), y, z,
                                               IGNORE, None)
    accept("losses", losses, e_losses, r_losses, TOL32)
    accept("z_losses", z_losses, e_z, r_z, TOL32)
    accept("lse", lse, e_lse, r_lse, TOL32)
    dx = x.clone()
    for a, b in halves:  # in place on the slices (16-byte accesses), and into a tensor of another pitch (element accesses)
        xent._xent_bwd_inplace(d, dx[:, a:b], y, lse, s, scale, z, IGNORE, a, n)
    apart = torch.cat([xent._xent_bwd(d, x[:, a:b], y, lse, s, scale, z, IGNORE, a, n) for a, b in halves], dim=1)
    accept("dlogits in place", dx, e_dx, r_dx, TOL32 if dtype == FP32 else TOL16)
    accept("dlogits apart", apart, e_dx, r_dx, TOL32 if dtype == FP32 else TOL16)


# ---- odd layouts ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [203, 50257])
def test_strided_offset_rows_and_their_neighbours(n, dtype):
    """A row stride above N, a base off by three elements, canary columns between the rows; a gradient tensor of the same
    phase (16-byte accesses) and one of another phase (element accesses): the same values, and no canary touched."""
    s, scale, z, canary = 0.1, 0.7, 1e-2, 77.0
    x, y, d = problem(n, dtype, seed=17)
    _, _, _, e_dx = eager32(x, y, d, s, scale, z)
    r_losses, _, r_lse, r_dx = ref64(x, y, d, s, scale, z)

    def framed(left, right):
        buf = torch.full((M, left + n + right), canary, device=DEV, dtype=dtype)
        return buf, buf[:, left:left + n]

    def untouched(buf, left):
        return (buf[:, :left] == canary).all() and (buf[:, left + n:] == canary).all()
    buf, logits = framed(3, 4)
    logits.copy_(x)
    losses, lse, _ = xent._xent_fwd(logits, y, None, s, scale, z, IGNORE, 0, n, False)
    accept("losses", losses, eager32(x, y, d, s, scale, z)[0], r_losses, TOL32)
    tol = TOL32 if dtype == FP32 else TOL16
    same_buf, same = framed(3, 4)
    other_buf, other = framed(2, 2)
    args = (s, scale, z, IGNORE, 0, n)
    binding().xent_bwd(d, logits, y, lse, same, *args)
    binding().xent_bwd(d, logits, y, lse, other, *args)
    accept("dlogits same phase", same, e_dx, r_dx, tol)
    assert torch.equal(same, other)
    assert untouched(same_buf, 3) and untouched(other_buf, 2) and torch.equal(logits, x)
    xent._xent_bwd_inplace(d, logits, y, lse, *args)
    assert torch.equal(logits, same) and untouched(buf, 3)


# ---- further cases ----------------------------------------------------------------------------------------------------------------
def test_same_call_same_bits():
    x, y, d = problem(50257, BF16, seed=19)
    a, b = ours(x, y, d, 0.1, 0.7, 1e-2), ours(x, y, d, 0.1, 0.7, 1e-2)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])


@pytest.mark.parametrize("m", [1, 0])
def test_one_row_and_no_rows(m):
    n = 4099
    x, y, d = problem(n, FP16, seed=23, m=m)
    losses, z_losses, dx, _ = ours(x, y, d, 0.1, 0.7, 1e-2)
    assert losses.shape == z_losses.shape == (m,) and dx.shape == (m, n)
    if m:
        e_losses, _, _, e_dx = eager32(x, y, d, 0.1, 0.7, 1e-2)
        r_losses, _, _, r_dx = ref64(x, y, d, 0.1, 0.7, 1e-2)
        accept("losses", losses, e_losses, r_losses, TOL32)
        accept("dlogits", dx, e_dx, r_dx, TOL16)
    loss = CrossEntropyLoss(reduction="sum")(x, y)
    assert loss.shape == () and (m or loss.item() == 0.0)


def test_non_unit_last_stride_is_made_contiguous():
    x, y, d = problem(203, BF16, seed=29)
    a = ours(x, y, d)
    xt = x.t().contiguous().t()
    assert xt.stride(-1) != 1
    xl = xt.detach().requires_grad_(True)
    losses, _ = cross_entropy_loss(xl, y)
    (dx,) = torch.autograd.grad(losses, xl, d)
    assert torch.equal(losses, a[0]) and torch.equal(dx, a[2])


def test_compile_fullgraph():
    x, y, d = problem(203, BF16, seed=31)

    def step(logits, labels, dloss):
        losses, z_losses = cross_entropy_loss(logits, labels, None, 0.1, 0.7, 1e-2)
        return losses, z_losses, (losses * dloss).sum()

    def run(fn):
        xl = x.detach().clone().requires_grad_(True)
        losses, z_losses, total = fn(xl, y, d)
        (dx,) = torch.autograd.grad(total, xl)
        return losses.detach(), z_losses, dx
    for got, want in zip(run(torch.compile(step, backend="aot_eager", fullgraph=True)), run(step)):
        assert got.dtype == want.dtype and torch.equal(got, want)


@pytest.mark.parametrize("inplace", [False, True])
def test_hip_graph_capture_and_replay(inplace):
    n = 50257
    x, y, d = problem(n, BF16, seed=37)
    fresh = problem(n, BF16, seed=38)[0]

    def step():
        losses, lse, z_losses = xent._xent_fwd(x, y, None, 0.1, 0.7, 1e-2, IGNORE, 0, n, False)
        if inplace:
            work = x.clone()
            xent._xent_bwd_inplace(d, work, y, lse, 0.1, 0.7, 1e-2, IGNORE, 0, n)
            return losses, lse, z_losses, work
        return losses, lse, z_losses, xent._xent_bwd(d, x, y, lse, 0.1, 0.7, 1e-2, IGNORE, 0, n)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step()
    x.copy_(fresh)
    graph.replay()
    torch.cuda.synchronize()
    for got, want in zip(outs, step()):
        assert torch.equal(got, want)


# ---- memory, and rows beyond 2^31 elements ------------------------------------------------------------------------------------
def test_memory_of_forward_and_in_place_backward():
    """bf16 logits of M x N: the forward allocates three fp32 vectors of M, the in-place backward nothing of the logits' size.
    Both stay under an eighth of the logits; the eager evaluation allocates several times the logits."""
    m, n = 4096, 32000
    bound = m * n * 2 // 8
    x = torch.randn(m, n, device=DEV, dtype=BF16).requires_grad_(True)
    y = torch.randint(0, n, (m,), device=DEV)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    losses, _ = cross_entropy_loss(x, y, inplace_backward=True)
    torch.cuda.synchronize()
    forward = torch.cuda.max_memory_allocated() - before
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    (dx,) = torch.autograd.grad(losses.sum(), x)
    torch.cuda.synchronize()
    backward = torch.cuda.max_memory_allocated() - before
    print(f"forward {forward} B, in-place backward {backward} B, bound {bound} B")
    assert dx.data_ptr() == x.data_ptr()
    assert forward < bound and backward < bound


def test_rows_beyond_2_31_elements():
    """bf16, 16400 x 131072 (4.3 GB), in place: the rows around element 2^31 and the last, against the oracle on those rows."""
    m, n = 16400, 131072
    rows = torch.tensor([0, 16383, 16384, 16399], device=DEV)
    assert 16384 * n == 1 << 31
    x = torch.empty(m, n, device=DEV, dtype=BF16)
    x.view(torch.int16).zero_()
    g = torch.Generator(device=DEV).manual_seed(41)
    x[rows] = (torch.randn(4, n, device=DEV, generator=g) * 2).to(BF16)
    y = torch.randint(0, n, (m,), device=DEV, generator=g)
    d = torch.randn(m, device=DEV, generator=g)
    kept = x[rows].clone()
    losses, lse, _ = xent._xent_fwd(x, y, None, 0.0, 1.0, 0.0, IGNORE, 0, n, False)
    xent._xent_bwd_inplace(d, x, y, lse, 0.0, 1.0, 0.0, IGNORE, 0, n)
    e_losses, _, e_lse, e_dx = eager32(kept, y[rows], d[rows])
    r_losses, _, r_lse, r_dx = ref64(kept, y[rows], d[rows])
    accept("losses", losses[rows], e_losses, r_losses, TOL32)
    accept("lse", lse[rows], e_lse, r_lse, TOL32)
    accept("dlogits", x[rows], e_dx, r_dx, TOL16)
    # a row of zeros between them: lse = log(n), and the gradient d * (1 / n - [col == label])
    assert abs(lse[5].item() - torch.log(torch.tensor(float(n))).item()) < 1e-5
