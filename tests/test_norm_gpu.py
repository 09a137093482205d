"""GPU tests of the fused residual-add + LayerNorm / RMSNorm (flash_attention_annotated_amd.ops.norm over csrc/fa_norm.hip).

Shapes are M x N with M = 3 * 37 rows -- no multiple of any rows-per-workgroup, seven workgroups in the backward -- and N from
NS: one 16-byte chunk, a small regular row, the element path, several chunks with a ragged tail, the reference's size, a
large row, and the 64 KiB limit of a 16-bit row (M = 16), which takes the wide forms.  The acceptance bound is the reference's
(tests/ops/triton/test_layer_norm.py:64-86) with its constants; the oracle is this package's layer_norm_ref / rms_norm_ref.
"""
import random

import pytest
import torch
import torch.nn.functional as F

from flash_attention_annotated_amd.ops import norm
from flash_attention_annotated_amd.ops.rms_norm import rms_norm
from flash_attention_annotated_amd.ops.triton.layer_norm import RMSNorm, layer_norm_fn, layer_norm_linear_fn, rms_norm_fn

pytestmark = pytest.mark.gpu
DEV = "cuda"
M = 3 * 37
NS = (8, 192, 203, 3000, 4096, 8192, 32768)
BF16, FP16, FP32 = torch.bfloat16, torch.float16, torch.float32


def rows_of(n):
    return 16 if n == 32768 else M


def atol_of(*dtypes):
    return 5e-2 if BF16 in dtypes else 1e-2 if FP16 in dtypes else 1e-4


def accept(name, ours, pt, ref, atol):
    """max|ours - ref_upcast| <= 2 max|ref_in_dtype - ref_upcast| + atol"""
    err = (ours.float() - ref.float()).abs().max().item()
    base = (pt.float() - ref.float()).abs().max().item()
    print(f"{name}: err {err:.3e} bound 2 * {base:.3e} + {atol:g}")
    assert err <= 2 * base + atol, f"{name}: {err} > 2 * {base} + {atol}"


# ---- the grid: a seeded subset of the product, every value of every axis and every N present ---------------------------------
AXES = dict(rms=(False, True), residual=("none", "same", "fp32"), residual_in_fp32=(False, True), prenorm=(False, True),
            rowscale=(False, True), zero_centered_weight=(False, True), wdtype=(FP32, BF16, FP16), dtype=(BF16, FP16, FP32),
            out_dtype=(None, FP32, BF16))


def _grid():
    rng = random.Random(20261019)
    cases = []
    for n in NS:
        for _ in range(5):
            c = {k: rng.choice(v) for k, v in AXES.items()}
            if n == 32768:  # a row of 64 KiB: 16-bit x; the backward reads the stream, which must fit too
                c["dtype"] = rng.choice((BF16, FP16))
                c["residual"] = rng.choice(("none", "same"))
                c["residual_in_fp32"] = False
            if c["dtype"] == FP32 and c["residual"] == "same":
                c["residual"] = "fp32"
            c["n"] = n
            cases.append(c)
    return cases


GRID = _grid()


def _id(c):
    short = {BF16: "bf16", FP16: "fp16", FP32: "fp32", None: "same"}
    return (f"n{c['n']}-{'rms' if c['rms'] else 'ln'}-{short[c['dtype']]}-w{short[c['wdtype']]}-res_{c['residual']}"
            f"{'-r32' if c['residual_in_fp32'] else ''}{'-pre' if c['prenorm'] else ''}{'-rs' if c['rowscale'] else ''}"
            f"{'-zc' if c['zero_centered_weight'] else ''}-o{short[c['out_dtype']]}")


def test_grid_covers_every_axis_value_and_every_n():
    for axis, values in AXES.items():
        assert {c[axis] for c in GRID} == set(values), axis
    assert {c["n"] for c in GRID} == set(NS)
    for n in NS:
        assert {c["rms"] for c in GRID if c["n"] == n} == {False, True}, n


def _leaves(*ts):
    return [t.detach().clone().requires_grad_(True) if t is not None else None for t in ts]


@pytest.mark.parametrize("c", GRID, ids=_id)
def test_acceptance(c):
    n, dtype, wdtype = c["n"], c["dtype"], c["wdtype"]
    m = rows_of(n)
    torch.manual_seed(n)
    res_dtype = {"none": FP32 if c["residual_in_fp32"] else dtype, "same": dtype, "fp32": FP32}[c["residual"]]
    atol = atol_of(dtype, wdtype, res_dtype, c["out_dtype"])
    x = torch.randn(3, m // 3, n, device=DEV, dtype=dtype) if m % 3 == 0 else torch.randn(m, n, device=DEV, dtype=dtype)
    res = torch.randn_like(x, dtype=res_dtype) if c["residual"] != "none" else None
    w = torch.randn(n, device=DEV, dtype=wdtype)
    b = None if c["rms"] else torch.randn(n, device=DEV, dtype=wdtype)
    rowscale = torch.randn(x.shape[:-1], device=DEV, dtype=dtype) if c["rowscale"] else None
    ref_fn = norm.rms_norm_ref if c["rms"] else norm.layer_norm_ref
    kw = dict(eps=1e-6, rowscale=rowscale, prenorm=c["prenorm"], zero_centered_weight=c["zero_centered_weight"])
    sets = [_leaves(x, w, b, res) for _ in range(3)]
    (x0, w0, b0, r0), (x1, w1, b1, r1), (x2, w2, b2, r2) = sets
    out = layer_norm_fn(x0, w0, b0, residual=r0, residual_in_fp32=c["residual_in_fp32"], is_rms_norm=c["rms"],
                        out_dtype=c["out_dtype"], **kw)
    out_pt = ref_fn(x1, w1, b1, residual=r1, **kw)
    out_ref = ref_fn(x2, w2, b2, residual=r2, upcast=True, **kw)
    if c["prenorm"]:
        (out, residual), (out_pt, residual_pt), (out_ref, residual_ref) = out, out_pt, out_ref
        assert residual.dtype == res_dtype
        accept("residual_out", residual, residual_pt, residual_ref, atol)
    assert out.dtype == (dtype if c["out_dtype"] is None else c["out_dtype"]) and out.shape == x.shape
    accept("y", out, out_pt, out_ref, atol)
    g = torch.randn_like(out_pt) / 8
    if not c["prenorm"]:
        out.backward(g.to(out.dtype))
        out_pt.backward(g)
        out_ref.backward(g)
    else:
        (out * F.sigmoid(residual)).backward(g.to(out.dtype))
        (out_pt * F.sigmoid(residual_pt)).backward(g)
        (out_ref * F.sigmoid(residual_ref.to(dtype=res_dtype))).backward(g)
    accept("dx", x0.grad, x1.grad, x2.grad, atol)
    assert x0.grad.dtype == dtype
    if res is not None:
        assert r0.grad.dtype == res_dtype
        accept("dresidual", r0.grad, r1.grad, r2.grad, atol)
    assert w0.grad.dtype == wdtype
    accept("dw", w0.grad, w1.grad, w2.grad, atol)
    if b is not None:
        accept("db", b0.grad, b1.grad, b2.grad, atol)


# ---- the tighter forward bound -------------------------------------------------------------------------------------------------
def ordered_bits(t):
    """16-bit floats as integers in value order: neighbouring values differ by one"""
    i = t.view(torch.int16).to(torch.int32)
    return torch.where(i < 0, -(i & 0x7FFF), i)


FP32_ROUNDINGS = 8  # see assert_one_ulp


def ulp16(t):
    """the spacing of t's 16-bit dtype at |t|, in fp64: 2^(e - mant) among the normal values, the one spacing of the subnormal
    ones below them (2^-24 in fp16, where a result under 2^-14 is met in practice)"""
    mant, least = (7, 2.0 ** -133) if t.dtype == BF16 else (10, 2.0 ** -24)
    return torch.exp2(torch.frexp(t.double()).exponent.double() - 1 - mant).clamp_min(least)


def assert_one_ulp(y, want, bias=None, what="y"):
    """Every element of the 16-bit y within 1 ulp of the fp64 result rounded to y's dtype: bit patterns one apart at most.
    With a bias the output ends in an add that can cancel, and the fp32 error of the operands, which no fp32 evaluation avoids,
    can exceed the ulp of a small result.  There the bound is 1 ulp at the result plus what fp32 costs:
        |y - want16| <= ulp16(want16) + c 2^-24 (|w xhat| + |b|),   c = 8:
    four roundings on the way from z to y (the subtraction, two products, the add), each at most 2^-24 of the operands, and as
    much again for the errors mean and rstd carry in from their sums.  Where nothing cancels the second term is below 2^-12 ulp:
    the issue's bound."""
    want16 = want.to(y.dtype)
    if bias is None:
        flips = (ordered_bits(y.contiguous()) - ordered_bits(want16)).abs()
        print(f"{what}: {int((flips > 0).sum())} of {flips.numel()} elements off by one ulp, max {int(flips.max())}")
        assert int(flips.max()) <= 1
        return
    operands = (want - bias.double()).abs() + bias.double().abs()
    err = (y.double() - want16.double()).abs()
    spare = (err - ulp16(want16)).clamp(min=0) / (2.0 ** -24 * operands)
    print(f"{what}: max {float((err / ulp16(want16)).max()):.2f} ulp at the result; beyond 1 ulp, {float(spare.max()):.2f} x 2^-24 of the operands")
    assert bool((err <= ulp16(want16) + FP32_ROUNDINGS * 2.0 ** -24 * operands).all())


def fp64_forward(x, w, b, res, rowscale, eps, rms, zero_centered_weight):
    z = x.double()
    if rowscale is not None:
        z = z * rowscale.double()[:, None]
    if res is not None:
        z = z + res.double()
    mean = torch.zeros(z.shape[0], dtype=torch.float64, device=z.device) if rms else z.mean(-1)
    var = ((z - mean[:, None]) ** 2).mean(-1)
    rstd = 1 / torch.sqrt(var + eps)
    wd = w.double() + (1.0 if zero_centered_weight else 0.0)
    y = (z - mean[:, None]) * rstd[:, None] * wd
    return (y + b.double() if b is not None else y), mean, rstd


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("rms", [False, True], ids=["ln", "rms"])
@pytest.mark.parametrize("dtype,res_dtype", [(BF16, FP32), (FP16, FP16)], ids=["bf16_fp32res", "fp16_fp16res"])
def test_forward_one_ulp_and_exact_residual(n, rms, dtype, res_dtype):
    """fp32 arithmetic is far below half a 16-bit ulp: y is the fp64 result rounded, or its neighbour where a rounding flips --
    every element, LayerNorm and RMSNorm, with and without rowscale; with a bias (with and without rowscale) see assert_one_ulp.
    Without rowscale the sum is one fp32 add of two values exact in fp32: residual_out is bit-equal.

    Measured on an MI355X with a bias under the plain rule (ulp at |y|): up to 4 ulp at elements where weight * xhat cancels
    against the bias (bf16, LayerNorm, N = 3000); without a bias the maximum is 1."""
    m = rows_of(n)
    torch.manual_seed(n + 1)
    x = torch.randn(m, n, device=DEV, dtype=dtype)
    res = torch.randn(m, n, device=DEV, dtype=res_dtype)
    w = torch.randn(n, device=DEV, dtype=FP32)
    bias = torch.randn(n, device=DEV, dtype=dtype)
    scale = torch.rand(m, device=DEV, dtype=dtype) + 0.5
    for rowscale, b in ((None, None), (scale, None), (None, bias), (scale, bias)):
        y, residual_out, mean, rstd = norm._launch_forward(x, w, b, 1e-5, res, rowscale=rowscale, is_rms_norm=rms)
        want, _, rstd64 = fp64_forward(x, w, b, res, rowscale, 1e-5, rms, False)
        assert_one_ulp(y, want, b, f"n{n} y")
        assert residual_out.dtype == res_dtype and (mean is None) == rms
        if rowscale is None:
            z = x.float() + res.float()
            assert torch.equal(residual_out, z if res_dtype == FP32 else z.to(res_dtype))
        assert torch.allclose(rstd.double(), rstd64, rtol=1e-5, atol=0)


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("dtype", [BF16, FP32], ids=["bf16", "fp32"])
def test_statistics_match_fp64(n, dtype):
    """mean and rstd to 1e-5 relative.  A relative bound on a mean needs rows that have one: every row is offset (by 1 to 4)."""
    if dtype == FP32 and n > 16384:
        n = 16384  # (the widest fp32 row)
    m = rows_of(n)
    torch.manual_seed(n + 2)
    x = (torch.randn(m, n, device=DEV) + torch.linspace(1, 4, m, device=DEV)[:, None]).to(dtype)
    res = torch.randn(m, n, device=DEV)
    w = torch.ones(n, device=DEV)
    for rowscale in (None, torch.rand(m, device=DEV, dtype=dtype) + 0.5):
        _, _, mean, rstd = norm._launch_forward(x, w, None, 1e-5, res, rowscale=rowscale)
        _, mean64, rstd64 = fp64_forward(x, w, None, res, rowscale, 1e-5, False, False)
        print(f"n{n}: mean rel {float(((mean.double() - mean64) / mean64).abs().max()):.2e}, "
              f"rstd rel {float(((rstd.double() - rstd64) / rstd64).abs().max()):.2e}")
        assert torch.allclose(mean.double(), mean64, rtol=1e-5, atol=0)
        assert torch.allclose(rstd.double(), rstd64, rtol=1e-5, atol=0)


# ---- determinism, in place, strides ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [192, 203, 4096, 32768])
def test_backward_is_deterministic(n):
    m = rows_of(n) if n == 32768 else 1000
    torch.manual_seed(2)
    x, dy, dres = (torch.randn(m, n, device=DEV, dtype=BF16) for _ in range(3))
    w, b = torch.randn(n, device=DEV), torch.randn(n, device=DEV)
    _, _, mean, rstd = norm._launch_forward(x, w, b, 1e-5)
    runs = [norm._launch_backward(dy, x, w, b, mean, rstd, dres, has_residual=True) for _ in range(2)]
    for a, c in zip(runs[0][:3], runs[1][:3]):
        assert torch.equal(a, c)
    assert runs[0][3] is runs[0][0]  # dx serves as dresidual_in: same dtype, no rowscale


def test_in_place_and_out_dtype():
    n = 4096
    torch.manual_seed(3)
    x = torch.randn(M, n, device=DEV, dtype=BF16)
    res = torch.randn(M, n, device=DEV, dtype=FP32)
    w, b = torch.randn(n, device=DEV, dtype=BF16), torch.randn(n, device=DEV, dtype=BF16)
    y0, r0 = layer_norm_fn(x, w, b, residual=res, prenorm=True)
    out, stream = torch.full_like(y0, 7.0), torch.full_like(res, 7.0)
    y1, r1 = layer_norm_fn(x, w, b, residual=res, prenorm=True, out=out, residual_out=stream)
    assert y1.data_ptr() == out.data_ptr() and r1.data_ptr() == stream.data_ptr()
    assert torch.equal(out, y0) and torch.equal(stream, r0)
    # the stream updated in place
    live = res.clone()
    y2, r2 = layer_norm_fn(x, w, b, residual=live, prenorm=True, residual_out=live)
    assert r2.data_ptr() == live.data_ptr() and torch.equal(live, r0) and torch.equal(y2, y0)
    # fp32 out under bf16 x: written as fp32, the rounding of it is the bf16 output
    y3 = layer_norm_fn(x, w, b, residual=res, out_dtype=FP32)
    assert y3.dtype == FP32 and torch.equal(y3.to(BF16), y0) and not torch.equal(y3, y0.float())
    out32 = torch.zeros(M, n, device=DEV, dtype=FP32)
    layer_norm_fn(x, w, b, residual=res, out=out32)
    assert torch.equal(out32, y3)
    # a residual_out given where the stream is x itself is written all the same
    spare = torch.zeros_like(x)
    _, r4 = layer_norm_fn(x, w, b, prenorm=True, residual_out=spare)
    assert r4.data_ptr() == spare.data_ptr() and torch.equal(spare, x)
    with pytest.raises(ValueError, match="residual_out"):
        layer_norm_fn(x, w, b, prenorm=True, residual_out=torch.zeros_like(res))
    # a supplied tensor whose leading dims do not collapse is refused, not filled through a copy
    x3 = x.view(3, 37, n)
    for kw in (dict(out=torch.zeros(3, 40, n, device=DEV, dtype=BF16)[:, :37]),
               dict(residual_out=torch.zeros(3, 40, n, device=DEV, dtype=FP32)[:, :37], residual=res.view(3, 37, n))):
        with pytest.raises(RuntimeError, match="view"):
            layer_norm_fn(x3, w, b, **kw)


@pytest.mark.parametrize("n", [192, 3000])
@pytest.mark.parametrize("offset", [8, 3], ids=["aligned_view", "misaligned_base"])
def test_row_strided_views(n, offset):
    """x, residual, out and residual_out as slices of wider buffers; offset 3 puts the base off the 16 bytes: the element path
    under 16-bit types.  Nothing beside the slices is written."""
    pad = 24
    torch.manual_seed(4)
    bufs = [torch.randn(M, n + pad, device=DEV, dtype=BF16) for _ in range(4)]
    keep = [t.clone() for t in bufs]
    x, res, out, stream = (t[:, offset:offset + n] for t in bufs)
    w, b = torch.randn(n, device=DEV), torch.randn(n, device=DEV)
    y, r = layer_norm_fn(x, w, b, residual=res, prenorm=True, eps=1e-5, out=out, residual_out=stream)
    assert y.data_ptr() == out.data_ptr() and r.data_ptr() == stream.data_ptr()
    want, _, _ = fp64_forward(x, w, b, res, None, 1e-5, False, False)
    assert_one_ulp(out, want, b)
    assert torch.equal(stream, (x.float() + res.float()).to(BF16))
    for t, k in zip(bufs, keep):
        assert torch.equal(t[:, :offset], k[:, :offset]) and torch.equal(t[:, offset + n:], k[:, offset + n:])
    assert torch.equal(bufs[0], keep[0]) and torch.equal(bufs[1], keep[1])
    # backward through strided x / dy
    xl = bufs[0].clone().requires_grad_(True)
    yl = layer_norm_fn(xl[:, offset:offset + n], w, b, eps=1e-5)
    gbuf = torch.randn(M, n + pad, device=DEV, dtype=BF16)
    yl.backward(gbuf[:, offset:offset + n])
    xc = x.contiguous().requires_grad_(True)
    layer_norm_fn(xc, w, b, eps=1e-5).backward(gbuf[:, offset:offset + n].contiguous())
    x_ref = x.float().requires_grad_(True)
    norm.layer_norm_ref(x_ref, w, b, eps=1e-5).backward(gbuf[:, offset:offset + n].float())
    accept("dx strided", xl.grad[:, offset:offset + n], xc.grad, x_ref.grad, 5e-2)
    assert not xl.grad[:, :offset].any() and not xl.grad[:, offset + n:].any()


# ---- layer_norm_linear_fn ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [192, 3000])
@pytest.mark.parametrize("prenorm", [False, True])
@pytest.mark.parametrize("rms", [False, True], ids=["ln", "rms"])
def test_layer_norm_linear(n, prenorm, rms):
    torch.manual_seed(5)
    dtype, atol = BF16, 5e-2
    x = torch.randn(M, n, device=DEV, dtype=dtype)
    res = torch.randn(M, n, device=DEV, dtype=FP32)
    nw = torch.randn(n, device=DEV)
    nb = None if rms else torch.randn(n, device=DEV)
    lw = torch.empty(2 * n, n, device=DEV)
    torch.nn.init.xavier_uniform_(lw)
    lb = None if rms else torch.randn(2 * n, device=DEV)
    ref_fn = norm.rms_norm_ref if rms else norm.layer_norm_ref
    sets = [_leaves(x, res, nw, nb, lw, lb) for _ in range(3)]
    a, pt, rf = sets
    with torch.autocast(device_type="cuda", dtype=dtype):
        ret = layer_norm_linear_fn(a[0], a[2], a[3], a[4], a[5], residual=a[1], eps=1e-6, prenorm=prenorm, is_rms_norm=rms)
    out, residual = ret if prenorm else (ret, None)
    o_pt, *rest_pt = ref_fn(pt[0], pt[2], pt[3], residual=pt[1], eps=1e-6, prenorm=True)
    with torch.autocast(device_type="cuda", dtype=dtype):
        o_pt = F.linear(o_pt, pt[4], pt[5])
    o_rf, *rest_rf = ref_fn(rf[0], rf[2], rf[3], residual=rf[1], eps=1e-6, prenorm=True, upcast=True)
    o_rf = F.linear(o_rf.to(rf[4].dtype), rf[4], rf[5])
    if prenorm:
        assert residual.dtype == FP32
        accept("residual_out", residual, rest_pt[0], rest_rf[0], atol)
    assert out.dtype == dtype
    accept("out", out, o_pt, o_rf, atol)
    g = torch.randn_like(out) / 4
    out.backward(g)
    o_pt.backward(g)
    o_rf.backward(g)
    names = ("dx", "dresidual", "dnorm_weight", "dnorm_bias", "dlinear_weight", "dlinear_bias")
    for name, t0, t1, t2 in zip(names, a, pt, rf):
        if t0 is not None:
            accept(name, t0.grad, t1.grad, t2.grad, atol)


# ---- sizes -------------------------------------------------------------------------------------------------------------------------
def test_2_31_elements_forward():
    """M * N = 2^31 + N at bf16: the last rows start past 2^32 bytes.  The first and last 8 rows are compared."""
    n = 4096
    m = (1 << 31) // n + 1
    x = torch.empty(m, n, device=DEV, dtype=BF16)
    for lo in range(0, m, 1 << 16):  # (filled in slabs: no fp32 copy of the whole tensor)
        x[lo:lo + (1 << 16)].normal_()
    w = torch.randn(n, device=DEV, dtype=BF16)
    y = rms_norm_fn(x, w, None, eps=1e-5)
    assert y.shape == x.shape
    for rows in (slice(0, 8), slice(m - 8, m)):
        want, _, _ = fp64_forward(x[rows], w, None, None, None, 1e-5, True, False)
        assert_one_ulp(y[rows], want)


def test_one_row_and_no_rows():
    n = 203
    torch.manual_seed(6)
    w, b = torch.randn(n, device=DEV, requires_grad=True), torch.randn(n, device=DEV, requires_grad=True)
    x = torch.randn(1, n, device=DEV, dtype=BF16, requires_grad=True)
    y = layer_norm_fn(x, w, b, eps=1e-5)
    want, _, _ = fp64_forward(x.detach(), w.detach(), b.detach(), None, None, 1e-5, False, False)
    assert_one_ulp(y.detach(), want, b.detach())
    y.float().sum().backward()
    assert torch.allclose(b.grad, torch.ones(n, device=DEV)) and x.grad.shape == x.shape
    # an empty batch: empty tensors, zero dw / db, nothing launched over zero rows
    w.grad = b.grad = None
    e = torch.empty(0, 5, n, device=DEV, dtype=BF16, requires_grad=True)
    res = torch.empty(0, 5, n, device=DEV, dtype=FP32)
    ye, re_ = layer_norm_fn(e, w, b, residual=res, prenorm=True)
    assert ye.shape == (0, 5, n) and re_.shape == (0, 5, n) and re_.dtype == FP32
    (ye.float().sum() + re_.sum()).backward()
    torch.cuda.synchronize()
    assert e.grad.shape == (0, 5, n)
    assert torch.equal(w.grad, torch.zeros(n, device=DEV)) and torch.equal(b.grad, torch.zeros(n, device=DEV))


def test_modules_and_rms_norm_function():
    n = 192
    torch.manual_seed(7)
    x = torch.randn(2, 37, n, device=DEV, dtype=BF16)
    m = RMSNorm(n, device=DEV, dtype=BF16)
    y, r = m(x, residual=x.float(), prenorm=True)
    want, _, _ = fp64_forward(x.reshape(-1, n), m.weight.detach(), None, x.reshape(-1, n).float(), None, 1e-5, True, False)
    assert_one_ulp(y.detach().reshape(-1, n), want)
    assert r.dtype == FP32
    z = rms_norm(x, m.weight.detach(), 1e-5)
    want, _, _ = fp64_forward(x.reshape(-1, n), m.weight.detach(), None, None, None, 1e-5, True, False)
    assert z.dtype == BF16
    assert_one_ulp(z.reshape(-1, n), want)
    with pytest.raises(NotImplementedError, match="dropout_p"):
        RMSNorm(n, dropout_p=0.1, device=DEV, dtype=BF16)(x)
    with pytest.raises(RuntimeError, match="feature dim >= 64KB"):
        rms_norm_fn(torch.zeros(2, 32776, device=DEV, dtype=BF16), torch.ones(32776, device=DEV), None)


# ---- graphs and compile ------------------------------------------------------------------------------------------------------------
def _step(x, res, dy, w, b):
    y, stream, mean, rstd = norm._launch_forward(x, w, b, 1e-5, res)
    dx, dw, db, *_ = norm._launch_backward(dy, stream, w, b, mean, rstd, has_residual=True, dx_dtype=x.dtype)
    return y, stream, dx, dw, db


def test_hip_graph_capture_and_replay():
    n = 3000
    torch.manual_seed(8)
    x, dy = torch.randn(M, n, device=DEV, dtype=BF16), torch.randn(M, n, device=DEV, dtype=BF16)
    res = torch.randn(M, n, device=DEV, dtype=FP32)
    w, b = torch.randn(n, device=DEV), torch.randn(n, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _step(x, res, dy, w, b)  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = _step(x, res, dy, w, b)
    x.copy_(torch.randn(M, n, device=DEV, dtype=BF16))
    graph.replay()
    torch.cuda.synchronize()
    for got, want in zip(outs, _step(x, res, dy, w, b)):
        assert torch.equal(got, want)


def test_compile_fullgraph():
    n = 192
    torch.manual_seed(9)
    x = torch.randn(2, 37, n, device=DEV, dtype=BF16)
    res = torch.randn(2, 37, n, device=DEV, dtype=FP32)
    w = torch.randn(n, device=DEV, dtype=BF16)
    g = torch.randn(2, 37, n, device=DEV, dtype=BF16)

    def step(x, res, w):
        y, stream = rms_norm_fn(x, w, None, residual=res, prenorm=True, eps=1e-5)
        return y, stream

    def run(fn):
        xl, rl, wl = _leaves(x, res, w)
        y, stream = fn(xl, rl, wl)
        grads = torch.autograd.grad((y * F.sigmoid(stream).to(y.dtype)).float().sum() + (y * g).float().sum(), (xl, rl, wl))
        return (y.detach(), stream.detach(), *grads)
    for got, want in zip(run(torch.compile(step, backend="aot_eager", fullgraph=True)), run(step)):
        assert got.dtype == want.dtype and torch.equal(got, want)
