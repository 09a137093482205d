"""GPU tests of every launch form of csrc/fa_norm.hip: the case table of tests/norm_plan_universe.py -- both sides of every team
boundary in every access shape, the wide forms with ragged and full last slabs -- against fp64, element by element.  Every case
first asks the plan (norm._plan_forward / _plan_backward on the very tensors) which form the call takes and holds it to the
cell the case names, so an allocator or a view cannot move a case to another form unnoticed.

Forward: test_norm_gpu.py's assert_one_ulp, its exact residual_out rule and its 1e-5 relative bound on mean / rstd.
Backward: an fp64 backward written here, mean / rstd given to the kernel as the fp64 statistics rounded to fp32, and
    |dx - ref64| <= [ulp16(ref64) +] c T,   T = rstd (|w dy| + |xhat| mean|xhat w dy| + mean|w dy|) + |dresidual|
    |dw - ref64| <= ulp(ref64) + c sum_rows |dy xhat|,   |db - ref64| <= ulp(ref64) + c sum_rows |dy|
per element and per column: one rounding to the output's dtype, and an fp32 error in proportion to the terms that are added.
"""
import pytest
import torch

import norm_plan_universe as U
from flash_attention_annotated_amd.ops import norm
from test_norm_gpu import FP32_ROUNDINGS, assert_one_ulp, fp64_forward

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, FP16, FP32 = torch.bfloat16, torch.float16, torch.float32
TORCH = {"bf16": BF16, "fp16": FP16, "fp32": FP32}
EPS = 1e-5
FWD_CASES = [c for c in U.CASES if c.cell.direction == "fwd"]
BWD_CASES = [c for c in U.CASES if c.cell.direction == "bwd"]

# C_EAGER: what torch's eager fp32 evaluation of the same backward (layer_norm_ref / rms_norm_ref on the inputs upcast to fp32,
# its gradients rounded to the case's dtypes) needs as c over BWD_CASES, the recompute, row-loop and canary cases below, measured
# on an MI355X: 2.218e-7 for dx and dresidual_in (ours: 1.427e-7), 2.083e-7 for dw and db (ours: 1.430e-7); 16-bit dx needs
# none at all in most cases: it is the fp64 result rounded.  Ours is allowed twice the eager figure: the two add a row's and a
# column's terms in different orders, and neither order is the more exact.  DESIGN 4.22.
C_EAGER = {"dx": 2.22e-7, "dw": 2.09e-7}


def ulp_of(ref, dtype):
    """the spacing of `dtype` at |ref|, in fp64"""
    mant = {BF16: 7, FP16: 10, FP32: 23}[dtype]
    return torch.exp2(torch.frexp(ref).exponent.double() - 1 - mant)


def needed_c(got, ref, terms, dtype, rounding):
    """the smallest c with |got - ref| <= [ulp(ref)] + c terms"""
    over = (got.double() - ref).abs()
    if rounding:
        over = (over - ulp_of(ref, dtype)).clamp_min(0.0)
    return float((over / terms.clamp_min(1e-300)).max())


def cell_of(direction, plan):
    return U.cell_of_plan(direction, plan)


def operands(c, seed):
    """the tensors of a case, forward or backward: rows in c.x_dtype, weight and bias in the weight's dtype"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    rand = lambda *shape, dtype: torch.randn(*shape, device=DEV, generator=g).to(dtype)  # noqa: E731
    xt, dt, wt = TORCH[c.x_dtype], TORCH[c.dx_dtype], TORCH[U.weight_dtype(c)]
    o = dict(x=rand(c.m, c.n, dtype=xt), w=rand(c.n, dtype=wt), b=rand(c.n, dtype=wt) if c.bias else None,
             rowscale=(torch.rand(c.m, device=DEV, generator=g) + 0.5).to(dt) if c.rowscale else None)
    if c.cell.direction == "fwd":
        o["res"] = rand(c.m, c.n, dtype=TORCH[U.residual_dtype(c)]) if c.residual else None
    else:
        o["dy"] = rand(c.m, c.n, dtype=dt) / 8
        o["dres"] = rand(c.m, c.n, dtype=xt) if c.residual else None
    return o


# ---- forward -------------------------------------------------------------------------------------------------------------------
def check_forward(x, w, b, res, rowscale, rms, y, stream, mean, rstd, what):
    want, mean64, rstd64 = fp64_forward(x, w, b, res, rowscale, EPS, rms, False)
    if y.dtype != FP32:
        assert_one_ulp(y, want, b, what)
    else:
        # an fp32 y has no 16-bit rounding to hide behind.  y = (z - mean) rstd w + b: the subtraction, two products and the add
        # round to 2^-24 of their operands, and mean and rstd carry as much again from their sums (assert_one_ulp: c = 8); mean's
        # error is relative to mean|z|, not to |z - mean|, so the terms are |w| rstd (|z| + |mean| + mean|z|) + |w xhat| + |b|
        z = x.double() * (rowscale.double()[:, None] if rowscale is not None else 1.0) + (res.double() if res is not None else 0.0)
        wd = w.double().abs()
        terms = wd * rstd64[:, None] * (z.abs() + mean64.abs()[:, None] + z.abs().mean(-1, keepdim=True))
        terms = terms + (want - (b.double() if b is not None else 0.0)).abs() + (b.double().abs() if b is not None else 0.0)
        need = needed_c(y, want, terms * 2.0 ** -24, FP32, False)
        print(f"{what}: fp32 y needs {need:.2f} x 2^-24 of the operands")
        assert need <= FP32_ROUNDINGS
    if res is not None or rowscale is not None:
        # one product that is exact in fp32 (16-bit factors) and one add: the stream is bit-equal to torch's.  An fp32 x with
        # both has two roundings in torch and may have one (an fma) in the kernel
        z = x.float() * rowscale.float()[:, None] if rowscale is not None else x.float()
        z = z + res.float() if res is not None else z
        if x.dtype == FP32 and res is not None and rowscale is not None:
            assert torch.allclose(stream, z, rtol=2.0 ** -22, atol=0)
        else:
            assert torch.equal(stream, z.to(stream.dtype)), what
    else:
        assert stream is x
    assert (mean is None) == rms
    assert torch.allclose(rstd.double(), rstd64, rtol=1e-5, atol=0), what


def check_statistics(x, w, b, res, rowscale, rms, cell, lo=1.0, **kw):
    """mean and rstd to 1e-5 relative.  A relative bound on a mean needs rows that have one: every row of x is offset (by lo to
    lo + 3), in place, so that a view keeps its strides, and the same launch is made again for its statistics alone."""
    x.copy_((x.float() + torch.linspace(lo, lo + 3, x.shape[0], device=DEV)[:, None]).to(x.dtype))
    plan = norm._plan_forward(x, w, b, EPS, res, rowscale=rowscale, is_rms_norm=rms, **kw)
    assert cell_of("fwd", plan) == cell
    _, _, mean, rstd = norm._launch_forward(x, w, b, EPS, res, rowscale=rowscale, is_rms_norm=rms, **kw)
    _, mean64, rstd64 = fp64_forward(x, w, b, res, rowscale, EPS, rms, False)
    assert torch.allclose(rstd.double(), rstd64, rtol=1e-5, atol=0)
    if not rms:
        assert torch.allclose(mean.double(), mean64, rtol=1e-5, atol=0)
    return plan


@pytest.mark.parametrize("c", FWD_CASES, ids=U.case_id)
def test_forward_case(c):
    o = operands(c, c.n)
    args = (o["x"], o["w"], o["b"], EPS, o["res"])
    kw = dict(rowscale=o["rowscale"], is_rms_norm=c.rms)
    assert cell_of("fwd", norm._plan_forward(*args, **kw)) == c.cell
    y, stream, mean, rstd = norm._launch_forward(*args, **kw)
    assert y.dtype == o["x"].dtype and (o["res"] is None or stream.dtype == o["res"].dtype)
    check_forward(o["x"], o["w"], o["b"], o["res"], o["rowscale"], c.rms, y, stream, mean, rstd, U.case_id(c))
    check_statistics(o["x"], o["w"], o["b"], o["res"], o["rowscale"], c.rms, c.cell)


# ---- backward ------------------------------------------------------------------------------------------------------------------
def statistics(x, rms):
    """mean and rstd of the rows of x in fp64, rounded to fp32: what the kernel is given and what the oracle computes with"""
    xd = x.double()
    mean = torch.zeros(x.shape[0], dtype=torch.float64, device=x.device) if rms else xd.mean(-1)
    rstd = 1 / torch.sqrt(((xd - mean[:, None]) ** 2).mean(-1) + EPS)
    return mean.float(), rstd.float()


def fp64_backward(x, dy, w, b, mean, rstd, dres, rowscale, rms):
    """plain torch in double -> dx, dresidual_in, dw, db, y and the terms T, sum|dy xhat|, sum|dy| of the bounds"""
    mean, rstd = mean.double()[:, None], rstd.double()[:, None]
    xhat, wdy = (x.double() - mean) * rstd, w.double() * dy.double()
    c1 = (xhat * wdy).mean(-1, keepdim=True)
    c2 = torch.zeros_like(c1) if rms else wdy.mean(-1, keepdim=True)
    dres_in = (wdy - (xhat * c1 + c2)) * rstd + (dres.double() if dres is not None else 0.0)
    dx = dres_in * rowscale.double()[:, None] if rowscale is not None else dres_in
    terms = rstd * (wdy.abs() + xhat.abs() * (xhat * wdy).abs().mean(-1, keepdim=True) + wdy.abs().mean(-1, keepdim=True))
    terms = terms + (dres.double().abs() if dres is not None else 0.0)
    dyd = dy.double()
    y = xhat * w.double() + (b.double() if b is not None else 0.0)
    return dict(dx=dx, dres_in=dres_in, dw=(dyd * xhat).sum(0), db=dyd.sum(0), y=y, t=terms, t_dw=(dyd * xhat).abs().sum(0),
                t_db=dyd.abs().sum(0))


def eager_backward(x, dy, w, b, dres, rowscale, rms, dx_dtype):
    """torch's eager fp32 evaluation of the same backward, its outputs rounded to the dtypes ours are written in"""
    leaf = lambda t: t.detach().float().clone().requires_grad_(True)  # noqa: E731  (a copy: .float() of an fp32 tensor is itself)
    s, w32, b32 = leaf(x), leaf(w), leaf(b) if b is not None else None
    y = (norm.rms_norm_ref if rms else norm.layer_norm_ref)(s, w32, b32, eps=EPS, upcast=True)
    grads = torch.autograd.grad(y, [s, w32] + ([b32] if b is not None else []), dy.float())
    dres_in = grads[0] + dres.float() if dres is not None else grads[0]
    dx = dres_in * rowscale.float()[:, None] if rowscale is not None else dres_in
    return dict(dx=dx.to(dx_dtype), dres_in=dres_in.to(x.dtype), dw=grads[1].to(w.dtype), db=grads[2].to(b.dtype) if b is not None else None)


def check_backward(o, rms, has_residual, dx_dtype, want_cell, what, recompute=False):
    """launch on the tensors of `o`, compare every output with fp64; returns the recomputed y"""
    x, dy, w, b, dres, rowscale = o["x"], o["dy"], o["w"], o["b"], o["dres"], o["rowscale"]
    mean, rstd = statistics(x, rms)
    args = (dy, x, w, b, None if rms else mean, rstd, dres, rowscale, has_residual, False, rms, dx_dtype, recompute)
    plan = norm._plan_backward(*args)
    assert cell_of("bwd", plan) == want_cell, what
    assert plan["grid_y"] == (-(-x.shape[1] // U.BWD_SLAB) if want_cell.team == "wide" else 1)
    dx, dw, db, dres_in, y = norm._launch_backward(*args)
    r = fp64_backward(x, dy, w, b, mean, rstd, dres, rowscale, rms)
    e = eager_backward(x, dy, w, b, dres, rowscale, rms, dx_dtype)
    assert dx.dtype == dx_dtype and dw.dtype == w.dtype and (db is None) == (b is None)
    scale = rowscale.double().abs()[:, None] if rowscale is not None else 1.0
    rows = [("dx", dx, e["dx"], r["dx"], r["t"] * scale)]
    if has_residual:
        assert dres_in.dtype == x.dtype
        assert (dres_in is dx) == (rowscale is None and dx_dtype == x.dtype)
        rows.append(("dx", dres_in, e["dres_in"], r["dres_in"], r["t"]))
    else:
        assert dres_in is None
    rows.append(("dw", dw, e["dw"], r["dw"], r["t_dw"]))
    if b is not None:
        rows.append(("dw", db, e["db"], r["db"], r["t_db"]))
    need = {}
    for kind, got, eager, ref, terms in rows:
        rounding = kind == "dw" or got.dtype != FP32
        need[kind] = tuple(max(a, b_) for a, b_ in zip(need.get(kind, (0.0, 0.0)), (
            needed_c(eager, ref, terms, got.dtype, rounding), needed_c(got, ref, terms, got.dtype, rounding))))
    print(f"c: {what} dx eager {need['dx'][0]:.3e} ours {need['dx'][1]:.3e} | dw eager {need['dw'][0]:.3e} ours {need['dw'][1]:.3e}")
    for kind, (_, c_ours) in need.items():
        assert c_ours <= 2 * C_EAGER[kind], f"{what} {kind}: ours needs c = {c_ours}, allowed {2 * C_EAGER[kind]}"
    if recompute:
        assert y.dtype == dy.dtype
        assert_one_ulp(y, r["y"], b, f"{what} y")
    return y


@pytest.mark.parametrize("c", BWD_CASES, ids=U.case_id)
def test_backward_case(c):
    check_backward(operands(c, c.n + 1), c.rms, c.residual, TORCH[c.dx_dtype], c.cell, U.case_id(c))


@pytest.mark.parametrize("cell,n", [(U.Cell("bwd", 8, "wide"), 8200), (U.Cell("bwd", 8, 256), 520)], ids=["wide", "team256"])
def test_backward_recomputes_y(cell, n):
    """p.y != NULL, what layer_norm_linear_fn asks for: y = xhat w + b written beside dx, held to assert_one_ulp"""
    c = next(c for c in BWD_CASES if c.cell == cell and c.n == n)._replace(bias=True, rms=False)
    assert c.x_dtype == c.dx_dtype == "bf16"
    check_backward(operands(c, 7), False, c.residual, BF16, cell, f"recompute {U.case_id(c)}", recompute=True)


# ---- the row loops: more rows per workgroup than the minimum, a ragged last workgroup; every row compared ---------------------
@pytest.mark.parametrize("m,n,team", [(8195, 1032, 256), (16389, 8, "wave")], ids=["team256_m8195", "wave_m16389"])
def test_forward_row_loop(m, n, team):
    c = U.Case(U.Cell("fwd", 8, team), n, m, True, "bf16", "bf16", False, False, False, True)
    o = operands(c, m)
    plan = norm._plan_forward(o["x"], o["w"], None, EPS, is_rms_norm=True)
    rows = U.fwd_rows_per_wg(m, team)
    assert cell_of("fwd", plan) == c.cell and plan["rows_per_wg"] == rows == {256: 4, "wave": 8}[team]
    assert m % rows and plan["grid_x"] == -(-m // rows)  # more than one row per team, and a ragged last workgroup
    y, stream, mean, rstd = norm._launch_forward(o["x"], o["w"], None, EPS, is_rms_norm=True)
    check_forward(o["x"], o["w"], None, None, None, True, y, stream, mean, rstd, f"m{m} n{n}")
    # the LayerNorm of the same rows for its statistics: the mean store of every row of the loop.  (Offsets from 4: the mean of
    # a row of 8 columns scatters by 0.35, and thousands of rows at an offset of 1 would put some means near zero)
    assert check_statistics(o["x"], o["w"], None, None, None, False, c.cell, lo=4.0)["rows_per_wg"] == rows


@pytest.mark.parametrize("n,team", [(8, "wave"), (520, 256)])
def test_backward_row_loop(n, team):
    m = 20487
    c = U.Case(U.Cell("bwd", 8, team), n, m, False, "bf16", "bf16", False, True, False, True)
    o = operands(c, m + n)
    mean, rstd = statistics(o["x"], False)
    plan = norm._plan_backward(o["dy"], o["x"], o["w"], o["b"], mean, rstd)
    assert plan["rows_per_wg"] == U.bwd_rows_per_wg(m) == 24 and m % 24 and plan["grid_x"] == -(-m // 24)
    check_backward(o, False, False, BF16, c.cell, f"m{m} n{n}")


# ---- element accesses on strided rows between canary columns -------------------------------------------------------------------
LEFT, PAD, CANARY = 3, 24, 77.0


def framed(t):
    """t's values in a buffer of row pitch N + 24 from column 3 on, canaries around: (buffer, the slice)"""
    buf = torch.full((t.shape[0], t.shape[1] + PAD), CANARY, device=DEV, dtype=t.dtype)
    view = buf[:, LEFT:LEFT + t.shape[1]]
    view.copy_(t)
    return buf, view


def canaries_intact(buf, n):
    return bool((buf[:, :LEFT] == CANARY).all() and (buf[:, LEFT + n:] == CANARY).all())


@pytest.mark.parametrize("n,team", [(8193, 1024), (16411, "wide")], ids=["team1024", "wide"])
def test_forward_strided_rows_between_canaries(n, team):
    c = next(c for c in FWD_CASES if c.cell == U.Cell("fwd", 1, team) and c.n == n)._replace(residual=True, bias=True, rowscale=False)
    o = operands(c, 11)
    (xb, x), (rb, res) = framed(o["x"]), framed(o["res"])
    (yb, out), (sb, stream) = framed(torch.zeros_like(o["x"])), framed(torch.zeros_like(o["res"]))
    kw = dict(is_rms_norm=c.rms, out=out, residual_out=stream)
    assert cell_of("fwd", norm._plan_forward(x, o["w"], o["b"], EPS, res, **kw)) == c.cell
    y, s, mean, rstd = norm._launch_forward(x, o["w"], o["b"], EPS, res, **kw)
    assert y.data_ptr() == out.data_ptr() and s.data_ptr() == stream.data_ptr()
    check_forward(o["x"], o["w"], o["b"], o["res"], None, c.rms, y, s, mean, rstd, f"strided n{n}")
    assert all(canaries_intact(t, n) for t in (xb, rb, yb, sb))
    assert torch.equal(x, o["x"]) and torch.equal(res, o["res"])
    # mean and rstd of the strided rows (LayerNorm, whatever the case's norm is)
    check_statistics(x, o["w"], o["b"], res, None, False, c.cell, out=out, residual_out=stream)
    assert all(canaries_intact(t, n) for t in (xb, rb, yb, sb))


def test_wide_backward_strided_rows_between_canaries():
    """The canaries surround what the caller owns: x, dy and dresidual, which the launch must leave as they are.  dx,
    dresidual_in, dw and db are allocated contiguous inside the binding and cannot be framed; their values are held to fp64 and
    to the bits of the same launch on contiguous rows."""
    n = 8203
    c = next(c for c in BWD_CASES if c.cell == U.Cell("bwd", 1, "wide") and c.n == n)._replace(residual=True, bias=True)
    o = operands(c, 13)
    frames = {k: framed(o[k]) for k in ("x", "dy", "dres")}
    strided = dict(o, **{k: v[1] for k, v in frames.items()})
    check_backward(strided, c.rms, True, BF16, c.cell, f"strided n{n}")
    for k, (buf, view) in frames.items():
        assert canaries_intact(buf, n) and torch.equal(view, o[k]), k
    # the same element kernel on contiguous rows: the same bits
    mean, rstd = statistics(o["x"], c.rms)
    args = (None if c.rms else mean, rstd)
    a = norm._launch_backward(strided["dy"], strided["x"], o["w"], o["b"], *args, strided["dres"], o["rowscale"], True, False, c.rms, BF16)
    b = norm._launch_backward(o["dy"], o["x"], o["w"], o["b"], *args, o["dres"], o["rowscale"], True, False, c.rms, BF16)
    assert all(torch.equal(p, q) for p, q in zip(a[:4], b[:4]))
