"""GPU tests of every launch form of csrc/fa_dropout_norm.hip against fp64, element by element.  The two custom ops are called
directly (ops.layer_norm._dropout_norm_fwd / _dropout_norm_bwd on the arguments of _forward_args), as the autograd functions call
them: the backward is given its statistics and its rng_state, nothing goes through autograd, and every call first asks the plan
of the very tensors which form it takes and holds that to the cell the case names.

Decisions: the forward returns rng_state, and dropout_norm_oracle.mask_ref restates the hash on the host side; a returned mask
must equal it bit for bit, and every oracle below runs under mask_ref's decisions, not the kernel's.
Forward: the stream against the fp64 contract, |x - x64| <= [ulp(x64)] + K_STREAM 2^-24 A, A the sum of the absolute values of the
terms added (bit-equal to torch's fp32 evaluation rounded once where nothing is dropped or scaled); mu and rsigma to 1e-5 relative
and z0 / z1 under test_norm_gpu's one-ulp rule, all three against fp64 statistics of the stream the kernel returned.
Backward: mu / rsigma given as the fp64 statistics of the saved stream rounded to fp32, and per element and per column
    |g - ref64| <= [ulp(ref64)] + c terms,
the terms those of dropout_norm_oracle.backward_ref, c twice what torch's eager fp32 evaluation of the same formulas needs
(C_EAGER).  The p of the oracles is the float the C ABI carries (fa_dropout_norm_*_params.p_dropout), the p of the decisions
the caller's.
"""
import pytest
import torch

import dropout_norm_oracle as O
import dropout_norm_plan_universe as U
from flash_attention_annotated_amd.ops import layer_norm as L
from flash_attention_annotated_amd.ops.norm import _DTYPE_CODE
from test_dropout_norm_gpu import DT, EPS, operands
from test_norm_forms_gpu import canaries_intact, framed, ulp_of
from test_norm_gpu import FP32_ROUNDINGS, assert_one_ulp, ordered_bits, ulp16

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, FP16, FP32 = torch.bfloat16, torch.float16, torch.float32

# The fp32 roundings fwd_x can make on the way to one element of the stream, each at most 2^-24 of a value that A bounds: the
# product by rowscale, the product by colscale, the product by 1 / (1 - p) and the rounding of 1 / (1 - p) itself to fp32 (four
# on the x0 term; the x1 term has the last two), then the add of the x1 term and the add of the residual (each 2^-24 of a partial
# sum, which A bounds).  The rounding to a 16-bit stream is the ulp term.
K_STREAM = 6

# C_EAGER: what torch's eager fp32 evaluation of the same backward (dropout_norm_oracle.backward_ref on fp32 upcasts under the
# same masks, its gradients rounded to the dtypes ours are written in) needs as c over every backward case of this file (85),
# measured on an MI355X: 2.371e-7 for dx0, dx1 and dresidual (ours: 2.106e-7, the same case: cw 4, N = 4096, scaled, p = 0.17),
# 2.321e-7 for dw, db and dcolscale (ours: 1.949e-7, the same case: cw 8, N = 4088, two weights, p = 0.9); a 16-bit gradient
# needs none at all in most cases: it is the fp64 result rounded.  Ours is allowed twice the eager figure: the two add a row's
# and a column's terms in different orders, and neither order is the more exact.  DESIGN 4.26.
C_EAGER = {"row": 2.38e-7, "col": 2.33e-7}


def abi_p(p):
    return float(torch.tensor(p, dtype=FP32))


def spacing(ref, dtype):
    """the spacing of `dtype` at |ref| in fp64: ulp_of above the subnormals, nothing at an exact zero"""
    least = {BF16: 2.0 ** -133, FP16: 2.0 ** -24, FP32: 2.0 ** -149}[dtype]
    return torch.where(ref == 0, torch.zeros_like(ref), ulp_of(ref, dtype).clamp_min(least))


def needed_c(got, ref, terms, rounding):
    """the smallest c with |got - ref| <= [ulp(ref)] + c terms"""
    over = (got.double() - ref).abs()
    if rounding:
        over = (over - spacing(ref, got.dtype)).clamp_min(0.0)
    return float((over / terms.clamp_min(1e-300)).max())


def named_columns(n, cw, threads):
    """the first and the last column of every chunk of threads * cw columns -- chunk k of the threads, a walk of a wide forward,
    a chunk of a slab of a wide backward -- full (body) or cut by the row's end (tail)"""
    span, cols = threads * cw, {}
    for k in range(-(-n // span)):
        kind = "body" if (k + 1) * span <= n else "tail"
        cols[f"chunk {k} ({kind}) first"] = k * span
        cols[f"chunk {k} ({kind}) last"] = min(n, (k + 1) * span) - 1
    return cols


def assert_ok(what, ok, cols):
    if bool(ok.all()):
        return
    for where, col in cols.items():
        assert bool(ok[..., col].all()), f"{what}: {where} (column {col})"
    raise AssertionError(f"{what}: first element out of bounds at {(~ok).nonzero()[0].tolist()}")


def tensors(c, seed=None):
    x0, kw = operands(c.m, c.n, DT[c.x0], DT[c.w], c.res, c.rms, c.form, c.bias, c.n if seed is None else seed)
    return dict(x0=x0, x1=kw.get("x1"), res=kw.get("res"), w0=kw["w0"], b0=kw.get("b0"), w1=kw.get("w1"), b1=kw.get("b1"),
                rowscale=kw.get("rowscale"), colscale=kw.get("colscale"))


# ---- forward -------------------------------------------------------------------------------------------------------------------
def forward(c, o, mask):
    """-> the plan of the call and (z0, z1, x, dmask0, dmask1, mu, rsigma, rng_state)"""
    raw = (o["x0"], o["x1"], o["res"], o["w0"], o["b0"], o["w1"], o["b1"], o["rowscale"], o["colscale"], c.p, EPS, c.r32, c.rms,
           True, mask)
    return L._plan_forward(*raw), L._dropout_norm_fwd(*L._forward_args(*raw))


def assert_forward_plan(c, plan):
    form = U.form_of("fwd", c)
    assert U.form_of_plan(plan) == form, plan
    rows = U.fwd_rows_per_wg(c.m, form[1])
    assert plan["grid_y"] == 1 and plan["rows_per_wg"] == rows and plan["grid_x"] == -(-c.m // rows) and plan["sums"] == 0


def decisions(c, rng_state):
    """mask_ref's decisions of the two streams under the rng_state the forward returned (None: nothing is drawn)"""
    if c.p == 0.0:
        return None, None
    seed, offset = rng_state.tolist()
    return (O.mask_ref(seed, offset, c.m, c.n, 0, c.p, device=DEV),
            O.mask_ref(seed, offset, c.m, c.n, 1, c.p, device=DEV) if U.has_x1(c) else None)


def oracle_forward(c, o, keep0, keep1, **kw):
    return O.forward_ref(o["x0"], o["w0"], o["b0"], o["x1"], o["res"], o["w1"], o["b1"], o["rowscale"], o["colscale"], abi_p(c.p),
                         keep0, keep1, EPS, c.rms, **kw)


def one_ulp_ok(y, want, bias):
    """test_norm_gpu.assert_one_ulp's rule, element by element"""
    want16 = want.to(y.dtype)
    if bias is None:
        return (ordered_bits(y.contiguous()) - ordered_bits(want16)).abs() <= 1
    operands_ = (want - bias.double()).abs() + bias.double().abs()
    return (y.double() - want16.double()).abs() <= ulp16(want16) + FP32_ROUNDINGS * 2.0 ** -24 * operands_


def check_z(what, z, want, w, b, f, x, cols):
    if z.dtype != FP32:
        assert_ok(what, one_ulp_ok(z, want, b), cols)
        assert_one_ulp(z, want, b, what)
        return
    # an fp32 z: test_norm_forms_gpu.check_forward's rule, FP32_ROUNDINGS x 2^-24 of the operands
    xd, bd = x.double(), b.double() if b is not None else 0.0
    terms = w.double().abs() * f["rsigma"][:, None] * (xd.abs() + f["mu"].abs()[:, None] + xd.abs().mean(-1, keepdim=True))
    terms = (terms + (want - bd).abs() + (b.double().abs() if b is not None else 0.0)) * 2.0 ** -24
    print(f"{what}: fp32 z needs {needed_c(z, want, terms, False):.2f} x 2^-24 of the operands")
    assert_ok(what, (z.double() - want).abs() <= FP32_ROUNDINGS * terms, cols)


def check_mean(c, o, mask, form):
    """mu (and rsigma) to 1e-5 relative on rows that have a mean: every row of x0, x1 and the residual offset by 4 .. 7 and the
    layerscale made positive, so that a row's terms have one sign; the same launch again for its statistics alone"""
    off = torch.linspace(4.0, 7.0, c.m, device=DEV)[:, None]
    o = dict(o, **{k: (o[k].float() + off).to(o[k].dtype) for k in ("x0", "x1", "res") if o[k] is not None})
    if o["colscale"] is not None:
        o["colscale"] = o["colscale"].abs()
    plan, outs = forward(c, o, mask)
    assert U.form_of_plan(plan) == form
    mu64, rs64 = O.statistics(outs[2], EPS, c.rms)
    assert torch.allclose(outs[6].double(), rs64, rtol=1e-5, atol=0)
    assert torch.allclose(outs[5].double(), mu64, rtol=1e-5, atol=0)


def check_forward(c, o, what, mask=True, outs=None, mean=True):
    """one forward against the plan, mask_ref and fp64 -> (x, rng_state, keep0, keep1)"""
    if outs is None:
        plan, outs = forward(c, o, mask)
        assert_forward_plan(c, plan)
    z0, z1, x, dmask0, dmask1, mu, rsigma, rng_state = outs
    form = U.form_of("fwd", c)
    cols = named_columns(c.n, form[0], 1024 if form[1] == "wide" else form[1])
    stream_dtype = o["res"].dtype if o["res"] is not None else FP32 if c.r32 else o["x0"].dtype
    assert x.shape == z0.shape == o["x0"].shape and x.dtype == stream_dtype and z0.dtype == o["x0"].dtype
    assert (z1.numel() > 0) == U.two_weights(c) and mu.numel() == (0 if c.rms else c.m) and rsigma.numel() == c.m
    keep0, keep1 = decisions(c, rng_state)
    assert dmask0.numel() == (x.numel() if mask and c.p > 0 else 0)
    assert dmask1.numel() == (x.numel() if mask and c.p > 0 and U.has_x1(c) else 0)
    if dmask0.numel():
        assert_ok(f"{what} dmask0", dmask0 == keep0, cols)
    if dmask1.numel():
        assert_ok(f"{what} dmask1", dmask1 == keep1, cols)
    # the stream
    f = oracle_forward(c, o, keep0, keep1)
    bound = K_STREAM * 2.0 ** -24 * f["a"] + (spacing(f["x"], x.dtype) if x.dtype != FP32 else 0.0)
    eager = oracle_forward(c, o, keep0, keep1, dtype=FP32)["x"].to(x.dtype)
    assert bool(((eager.double() - f["x"]).abs() <= bound).all()), f"{what}: torch's fp32 stream is out of the bound"
    assert_ok(f"{what} x", (x.double() - f["x"]).abs() <= bound, cols)
    if c.p == 0.0 and c.form != "scaled":  # no product, only adds: torch's fp32 evaluation in the same order, rounded once
        assert_ok(f"{what} x bits", x == eager, cols)
    # the statistics and the outputs, of the stream that was returned
    g = oracle_forward(c, o, keep0, keep1, x=x)
    assert torch.allclose(rsigma.double(), g["rsigma"], rtol=1e-5, atol=0), what
    if not c.rms and mean:
        check_mean(c, o, mask, form)
    check_z(f"{what} z0", z0, g["z0"], o["w0"], o["b0"], g, x, cols)
    if U.two_weights(c):
        check_z(f"{what} z1", z1, g["z1"], o["w1"], o["b1"], g, x, cols)
    return x, rng_state, keep0, keep1


# ---- backward ------------------------------------------------------------------------------------------------------------------
def gradients_in(c, o, x, seed):
    """dz0, dz1 ~ N(0, 1) / 8 in the output dtype, dx ~ N(0, 1) in the stream's (prenorm)"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    rand = lambda dtype, scale: (torch.randn(c.m, c.n, device=DEV, generator=g) * scale).to(dtype)  # noqa: E731
    dz0 = rand(o["x0"].dtype, 0.125)
    dz1 = rand(o["x0"].dtype, 0.125) if U.two_weights(c) else None
    return dz0, dz1, rand(x.dtype, 1.0) if c.prenorm else None


def backward_args(c, o, x, rng_state, dz0, dz1, dx):
    mu64, rs64 = O.statistics(x, EPS, c.rms)
    return (dz0, dz1, dx, x, o["x0"] if o["colscale"] is not None else None, None if c.rms else mu64.float(), rs64.float(), o["w0"],
            o["w1"], o["rowscale"], o["colscale"], rng_state, c.p, U.has_x1(c), o["res"] is not None, o["b0"] is not None, c.rms)


def backward(c, o, args):
    return L._plan_backward(*args, o["x0"].dtype), L._dropout_norm_bwd(*args, _DTYPE_CODE[o["x0"].dtype])


def assert_backward_plan(c, plan):
    assert U.form_of_plan(plan) == U.form_of("bwd", c), plan
    rows = U.bwd_rows_per_wg(c.m)
    assert plan["grid_y"] == U.grid_y_of("bwd", c) and plan["rows_per_wg"] == rows and plan["grid_x"] == -(-c.m // rows)
    assert plan["sums"] == U.sums_of(c)


def check_backward(c, o, x, rng_state, keep0, keep1, what, grads=None, outs=None):
    dz0, dz1, dx = grads or gradients_in(c, o, x, c.n + 1)
    args = backward_args(c, o, x, rng_state, dz0, dz1, dx)
    if outs is None:
        plan, outs = backward(c, o, args)
        assert_backward_plan(c, plan)
    form = U.form_of("bwd", c)
    cols = named_columns(c.n, form[0], 1024 if form[1] == "wide" else form[1])
    kw = dict(x0=o["x0"], rowscale=o["rowscale"], colscale=o["colscale"], p=abi_p(c.p), keep0=keep0, keep1=keep1,
              has_x1=U.has_x1(c), rms=c.rms)
    r = O.backward_ref(x, args[5], args[6], dz0, o["w0"], dz1, o["w1"], dx, **kw)
    e = O.backward_ref(x, args[5], args[6], dz0, o["w0"], dz1, o["w1"], dx, dtype=FP32, **kw)
    names = ("dx0", "dx1", "dresidual", "dw0", "db0", "dw1", "db1", "dcolscale")
    need = {"row": (0.0, 0.0), "col": (0.0, 0.0)}
    for name, got in zip(names, outs):
        if not got.numel():  # (dresidual: none where there is no residual, or where dx0 serves)
            assert name not in ("dx0", "dw0") and (name != "dx1" or not U.has_x1(c))
            continue
        kind = "row" if name in ("dx0", "dx1", "dresidual") else "col"
        want_dtype = o["x0"].dtype if name in ("dx0", "dx1") else x.dtype if name == "dresidual" else \
            o["colscale"].dtype if name == "dcolscale" else o["w0"].dtype
        assert got.dtype == want_dtype and got.shape == (r[name].shape), name
        terms, rounding = r["t" if name == "dresidual" else "t_" + name], kind == "col" or got.dtype != FP32
        need[kind] = (max(need[kind][0], needed_c(e[name].to(got.dtype), r[name], terms, rounding)),
                      max(need[kind][1], needed_c(got, r[name], terms, rounding)))
        bound = 2 * C_EAGER[kind] * terms + (spacing(r[name], got.dtype) if rounding else 0.0)
        assert_ok(f"{what} {name}", (got.double() - r[name]).abs() <= bound, cols)
    print(f"c: {what} row eager {need['row'][0]:.3e} ours {need['row'][1]:.3e} | col eager {need['col'][0]:.3e} ours {need['col'][1]:.3e}")
    for kind, (_, ours) in need.items():
        assert ours <= 2 * C_EAGER[kind], f"{what} {kind}: ours needs c = {ours}, allowed {2 * C_EAGER[kind]}"
    if c.p > 0.0:  # dropped elements are exactly zero
        assert not bool(outs[0][keep0 == 0].any())
        assert not U.has_x1(c) or not bool(outs[1][keep1 == 0].any())
    return outs


def run_case(c, what=None, mask=True, bwd_cw=None):
    """bwd_cw: the access shape of the backward where it is not the forward's (a returned mask binds the forward alone)"""
    what = what or U.case_id(c)
    o = tensors(c)
    x, rng_state, keep0, keep1 = check_forward(c, o, what, mask)
    check_backward(c._replace(cw=bwd_cw or c.cw), o, x, rng_state, keep0, keep1, what)


# ---- every universe case -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", U.CASES, ids=U.case_id)
def test_universe_case(c):
    run_case(c)


# ---- the 16-byte forms with dropout at N % 16 != 0: no returned mask, the decisions from mask_ref -----------------------------
def _ragged_cases():
    """cw = 8: a row that ends in half a mask word (N % 16 == 8), at the narrow widths of the seeded grid, 1032, and on both
    sides of every team boundary of both directions, for bf16 and fp16.  cw = 4: N % 16 in (4, 12), on both sides of the boundary
    that both directions have at 2048, and one wide row; fp32 weights, since 16-byte rows of a 16-bit vector need N % 8 == 0"""
    cases = []
    ns8 = sorted({8, 24, 264, 1032} | {b + d for b in U.boundaries(8) for d in (-8, 8)})
    for x0 in ("bf16", "fp16"):
        for i, n in enumerate(ns8, start=int(x0 == "fp16")):  # (fp16 one step on: every width meets other options)
            form = U.FORMS[i % 5]
            res = (None, "fp32", "same")[i % 3] if form != U.FORMS[4] else None
            r32 = res is None and i % 2 == 1
            if n * 4 > U.MAX_ROW_BYTES:
                res, r32 = ("same" if res else None), False
            wide = U.team_of("bwd", 8, n) == "wide"
            cases.append(U.Case(n, U.WIDE_ROWS if wide else U.ROWS, 8, x0, ("fp32", "bf16", "fp16")[i % 3], (0.17, 0.9)[i % 2],
                                bool((i // 2) % 2), form, res, r32, bool((i + 1) % 2), i % 3 != 1))
    for i, n in enumerate((4, 12, 36, 260, 2044, 2052, 8196)):
        form = U.FORMS[i % 5]
        wide = U.team_of("bwd", 4, n) == "wide"
        cases.append(U.Case(n, U.WIDE_ROWS if wide else U.ROWS, 4, "fp32", "fp32", (0.17, 0.9)[i % 2], bool((i // 2) % 2), form,
                            (None, "fp32")[i % 2] if form != U.FORMS[4] else None, False, bool((i + 1) % 2), i % 3 != 1))
    return cases


RAGGED = _ragged_cases()


def test_ragged_cases_cover_what_they_are_for():
    for cw in (8, 4):
        cases = [c for c in RAGGED if c.cw == cw]
        assert all(c.p > 0 and c.n % 16 != 0 and c.n % cw == 0 for c in cases)
        assert {c.p for c in cases} == {0.17, 0.9} and {c.rms for c in cases} == {False, True}
        assert {c.form for c in cases} == set(U.FORMS)
        assert {c.n % 16 for c in cases} == ({8} if cw == 8 else {4, 12})
    for x0 in ("bf16", "fp16"):
        ns = {c.n for c in RAGGED if c.x0 == x0}
        assert {8, 24, 264, 1032} <= ns
        for direction in ("fwd", "bwd"):  # both sides of every team boundary
            assert {U.team_of(direction, 8, n) for n in ns} == set(U.TEAMS)
            for t in (64, 256, 512, 1024):
                b = t * U.COLS[direction][8]
                assert {b - 8, b + 8} <= ns or b >= U.max_n(8)
    assert {4, 12, 36, 260, 2052} <= {c.n for c in RAGGED if c.cw == 4}
    assert U.team_of("fwd", 4, 2044) != U.team_of("fwd", 4, 2052) and U.team_of("bwd", 4, 2044) != U.team_of("bwd", 4, 2052)


def test_every_kernel_and_every_cell_is_reached():
    """from the case tables: every case asserts the plan of its own call against its cell, in both directions"""
    reached = set()
    for c in U.CASES:
        reached |= U.kernels_of(c)
    assert reached == U.KERNELS
    ragged = {(d, c.cw) for c in RAGGED for d in ("fwd", "bwd")}
    assert ragged == {(d, cw) for d in ("fwd", "bwd") for cw in (8, 4)}
    cells = {(d,) + U.form_of(d, c)[:3] for c in U.CASES for d in ("fwd", "bwd")}
    assert {cell[:3] for cell in cells} == {(d, cw, t) for d in ("fwd", "bwd") for cw in (8, 4, 1) for t in U.TEAMS}
    assert {(cell[1], cell[3]) for cell in cells} == {(cw, drop) for cw in (8, 4, 1) for drop in (False, True)}


def test_a_returned_mask_changes_no_bits():
    """the premise of the cases below, at a width where the 16-byte form can return its mask: with and without return_dmask
    the same kernel draws the same decisions and writes the same z0, x, mu and rsigma"""
    c = next(c for c in U.CASES if c.cw == 8 and c.n == 1040 and c.p > 0)
    o = tensors(c)
    runs = []
    for mask in (True, False):
        torch.manual_seed(40)
        plan, outs = forward(c, o, mask)
        assert plan["cw"] == 8 and plan["dropout"]
        runs.append((plan, outs))
    assert runs[0][0] == runs[1][0]
    for i in (0, 1, 2, 5, 6, 7):
        assert torch.equal(runs[0][1][i], runs[1][1][i]), i
    assert runs[0][1][3].numel() and not runs[1][1][3].numel()


@pytest.mark.parametrize("c", RAGGED, ids=U.case_id)
def test_16_byte_forms_with_dropout_at_ragged_widths(c):
    o = tensors(c)
    raw = (o["x0"], o["x1"], o["res"], o["w0"], o["b0"], o["w1"], o["b1"], o["rowscale"], o["colscale"], c.p, EPS, c.r32, c.rms, True)
    assert L._plan_forward(*raw, True)["cw"] == 1  # (a returned mask would take the element form)
    plan = L._plan_forward(*raw, False)
    assert plan["cw"] == c.cw and plan["dropout"]
    x, rng_state, keep0, keep1 = check_forward(c, o, U.case_id(c), mask=False)
    args = backward_args(c, o, x, rng_state, *gradients_in(c, o, x, c.n + 1))
    plan = L._plan_backward(*args, o["x0"].dtype)
    assert plan["cw"] == c.cw and plan["dropout"]
    check_backward(c, o, x, rng_state, keep0, keep1, U.case_id(c))


# ---- the row loops: every row compared -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask", [True, False], ids=["elements_mask", "16_bytes_no_mask"])
@pytest.mark.parametrize("m,n,rows", [(3 * 2048 + 5, 24, 3), (8 * 2048 + 3, 264, 8)])
def test_forward_row_loop(m, n, rows, mask):
    """more than one row per workgroup and a ragged last workgroup; with the mask returned (N % 16 == 8: the element form) every
    row's mask against mask_ref, without it the 16-byte form under mask_ref's decisions"""
    c = U.Case(n, m, 1 if mask else 8, "bf16", "bf16", 0.17, False, "parallel", "same", False, True, True)
    assert U.fwd_rows_per_wg(m, U.team_of("fwd", c.cw, n)) == rows and m % rows  # (the plan is held to it in check_forward)
    run_case(c, f"fwd rows m{m} n{n}", mask, bwd_cw=8)  # (the backward has no mask: 16-byte accesses either way)


@pytest.mark.parametrize("n", [24, 520])
def test_backward_row_loop(n):
    """M = 20487: 21 rows per workgroup, 12 in the last"""
    m = 20487
    c = U.Case(n, m, 8, "bf16", "fp32", 0.17, False, "scaled", "fp32", False, True, True)
    assert U.bwd_rows_per_wg(m) == 21 and m % 21 == 12
    run_case(c, f"bwd rows m{m} n{n}", mask=False)


@pytest.mark.parametrize("form", ["parallel", "scaled"])
def test_wide_backward_three_workgroups(form):
    """M = 37 over slabs: workgroups of 16, 16 and 5 rows, whose partial rows must carry the sums of all their rows"""
    c = U.Case(8208, 37, 8, "bf16", "bf16", 0.17, False, form, "same", False, True, True)
    assert U.team_of("bwd", 8, c.n) == "wide" and U.bwd_rows_per_wg(c.m) == 16 and U.grid_y_of("bwd", c) == 2
    run_case(c, f"wide bwd m37 {form}")


# ---- element accesses on strided rows between canary columns -------------------------------------------------------------------
@pytest.mark.parametrize("n,team,res", [(2047, 1024, "same"), (2049, "wide", "fp32")], ids=["team1024", "wide"])
def test_strided_rows_between_canaries(n, team, res):
    """x0, x1, the residual, dz0 and dx at a pitch of N + 24 from column 3 on: the launches leave them and the canaries as they
    are, and write the bits of the same launches on contiguous copies"""
    c = U.Case(n, U.ROWS, 1, "bf16", "fp32", 0.17, False, "parallel", res, False, True, True)
    assert U.team_of("fwd", 1, n) == U.team_of("bwd", 1, n) == team
    o = tensors(c)
    frames = {k: framed(o[k]) for k in ("x0", "x1", "res")}
    strided = dict(o, **{k: v[1] for k, v in frames.items()})
    runs = []
    for operands_ in (strided, o):
        torch.manual_seed(n)
        runs.append(forward(c, operands_, True))
    (plan, outs), (plan_c, outs_c) = runs
    assert_forward_plan(c, plan)
    assert plan == plan_c and all(torch.equal(a, b) for a, b in zip(outs, outs_c))
    for k, (buf, view) in frames.items():
        assert canaries_intact(buf, n) and torch.equal(view, o[k]), k
    x, rng_state, keep0, keep1 = check_forward(c, o, f"strided n{n}", outs=outs, mean=False)
    dz0, dz1, dx = gradients_in(c, o, x, n + 1)
    gframes = {"dz0": framed(dz0), "dx": framed(dx)}
    args = backward_args(c, o, x, rng_state, dz0, dz1, dx)
    args_s = (gframes["dz0"][1], dz1, gframes["dx"][1]) + args[3:]
    (plan, bouts), (plan_c, bouts_c) = backward(c, o, args_s), backward(c, o, args)
    assert_backward_plan(c, plan)
    assert plan == plan_c and all(torch.equal(a, b) for a, b in zip(bouts, bouts_c))
    for (buf, view), t in zip(gframes.values(), (dz0, dx)):
        assert canaries_intact(buf, n) and torch.equal(view, t)
    check_backward(c, o, x, rng_state, keep0, keep1, f"strided n{n}", grads=(dz0, dz1, dx), outs=bouts)


# ---- the mask of the widest row ------------------------------------------------------------------------------------------------
def test_mask_structure_in_the_wide_form():
    """N = 32768 in the 16-byte form: three walks of 1024 threads x 8 columns x 4 steps; both masks are mask_ref's, so no
    decision repeats with the walk, the step or the stream"""
    c = U.Case(32768, 5, 8, "bf16", "bf16", 0.5, False, "parallel", None, False, True, True)
    assert U.team_of("fwd", 8, c.n) == "wide"
    o = tensors(c)
    plan, outs = forward(c, o, True)
    assert_forward_plan(c, plan)
    seed, offset = outs[7].tolist()
    for stream in (0, 1):
        assert torch.equal(outs[3 + stream], O.mask_ref(seed, offset, c.m, c.n, stream, c.p, device=DEV)), stream
    assert not torch.equal(outs[3], outs[4])
    check_forward(c, o, "widest row", outs=outs)
