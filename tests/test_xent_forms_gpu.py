"""GPU tests of csrc/fa_xent.hip by form: the label at every place where another piece of code finds it (element head, element
tail, first / last element of a chunk, first / last chunk of a slab), on the 16-byte and on the element kernel, and the walking
loops with their grid cap exceeded (tests/xent_plan_universe.py).  Every case asks the plan which form the call takes first.
Oracle, bounds and C_EAGER are those of tests/test_xent_gpu.py."""
import pytest
import torch

import xent_plan_universe as U
from flash_attention_annotated_amd.ops.triton import cross_entropy as xent
from flash_attention_annotated_amd.ops.triton.cross_entropy import cross_entropy_grad_ref, cross_entropy_ref
from test_xent_gpu import C_EAGER, IGNORE, TOL16, TOL32, accept, ulp16

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, FP32 = torch.bfloat16, torch.float32
TORCH = {"bf16": BF16, "fp32": FP32}
SETTINGS = [(0.0, 1.0, 0.0), (0.1, 0.7, 1e-2)]  # (smoothing, logit_scale, lse_square_scale) of test_16_bit_gradient_is_rounded_once


def rows_at_phase(m, n, dtype, head, fill=None):
    """(m, n) rows in a buffer of pitch N + pad, a multiple of 16 bytes, whose every row begins `head` elements before a 16-byte
    boundary: (buffer, the rows)"""
    cw = 16 // dtype.itemsize
    pitch = -(-n // cw) * cw + cw
    off = (cw - head) % cw
    buf = torch.zeros(off + m * pitch + cw, device=DEV, dtype=dtype)
    assert buf.data_ptr() % 16 == 0
    rows = buf[off:off + m * pitch].view(m, pitch)[:, :n]
    if fill is not None:
        rows.copy_(fill)
    return buf, rows


def rounding_bound(r_dx, terms, dtype):
    """test_16_bit_gradient_is_rounded_once's rule with its allowance 2 * C_EAGER; an fp32 gradient rounds to fp32"""
    ulp = ulp16(r_dx, dtype) if dtype != FP32 else torch.exp2(torch.frexp(r_dx).exponent.double() - 24)
    return ulp + 2 * C_EAGER * terms


def label_problem(dtype, head, tail, start=0):
    """one row per label position of the geometry (head, tail); with start > 0 also labels just outside the columns"""
    name = "bf16" if dtype == BF16 else "fp32"
    cw, n = U.cw_of(name), U.label_width(name, head, tail)
    probe = rows_at_phase(1, n, dtype, head)[1]
    g = U.pieces_of(probe.data_ptr(), name, n, cw)
    assert (g.head, g.nbody, g.tail) == (head, U.BWD_SLAB + 300, tail)
    at = U.label_positions(g, cw, n)
    names, cols = list(at), list(at.values())
    if start:  # just below and just above the columns this rank holds: out of range, the -1 path
        names += ["label below the first column", "label above the last column"]
        cols += [-1, n]
    m = len(cols)
    gen = torch.Generator(device=DEV).manual_seed(1000 * head + 10 * tail + cw)
    x = (torch.randn(m, n, device=DEV, generator=gen) * 2).to(dtype)
    y = torch.tensor(cols, device=DEV) + start
    d = torch.randn(m, device=DEV, generator=gen)
    return names, g, n, x, y, d


@pytest.mark.parametrize("start", [0, 4096], ids=["whole", "split"])
@pytest.mark.parametrize("element_kernel", [False, True], ids=["vec", "elem"])
@pytest.mark.parametrize("dtype", [BF16, FP32], ids=["bf16", "fp32"])
def test_label_at_every_position(dtype, element_kernel, start):
    cw = 16 // dtype.itemsize
    tol = TOL32 if dtype == FP32 else TOL16
    for head in U.edges(cw):
        for tail in U.edges(cw):
            names, g, n, x, y, d = label_problem(dtype, head, tail, start)
            m, total = len(names), n + (start + 100 if start else 0)
            _, logits = rows_at_phase(m, n, dtype, head, x)
            # dlogits of the same phase: the 16-byte kernel; of another phase: the element kernel
            out_buf, out = rows_at_phase(m, n, dtype, (head + 1) % cw if element_kernel else head)
            for s, scale, z in SETTINGS:
                args = (s, scale, z, IGNORE, start, total)
                fplan = xent._plan_forward(logits, y, None, *args, False)
                assert (fplan["cw"], fplan["grid_x"], fplan["lse_given"]) == (cw, m, 0)
                losses, lse, _ = xent._xent_fwd(logits, y, None, *args, False)
                r_losses, _, r_lse = cross_entropy_ref(x.double(), y, None, s, scale, z, IGNORE, start, total)
                e_losses, _, _ = cross_entropy_ref(x, y, None, s, scale, z, IGNORE, start, total)
                accept(f"losses h{head} t{tail}", losses, e_losses, r_losses, TOL32)
                bplan = xent._plan_backward(d, logits, y, lse, out, *args)
                assert bplan["cw"] == (1 if element_kernel else cw) and bplan["grid_y"] == m
                assert bplan["grid_x"] == -(-(n if element_kernel else -(-n // cw)) // U.BWD_SLAB) >= 2
                out_buf.fill_(77.0)
                xent._binding().xent_bwd(d, logits, y, lse, out, *args)
                r_dx = cross_entropy_grad_ref(x.double(), y, r_lse, d, s, scale, z, IGNORE, start, total)
                e_dx = cross_entropy_grad_ref(x, y, r_lse.float(), d, s, scale, z, IGNORE, start, total).to(dtype)
                accept(f"dlogits h{head} t{tail}", out, e_dx, r_dx, tol)
                # by name: at the label's column dlogits - d scale p (1 + 2 z lse) is -d scale (1 - s + s / N), at its
                # neighbours -d scale s / N -- r_dx holds exactly that -- to the rounding rule, every column of the row
                p = torch.exp(x.double() * scale - r_lse[:, None])
                lab = y - start
                at_label = torch.arange(n, device=DEV)[None, :] == lab[:, None]
                terms = (d.double().abs() * scale)[:, None] * (p * (1 + 2 * z * r_lse.abs())[:, None] + at_label.double())
                good = (out.double() - r_dx).abs() <= rounding_bound(r_dx, terms, dtype)
                for r, name in enumerate(names):
                    where = f"{name} (column {int(lab[r])}, head {g.head}, tail {g.tail}, s {s})"
                    for col in (int(lab[r]) - 1, int(lab[r]), int(lab[r]) + 1):
                        if 0 <= col < n:
                            assert bool(good[r, col]), f"label at the {where}: dlogits wrong at column {col}"
                    assert bool(good[r].all()), f"label at the {where}: dlogits wrong elsewhere in the row"
                # nothing outside the rows is written
                assert int((out_buf == 77.0).sum()) == out_buf.numel() - m * n


# ---- the walking loops -------------------------------------------------------------------------------------------------------
def walk(name):
    w = next(w for w in U.WALKS if w.name == name)
    items, extent = U.cap_exceeded(w)
    assert items > extent
    return w


def walk_problem(w, ignored_rows, label_dtype=torch.int64):
    gen = torch.Generator(device=DEV).manual_seed(w.m % 1000 + w.n)
    x = (torch.randn(w.m, w.n, device=DEV, generator=gen) * 2).to(TORCH[w.dtype])
    y = torch.randint(0, w.n, (w.m,), device=DEV, generator=gen)
    y[ignored_rows] = IGNORE
    x[ignored_rows] = float("nan")  # ignored rows are not read
    return x, y.to(label_dtype), torch.randn(w.m, device=DEV, generator=gen)


def check_plan(plan, w):
    assert U.Plan(plan["cw"], plan["grid_x"], plan["grid_y"], plan["lse_given"]) == U.walk_plan(w)


def reference_dlogits(x, y, lse, d):
    r_dx = cross_entropy_grad_ref(x.double(), y, lse.double(), d)
    e_dx = cross_entropy_grad_ref(x, y, lse, d).to(x.dtype)
    return r_dx, e_dx


def test_walk_backward_rows():
    """Rows beyond grid.y, every row against the oracle: a row step that is too large, or a walk that ends early, leaves rows
    unwritten.  A step that is too small is not reliably seen here, although the call is in place: with the step gridDim.y - 1
    row 65534 is taken twice, but at N = 8 the tensor is 1 MB and the second workgroup mostly reads the row's original logits
    still, so both write the same gradient (MI355X: seen in one run of six).  test_walk_backward_rows_wide is the case for
    that."""
    w = walk("backward rows")
    ignored = torch.tensor([7, 65533, 65536, 65540], device=DEV)  # (rows 0 and 65534 are kept: the ends of the first pass)
    x, y, d = walk_problem(w, ignored)
    losses, lse, _ = xent._xent_fwd(x, y, None, 0.0, 1.0, 0.0, IGNORE, 0, w.n, False)
    r_dx, e_dx = reference_dlogits(x, y, lse, d)
    at_label = torch.arange(w.n, device=DEV)[None, :] == y[:, None]
    terms = d.double().abs()[:, None] * (torch.exp(x.double() - lse.double()[:, None]) + at_label.double())
    check_plan(xent._plan_backward(d, x, y, lse, x), w)
    xent._xent_bwd_inplace(d, x, y, lse, 0.0, 1.0, 0.0, IGNORE, 0, w.n)
    accept("dlogits", x, e_dx, r_dx, TOL16)
    assert (x[ignored].view(torch.int16) == 0).all()
    keep = y != IGNORE
    assert bool(((x.double() - r_dx).abs() <= rounding_bound(r_dx, terms, BF16))[keep].all())


def test_walk_backward_rows_wide():
    """The rows walk in place at N = 1024: a row taken twice is the gradient of the gradient.  Observed on an MI355X with the
    row step gridDim.y - 1: row 65534, which workgroups 0 and 65534 both take, differs at N = 256, 1024 and 2048 (three runs
    each, and once more in this test) and in one run of six at N = 8.  Supposed, not measured: the row written first has left the cache it was written to by the time
    it is read again only when the tensor is larger than the caches.  All rows are held to the bits of the same launch out of
    place, which reads nothing it writes; the first, the last and the rows around the grid's end to the oracle."""
    w = walk("backward rows, wide")
    ignored = torch.tensor([7, 65533, 65536, 65540], device=DEV)
    x, y, d = walk_problem(w, ignored)
    _, lse, _ = xent._xent_fwd(x, y, None, 0.0, 1.0, 0.0, IGNORE, 0, w.n, False)
    apart = xent._xent_bwd(d, x, y, lse, 0.0, 1.0, 0.0, IGNORE, 0, w.n)
    rows = torch.cat([torch.arange(0, 16, device=DEV), torch.arange(65520, w.m, device=DEV)])
    r_dx, e_dx = reference_dlogits(x[rows], y[rows], lse[rows], d[rows])
    check_plan(xent._plan_backward(d, x, y, lse, x), w)
    xent._xent_bwd_inplace(d, x, y, lse, 0.0, 1.0, 0.0, IGNORE, 0, w.n)
    differ = (x.view(torch.int16) != apart.view(torch.int16)).any(1).nonzero().flatten().tolist()
    assert not differ, f"in place differs from out of place in rows {differ[:8]}: taken twice?"
    accept("dlogits", x[rows], e_dx, r_dx, TOL16)
    assert (x[ignored].view(torch.int16) == 0).all()


@pytest.mark.parametrize("name", ["backward slabs, element kernel", "backward slabs, 16-byte kernel"])
def test_walk_backward_slabs(name):
    w = walk(name)
    dtype = TORCH[w.dtype]
    cw = 16 // dtype.itemsize
    gen = torch.Generator(device=DEV).manual_seed(w.n)
    x = (torch.randn(w.m, w.n, device=DEV, generator=gen) * 2).to(dtype)
    y = torch.tensor([w.n - 1, 256 * U.BWD_SLAB * (cw if w.same_phase else 1) + 1], device=DEV)  # in the walked slabs
    d = torch.randn(w.m, device=DEV, generator=gen)
    _, logits = rows_at_phase(w.m, w.n, dtype, 0, x)
    out_buf, out = rows_at_phase(w.m, w.n, dtype, 0 if w.same_phase else 1)
    out_buf.fill_(77.0)
    _, lse, _ = xent._xent_fwd(logits, y, None, 0.0, 1.0, 0.0, IGNORE, 0, w.n, False)
    check_plan(xent._plan_backward(d, logits, y, lse, out), w)
    xent._binding().xent_bwd(d, logits, y, lse, out, 0.0, 1.0, 0.0, IGNORE, 0, w.n)
    r_dx, e_dx = reference_dlogits(x, y, lse, d)
    accept("dlogits", out, e_dx, r_dx, TOL32 if dtype == FP32 else TOL16)
    at_label = torch.arange(w.n, device=DEV)[None, :] == y[:, None]
    terms = d.double().abs()[:, None] * (torch.exp(x.double() - lse.double()[:, None]) + at_label.double())
    assert bool(((out.double() - r_dx).abs() <= rounding_bound(r_dx, terms, dtype)).all())
    assert int((out_buf == 77.0).sum()) == out_buf.numel() - w.m * w.n
    # an ignored row among them: zeros over every slab, its logits unread
    y[0] = IGNORE
    logits[0] = float("nan")
    out_buf.fill_(77.0)
    xent._binding().xent_bwd(d, logits, y, lse, out, 0.0, 1.0, 0.0, IGNORE, 0, w.n)
    assert not out[0].any() and int((out_buf == 77.0).sum()) == out_buf.numel() - w.m * w.n
    assert bool(((out[1].double() - r_dx[1]).abs() <= rounding_bound(r_dx[1], terms[1], dtype)).all())


def test_walk_forward_rows():
    w = walk("forward rows")
    ignored = torch.tensor([1, (1 << 20) - 1, 1 << 20, (1 << 20) + 2], device=DEV)
    x, y, _ = walk_problem(w, ignored)
    check_plan(xent._plan_forward(x, y), w)
    losses, lse, z_losses = xent._xent_fwd(x, y, None, 0.0, 1.0, 1e-2, IGNORE, 0, w.n, False)
    clean = x.clone()
    clean[ignored] = 0.0
    r_losses, r_z, r_lse = cross_entropy_ref(clean.double(), y, lse_square_scale=1e-2)
    e_losses, e_z, e_lse = cross_entropy_ref(clean, y, lse_square_scale=1e-2)
    accept("losses", losses, e_losses, r_losses, TOL32)
    accept("z_losses", z_losses, e_z, r_z, TOL32)
    keep = y != IGNORE
    accept("lse", lse[keep], e_lse[keep], r_lse[keep], TOL32)
    assert not losses[ignored].any() and not z_losses[ignored].any()


def test_walk_lse_given_rows():
    w = walk("lse_given rows")
    ignored = torch.tensor([3, 65536 * 256 - 1, 65536 * 256, 65536 * 256 + 4], device=DEV)
    x, y, _ = walk_problem(w, ignored, torch.int32)
    lse = torch.logsumexp(x.float(), dim=1)
    check_plan(xent._plan_forward(x, y, lse), w)
    losses, _, z_losses = xent._xent_fwd(x, y, lse, 0.0, 1.0, 1e-2, IGNORE, 0, w.n, False)
    keep = y != IGNORE
    x_lab = x.gather(1, y.long().clamp(0, w.n - 1)[:, None])[:, 0].double()
    z64 = 1e-2 * lse.double().square()
    r_losses = torch.where(keep, lse.double() - x_lab + z64, torch.zeros_like(z64))
    e_losses = torch.where(keep, lse - x_lab.float() + 1e-2 * lse.square(), torch.zeros_like(lse))
    accept("losses", losses, e_losses, r_losses, TOL32)
    accept("z_losses", z_losses, torch.where(keep, 1e-2 * lse.square(), torch.zeros_like(lse)), torch.where(keep, z64, torch.zeros_like(z64)), TOL32)
    assert not losses[ignored].any() and not z_losses[ignored].any()
