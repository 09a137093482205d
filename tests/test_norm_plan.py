"""CPU tests of fa_norm_fwd_plan / fa_norm_bwd_plan (include/fa_norm.h) against tests/norm_plan_universe.py: every case of the
table plans into the cell it names, every cell has its cases, and the plan's grid, rows per workgroup and workspace are what the
universe's restatement of DESIGN 4.22 says.  Dummy aligned addresses, nothing dereferenced, no device;
tests/test_norm_forms_gpu.py runs the same table on the kernels."""
import pytest

import norm_plan_universe as U
from flash_attention_annotated_amd import _lib

ADDR = 0x10000
OK, NULLP, BAD_SHAPE = 0, -1, -5
CODE = {"bf16": _lib.FA_DTYPE_BF16, "fp16": _lib.FA_DTYPE_FP16, "fp32": _lib.FA_DTYPE_FP32}
FWD_ROWS = ("x", "residual", "y", "residual_out")
BWD_ROWS = ("x", "dy", "dresidual", "dx", "dresidual_in", "y")


def fwd_params(c, **fields):
    p = _lib.new_norm_fwd_params()
    p.M, p.N = c.m, c.n
    p.x = p.y = p.weight = p.rstd = ADDR
    p.mean = 0 if c.rms else ADDR
    p.flags = _lib.FA_NORM_RMS if c.rms else 0
    p.x_dtype = p.y_dtype = CODE[c.x_dtype]
    p.weight_dtype = p.bias_dtype = CODE[U.weight_dtype(c)]
    if c.bias:
        p.bias = ADDR
    if c.rowscale:
        p.rowscale, p.rowscale_dtype = ADDR, p.x_dtype
    if c.residual:
        p.residual = p.residual_out = ADDR
        p.residual_dtype = p.residual_out_dtype = CODE[U.residual_dtype(c)]
    elif c.rowscale:
        p.residual_out, p.residual_out_dtype = ADDR, p.x_dtype
    for t in FWD_ROWS:
        setattr(p, f"{t}_row_stride", c.n)
    for k, v in fields.items():
        setattr(p, k, v)
    return p


def bwd_params(c, sized=True, **fields):
    p = _lib.new_norm_bwd_params()
    p.M, p.N = c.m, c.n
    p.x = p.dy = p.weight = p.rstd = p.dx = p.dw = ADDR
    p.mean = 0 if c.rms else ADDR
    p.flags = _lib.FA_NORM_RMS if c.rms else 0
    p.x_dtype = p.dresidual_dtype = p.dresidual_in_dtype = CODE[c.x_dtype]
    p.dx_dtype = p.dy_dtype = p.y_dtype = CODE[c.dx_dtype]
    p.weight_dtype = p.bias_dtype = CODE[U.weight_dtype(c)]
    if c.bias:
        p.bias = p.db = ADDR
    if c.rowscale:
        p.rowscale, p.rowscale_dtype = ADDR, p.dx_dtype
    if c.residual:
        p.dresidual = ADDR
        if c.rowscale or c.dx_dtype != c.x_dtype:
            p.dresidual_in = ADDR
    for t in BWD_ROWS:
        setattr(p, f"{t}_row_stride", c.n)
    for k, v in fields.items():
        setattr(p, k, v)
    if sized:
        p.workspace, p.workspace_bytes = ADDR, _lib.load().fa_norm_bwd_workspace_bytes(p)
    return p


def plan_of(c, **fields):
    lib, plan = _lib.load(), _lib.FaNormPlan()
    if c.cell.direction == "fwd":
        st = lib.fa_norm_fwd_plan(fwd_params(c, **fields), plan)
    else:
        st = lib.fa_norm_bwd_plan(bwd_params(c, **fields), plan)
    assert st == OK, (U.case_id(c), st)
    return plan


# ---- the universe itself -----------------------------------------------------------------------------------------------------
def test_cells_are_the_forms_of_the_design():
    fwd = {(c.cw, c.team) for c in U.CELLS if c.direction == "fwd"}
    bwd = {(c.cw, c.team) for c in U.CELLS if c.direction == "bwd"}
    assert fwd == {(cw, t) for cw in (8, 4, 1) for t in ("wave", 256, 512, 1024)} | {(8, "wide"), (1, "wide")}
    assert bwd == {(cw, t) for cw in (8, 4, 1) for t in U.TEAMS}


# both sides of every boundary, the ragged last slabs and the limits: what a cell's smallest and largest N come to
PINNED = {
    ("fwd", 8): {8, 1024, 1032, 4096, 4104, 8192, 8200, 16384, 16392, 32768},
    ("fwd", 4): {4, 1024, 1028, 4096, 4100, 8192, 8196, 16384},
    ("fwd", 1): {1, 1023, 1025, 4095, 4097, 8191, 8193, 16383, 16385, 16411, 32767},
    ("bwd", 8): {8, 512, 520, 2048, 2056, 4096, 4104, 8192, 8200, 32768},
    ("bwd", 4): {4, 512, 516, 2048, 2052, 4096, 4100, 8192, 8196, 16384},
    ("bwd", 1): {1, 511, 513, 2047, 2049, 4095, 4097, 8191, 8193, 8203, 32767},
}


def test_every_cell_has_its_cases():
    by_cell = {}
    for c in U.CASES:
        by_cell.setdefault(c.cell, []).append(c)
    assert set(by_cell) == set(U.CELLS)
    for cell in U.CELLS:
        cases = by_cell[cell]
        assert [c.n for c in cases] == U.widths(cell), cell
        assert {c.rms for c in cases} == {False, True}, cell  # LayerNorm and RMSNorm across the cell's widths
        assert all(c.m == (U.WIDE_ROWS if cell.team == "wide" else U.ROWS) for c in cases)
        for feature in ("residual", "bias", "rowscale", "w_fp32"):
            assert any(getattr(c, feature) for c in cases), (cell, feature)
    for (direction, cw), ns in PINNED.items():
        assert {c.n for c in U.CASES if c.cell.direction == direction and c.cell.cw == cw} == ns, (direction, cw)
    assert len({U.case_id(c) for c in U.CASES}) == len(U.CASES)


def test_case_widths_fit_their_cw():
    for c in U.CASES:
        assert c.n % c.cell.cw == 0 and (c.cell.cw != 1 or c.n % 2 == 1), U.case_id(c)
        assert (c.x_dtype == "fp32") == (c.cell.cw == 4)
        assert c.n * (4 if c.x_dtype == "fp32" else 2) <= U.MAX_ROW_BYTES
    # an fp32 stream with a 16-bit gradient and with an fp32 one, in the wide form too
    wide4 = [c for c in U.CASES if c.cell == U.Cell("bwd", 4, "wide")]
    assert {c.dx_dtype for c in wide4} == {"bf16", "fp32"}
    # wide cases: a last slab that is ragged by whole chunks, one ragged by elements, and a full one at the limit
    for direction, span in (("fwd", 1024 * 8), ("bwd", U.BWD_SLAB)):
        rest = {c.n % span for c in U.CASES if c.cell.direction == direction and c.cell.team == "wide"}
        assert 0 in rest and 8 in rest and any(r % 8 for r in rest), (direction, rest)


# ---- the plan against the universe ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", U.CASES, ids=U.case_id)
def test_case_plans_into_its_cell(c):
    plan = plan_of(c)
    assert U.cell_of_plan(c.cell.direction, plan) == c.cell
    team = c.cell.team
    assert plan.threads == (1024 if team == "wide" else 256 if team == "wave" else team)
    assert plan.grid_y == U.grid_y_of(c)
    assert (plan.grid_y > 1) == (c.cell.direction == "bwd" and team == "wide")
    rows = U.fwd_rows_per_wg(c.m, team) if c.cell.direction == "fwd" else U.bwd_rows_per_wg(c.m)
    assert plan.rows_per_wg == rows and plan.grid_x == -(-c.m // rows)
    if c.cell.direction == "bwd":
        assert _lib.load().fa_norm_bwd_workspace_bytes(bwd_params(c, sized=False)) == U.bwd_workspace_bytes(c.m, c.n)
        assert U.bwd_workspace_bytes(c.m, c.n) == plan.grid_x * c.n * 8 + (c.m * 8 if plan.wide else 0)


def test_grid_y_is_the_slab_count_exactly_when_wide_backward():
    c = next(c for c in U.CASES if c.cell == U.Cell("bwd", 8, "wide"))
    for n, slabs in ((8192, 1), (8200, 2), (16384, 2), (16392, 3), (24576, 3), (24584, 4), (32768, 4)):
        plan = plan_of(c._replace(n=n))
        assert plan.grid_y == slabs and bool(plan.wide) == (n > 8192)
    f = next(c for c in U.CASES if c.cell == U.Cell("fwd", 8, "wide"))
    for n in (16392, 32768):
        plan = plan_of(f._replace(n=n))
        assert plan.wide and plan.grid_y == 1 and plan.grid_x == f.m and plan.rows_per_wg == 1


def test_fp32_rows_are_never_wide_in_the_forward():
    """check_shape ends an fp32 row where the forward's wide form begins"""
    c = next(c for c in U.CASES if c.cell == U.Cell("fwd", 4, 1024) and c.n == 16384)
    plan = plan_of(c)
    assert not plan.wide and plan.threads == 1024 and plan.cw == 4
    lib = _lib.load()
    assert lib.fa_norm_fwd_plan(fwd_params(c._replace(n=16388)), _lib.FaNormPlan()) == BAD_SHAPE
    assert lib.fa_norm_fwd_validate(fwd_params(c._replace(n=16388))) == BAD_SHAPE
    # ... and element accesses of an fp32 x end there too
    assert not plan_of(c._replace(n=16383)).wide
    assert lib.fa_norm_fwd_plan(fwd_params(c._replace(n=16385)), _lib.FaNormPlan()) == BAD_SHAPE


@pytest.mark.parametrize("m", [1, 37, 2048, 4095, 4096, 8195, 16384, 16389, 20487, 65536, 1 << 20])
def test_rows_per_workgroup(m):
    wave = next(c for c in U.CASES if c.cell == U.Cell("fwd", 8, "wave"))
    team = next(c for c in U.CASES if c.cell == U.Cell("fwd", 8, 256))
    for c in (wave, team):
        plan = plan_of(c._replace(m=m))
        assert plan.rows_per_wg == U.fwd_rows_per_wg(m, c.cell.team) and plan.grid_x == -(-m // plan.rows_per_wg)
    for cell in (U.Cell("bwd", 8, "wave"), U.Cell("bwd", 8, 256)):
        c = next(c for c in U.CASES if c.cell == cell)
        plan = plan_of(c._replace(m=m))
        assert plan.rows_per_wg == U.bwd_rows_per_wg(m) and plan.grid_x == -(-m // plan.rows_per_wg)
    assert U.fwd_rows_per_wg(8195, 256) == 4 and U.fwd_rows_per_wg(16389, "wave") == 8
    assert U.bwd_rows_per_wg(20487) == 24 and U.bwd_rows_per_wg(16384) == 16


VEC_CASES = [c for c in U.CASES if c.cell.cw != 1 and c.n in (8, 4, 1032, 4100, 16392, 520, 8200, 8196)]


@pytest.mark.parametrize("c", VEC_CASES, ids=U.case_id)
def test_misalignment_turns_16_byte_accesses_into_element_accesses(c):
    """A base off by an element, a row pitch that is no multiple of 16 bytes, or a weight off 16 bytes: cw 1, same team."""
    es = 4 if c.x_dtype == "fp32" else 2
    rows = FWD_ROWS if c.cell.direction == "fwd" else BWD_ROWS
    build = fwd_params if c.cell.direction == "fwd" else bwd_params
    present = [t for t in rows if getattr(build(c), t)]
    changes = [{"weight": ADDR + 4}, {"weight": ADDR + 8}]
    for t in present:
        size = 4 if getattr(build(c), f"{t}_dtype") == _lib.FA_DTYPE_FP32 else 2
        changes.append({t: ADDR + max(2, size)})  # off by 2 bytes where the element allows it
        changes.append({f"{t}_row_stride": c.n + 16 // size - 1})
    if c.bias and c.cell.direction == "fwd":
        changes.append({"bias": ADDR + 4})
    assert "x" in present and es
    for change in changes:
        plan = plan_of(c, **change)
        assert plan.cw == 1, change
        assert U.cell_of_plan(c.cell.direction, plan) == c.cell._replace(cw=1), change
    # what does not bear on the accesses changes nothing: an aligned pitch, statistics and rowscale off 16 bytes
    for change in ({"x_row_stride": c.n + 16 // es}, {"rstd": ADDR + 4}, {"dw": ADDR + 4} if c.cell.direction == "bwd" else {}):
        assert plan_of(c, **change).cw == c.cell.cw, change
    if c.cell.direction == "bwd" and c.bias:  # the backward reads the bias only for y
        assert plan_of(c, bias=ADDR + 4).cw == c.cell.cw
        assert plan_of(c, bias=ADDR + 4, y=ADDR).cw == 1


def test_backward_partial_count_does_not_depend_on_cw():
    for cell in (U.Cell("bwd", 8, 256), U.Cell("bwd", 8, "wide"), U.Cell("bwd", 4, "wave")):
        c = next(c for c in U.CASES if c.cell == cell)
        for m in (37, 3000, 20487):
            vec, elem = plan_of(c._replace(m=m)), plan_of(c._replace(m=m), x=ADDR + 4)
            assert vec.cw == cell.cw and elem.cw == 1
            assert (vec.grid_x, vec.grid_y, vec.rows_per_wg, vec.threads) == (elem.grid_x, elem.grid_y, elem.rows_per_wg, elem.threads)


def test_plan_validates_first():
    lib = _lib.load()
    c = U.CASES[0]
    plan = _lib.FaNormPlan(cw=-7)
    assert lib.fa_norm_fwd_plan(None, plan) == NULLP and lib.fa_norm_bwd_plan(None, plan) == NULLP
    assert lib.fa_norm_fwd_plan(fwd_params(c, x=0), plan) == NULLP
    assert lib.fa_norm_fwd_plan(fwd_params(c, N=0), plan) == BAD_SHAPE
    b = next(c for c in U.CASES if c.cell.direction == "bwd")
    assert lib.fa_norm_bwd_plan(bwd_params(b, dx=0), plan) == NULLP
    assert lib.fa_norm_bwd_plan(bwd_params(b, sized=False), plan) == -11  # FA_ERR_WORKSPACE, as the launch
    assert plan.cw == -7  # untouched
    assert lib.fa_norm_fwd_plan(fwd_params(c), None) == NULLP and lib.fa_norm_bwd_plan(bwd_params(b), None) == NULLP
