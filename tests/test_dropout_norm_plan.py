"""CPU tests of fa_dropout_norm_fwd_plan / fa_dropout_norm_bwd_plan (include/fa_dropout_norm.h) against
tests/dropout_norm_plan_universe.py: every case plans into the form the universe names for it, in both directions; both sides of
every boundary are among the cases; every kernel of the unit is reached.  Dummy aligned addresses, nothing dereferenced, no
device; tests/test_dropout_norm_gpu.py runs the same table on the kernels."""
import pytest

import dropout_norm_plan_universe as U
from flash_attention_annotated_amd import _lib

ADDR = 0x10000
OK, NULLP, BAD_SHAPE = 0, -1, -5
CODE = {"bf16": _lib.FA_DTYPE_BF16, "fp16": _lib.FA_DTYPE_FP16, "fp32": _lib.FA_DTYPE_FP32}
FWD_ROWS = ("x0", "x1", "residual", "z0", "z1", "x")
BWD_ROWS = ("dz0", "dz1", "dx", "x", "x0", "dx0", "dx1", "dresidual")


def stream_code(c):
    return CODE["fp32"] if U.stream_bytes(c) == 4 else CODE[c.x0]


def fwd_params(c, mask=True, **fields):
    """the forward of the case as the binding fills it: the stream written wherever it is not x0 itself, the mask asked for"""
    p = _lib.new_dropout_norm_fwd_params()
    p.M, p.N, p.p_dropout = c.m, c.n, c.p
    p.x0 = p.z0 = p.weight0 = p.rsigma = ADDR
    p.mu = 0 if c.rms else ADDR
    p.flags = _lib.FA_DROPOUT_NORM_RMS if c.rms else 0
    p.x0_dtype = p.z_dtype = p.rowscale_dtype = CODE[c.x0]
    p.weight_dtype = p.colscale_dtype = CODE[c.w]
    p.x_dtype = p.residual_dtype = stream_code(c)
    if c.bias:
        p.bias0 = ADDR
    if c.res:
        p.residual = ADDR
    if c.form == "scaled":
        p.rowscale = p.colscale = ADDR
    if U.two_weights(c):
        p.weight1 = p.z1 = ADDR
        p.bias1 = ADDR if c.bias else 0
    if U.has_x1(c):
        p.x1 = ADDR
    if c.p > 0:
        p.rng_state = ADDR
        if mask:
            p.dmask0 = ADDR
            p.dmask1 = ADDR if U.has_x1(c) else 0
    if c.prenorm or c.p > 0 or c.res or c.form in ("scaled", "parallel") or p.x_dtype != p.x0_dtype:
        p.x = ADDR
    for t in FWD_ROWS:
        setattr(p, f"{t}_row_stride", c.n)
    for k, v in fields.items():
        setattr(p, k, v)
    return p


def bwd_params(c, sized=True, **fields):
    p = _lib.new_dropout_norm_bwd_params()
    p.M, p.N, p.p_dropout = c.m, c.n, c.p
    p.dz0 = p.x = p.weight0 = p.rsigma = p.dx0 = p.dw0 = ADDR
    p.mu = 0 if c.rms else ADDR
    p.flags = _lib.FA_DROPOUT_NORM_RMS if c.rms else 0
    p.x0_dtype = p.dz_dtype = p.rowscale_dtype = CODE[c.x0]
    p.weight_dtype = p.colscale_dtype = CODE[c.w]
    p.x_dtype = stream_code(c)
    if c.bias:
        p.db0 = ADDR
    if c.prenorm:
        p.dx = ADDR
    if c.res and (c.p > 0 or c.form == "scaled" or p.x_dtype != p.x0_dtype):
        p.dresidual = ADDR
    if c.form == "scaled":
        p.rowscale = p.colscale = p.x0 = p.dcolscale = ADDR
    if U.two_weights(c):
        p.weight1 = p.dz1 = p.dw1 = ADDR
        p.db1 = ADDR if c.bias else 0
    if U.has_x1(c):
        p.dx1 = ADDR
    if c.p > 0:
        p.rng_state = ADDR
    for t in BWD_ROWS:
        setattr(p, f"{t}_row_stride", c.n)
    for k, v in fields.items():
        setattr(p, k, v)
    if sized:
        p.workspace, p.workspace_bytes = ADDR, _lib.load().fa_dropout_norm_bwd_workspace_bytes(p)
    return p


def plan_of(direction, c, **fields):
    lib, plan = _lib.load(), _lib.FaDropoutNormPlan()
    if direction == "fwd":
        st = lib.fa_dropout_norm_fwd_plan(fwd_params(c, **fields), plan)
    else:
        st = lib.fa_dropout_norm_bwd_plan(bwd_params(c, **fields), plan)
    assert st == OK, (U.case_id(c), direction, st)
    return plan


# ---- the universe itself -----------------------------------------------------------------------------------------------------
# both sides of every boundary of both directions, the narrowest and the widest row
PINNED = {
    8: [16, 512, 528, 1024, 1040, 2048, 2064, 4096, 4112, 8192, 8208, 16384, 16400, 32768],
    4: [16, 256, 272, 512, 528, 1024, 1040, 2048, 2064, 4096, 4112, 8192, 8208, 16384],
    1: [1, 127, 129, 203, 511, 513, 1023, 1025, 2047, 2049, 32767],
}


def test_cases_sit_on_both_sides_of_every_boundary():
    for cw, ns in PINNED.items():
        assert [c.n for c in U.CASES if c.cw == cw] == ns == U.widths(cw)
        for direction in ("fwd", "bwd"):
            cols = U.COLS[direction][cw]
            teams = {}
            for n in ns:
                teams.setdefault(U.team_of(direction, cw, n), []).append(n)
            assert set(teams) == set(U.TEAMS), (direction, cw)  # every team, the wide form included
            for team in (64, 256, 512, 1024):  # its last N is the boundary (the odd N next to it, for elements)
                assert max(teams[team]) == team * cols - (cw == 1), (direction, cw, team)
            for team in (256, 512, 1024, "wide"):  # its first N is the next possible one above the boundary below
                below = {256: 64, 512: 256, 1024: 512, "wide": 1024}[team] * cols
                assert min(teams[team]) == below + (1 if cw == 1 else 16), (direction, cw, team)
    assert len({U.case_id(c) for c in U.CASES}) == len(U.CASES)


def test_cases_cover_every_option_on_both_sides():
    for cw in (8, 4, 1):
        cases = [c for c in U.CASES if c.cw == cw]
        assert {c.p > 0 for c in cases} == {False, True}  # p = 0 against p > 0
        assert {c.p for c in U.CASES} == {0.0, 0.17, 0.9}
        assert {U.two_weights(c) for c in cases} == {False, True}  # one weight against two
        assert {c.form for c in cases} == set(U.FORMS)  # scales, x1: present and absent
        assert {c.rms for c in cases} == {False, True}
        assert {c.res is None for c in cases} == {False, True} and {c.prenorm for c in cases} == {False, True}
        assert {c.bias for c in cases} == {False, True}
        assert {U.stream_bytes(c) for c in cases} == ({4} if cw == 4 else {2, 4})
        wide = [c for c in cases if U.team_of("bwd", cw, c.n) == "wide"]
        assert {c.p > 0 for c in wide} == {False, True}, cw  # the slabs with and without decisions
    assert {c.x0 for c in U.CASES} == {"bf16", "fp16", "fp32"} == {c.w for c in U.CASES}
    for c in U.CASES:
        assert c.n * (4 if c.x0 == "fp32" else 2) <= U.MAX_ROW_BYTES and c.n * U.stream_bytes(c) <= U.MAX_ROW_BYTES
        assert (c.n % 16 == 0) == (c.cw != 1) and (c.x0 == "fp32") == (c.cw == 4)


def test_every_kernel_is_reached():
    reached = set()
    for c in U.CASES:
        reached |= U.kernels_of(c)
    assert reached == U.KERNELS


# ---- the plan against the universe ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", U.CASES, ids=U.case_id)
def test_case_plans_into_its_form(c):
    for direction in ("fwd", "bwd"):
        plan = plan_of(direction, c)
        assert U.form_of_plan(plan) == U.form_of(direction, c), direction
        team = U.team_of(direction, c.cw, c.n)
        assert plan.threads == (1024 if team == "wide" else team)
        assert plan.grid_y == U.grid_y_of(direction, c)
        assert (plan.grid_y > 1) == (direction == "bwd" and team == "wide")
        rows = U.fwd_rows_per_wg(c.m, team) if direction == "fwd" else U.bwd_rows_per_wg(c.m)
        assert plan.rows_per_wg == rows and plan.grid_x == -(-c.m // rows)
        assert plan.sums == (U.sums_of(c) if direction == "bwd" else 0)
    assert _lib.load().fa_dropout_norm_bwd_workspace_bytes(bwd_params(c, sized=False)) == U.bwd_workspace_bytes(c.m, c.n, U.sums_of(c))


def _case(cw, at=None, **kw):
    c = next(c for c in U.CASES if c.cw == cw and (at is None or c.n == at))
    return c._replace(**kw)


def test_exact_boundaries_of_the_element_form():
    """an even N is an element case through a misaligned base: the last N of every team and the first of the next"""
    for direction in ("fwd", "bwd"):
        for n, team in ((128, 64), (130, 256), (512, 256), (514, 512), (1024, 512), (1026, 1024), (2048, 1024), (2050, "wide")):
            plan = plan_of(direction, _case(1, 203, n=n), **{"x0" if direction == "fwd" else "dz0": ADDR + 2})
            assert U.form_of_plan(plan)[:2] == (1, team), (direction, n)


def test_p_selects_the_instantiation_and_nothing_else():
    for cw in (8, 4, 1):
        c = _case(cw, form="plain", res=None)
        for direction in ("fwd", "bwd"):
            a, b = plan_of(direction, c._replace(p=0.0)), plan_of(direction, c._replace(p=0.5))
            assert (a.dropout, b.dropout) == (0, 1)
            assert [getattr(a, f) for f in ("cw", "threads", "wide", "rows_per_wg", "grid_x", "grid_y", "sums")] == \
                   [getattr(b, f) for f in ("cw", "threads", "wide", "rows_per_wg", "grid_x", "grid_y", "sums")]


def test_grid_y_is_the_slab_count_exactly_when_wide_backward():
    c = _case(8, 32768)
    for n, slabs in ((8192, 1), (8208, 2), (16384, 2), (16400, 3), (24576, 3), (24592, 4), (32768, 4)):
        plan = plan_of("bwd", c._replace(n=n))
        assert plan.grid_y == slabs and bool(plan.wide) == (n > 8192)
    for n in (16400, 32768):
        plan = plan_of("fwd", c._replace(n=n))
        assert plan.wide and plan.grid_y == 1 and plan.grid_x == c.m and plan.rows_per_wg == 1 and plan.threads == 1024
    e = _case(1, 32767)
    assert plan_of("bwd", e).grid_y == 16 and plan_of("bwd", e._replace(n=2049)).grid_y == 2


@pytest.mark.parametrize("m", [1, 37, 2048, 4095, 4096, 8195, 16384, 20487, 65536, 1 << 20])
def test_rows_per_workgroup(m):
    c = _case(8, 1024, m=m)
    f, b = plan_of("fwd", c), plan_of("bwd", c)
    assert f.rows_per_wg == U.fwd_rows_per_wg(m, 64) and f.grid_x == -(-m // f.rows_per_wg)
    assert b.rows_per_wg == U.bwd_rows_per_wg(m) and b.grid_x == -(-m // b.rows_per_wg)
    assert U.fwd_rows_per_wg(8195, 256) == 4 and U.bwd_rows_per_wg(20487) == 21 and U.bwd_rows_per_wg(16384) == 16


VEC_CASES = [c for c in U.CASES if c.cw != 1 and c.n in (16, 1040, 4112, 16400)]


@pytest.mark.parametrize("c", VEC_CASES, ids=U.case_id)
def test_misalignment_turns_16_byte_accesses_into_element_accesses(c):
    """A base off 16 bytes, a row pitch that is no multiple of 16 bytes, a row of any operand that is no multiple of 16 bytes --
    the mask's included: cw 1, and the team of cw 1."""
    for direction, rows, build in (("fwd", FWD_ROWS, fwd_params), ("bwd", BWD_ROWS, bwd_params)):
        base = build(c)
        changes = [{"weight0": ADDR + 4}, {"weight0": ADDR + 8}]
        for t in (t for t in rows if getattr(base, t)):
            changes.append({t: ADDR + 4})
            changes.append({f"{t}_row_stride": c.n + 1})
        if direction == "fwd" and c.p > 0:
            changes.append({"dmask0": ADDR + 8})
        for change in changes:
            plan = plan_of(direction, c, **change)
            assert plan.cw == 1, (direction, change)
            assert U.form_of_plan(plan)[1] == U.team_of(direction, 1, c.n), (direction, change)
        # what does not bear on the accesses changes nothing: an aligned pitch, statistics and the row scale off 16 bytes
        for change in ({f"{rows[0]}_row_stride": c.n + 16}, {"rsigma": ADDR + 4}, {"rng_state": ADDR + 8} if c.p > 0 else {}):
            assert plan_of(direction, c, **change).cw == c.cw, (direction, change)
    # N a multiple of 8 but not of 16: 16-byte rows of every tensor, but not of the mask
    n8 = c._replace(n=c.n + 8)
    if c.p > 0 and n8.n * U.stream_bytes(c) <= U.MAX_ROW_BYTES:
        assert plan_of("fwd", n8).cw == 1 and plan_of("fwd", n8, mask=False).cw == c.cw
        assert plan_of("bwd", n8).cw == c.cw  # the backward has no mask


def test_backward_partial_count_does_not_depend_on_cw():
    for c in (_case(8, 1040), _case(8, 16400), _case(4, 16)):
        for m in (37, 3000, 20487):
            vec, elem = plan_of("bwd", c._replace(m=m)), plan_of("bwd", c._replace(m=m), x=ADDR + 4)
            assert vec.cw == c.cw and elem.cw == 1
            assert (vec.grid_x, vec.rows_per_wg, vec.sums) == (elem.grid_x, elem.rows_per_wg, elem.sums)
            sized = bwd_params(c._replace(m=m))
            assert _lib.load().fa_dropout_norm_bwd_validate(bwd_params(c._replace(m=m), x=ADDR + 4)) == OK
            assert sized.workspace_bytes == U.bwd_workspace_bytes(m, c.n, U.sums_of(c))


def test_plan_validates_first():
    lib = _lib.load()
    c = U.CASES[0]
    plan = _lib.FaDropoutNormPlan(cw=-7)
    assert lib.fa_dropout_norm_fwd_plan(None, plan) == NULLP and lib.fa_dropout_norm_bwd_plan(None, plan) == NULLP
    assert lib.fa_dropout_norm_fwd_plan(fwd_params(c, x0=0), plan) == NULLP
    assert lib.fa_dropout_norm_fwd_plan(fwd_params(c, N=0), plan) == BAD_SHAPE
    assert lib.fa_dropout_norm_bwd_plan(bwd_params(c, dx0=0), plan) == NULLP
    assert lib.fa_dropout_norm_bwd_plan(bwd_params(c, sized=False), plan) == -11  # FA_ERR_WORKSPACE, as the launch
    assert plan.cw == -7  # untouched
    assert lib.fa_dropout_norm_fwd_plan(fwd_params(c), None) == NULLP and lib.fa_dropout_norm_bwd_plan(bwd_params(c), None) == NULLP
