"""CPU tests of fa_gemm_act_fwd_plan / fa_gemm_act_dgrad_plan (include/fa_gemm_act.h) against tests/gemm_act_plan_universe.py:
the tile switch at M = 64, K-steps, the ragged flags, the grid and the dbias partial rows, on both sides of every boundary.
Dummy addresses, nothing dereferenced, no device; tests/test_gemm_act_gpu.py runs the cases on the kernels."""
import pytest

import gemm_act_plan_universe as U
from flash_attention_annotated_amd import _lib

ADDR = 0x10000
OK, NULLP, BAD_SHAPE = 0, -1, -5


def params(direction, m, n, k, dbias=False, **fields):
    if direction == "fwd":
        p = _lib.new_gemm_act_fwd_params()
        p.x, p.weight, p.out = ADDR, ADDR + (1 << 40), ADDR + (2 << 40)
        p.x_row_stride, p.weight_row_stride, p.out_row_stride, p.act_input_row_stride = k, k, n, n
    else:
        p = _lib.new_gemm_act_dgrad_params()
        p.grad_out, p.weight, p.grad_in, p.act_input = ADDR, ADDR + (1 << 40), ADDR + (2 << 40), ADDR + (3 << 40)
        p.grad_out_row_stride, p.weight_row_stride, p.grad_in_row_stride, p.act_input_row_stride = k, n, n, n
        if dbias:
            p.dbias, p.workspace, p.workspace_bytes = ADDR + (4 << 40), ADDR + (5 << 40), 1 << 50
    p.M, p.N, p.K, p.activation = m, n, k, _lib.FA_ACT_SQRELU
    for key, v in fields.items():
        setattr(p, key, v)
    return p


def plan_of(direction, p):
    plan = _lib.FaGemmActPlan()
    st = getattr(_lib.load(), f"fa_gemm_act_{direction}_plan")(p, plan)
    assert st == OK, st
    assert plan.dgrad == (direction == "dgrad") and plan.dtype == _lib.FA_DTYPE_BF16
    return U.Plan(*(getattr(plan, f) for f in U.Plan._fields))


def test_the_case_table_covers_every_boundary():
    assert U.boundaries_covered()
    assert all(U.form(*c) == "fused" for c in U.CASES) and all(U.form(*c) == "mm_act" for c in U.FALLBACK_CASES)
    assert U.form(128, 128, 64, "fp32") == "mm_act"
    # the pairs that straddle a boundary
    assert U.plan(64, 128, 64).tile_m == 64 and U.plan(65, 128, 64).tile_m == 128
    assert U.plan(128, 128, 64).k_steps == 1 and U.plan(128, 128, 72).k_steps == 2
    assert U.plan(1100, 1032, 264).tiles_m > U.GROUP_M


@pytest.mark.parametrize("case", U.CASES, ids=lambda c: "x".join(map(str, c)))
@pytest.mark.parametrize("direction", ["fwd", "dgrad"])
def test_plan_matches_the_universe(direction, case):
    m, n, k = case
    assert plan_of(direction, params(direction, m, n, k)) == U.plan(m, n, k)
    if direction == "dgrad":
        assert plan_of(direction, params(direction, m, n, k, dbias=True)) == U.plan(m, n, k, dbias=True)


@pytest.mark.parametrize("case", U.FALLBACK_CASES, ids=lambda c: "x".join(map(str, c)))
def test_fallback_shapes_are_refused_by_the_library(case):
    m, n, k = case
    lib, plan = _lib.load(), _lib.FaGemmActPlan()
    assert lib.fa_gemm_act_fwd_plan(params("fwd", m, n, k), plan) == BAD_SHAPE
    assert lib.fa_gemm_act_dgrad_plan(params("dgrad", m, n, k), plan) == BAD_SHAPE


def test_tile_switch_grid_and_partial_rows():
    lib = _lib.load()
    for m, tile_m, tiles_m in ((1, 64, 1), (64, 64, 1), (65, 128, 1), (128, 128, 1), (129, 128, 2), ((1 << 28) + 128, 128, (1 << 21) + 1)):
        p = params("dgrad", m, 8, 8, dbias=True)
        got = plan_of("dgrad", p)
        assert (got.tile_m, got.tiles_m, got.partial_rows, got.grid_x) == (tile_m, tiles_m, tiles_m, tiles_m)
        assert lib.fa_gemm_act_dgrad_workspace_bytes(p) == tiles_m * 8 * 4
    assert plan_of("fwd", params("fwd", 0, 8, 8)).grid_x == 0 == plan_of("dgrad", params("dgrad", 0, 8, 8, dbias=True)).grid_x
    assert plan_of("dgrad", params("dgrad", 300, 4096, 64, dbias=True)).reduce_grid_x == 2  # (512 chunks of 8 columns)
    # the plan is a function of the shape: strides and the optional tensors do not change it
    base = plan_of("fwd", params("fwd", 300, 264, 200))
    assert plan_of("fwd", params("fwd", 300, 264, 200, x_row_stride=208, bias=ADDR, act_input=ADDR + (3 << 40))) == base


def test_plan_validates_first():
    lib = _lib.load()
    plan = _lib.FaGemmActPlan(tile_m=-7)
    assert lib.fa_gemm_act_fwd_plan(None, plan) == NULLP and lib.fa_gemm_act_dgrad_plan(None, plan) == NULLP
    assert lib.fa_gemm_act_fwd_plan(params("fwd", 37, 12, 8), plan) == BAD_SHAPE
    assert lib.fa_gemm_act_dgrad_plan(params("dgrad", 37, 8, 8, grad_in=0), plan) == NULLP
    assert plan.tile_m == -7  # untouched
    assert lib.fa_gemm_act_fwd_plan(params("fwd", 37, 8, 8), None) == NULLP
    assert lib.fa_gemm_act_dgrad_plan(params("dgrad", 37, 8, 8), None) == NULLP
