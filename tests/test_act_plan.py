"""CPU tests of fa_act_fwd_plan / fa_act_bwd_plan (include/fa_act.h) against tests/act_plan_universe.py: cw from dtype and
alignment, the caps of grid.x / grid.y, and the walking cases planned with their cap actually exceeded.  Dummy addresses,
nothing dereferenced, no device; tests/test_act_forms_gpu.py runs the cells and the walks on the kernels."""
import pytest

import act_plan_universe as U
from flash_attention_annotated_amd import _lib

ADDR = 0x10000
OK, NULLP, BAD_SHAPE = 0, -1, -5
CODE = {"bf16": _lib.FA_DTYPE_BF16, "fp16": _lib.FA_DTYPE_FP16, "fp32": _lib.FA_DTYPE_FP32}


def params(direction, m, h, dtype="bf16", gated=False, vec=True, dbias=False, recompute=False, **fields):
    """contiguous tensors (gated: the halves of (m, 2h) tensors) at aligned addresses where `vec`, else with pre one element off"""
    p = (_lib.new_act_fwd_params if direction == "fwd" else _lib.new_act_bwd_params)()
    es = U.ESIZE[dtype]
    pitch = -(-h // (16 // es)) * (16 // es) if vec else h  # (a pitch of whole 16 bytes, or the bare width)
    for t in ("pre", "up", "bias", "out") + (() if direction == "fwd" else ("dout", "dpre", "dup", "dbias")):
        setattr(p, f"{t}_dtype", CODE[dtype])
    p.M, p.H, p.activation = m, h, _lib.FA_ACT_SILU
    p.pre = ADDR if vec else ADDR + es
    p.pre_row_stride = p.out_row_stride = pitch
    if gated:
        p.flags, p.up, p.pre_row_stride = _lib.FA_ACT_GATED, p.pre + pitch * es, 2 * pitch
    if direction == "fwd":
        p.out = ADDR + (1 << 40)
    else:
        p.dout, p.dpre, p.dout_row_stride, p.dpre_row_stride = ADDR + (1 << 40), ADDR + (2 << 40), pitch, pitch
        if gated:
            p.dup, p.dpre_row_stride = p.dpre + pitch * es, 2 * pitch
        if dbias:
            p.dbias, p.workspace, p.workspace_bytes = ADDR + (3 << 40), ADDR + (4 << 40), 1 << 40
        if recompute:
            p.recompute_out = ADDR + (5 << 40)
    for k, v in fields.items():
        setattr(p, k, v)
    return p


def plan_of(direction, p):
    plan = _lib.FaActPlan()
    st = getattr(_lib.load(), f"fa_act_{direction}_plan")(p, plan)
    assert st == OK, st
    return U.Plan(plan.cw, plan.threads, plan.grid_x, plan.grid_y, plan.rows_per_wg)


@pytest.mark.parametrize("cell", U.CELLS, ids=lambda c: f"{c.direction}-{'gated' if c.gated else 'plain'}-{c.dtype}-{'vec' if c.vec else 'elem'}")
def test_every_cell_at_every_boundary(cell):
    cw = U.cw_of(cell.dtype, cell.vec)
    for h in U.widths(cw):
        for m in (1, 2, 37):
            got = plan_of(cell.direction, params(cell.direction, m, h, cell.dtype, cell.gated, cell.vec or m == 1))
            want = U.plan(cell.direction, m, h, cell.dtype, cell.vec or m == 1)  # (one row at an aligned base: no pitch to break it)
            if not cell.vec and m == 1:
                continue  # (the element cell needs the misaligned base: below)
            assert got == want, (h, m)
        if not cell.vec:
            assert plan_of(cell.direction, params(cell.direction, 1, h, cell.dtype, cell.gated, False)).cw == 1
    assert [U.plan(cell.direction, 2, h, cell.dtype, cell.vec).grid_x for h in (1, 256 * cw, 256 * cw + cw, 256 * 256 * cw, 1 << 30)] == [1, 1, 2, 256, 256]


@pytest.mark.parametrize("dtype", ["bf16", "fp16", "fp32"])
def test_cw_is_from_dtype_and_every_tensor(dtype):
    es, cw = U.ESIZE[dtype], 16 // U.ESIZE[dtype]
    m, h = 37, 4096
    assert plan_of("fwd", params("fwd", m, h, dtype)).cw == cw
    assert plan_of("fwd", params("fwd", m, h, dtype, bias=ADDR + 16)).cw == cw
    fwd_breaks = [{"pre": ADDR + es}, {"out": ADDR + (1 << 40) + es}, {"pre_row_stride": h + 1}, {"out_row_stride": h + cw - 1}, {"bias": ADDR + 4}]
    for change in fwd_breaks:
        assert plan_of("fwd", params("fwd", m, h, dtype, **change)).cw == 1, change
    assert plan_of("fwd", params("fwd", m, h, dtype, gated=True)).cw == cw
    assert plan_of("fwd", params("fwd", m, h, dtype, gated=True, up=ADDR + 2 * h * es + es)).cw == 1
    assert plan_of("fwd", params("fwd", 1, h, dtype, pre_row_stride=h + 1)).cw == cw  # (one row: the pitches say nothing)
    # the plain form ignores up and dup: a stale, misaligned pointer left in the fields does not change the plan
    assert plan_of("fwd", params("fwd", m, h, dtype, up=ADDR + es)).cw == cw
    assert plan_of("bwd", params("bwd", m, h, dtype, up=ADDR + es, dup=ADDR + es)).cw == cw
    assert plan_of("bwd", params("bwd", m, h, dtype, gated=True, recompute=True)).cw == cw
    assert plan_of("bwd", params("bwd", m, h, dtype, dbias=True, bias=ADDR + 32)).cw == cw
    bwd_breaks = [{"dout": ADDR + (1 << 40) + es}, {"dpre": ADDR + (2 << 40) + 16 - es}, {"dpre_row_stride": h + 1}, {"dout_row_stride": h + 1},
                  {"recompute_out": ADDR + es}, {"recompute_out": ADDR, "out_row_stride": h + 1}]
    for change in bwd_breaks:
        assert plan_of("bwd", params("bwd", m, h, dtype, **change)).cw == 1, change
    assert plan_of("bwd", params("bwd", m, h, dtype, gated=True, dup=ADDR + (2 << 40) + 2 * h * es + es)).cw == 1
    # H = 203 inside a pitch of 406: the up half starts 406 bytes (16-bit) after the gate half, so the call takes elements,
    # and the plan says so
    assert plan_of("fwd", params("fwd", m, 203, dtype, gated=True, vec=False, pre=ADDR)).cw == 1
    assert plan_of("bwd", params("bwd", m, 203, dtype, gated=True, vec=False, pre=ADDR)).cw == 1


def test_row_block_caps_and_partial_rows():
    for m, blocks in ((1, 1), (4, 1), (5, 2), (4 * 65535, 65535), (4 * 65535 + 1, 65535), (1 << 31, 65535)):
        assert plan_of("fwd", params("fwd", m, 8)).grid_y == blocks == U.plan("fwd", m, 8, "bf16", True).grid_y
    lib = _lib.load()
    for m, blocks in ((1, 1), (32, 1), (33, 2), (32 * 1024, 1024), (32 * 1024 + 1, 1024), (1 << 31, 1024)):
        p = params("bwd", m, 8, dbias=True)
        assert plan_of("bwd", p).grid_y == blocks == U.partial_rows(m)
        assert lib.fa_act_bwd_workspace_bytes(p) == blocks * 8 * 4
    assert plan_of("fwd", params("fwd", 0, 8)).grid_y == 0 == plan_of("bwd", params("bwd", 0, 8)).grid_y


@pytest.mark.parametrize("w", U.WALKS, ids=[w.name for w in U.WALKS])
def test_walks_exceed_their_cap(w):
    got = plan_of(w.direction, params(w.direction, w.m, w.h, w.dtype, vec=w.vec))
    assert got == U.plan(w.direction, w.m, w.h, w.dtype, w.vec)
    items, extent = U.cap_exceeded(w)
    assert items > extent, (w.name, items, extent)
    assert extent == {"forward row blocks": 65535, "backward row blocks": 1024}.get(w.name, 256)


def test_plan_validates_first():
    lib = _lib.load()
    plan = _lib.FaActPlan(cw=-7)
    assert lib.fa_act_fwd_plan(None, plan) == NULLP and lib.fa_act_bwd_plan(None, plan) == NULLP
    assert lib.fa_act_fwd_plan(params("fwd", 37, 0), plan) == BAD_SHAPE
    assert lib.fa_act_bwd_plan(params("bwd", 37, 8, dpre=0), plan) == NULLP
    assert plan.cw == -7  # untouched
    assert lib.fa_act_fwd_plan(params("fwd", 37, 8), None) == NULLP and lib.fa_act_bwd_plan(params("bwd", 37, 8), None) == NULLP
