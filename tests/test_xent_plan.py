"""CPU tests of fa_xent_fwd_plan / fa_xent_bwd_plan (include/fa_xent.h) against tests/xent_plan_universe.py: cw from dtype and
phase, the caps of grid.x / grid.y, and the walking cases planned with their cap actually exceeded.  Dummy addresses, nothing
dereferenced, no device; tests/test_xent_forms_gpu.py runs the walks and the label positions on the kernels."""
import pytest

import xent_plan_universe as U
from flash_attention_annotated_amd import _lib

ADDR = 0x10000
OK, NULLP, BAD_SHAPE = 0, -1, -5
CODE = {"bf16": _lib.FA_DTYPE_BF16, "fp16": _lib.FA_DTYPE_FP16, "fp32": _lib.FA_DTYPE_FP32}


def fwd_params(m, n, dtype="bf16", lse_given=False, **fields):
    p = _lib.new_xent_fwd_params()
    p.logits = p.labels = p.losses = p.lse = p.z_losses = ADDR
    p.M, p.N, p.logits_row_stride, p.total_classes, p.logits_dtype = m, n, n, n, CODE[dtype]
    p.flags = _lib.FA_XENT_PRECOMPUTED_LSE if lse_given else 0
    for k, v in fields.items():
        setattr(p, k, v)
    return p


def bwd_params(m, n, dtype="bf16", **fields):
    p = _lib.new_xent_bwd_params()
    p.logits = p.labels = p.lse = p.dloss = ADDR
    p.dlogits = ADDR + (1 << 32)
    p.M, p.N, p.logits_row_stride, p.dlogits_row_stride, p.dloss_stride, p.total_classes = m, n, n, n, 1, n
    p.logits_dtype = CODE[dtype]
    for k, v in fields.items():
        setattr(p, k, v)
    return p


def plan_of(direction, p):
    plan = _lib.FaXentPlan()
    st = getattr(_lib.load(), f"fa_xent_{direction}_plan")(p, plan)
    assert st == OK, st
    return U.Plan(plan.cw, plan.grid_x, plan.grid_y, plan.lse_given)


@pytest.mark.parametrize("dtype", ["bf16", "fp16", "fp32"])
def test_forward_cw_is_the_dtypes_and_the_grid_is_capped(dtype):
    for m in (1, 37, U.FWD_MAX_GRID - 1, U.FWD_MAX_GRID, U.FWD_MAX_GRID + 3, 1 << 24):
        for n in (1, 8, 203, 50257):
            # (whatever the phase of the rows: head and tail are taken by elements inside the kernel)
            for change in ({}, {"logits": ADDR + 4}, {"logits_row_stride": n + 3}):
                assert plan_of("fwd", fwd_params(m, n, dtype, **change)) == U.fwd_plan(m, dtype)
        given = plan_of("fwd", fwd_params(m, 8, dtype, lse_given=True))
        assert given == U.fwd_plan(m, dtype, lse_given=True) and given.lse_given == 1 and given.cw == 1
    assert U.fwd_plan(U.LSE_GIVEN_MAX_GRID * 256, dtype, True).grid_x == 65536 == U.fwd_plan(1 << 30, dtype, True).grid_x
    assert U.fwd_plan(U.LSE_GIVEN_MAX_GRID * 256 - 256, dtype, True).grid_x == 65535


@pytest.mark.parametrize("dtype", ["bf16", "fp16", "fp32"])
def test_backward_cw_is_from_dtype_and_phase(dtype):
    es, cw = U.ESIZE[dtype], U.cw_of(dtype)
    m, n = 37, 50257
    same = [{}, {"dlogits": ADDR}, {"logits": ADDR + es, "dlogits": ADDR + (1 << 32) + es + 16},
            {"logits_row_stride": n + 3, "dlogits_row_stride": n + 3 + 2 * cw}, {"logits_row_stride": n + cw, "dlogits_row_stride": n}]
    other = [{"dlogits": ADDR + (1 << 32) + es}, {"logits": ADDR + 16 - es}, {"dlogits_row_stride": n + 1},
             {"logits_row_stride": n + cw - 1, "dlogits_row_stride": n}]
    for change in same:
        assert plan_of("bwd", bwd_params(m, n, dtype, **change)) == U.bwd_plan(m, n, dtype, True), change
    for change in other:
        assert plan_of("bwd", bwd_params(m, n, dtype, **change)) == U.bwd_plan(m, n, dtype, False), change
    # one row: the pitches say nothing
    assert plan_of("bwd", bwd_params(1, n, dtype, dlogits_row_stride=n + 1)).cw == cw


def test_backward_grid_caps():
    for dtype in ("bf16", "fp32"):
        cw = U.cw_of(dtype)
        for same_phase in (True, False):
            per_slab = U.BWD_SLAB * (cw if same_phase else 1)
            change = {} if same_phase else {"dlogits": ADDR + (1 << 32) + U.ESIZE[dtype]}
            for n, slabs in ((1, 1), (per_slab, 1), (per_slab + 1, 2), (256 * per_slab, 256), (256 * per_slab + 1, 256), (1 << 24, 256)):
                plan = plan_of("bwd", bwd_params(2, n, dtype, **change))
                assert plan == U.bwd_plan(2, n, dtype, same_phase) and plan.grid_x == min(slabs, -(-n // per_slab)), (dtype, n)
    for m, rows in ((1, 1), (65535, 65535), (65536, 65535), (65544, 65535), (1 << 22, 65535)):
        assert plan_of("bwd", bwd_params(m, 8)).grid_y == rows


@pytest.mark.parametrize("w", U.WALKS, ids=[w.name for w in U.WALKS])
def test_walks_exceed_their_cap(w):
    if w.direction == "fwd":
        p = fwd_params(w.m, w.n, w.dtype, w.lse_given, labels_dtype=_lib.FA_XENT_LABELS_INT32 if w.lse_given else _lib.FA_XENT_LABELS_INT64)
    else:
        p = bwd_params(w.m, w.n, w.dtype, **({} if w.same_phase else {"dlogits": ADDR + (1 << 32) + U.ESIZE[w.dtype]}))
    plan = plan_of(w.direction, p)
    assert plan == U.walk_plan(w)
    items, extent = U.cap_exceeded(w)
    assert items > extent, (w.name, items, extent)
    assert extent == {"backward rows": 65535, "backward rows, wide": 65535, "backward slabs, element kernel": 256, "backward slabs, 16-byte kernel": 256,
                      "forward rows": 1 << 20, "lse_given rows": 65536}[w.name]
    assert plan.cw == {"backward slabs, element kernel": 1, "backward slabs, 16-byte kernel": 4, "lse_given rows": 1}.get(w.name, 8)


def test_walks_are_the_five_loops_and_the_wide_rows():
    assert [(w.m, w.n) for w in U.WALKS] == [(65544, 8), (65544, 1024), (2, 263173), (2, 1052675), ((1 << 20) + 3, 8), (16777221, 2)]


def test_label_positions_of_every_geometry():
    for dtype in ("bf16", "fp32"):
        cw = U.cw_of(dtype)
        for head in U.edges(cw):
            for tail in U.edges(cw):
                n = U.label_width(dtype, head, tail)
                address = ADDR + ((cw - head) % cw) * U.ESIZE[dtype]
                g = U.pieces_of(address, dtype, n, cw)
                assert (g.head, g.tail) == (head, tail) and g.nbody == U.BWD_SLAB + 300
                at = U.label_positions(g, cw, n)
                assert ("last head column" in at) == (head > 0) and ("first tail column" in at) == (tail > 0)
                assert len(at) == 8 + 1 * (head > 0) + 2 * (tail > 0)
                assert at["first element of slab 1"] - at["last element of slab 0"] == 1
                assert U.pieces_of(address, dtype, n, 1) == U.Pieces(0, n, 0)
    assert U.pieces_of(ADDR + 14, "bf16", 3, 8) == U.Pieces(1, 0, 2) and U.pieces_of(ADDR + 2, "bf16", 3, 8) == U.Pieces(3, 0, 0)


def test_plan_validates_first():
    lib = _lib.load()
    plan = _lib.FaXentPlan(cw=-7)
    assert lib.fa_xent_fwd_plan(None, plan) == NULLP and lib.fa_xent_bwd_plan(None, plan) == NULLP
    assert lib.fa_xent_fwd_plan(fwd_params(37, 0), plan) == BAD_SHAPE
    assert lib.fa_xent_bwd_plan(bwd_params(37, 8, dlogits=0), plan) == NULLP
    assert plan.cw == -7  # untouched
    assert lib.fa_xent_fwd_plan(fwd_params(37, 8), None) == NULLP and lib.fa_xent_bwd_plan(bwd_params(37, 8), None) == NULLP
