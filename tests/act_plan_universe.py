"""The forms of csrc/fa_act.hip as data, and the cases tests/test_act_forms_gpu.py runs.  Pure Python, no device, no library:
a model of the two launch rules and the case table of every cell -- form (forward / backward, plain / gated) x dtype width x
16-byte accesses or elements -- with the smallest and the largest H of the cell's boundaries.  tests/test_act_plan.py holds
fa_act_fwd_plan / fa_act_bwd_plan to it.

A row is H // cw chunks of 16 bytes and H % cw tail columns (cw = 1: H elements).  A workgroup of 256 threads takes a slab of
256 chunks (grid.x, at most 256 slabs; more are walked) of blocks of rows (grid.y: forward 4 rows a block, at most 65535
blocks; backward 32 rows a block, at most 1024 blocks, which is also the number of dbias partial rows)."""
import collections

THREADS = 256
FWD_ROWS, BWD_ROWS = 4, 32
MAX_SLABS = 256
FWD_MAX_BLOCKS, BWD_MAX_BLOCKS = 65535, 1024
ESIZE = {"bf16": 2, "fp16": 2, "fp32": 4}

Plan = collections.namedtuple("Plan", "cw threads grid_x grid_y rows_per_wg")


def cw_of(dtype, vec):
    return 16 // ESIZE[dtype] if vec else 1


def plan(direction, m, h, dtype, vec):
    """vec: every tensor of the call has a 16-byte aligned base and (m > 1) a pitch that is a multiple of 16 bytes"""
    cw = cw_of(dtype, vec)
    rows, cap = (FWD_ROWS, FWD_MAX_BLOCKS) if direction == "fwd" else (BWD_ROWS, BWD_MAX_BLOCKS)
    slabs = max(1, -(-(h // cw) // THREADS))
    return Plan(cw, THREADS, min(slabs, MAX_SLABS), min(-(-m // rows), cap), rows)


def partial_rows(m):
    return min(-(-m // BWD_ROWS), BWD_MAX_BLOCKS)


def widths(cw):
    """the H of a cell's boundaries: the tail alone; one chunk; tails of 0, 1 and cw - 1 columns beside a body; both sides of
    one slab; and more than one slab with a tail"""
    slab = THREADS * cw
    hs = {1, cw, slab - 1, slab, slab + 1, 2 * slab + cw + (cw - 1)}
    if cw > 1:
        hs |= {cw - 1, cw + 1, 3 * cw - 1}
    return sorted(hs)


Cell = collections.namedtuple("Cell", "direction gated dtype vec")
CELLS = tuple(Cell(d, g, t, v) for d in ("fwd", "bwd") for g in (False, True) for t in ("bf16", "fp32") for v in (True, False))


def named_columns(h, cw):
    """name -> column: the first and last column of the body, of the tail, of every slab, as far as this H has them"""
    nbody = h // cw
    at = collections.OrderedDict()
    at["column 0"] = 0
    if nbody:
        at["last body column"] = nbody * cw - 1
        at["last column of chunk 0"] = cw - 1
    if nbody > THREADS:
        at["last column of slab 0"] = THREADS * cw - 1
        at["first column of slab 1"] = THREADS * cw
    if cw > 1 and h % cw:
        at["first tail column"] = nbody * cw
    at["column H - 1"] = h - 1
    return at


# the walks: a grid cap exceeded.  (name, direction, M, H, dtype, vec)
Walk = collections.namedtuple("Walk", "name direction m h dtype vec")
WALKS = (
    Walk("forward row blocks", "fwd", FWD_ROWS * FWD_MAX_BLOCKS + 5, 8, "bf16", True),
    Walk("backward row blocks", "bwd", BWD_ROWS * BWD_MAX_BLOCKS + 37, 8, "bf16", True),
    Walk("forward slabs, element kernel", "fwd", 2, THREADS * MAX_SLABS + 259, "bf16", False),
    Walk("backward slabs, element kernel", "bwd", 2, THREADS * MAX_SLABS + 259, "fp32", False),
)


def cap_exceeded(w):
    """(items, the grid's extent over them), items > extent"""
    p = plan(w.direction, w.m, w.h, w.dtype, w.vec)
    if "row blocks" in w.name:
        return -(-w.m // p.rows_per_wg), p.grid_y
    return -(-(w.h // p.cw) // THREADS), p.grid_x
