"""The forms of csrc/fa_xent.hip as data, and the cases tests/test_xent_forms_gpu.py runs.  Pure Python, no device, no library:
a small model of the row geometry (`pieces_of`), of the two launch rules, the label positions that decide which code finds the
label, and the walking cases that exceed a grid cap.  tests/test_xent_plan.py holds fa_xent_fwd_plan / fa_xent_bwd_plan to it.

A row is an element head up to the first 16-byte boundary, a body of 16-byte chunks of cw elements, and an element tail.  The
backward takes the body in slabs of 1024 chunks over grid.x and the rows over grid.y; the forward a row per workgroup."""
import collections

THREADS, BWD_CHUNKS = 256, 4
BWD_SLAB = THREADS * BWD_CHUNKS       # body chunks of a slab
BWD_MAX_SLABS, BWD_MAX_ROWS = 256, 65535
FWD_MAX_GRID = 1 << 20
LSE_GIVEN_MAX_GRID = 65536
ESIZE = {"bf16": 2, "fp16": 2, "fp32": 4}

Pieces = collections.namedtuple("Pieces", "head nbody tail")
Plan = collections.namedtuple("Plan", "cw grid_x grid_y lse_given")


def cw_of(dtype):
    return 16 // ESIZE[dtype]


def pieces_of(address, dtype, n, cw):
    """the model of the kernels' pieces_of: `address` is that of the row's first element"""
    if cw == 1:
        return Pieces(0, n, 0)
    es = ESIZE[dtype]
    mis = address % 16
    head = min((16 - mis) // es if mis else 0, n)
    nbody = (n - head) // cw
    return Pieces(head, nbody, n - head - nbody * cw)


def fwd_plan(m, dtype, lse_given=False):
    if lse_given:
        return Plan(1, min(-(-m // THREADS), LSE_GIVEN_MAX_GRID), 1, 1)
    return Plan(cw_of(dtype), min(m, FWD_MAX_GRID), 1, 0)


def bwd_plan(m, n, dtype, same_phase):
    """same_phase: every row of dlogits is as far from a 16-byte boundary as the same row of logits"""
    cw = cw_of(dtype) if same_phase else 1
    slabs = -(-(-(-n // cw)) // BWD_SLAB)
    return Plan(cw, min(slabs, BWD_MAX_SLABS), min(m, BWD_MAX_ROWS), 0)


def label_positions(g, cw, n):
    """name -> column: the places where another piece of code finds the label.  Names whose column does not exist in this
    geometry (no head, no tail) are left out."""
    body_end = g.head + g.nbody * cw
    at = collections.OrderedDict()
    at["column 0"] = 0
    if g.head:
        at["last head column"] = g.head - 1
    at["first body column"] = g.head
    at["last element of chunk 0"] = g.head + cw - 1
    at["first element of the last chunk of slab 0"] = g.head + (BWD_SLAB - 1) * cw
    at["last element of slab 0"] = g.head + BWD_SLAB * cw - 1
    at["first element of slab 1"] = g.head + BWD_SLAB * cw
    at["last body column"] = body_end - 1
    if g.tail:
        at["first tail column"] = body_end
        at["last tail column"] = n - 1
    at["column N - 1"] = n - 1
    assert all(0 <= c < n for c in at.values()), (g, at)
    return at


def label_width(dtype, head, tail):
    """N with a full slab 0 and a partial slab 1 of 300 chunks behind `head`, and `tail` elements after the body"""
    return head + (BWD_SLAB + 300) * cw_of(dtype) + tail


def edges(cw):
    return (0, 1, cw - 1)


# the walking loops: (name, phase, M, N, dtype, what makes the form, the cap that is exceeded)
Walk = collections.namedtuple("Walk", "name direction m n dtype same_phase lse_given")
WALKS = (
    Walk("backward rows", "bwd", BWD_MAX_ROWS + 9, 8, "bf16", True, False),
    # the same walk over rows wide enough that the whole tensor (134 MB) does not stay in the L2 caches: see
    # test_walk_backward_rows_wide
    Walk("backward rows, wide", "bwd", BWD_MAX_ROWS + 9, 1024, "bf16", True, False),
    Walk("backward slabs, element kernel", "bwd", 2, 262144 + 1024 + 5, "bf16", False, False),
    Walk("backward slabs, 16-byte kernel", "bwd", 2, 4 * 1024 * 256 + 4 * 1024 + 3, "fp32", True, False),
    Walk("forward rows", "fwd", FWD_MAX_GRID + 3, 8, "bf16", True, False),
    Walk("lse_given rows", "fwd", LSE_GIVEN_MAX_GRID * THREADS + 5, 2, "bf16", True, True),
)


def walk_plan(w):
    return fwd_plan(w.m, w.dtype, w.lse_given) if w.direction == "fwd" else bwd_plan(w.m, w.n, w.dtype, w.same_phase)


def cap_exceeded(w):
    """the work beyond the grid: (items, the grid's extent over them), items > extent"""
    p = walk_plan(w)
    if w.lse_given:
        return -(-w.m // THREADS), p.grid_x
    if w.direction == "fwd" or w.name.startswith("backward rows"):
        return w.m, p.grid_x if w.direction == "fwd" else p.grid_y
    return -(-(-(-w.n // p.cw)) // BWD_SLAB), p.grid_x
