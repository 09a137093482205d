"""The forms of csrc/fa_norm.hip as a universe of *cells*, and the case table tests/test_norm_forms_gpu.py runs.  Pure Python, no
device, no library: the boundaries below restate DESIGN 4.22 as data, and tests/test_norm_plan.py holds fa_norm_fwd_plan /
fa_norm_bwd_plan to them.

A cell is (direction, cw, team): cw the columns per access (8: 16 bytes of a 16-bit x; 4: 16 bytes of an fp32 x; 1: elements),
team who takes a row -- one wavefront, the workgroup of 256 / 512 / 1024 threads, or the wide form.  A thread has at most 16
columns in the forward and 8 in the backward, so team t ends at N = t * cols and the wide form begins above 1024 * cols.  A row
of x is at most 64 KiB: 32768 columns of a 16-bit x, 16384 of an fp32 x -- which is where the forward's wide form begins, so
fp32 rows are never wide in the forward.

Every cell gets its smallest and its largest N for its cw (a multiple of 8, fp32 and a multiple of 4, odd), which puts a case
on both sides of every boundary.  Wide cells get further widths for the last slab of 1024 * cw columns (forward walk) or
1024 * 8 columns (backward slab): ragged by one chunk, ragged by elements, and full at the limit.
"""
import collections
import random

FWD_COLS, BWD_COLS = 16, 8
TEAMS = ("wave", 256, 512, 1024, "wide")
TEAM_THREADS = {"wave": 64, 256: 256, 512: 512, 1024: 1024}
MAX_ROW_BYTES = 65536
ROWS, WIDE_ROWS = 37, 5
BWD_SLAB = 1024 * BWD_COLS

Cell = collections.namedtuple("Cell", "direction cw team")
# x_dtype: of x in the forward, of the stream in the backward (where dx_dtype is the gradient's); n, m: columns, rows
Case = collections.namedtuple("Case", "cell n m rms x_dtype dx_dtype residual bias rowscale w_fp32")


def cols_of(direction):
    return FWD_COLS if direction == "fwd" else BWD_COLS


def x_dtype_of(cw):
    return "fp32" if cw == 4 else "bf16"


def max_n(cw):
    return MAX_ROW_BYTES // (4 if cw == 4 else 2)


def team_range(direction, team):
    """(lo, hi]: the widths a team takes, before the 64 KiB limit"""
    cols = cols_of(direction)
    ends = [0, 64 * cols, 256 * cols, 512 * cols, 1024 * cols, MAX_ROW_BYTES]
    i = TEAMS.index(team)
    return ends[i], ends[i + 1]


def cell_exists(cell):
    lo, _ = team_range(cell.direction, cell.team)
    return lo < max_n(cell.cw)


CELLS = tuple(c for c in (Cell(d, cw, t) for d in ("fwd", "bwd") for cw in (8, 4, 1) for t in TEAMS) if cell_exists(c))


def widths(cell):
    """the smallest and the largest N of the cell for its cw; wide cells: also the ragged last slabs"""
    lo, hi = team_range(cell.direction, cell.team)
    hi = min(hi, max_n(cell.cw))
    if cell.cw == 1:  # odd
        first, last = lo + 1 if lo % 2 == 0 else lo + 2, hi - 1 if hi % 2 == 0 else hi
    else:
        first, last = lo + cell.cw, hi // cell.cw * cell.cw
    ns = [first, last]
    if cell.team == "wide" and cell.cw == 1:  # a last slab of a few whole chunks and some elements
        ns.insert(1, lo + 27 if cell.direction == "fwd" else lo + 11)
    return ns


def _cases():
    rng = random.Random(20261020)
    cases = []
    for ci, cell in enumerate(CELLS):
        ns = widths(cell)
        # every feature in at least one case of the cell (a seeded pick of which), and by a coin in the others
        feats = {}
        for f in ("residual", "bias", "rowscale", "w_fp32"):
            must = rng.randrange(len(ns))
            feats[f] = [i == must or rng.random() < 0.5 for i in range(len(ns))]
        for i, n in enumerate(ns):
            x_dtype = x_dtype_of(cell.cw)
            # the gradient of an fp32 stream: fp32 at the smallest N, and 16-bit (the stream of a bf16 model kept in fp32) at
            # the largest -- a multiple of 8: every row pitch must be 16 bytes, and a 16-bit row of N = 4 mod 8 is not
            dx_dtype = x_dtype if cell.direction == "fwd" or x_dtype != "fp32" or i % 2 == 0 else "bf16"
            cases.append(Case(cell, n, WIDE_ROWS if cell.team == "wide" else ROWS, bool((i + ci) % 2), x_dtype, dx_dtype,
                              feats["residual"][i], feats["bias"][i], feats["rowscale"][i], feats["w_fp32"][i]))
    return tuple(cases)


CASES = _cases()


def residual_dtype(c):
    """of the forward's residual (hence of its stream): fp32 beside a 16-bit x, except where a row of it would pass 64 KiB"""
    return "fp32" if c.n * 4 <= MAX_ROW_BYTES else c.x_dtype


def weight_dtype(c):
    return "fp32" if c.w_fp32 else "bf16"


def case_id(c):
    return (f"{c.cell.direction}-cw{c.cell.cw}-{c.cell.team}-n{c.n}-{'rms' if c.rms else 'ln'}-{c.x_dtype}"
            f"{'-dx' + c.dx_dtype if c.dx_dtype != c.x_dtype else ''}{'-res' if c.residual else ''}{'-b' if c.bias else ''}"
            f"{'-rs' if c.rowscale else ''}{'-w32' if c.w_fp32 else ''}")


def cell_of_plan(direction, plan):
    """the cell a fa_norm_plan (anything with its fields as attributes or keys) names"""
    get = plan.get if isinstance(plan, dict) else lambda k: getattr(plan, k)
    team = "wide" if get("wide") else "wave" if get("team_wave") else get("threads")
    return Cell(direction, get("cw"), team)


def grid_y_of(case):
    """column slabs: 1 unless wide backward"""
    return -(-case.n // BWD_SLAB) if case.cell == Cell("bwd", case.cell.cw, "wide") else 1


def bwd_rows_per_wg(m):
    """the backward's rows per workgroup: 1024 workgroups of at least 16 rows, a multiple of 4 (the wavefront teams)"""
    return (max(-(-m // 1024), 16) + 3) // 4 * 4


def fwd_rows_per_wg(m, team):
    """the forward's: up to 8 rows per team from 2048 rows a team on; one row per workgroup where wide"""
    if team == "wide":
        return 1
    teams = 4 if team == "wave" else 1
    return min(max(m // (2048 * teams), 1), 8) * teams


def bwd_workspace_bytes(m, n):
    """one fp32 partial row of dw and of db per workgroup, and two row sums per row where wide"""
    partials = -(-m // bwd_rows_per_wg(m))
    return partials * n * 2 * 4 + (m * 2 * 4 if n > 1024 * BWD_COLS else 0)
