"""The forms of csrc/fa_dropout_norm.hip as data, and the case table tests/test_dropout_norm_gpu.py runs.  Pure Python, no
device, no library: the boundaries below restate DESIGN 4.26, and tests/test_dropout_norm_plan.py holds
fa_dropout_norm_fwd_plan / fa_dropout_norm_bwd_plan to them.

A call takes, per direction, the form (cw, team, dropout): cw the columns per access (8: 16 bytes of a 16-bit x0; 4: 16 bytes of
an fp32 x0; 1: elements), team the threads of the workgroup that takes a row (64 / 256 / 512 / 1024) or "wide", dropout whether
decisions are drawn (p > 0: an instantiation of its own).  A thread has at most COLS[direction][cw] columns, so team t ends at
N = t * cols and the wide form begins above 1024 * cols.  A row of x0 and of the stream is at most 64 KiB.

A case is one call, forward and backward.  Its N sits on one side of a boundary of one of the two directions: every team of
every (direction, cw) has its smallest and its largest N among the cases.  The 16-byte cases have N a multiple of 16 -- the
GPU test asks for the mask, one byte per element, and a row of it must be a multiple of 16 bytes too -- the element cases an
odd N.  What else varies (p, the norm, the one-weight / scaled / parallel form, residual, prenorm, dtypes) goes round by the
case's index, so that every value meets every cw.
"""
import collections

COLS = {"fwd": {8: 16, 4: 8, 1: 2}, "bwd": {8: 8, 4: 4, 1: 2}}
TEAMS = (64, 256, 512, 1024, "wide")
MAX_ROW_BYTES = 65536
ROWS, WIDE_ROWS = 37, 5
FORMS = ("plain", "scaled", "parallel", "parallel_no_x1", "two_weights_no_x1_no_res")

# n, m: columns, rows; x0: dtype of x0; res: None / "same" / "fp32" (the residual, hence the stream); r32: residual_in_fp32;
# form: plain (one weight), scaled (rowscale and layerscale), parallel (x1 and weight1), parallel_no_x1 (weight1 only)
Case = collections.namedtuple("Case", "n m cw x0 w p rms form res r32 prenorm bias")


def max_n(cw):
    return MAX_ROW_BYTES // (4 if cw == 4 else 2)


def team_of(direction, cw, n):
    cols = COLS[direction][cw]
    for t in (64, 256, 512, 1024):
        if n <= t * cols:
            return t
    return "wide"


def boundaries(cw):
    """the ends of the teams of both directions, below the widest row"""
    return sorted({t * COLS[d][cw] for d in ("fwd", "bwd") for t in (64, 256, 512, 1024) if t * COLS[d][cw] < max_n(cw)})


def widths(cw):
    """both sides of every boundary, the narrowest and the widest row; 16-byte forms in steps of 16, elements odd"""
    if cw == 1:
        ns = {1, 203, max_n(1) - 1}
        for b in boundaries(1):
            ns |= {b - 1, b + 1}
    else:
        ns = {16, max_n(cw)}
        for b in boundaries(cw):
            ns |= {b, b + 16}
    return sorted(ns)


def stream_bytes(c):
    return 4 if c.res == "fp32" or (c.res is None and c.r32) or c.x0 == "fp32" else 2


def _cases():
    cases = []
    for cw in (8, 4, 1):
        for i, n in enumerate(widths(cw)):
            x0 = "fp32" if cw == 4 else ("bf16", "fp16")[i % 2]
            form = FORMS[i % 4] if i % 8 != 7 else FORMS[4]
            res = (None, "fp32", "same")[i % 3] if form != FORMS[4] else None
            if x0 == "fp32" and res == "same":
                res = "fp32"
            r32 = res is None and i % 2 == 1
            if n * 4 > MAX_ROW_BYTES:  # an fp32 stream of such a row would pass 64 KiB
                res, r32 = ("same" if res else None), False
            wide = team_of("bwd", cw, n) == "wide"
            cases.append(Case(n, WIDE_ROWS if wide else ROWS, cw, x0, ("fp32", "bf16", "fp16")[(i + cw) % 3] if x0 != "fp32" else
                              ("fp32", "bf16")[i % 2], (0.17, 0.0, 0.9)[(i + i // 3) % 3], bool((i // 2) % 2), form, res, r32,
                              bool((i + 1) % 2), form == "plain" or i % 3 == 0))
    return tuple(cases)


CASES = _cases()


def case_id(c):
    return (f"cw{c.cw}-n{c.n}-p{c.p:g}-{'rms' if c.rms else 'ln'}-{c.form}-{c.x0}-w{c.w}-res_{c.res}"
            f"{'-r32' if c.r32 else ''}{'-pre' if c.prenorm else ''}{'-b' if c.bias else ''}")


def two_weights(c):
    return c.form in ("parallel", "parallel_no_x1", "two_weights_no_x1_no_res")


def has_x1(c):
    return c.form == "parallel"


def sums_of(c):
    """the column sums of the backward: dw0, db0; and dcolscale; or dw0, db0, dw1, db1"""
    return 4 if two_weights(c) else 3 if c.form == "scaled" else 2


def form_of(direction, c):
    """(cw, team, dropout, two_weights) the plan names for the case"""
    return c.cw, team_of(direction, c.cw, c.n), c.p > 0, two_weights(c)


def form_of_plan(plan):
    get = plan.get if isinstance(plan, dict) else lambda k: getattr(plan, k)
    return get("cw"), "wide" if get("wide") else get("threads"), bool(get("dropout")), bool(get("two_weights"))


def grid_y_of(direction, c):
    """column slabs: 1 unless wide backward"""
    cols = COLS["bwd"][c.cw]
    return -(-c.n // (1024 * cols)) if direction == "bwd" and team_of("bwd", c.cw, c.n) == "wide" else 1


def bwd_rows_per_wg(m):
    """1024 workgroups of at least 16 rows"""
    return max(-(-m // 1024), 16)


def fwd_rows_per_wg(m, team):
    """up to 8 rows per workgroup from 2048 rows on; one row per workgroup where wide"""
    return 1 if team == "wide" else min(max(m // 2048, 1), 8)


def bwd_workspace_bytes(m, n, sums):
    """one fp32 partial row per column sum and workgroup, and two row sums per row where some access shape is wide"""
    return -(-m // bwd_rows_per_wg(m)) * n * sums * 4 + (m * 8 if n > 1024 * min(COLS["bwd"].values()) else 0)


# every kernel of the unit: (name, cw, dropout) or (name, cw) or (name,)
KERNELS = ({("dropout_norm_fwd_kernel", cw, d) for cw in (8, 4, 1) for d in (False, True)}
           | {("dropout_norm_bwd_kernel", cw, d) for cw in (8, 4, 1) for d in (False, True)}
           | {("dropout_norm_bwd_row_sums_kernel", cw) for cw in (8, 4, 1)} | {("dropout_norm_reduce_kernel",)})


def kernels_of(c):
    """the kernels a forward and a backward of the case launch"""
    ks = {("dropout_norm_fwd_kernel", c.cw, c.p > 0), ("dropout_norm_bwd_kernel", c.cw, c.p > 0), ("dropout_norm_reduce_kernel",)}
    if team_of("bwd", c.cw, c.n) == "wide":
        ks.add(("dropout_norm_bwd_row_sums_kernel", c.cw))
    return ks
