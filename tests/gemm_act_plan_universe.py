"""The forms of csrc/fa_gemm_act.hip as data, and the cases tests/test_gemm_act_gpu.py runs.  Pure Python, no device, no
library: a model of the launch rule and a case table with both sides of every boundary.  tests/test_gemm_act_plan.py holds
fa_gemm_act_fwd_plan / fa_gemm_act_dgrad_plan to it.

A workgroup of 256 threads owns a tile_m x 128 tile of the (M, N) output, tile_m = 64 where M <= 64 and 128 above, and walks
ceil(K / 64) K-steps.  The grid is tiles_m * tiles_n workgroups.  A call with N or K no multiple of 8, or not in a 16-bit dtype,
is not fused: it takes torch.mm and the activation kernels ("mm_act")."""
import collections

THREADS = 256
TILE_N, TILE_K = 128, 64
TILE_M_MAIN, TILE_M_SMALL = 128, 64
SMALL_M = 64
GROUP_M = 8
REDUCE_THREADS = 256

Plan = collections.namedtuple("Plan", "tile_m tile_n tile_k threads tiles_m tiles_n grid_x k_steps ragged_m ragged_n ragged_k group_m "
                                      "partial_rows reduce_grid_x")


def form(m, n, k, dtype="bf16"):
    return "fused" if dtype in ("bf16", "fp16") and n >= 8 and k >= 8 and n % 8 == 0 and k % 8 == 0 else "mm_act"


def plan(m, n, k, dbias=False):
    tile_m = TILE_M_SMALL if m <= SMALL_M else TILE_M_MAIN
    tiles_m, tiles_n = -(-m // tile_m), -(-n // TILE_N)
    return Plan(tile_m, TILE_N, TILE_K, THREADS, tiles_m, tiles_n, tiles_m * tiles_n, -(-k // TILE_K), int(m % tile_m != 0),
                int(n % TILE_N != 0), int(k % TILE_K != 0), GROUP_M, tiles_m if dbias else 0,
                -(-(n // 8) // REDUCE_THREADS) if dbias and m > 0 else 0)


# the cells of the plan: what a fused call can be
Cell = collections.namedtuple("Cell", "tile_m many_k ragged_m ragged_n ragged_k")


def cell_of(m, n, k):
    p = plan(m, n, k)
    return Cell(p.tile_m, p.k_steps > 1, bool(p.ragged_m), bool(p.ragged_n), bool(p.ragged_k))


# (M, N, K): both sides of every boundary.  The first seven are the shapes the GPU tests must run.
CASES = (
    (128, 128, 64),     # whole in every dimension, one tile, one K-step
    (1, 8, 8),          # the smallest call: K below one K-step, one row, one chunk of columns
    (127, 136, 40),     # main tile, ragged everywhere, one short K-step
    (129, 264, 72),     # one row past a tile, a column tail, a K tail after one whole step
    (300, 128, 200),    # three row tiles, whole N, several K-steps with a tail
    (64, 512, 520),     # the small-M form at its limit: many K-steps with a K tail
    (1100, 1032, 264),  # 9 x 9 tiles: more row tiles than one group of GROUP_M, ragged in all three dimensions
    (65, 128, 64),      # the first M of the main tile
    (64, 128, 64),      # the small tile, whole
    (63, 120, 56),      # the small tile, ragged everywhere
    (256, 256, 128),    # whole tiles, two K-steps
    (128, 128, 72),     # whole M and N, ragged K
    (128, 136, 64),     # whole M and K, ragged N
    (130, 128, 64),     # ragged M alone
)

# shapes the kernels refuse: N or K no multiple of 8
FALLBACK_CASES = ((128, 130, 64), (128, 128, 36), (5, 7, 8))


def boundaries_covered():
    """every value of every cell field occurs in CASES"""
    cells = [cell_of(*c) for c in CASES]
    return all({getattr(c, f) for c in cells} == ({64, 128} if f == "tile_m" else {False, True}) for f in Cell._fields)
