"""The forms of csrc/fa_block_pattern.hip as data, and the cases tests/test_block_pattern_gpu.py runs.  Pure Python, no device, no
library: a small model of fa_block_pattern_plan_name / fa_block_pattern_workspace_size (include/fa_block_pattern.h).
tests/test_block_pattern_abi.py holds the two C functions to it, and the kernels of the unit to KERNELS.

The pooling has one workgroup per (b, head, block) of q and of k, with 16-byte loads where both bases are 16-byte aligned and
every stride is a multiple of 8 elements, else element loads; L = 16 lanes per row where d > 64, else 8.  The selection has one
workgroup per (m, h, b), of 256 threads up to 1024 key blocks, of 1024 above.  The transpose, one workgroup per (n, h, b), runs
with the key-major lists only."""
import collections
import itertools

BLOCK, MAX_BLOCKS = 128, 8192
SMALL_BLOCKS, SMALL_THREADS, LARGE_THREADS = 1024, 256, 1024

# (kernel, template argument) of every kernel in the unit
KERNELS = {("pool_kernel", "Lb1"), ("pool_kernel", "Lb0"), ("pattern_kernel", None), ("transpose_kernel", None)}


def blocks(s):
    return -(-s // BLOCK)


def form(vec, sk, transpose):
    return ("16B" if vec else "elem", SMALL_THREADS if blocks(sk) <= SMALL_BLOCKS else LARGE_THREADS, bool(transpose))


def plan(b, sq, sk, h, h_k, d, vec, transpose):
    pool, threads, transpose = form(vec, sk, transpose)
    nm, nk = blocks(sq), blocks(sk)
    tail = f" + transpose_kernel grid=({nk},{h},{b})" if transpose else " + no transpose"
    return (f"pool_kernel<{pool}> L={16 if d > 64 else 8} grid=({b * h * nm + b * h_k * nk}) + pattern_kernel m_per_wg=1 "
            f"threads={threads} grid=({nm},{h},{b})" + tail)


def workspace_size(b, sq, sk, h, h_k, d, transpose):
    nm, nk = blocks(sq), blocks(sk)
    r16 = lambda x: -(-x // 16) * 16  # noqa: E731
    return r16(b * h * nm * d * 4) + r16(b * h_k * nk * d * 4) + (r16(b * h * nm * -(-nk // 32) * 4) if transpose else 0)


FORMS = set(itertools.product(("16B", "elem"), (SMALL_THREADS, LARGE_THREADS), (False, True)))

# ---- the cases of the GPU test ----------------------------------------------------------------------------------------------
MASKS = {"full": dict(), "causal": dict(causal=True), "window_256_0": dict(window_size=(256, 0)), "window_128_128": dict(window_size=(128, 128))}
SHAPES = ((300, 300), (200, 700), (700, 200), (128, 128), (1, 129))
# layout: "contiguous", or q and k as views of one packed qkv buffer (b, s, h + 2 h_k, D): D = d, strided with 16-byte loads
# ("packed"), or D = d + 4, whose head stride is no multiple of 8 -- the element loads ("packed_odd")
LAYOUTS = {"contiguous": True, "packed": True, "packed_odd": False}  # -> 16-byte loads
Case = collections.namedtuple("Case", "b h h_k d sq sk dtype mask num_blocks layout bwd")


def num_blocks_of(sk):
    return (2, 3, blocks(sk) + 4)


GRID_CASES = tuple(Case(2, 4, 2, d, sq, sk, dtype, mask, nb, layout, bwd)
                   for d, dtype, layout, (sq, sk), mask, bwd in itertools.product(
                       (64, 128), ("bf16", "fp16"), ("contiguous", "packed_odd"), SHAPES, sorted(MASKS), (False, True))
                   for nb in num_blocks_of(sk))
# packed with 16-byte loads: the strides change nothing but the addresses, one dtype and head dim serve
PACKED_CASES = tuple(Case(2, 4, 2, 64, sq, sk, "bf16", mask, 3, "packed", True) for (sq, sk), mask in itertools.product(SHAPES, sorted(MASKS)))
# nk = 258: more key blocks than the 256 threads of the selection (two entries per thread in the compaction, a histogram walk of
# two rounds) and than the 256 digits of a pass; nk = 1025: the workgroup of 1024 threads
LONG_CASES = tuple(Case(1, 1, 1, 16, 200, sk, "bf16", mask, nb, layout, bwd)
                   for sk, mask, nb, layout, bwd in (
                       (128 * 257 + 5, "full", 40, "contiguous", True), (128 * 257 + 5, "causal", 3, "packed_odd", False),
                       (128 * 257 + 5, "window_256_0", 2, "contiguous", False), (128 * 1024 + 70, "full", 300, "contiguous", True),
                       (128 * 1024 + 70, "full", 7, "contiguous", False), (128 * 1024 + 70, "causal", 1100, "packed_odd", True),
                       (128 * 1024 + 70, "full", 5, "packed_odd", False)))
GPU_CASES = GRID_CASES + PACKED_CASES + LONG_CASES


def case_form(c):
    return form(LAYOUTS[c.layout], c.sk, c.bwd)
