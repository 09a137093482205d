"""The forms of csrc/fa_block_select.hip as data, and the cases tests/test_block_select_gpu.py runs.  Pure Python, no device, no
library: a small model of fa_block_summary_update_plan_name / fa_block_select_plan_name (include/fa_block_select.h).
tests/test_block_select_abi.py holds the two C functions to it, and the kernels of the unit to KERNELS.

Rows and summaries are taken by chunks of 8 channels, one chunk per lane: L = 16 lanes where d > 64, else 8.  The update has one
workgroup per (block the written range can meet, kv head, batch entry); the scoring one per (chunk of 1024 / L blocks, kv head,
batch entry) -- always the split form; the selection one per (kv head, batch entry), of 256 threads up to 1024 blocks, of 1024
above."""
import collections
import itertools

MAX_BLOCKS, MAX_ROWS = 8192, 128
SMALL_BLOCKS, SMALL_THREADS, LARGE_THREADS = 1024, 256, 1024

# (kernel, L) of every kernel in the unit
KERNELS = {(k, lanes) for k in ("summary_update_kernel", "block_score_kernel") for lanes in (16, 8)} | {("block_select_kernel", None)}


def lanes(d):
    return 16 if d > 64 else 8


def score_chunk(d):
    return 256 // lanes(d) * 4


def update_form(d, fp8, paged):
    return (lanes(d), "e4m3" if fp8 else "16", "paged" if paged else "dense")


def update_plan(b, h_k, d, max_blocks, block, max_seqlen_new, fp8, paged):
    L, cache, side = update_form(d, fp8, paged)
    return f"summary_update_kernel<{L}> cache={cache} {side} grid=({min(-(-max_seqlen_new // block) + 1, max_blocks)},{h_k},{b})"


def select_form(d, max_blocks, reduce):
    return (lanes(d), reduce, SMALL_THREADS if max_blocks <= SMALL_BLOCKS else LARGE_THREADS)


def select_plan(b, h_k, d, max_blocks, reduce):
    L, _, threads = select_form(d, max_blocks, reduce)
    split = -(-max_blocks // score_chunk(d))
    return f"block_score_kernel<{L}> {reduce} split={split} grid=({split},{h_k},{b}) + block_select_kernel threads={threads}"


UPDATE_FORMS = set(itertools.product((16, 8), ("16", "e4m3"), ("dense", "paged")))
SELECT_FORMS = set(itertools.product((16, 8), ("max", "sum"), (SMALL_THREADS, LARGE_THREADS)))

# ---- the summary cases of the GPU test: every combination -------------------------------------------------------------------
CAPACITY = 512
SummaryCase = collections.namedtuple("SummaryCase", "cache form block d h_k")  # cache: bf16 / fp16 / e4m3; form: dense / p16 / p64 / p256
SUMMARY_CASES = tuple(SummaryCase(*c) for c in itertools.product(("bf16", "fp16", "e4m3"), ("dense", "p16", "p64", "p256"), (64, 128),
                                                                  (64, 128), (1, 2)))


def fills_of(block):
    return (0, 1, block - 1, block, block + 1, CAPACITY)


# ---- the exact selection cases ----------------------------------------------------------------------------------------------
SelectCase = collections.namedtuple("SelectCase", "d g s_q reduce block num_blocks sink local max_blocks")
SMALL_MAX_BLOCKS = 40
RAGGED_N = (0, 1, 3, 37, SMALL_MAX_BLOCKS)  # n(b) over the batch of 5
SELECT_CASES = tuple(SelectCase(d, g, s_q, reduce, block, nb, sink, local, SMALL_MAX_BLOCKS)
                     for d, g, s_q, reduce, block, nb, (sink, local) in itertools.product(
                         (64, 128), (1, 4), (1, 3), ("max", "sum"), (64, 128), (2, 8, SMALL_MAX_BLOCKS), ((0, 0), (1, 1), (2, 3))))
# b = 1, h_k = 1, 4096 blocks: the scoring is split over 64 (d 128) / 32 (d 64) workgroups, the selection has 1024 threads
LARGE_CASES = tuple(SelectCase(d, 4, 1, reduce, 128, nb, 1, 1, 4096) for d, reduce, nb in
                    ((128, "max", 512), (128, "sum", 8), (64, "max", 1024), (64, "sum", 4096)))
