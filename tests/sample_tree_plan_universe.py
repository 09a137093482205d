"""The forms of csrc/fa_tree_sample.hip as data, and the cases tests/test_sample_tree_gpu.py runs.  Pure Python, no device, no
library: a small model of fa_tree_sample_plan (include/fa_tree_sample.h).  tests/test_sample_tree_plan.py holds
fa_tree_sample_plan to it on both sides of every boundary; tests/test_sample_tree_abi.py holds the kernels of the unit to KERNELS.

Rows are taken by 16-byte accesses of cw elements where every logits tensor given qualifies (bases, every pitch in bytes that is
used, the row length in bytes: multiples of 16), else by elements; by 256 threads up to 1024 accesses and by 1024 above, in both
phases.  The selection is the filter's: top-k runs from top_k = 1 on.  mode: "draft" (draft rows) or "onehot" (none)."""
import collections

from sample_plan_universe import ESIZE, MAX_FRAC, MAX_GRID, MAX_THREADS, RADIX, SMALL_ACCESSES, SMALL_THREADS, ceil_log2

Plan = collections.namedtuple("Plan", "cw threads drafts topk topp k key_bits key_passes index_bits index_passes frac_bits grid_a grid_b")

# (kernel, cw) of every kernel in the unit
KERNELS = {(k, cw) for k in ("tree_select_kernel", "tree_walk_kernel") for cw in (8, 4, 1)}


def plan(b, t, v, dtype, mode="draft", top_k=1, top_p=0.0, temperature=1.0, address=0x10000, draft_address=0x20000, strides=None,
         draft_strides=None):
    """strides: (batch, node) of logits in elements; default: contiguous"""
    es = ESIZE[dtype]
    strides = (t * v, v) if strides is None else strides
    draft_strides = (t * v, v) if draft_strides is None else draft_strides
    ok = lambda stride, used: not used or (stride * es) % 16 == 0
    wide = address % 16 == 0 and (v * es) % 16 == 0 and ok(strides[0], b > 1) and ok(strides[1], t > 1)
    if mode == "draft":
        wide = wide and draft_address % 16 == 0 and ok(draft_strides[0], b > 1) and ok(draft_strides[1], t > 1)
    cw = 16 // es if wide else 1
    topk = 1 <= top_k < v
    key_bits = 32 if temperature != 1.0 else {"bf16": 16, "fp16": 19, "fp32": 32}[dtype]
    index_bits = max(ceil_log2(v), 1)
    return Plan(cw=cw, threads=SMALL_THREADS if v // cw <= SMALL_ACCESSES else MAX_THREADS, drafts=int(mode == "draft"), topk=int(topk),
                topp=int(0.0 < top_p < 1.0), k=top_k if topk else 0, key_bits=key_bits, key_passes=-(-key_bits // RADIX),
                index_bits=index_bits, index_passes=-(-index_bits // RADIX), frac_bits=min(MAX_FRAC, 62 - ceil_log2(v)),
                grid_a=min(b * t, MAX_GRID), grid_b=min(b, MAX_GRID))


# the cases the GPU test runs so that every kernel and every boundary of the plan has run: (name, B, T, V, dtype, mode, tree shape,
# top_k, top_p, temperature, misaligned base of logits (elements), of the draft, node stride - V of both)
Case = collections.namedtuple("Case", "name b t v dtype mode shape top_k top_p temperature shift draft_shift pad")
CASES = (
    Case("16 bytes, bf16, 1024 accesses: the small workgroup", 3, 5, 8192, "bf16", "draft", "binary", 40, 0.9, 1.0, 0, 0, 0),
    Case("16 bytes, bf16, 1025 accesses: the large workgroup", 3, 5, 8200, "bf16", "draft", "star", 40, 0.9, 1.0, 0, 0, 0),
    Case("16 bytes, bf16, one-hot, the large workgroup", 3, 5, 8200, "bf16", "onehot", "star", 40, 0.9, 1.0, 0, 0, 0),
    Case("16 bytes, fp32", 3, 5, 516, "fp32", "draft", "forest", 0, 0.9, 1.0, 0, 0, 0),
    Case("16 bytes, fp32, one-hot", 3, 5, 516, "fp32", "onehot", "binary", 0, 0.9, 1.0, 0, 0, 0),
    Case("16 bytes, fp16, 19-bit keys", 3, 5, 4096, "fp16", "draft", "binary", 50, 0.9, 1.0, 0, 0, 0),
    Case("32-bit keys under a temperature", 3, 5, 4096, "bf16", "onehot", "star", 50, 0.9, 0.7, 0, 0, 0),
    Case("elements: an odd width", 3, 5, 4099, "fp16", "draft", "star", 30, 0.7, 1.0, 0, 0, 0),
    Case("elements: an odd width, one-hot", 3, 5, 4099, "fp16", "onehot", "star", 30, 0.7, 1.0, 0, 0, 0),
    Case("elements: the target's base off 16 bytes", 3, 5, 4096, "fp32", "draft", "chain", 50, 0.0, 1.0, 1, 0, 0),
    Case("elements: the draft's base off 16 bytes", 3, 5, 4096, "bf16", "draft", "binary", 50, 0.0, 1.0, 0, 1, 0),
    Case("16 bytes: one-hot, the draft's base does not count", 3, 5, 4096, "bf16", "onehot", "binary", 50, 0.0, 1.0, 0, 1, 0),
    Case("elements: a node pitch that is no multiple of 16 bytes", 3, 5, 4096, "bf16", "draft", "forest", 0, 0.8, 1.0, 0, 0, 3),
    Case("elements, 1024 accesses", 3, 2, 1024, "fp16", "draft", "chain", 7, 0.5, 1.0, 1, 0, 0),
    Case("elements, 1025 accesses", 3, 2, 1025, "fp16", "draft", "chain", 7, 0.5, 1.0, 0, 0, 0),
    Case("top_k = 1 selects", 3, 5, 208, "bf16", "draft", "star", 1, 0.0, 1.0, 0, 0, 0),
    Case("top_k = V - 1 selects", 3, 5, 208, "bf16", "onehot", "star", 207, 0.0, 1.0, 0, 0, 0),
    Case("top_k = V is the row", 3, 5, 208, "bf16", "draft", "binary", 208, 0.0, 1.0, 0, 0, 0),
    Case("11 index bits: one pass", 3, 5, 2048, "bf16", "draft", "star", 0, 0.0, 1.0, 0, 0, 0),
    Case("12 index bits: two passes", 3, 5, 2056, "bf16", "onehot", "star", 0, 0.0, 1.0, 0, 0, 0),
    Case("one node", 3, 1, 4096, "bf16", "draft", "chain", 50, 0.9, 1.0, 0, 0, 0),
    Case("64 nodes", 2, 64, 208, "bf16", "draft", "forest", 0, 0.0, 1.0, 0, 0, 0),
    Case("more rows than workgroups", (MAX_GRID + 9) // 3 + 1, 3, 8, "bf16", "draft", "star", 3, 0.0, 1.0, 0, 0, 0),
    Case("more sequences than workgroups", MAX_GRID + 9, 1, 8, "bf16", "onehot", "chain", 3, 0.0, 1.0, 0, 0, 0),
)


def case_plan(c):
    es = ESIZE[c.dtype]
    strides = (c.t * (c.v + c.pad), c.v + c.pad)
    return plan(c.b, c.t, c.v, c.dtype, c.mode, c.top_k, c.top_p, c.temperature, 0x10000 + c.shift * es, 0x20000 + c.draft_shift * es,
                strides, strides)


def kernels_of(p):
    return {("tree_select_kernel", p.cw), ("tree_walk_kernel", p.cw)}
