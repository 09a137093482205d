"""The forms of csrc/fa_sample.hip as data, and the cases tests/test_sample_gpu.py runs.  Pure Python, no device, no library: a
small model of fa_sample_plan (include/fa_sample.h).  tests/test_sample_plan.py holds fa_sample_plan to it on both sides of every
boundary; tests/test_sample_abi.py holds the kernels of the translation unit to KERNELS.

A row is taken by 16-byte accesses of cw elements where its base, its pitch in bytes (more than one row) and its length in bytes
are multiples of 16, else by elements; by 256 threads up to 1024 accesses and by 1024 above.  A phase descends 11 bits at a
time over the significant bits of a key or of a column index."""
import collections

ESIZE = {"bf16": 2, "fp16": 2, "fp32": 4}
SMALL_THREADS, MAX_THREADS, SMALL_ACCESSES = 256, 1024, 1024
RADIX = 11
MAX_GRID = 65535
MAX_FRAC = 40
DRAW, FILTER = 0, 1

Plan = collections.namedtuple("Plan", "cw threads mode greedy topk topp draw k key_bits key_passes index_bits index_passes "
                                      "frac_bits grid_x")

# (kernel, cw, mode) of every kernel in the unit; mode None: the argmax kernel has none
KERNELS = {("sample_greedy_kernel", cw, None) for cw in (8, 4, 1)} | {("sample_kernel", cw, mode) for cw in (8, 4, 1) for mode in (DRAW, FILTER)}


def ceil_log2(n):
    return max(n - 1, 0).bit_length()


def plan(b, v, dtype, top_k=1, top_p=0.0, temperature=1.0, mode=DRAW, address=0x10000, stride=None):
    es = ESIZE[dtype]
    stride = v if stride is None else stride
    wide = address % 16 == 0 and (v * es) % 16 == 0 and (b <= 1 or (stride * es) % 16 == 0)
    cw = 16 // es if wide else 1
    greedy = mode == DRAW and top_k == 1
    topk = not greedy and (2 if mode == DRAW else 1) <= top_k < v
    key_bits = 32 if temperature != 1.0 else {"bf16": 16, "fp16": 19, "fp32": 32}[dtype]
    index_bits = max(ceil_log2(v), 1)
    return Plan(cw=cw, threads=SMALL_THREADS if v // cw <= SMALL_ACCESSES else MAX_THREADS, mode=mode, greedy=int(greedy),
                topk=int(topk), topp=int(not greedy and 0.0 < top_p < 1.0), draw=int(not greedy and mode == DRAW),
                k=top_k if topk else 0, key_bits=key_bits, key_passes=-(-key_bits // RADIX), index_bits=index_bits,
                index_passes=-(-index_bits // RADIX), frac_bits=min(MAX_FRAC, 62 - ceil_log2(v)), grid_x=min(b, MAX_GRID))


def kernel_of(p):
    return ("sample_greedy_kernel", p.cw, None) if p.greedy else ("sample_kernel", p.cw, p.mode)


# the cases the GPU test runs so that every kernel and every boundary of the plan has run: (name, B, V, dtype, top_k, top_p,
# temperature, mode, misaligned base (elements), row stride - V)
Case = collections.namedtuple("Case", "name b v dtype top_k top_p temperature mode shift pad")
CASES = (
    Case("greedy, 16 bytes, bf16", 3, 4096, "bf16", 1, 0.0, 1.0, DRAW, 0, 0),
    Case("greedy, 16 bytes, fp32", 3, 516, "fp32", 1, 0.0, 1.0, DRAW, 0, 0),
    Case("greedy, elements", 3, 4099, "fp16", 1, 0.0, 0.7, DRAW, 0, 0),
    Case("draw, 1024 accesses: the small workgroup", 4, 8192, "bf16", 40, 0.9, 1.0, DRAW, 0, 0),
    Case("draw, 1025 accesses: the large workgroup", 4, 8200, "bf16", 40, 0.9, 1.0, DRAW, 0, 0),
    Case("draw, fp32 1024 accesses", 4, 4096, "fp32", 0, 0.9, 1.0, DRAW, 0, 0),
    Case("draw, fp32 1025 accesses", 4, 4100, "fp32", 0, 0.9, 1.0, DRAW, 0, 0),
    Case("draw, elements 1024", 4, 1024, "fp16", 7, 0.5, 1.0, DRAW, 1, 0),
    Case("draw, elements 1025", 4, 1025, "fp16", 7, 0.5, 1.0, DRAW, 0, 0),
    Case("draw, a pitch that is no multiple of 16 bytes", 4, 4096, "bf16", 0, 0.8, 1.0, DRAW, 0, 3),
    Case("draw, one row of any pitch stays on 16 bytes", 1, 4096, "bf16", 0, 0.8, 1.0, DRAW, 0, 3),
    Case("draw, a base off 16 bytes", 4, 4096, "fp32", 50, 0.0, 1.0, DRAW, 1, 0),
    Case("draw, 19-bit keys of fp16", 4, 4096, "fp16", 50, 0.9, 1.0, DRAW, 0, 0),
    Case("draw, 32-bit keys under a temperature", 4, 4096, "bf16", 50, 0.9, 0.7, DRAW, 0, 0),
    Case("draw, top_k = V - 1 selects", 4, 208, "bf16", 207, 0.0, 1.0, DRAW, 0, 0),
    Case("draw, top_k = V is the row", 4, 208, "bf16", 208, 0.0, 1.0, DRAW, 0, 0),
    Case("draw, 11 index bits: one pass", 4, 2048, "bf16", 0, 0.0, 1.0, DRAW, 0, 0),
    Case("draw, 12 index bits: two passes", 4, 2056, "bf16", 0, 0.0, 1.0, DRAW, 0, 0),
    Case("draw, 23 index bits: three passes", 1, (1 << 22) + 8, "bf16", 0, 0.9, 1.0, DRAW, 0, 0),
    Case("draw, more rows than workgroups", MAX_GRID + 9, 8, "bf16", 3, 0.0, 1.0, DRAW, 0, 0),
    Case("filter, top-k keeps ties", 4, 4096, "bf16", 50, 0.0, 1.0, FILTER, 0, 0),
    Case("filter, top-k = 1", 4, 4096, "bf16", 1, 0.0, 1.0, FILTER, 0, 0),
    Case("filter, top-p, fp32", 4, 516, "fp32", 0, 0.9, 1.0, FILTER, 0, 0),
    Case("filter, both, elements", 4, 4099, "fp16", 30, 0.7, 1.0, FILTER, 0, 0),
)


def case_plan(c):
    return plan(c.b, c.v, c.dtype, c.top_k, c.top_p, c.temperature, c.mode, 0x10000 + c.shift * ESIZE[c.dtype], c.v + c.pad)
