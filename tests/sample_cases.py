"""The inputs of the sampling tests (tests/test_sample_ref.py on the CPU, tests/test_sample_gpu.py on the device): the seeded grid,
its logits, and the rule that says which rows may be left out of an exact comparison.

Logits look like a language model's: a bulk of N(0, 1) and a head of up to 12 columns raised by 2.5 (ln V + 10) + N(0, 4), so that
at every temperature of the grid all but e^-10 of the mass is in few entries, and a cumulative sum rarely comes close to the
value it is compared with.

A *boundary row* has, in the fp64 oracle, a cumulative sum (top-p or draw) within tol(V) of its comparison value,
    tol(V) = min(64 * V * 2^-24, 2^-14).
The first term is the bound the cases were specified with.  From V = 16 on it exceeds what leaves any row to compare (at
V = 131080 it is 0.5), so it is capped: an fp32 probability exp(s - m) carries a relative error of at most
|s - m| * log2(e) * 2^-24 from the rounded argument plus 2^-22 from the exponential, below 2^-18 for |s - m| <= 40, which is then
also the error of a cumulative sum of probabilities (at most 1) in fixed point; 2^-14 is 16 times that.  The cap only ever
compares more rows.  Boundary rows may be at most 1 % of the rows of a test case (a (V, dtype) with all its blocks and settings), checked before
anything is compared."""
import math

import torch

VS = (1, 7, 16, 203, 4096, 4099, 32000, 131072 + 8)
DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16, "fp32": torch.float32}
BS = (1, 5, 64)
TOP_PS = (0.0, 0.1, 0.9, 1.0)
TEMPERATURES = (1.0, 0.7, 2.5)
CAP = 0.01


def top_ks(v):
    return (0, 1, 2, 50, v, v + 3)


def tol(v):
    return min(64 * v * 2.0 ** -24, 2.0 ** -14)


def settings(v):
    """[(top_k, top_p, temperature)]: the full product; with every B of BS it is the grid of a (V, dtype)"""
    return [(k, p, t) for k in top_ks(v) for p in TOP_PS for t in TEMPERATURES]


def make_logits(b, v, dtype, seed, device="cpu"):
    """(B, V) logits of `dtype` (a name), made on the CPU from `seed` whatever the device"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(b, v, generator=g)
    head = min(v, 12)
    cols = torch.stack([torch.randperm(v, generator=g)[:head] for _ in range(b)])
    x.scatter_add_(1, cols, max(TEMPERATURES) * (math.log(v) + 10.0) + 4.0 * torch.randn(b, head, generator=g))
    return x.to(DTYPES[dtype]).to(device)


def make_uniforms(b, seed, device="cpu"):
    g = torch.Generator().manual_seed(seed + 1)
    return torch.rand(b, generator=g).to(device)


def scaled(logits, temperature):
    """s in fp32, the one division the contract names, for an oracle of another precision to start from"""
    x = logits.float()
    return x / torch.tensor(temperature, dtype=torch.float32, device=x.device) + 0.0


def block_seed(v, dtype, b):
    """of the logits of the (B, V) block that all settings of a (V, dtype, B) share"""
    return 1000003 * v + 101 * list(DTYPES).index(dtype) + 7 * b


_ORACLES = {}


def oracles(v, dtype, b, j, x, device="cpu"):
    """The two oracles on setting j of settings(v) for the block x = make_logits(b, v, dtype, block_seed(v, dtype, b), device):
    (u, fp32 (token, kept, mass), fp64 (token, kept, mass), margin), computed once per session and device.  The fp64 oracle
    starts from the fp32 s: the division is part of the contract, not of the rounding under test."""
    from flash_attention_annotated_amd.utils import generation as G
    key = (v, dtype, b, j, device)
    if key not in _ORACLES:
        top_k, top_p, temperature = settings(v)[j]
        u = make_uniforms(b, block_seed(v, dtype, b) + 1000 * (j + 1), device)
        t64, k64, m64, margin = G.sample_ref(scaled(x, temperature).double(), top_k, top_p, 1.0, u, stats=True)
        t32, k32, m32, _ = G.sample_ref(x.float(), top_k, top_p, temperature, u, stats=True)
        _ORACLES[key] = (u, (t32, k32, m32), (t64, k64, m64), margin)
    return _ORACLES[key]


def check_oracles(v, dtype, bs, device="cpu"):
    """The condition an exact comparison rests on, over the blocks `bs` of a (V, dtype) and all settings: boundary rows (by the
    fp64 oracle) are within the cap, and on every other row the fp32 oracle gives the fp64 oracle's token, count and mass.
    -> (rows, left out)"""
    rows = left_out = 0
    for b in bs:
        x = make_logits(b, v, dtype, block_seed(v, dtype, b), device)
        for j, (top_k, top_p, temperature) in enumerate(settings(v)):
            _, (t32, k32, m32), (t64, k64, m64), margin = oracles(v, dtype, b, j, x, device)
            compared = margin > tol(v)
            rows, left_out = rows + b, left_out + int((~compared).sum())
            what = (v, dtype, b, top_k, top_p, temperature)
            assert torch.equal(t32[compared], t64[compared]) and torch.equal(k32[compared], k64[compared]), ("oracles disagree", what)
            if top_k != 1:
                assert torch.allclose(m32[compared].double(), m64[compared], rtol=1e-5, atol=0), ("oracle masses disagree", what)
    assert left_out <= CAP * rows, ("boundary rows above the cap", v, dtype, left_out, rows)
    return rows, left_out
