"""The inputs of the tree-sampling tests (tests/test_sample_tree_ref.py on the CPU, tests/test_sample_tree_gpu.py on the device):
the tree shapes, the seeded grid, its tensors, and the rule that says which sequences may be left out of an exact comparison.

Target logits are sample_cases.make_logits rows; draft logits are target + N(0, 1), cast to the dtype.  The token of node i is
drawn from the filtered draft distribution of its parent's row (inverse CDF of seeded uniforms; in the one-hot mode too, where
equal siblings then exercise the rejected-before rule), and some are planted by their flat position k = b * T + i: the argmax
of the parent's target row (k % 7 == 2), the token -1 (k % 17 == 5) and the token V (k % 23 == 7).

A *boundary sequence* has, in the fp64 oracle, a margin (utils.generation.sample_speculative_tree_ref: the least over every
comparison along the visited walk) of at most sample_cases.tol(V), and is left out of exact comparison.  Boundary sequences may
be at most 2 % (sample_spec_cases.CAP) of the sequences of a (V, dtype) case, checked before anything is compared."""
import torch

import sample_cases as C
from sample_spec_cases import CAP, scaled, settings  # noqa: F401  (the chain's cap and settings hold here)

VS = (1, 7, 203, 4096, 4099, 32000)
V_WIDE = 131072 + 8
TS = (1, 2, 5, 13, 64)
BS = (1, 5)
MODES = ("draft", "onehot")
SHAPES = ("chain", "star", "binary", "forest")
DTYPES = C.DTYPES
WIDE = (V_WIDE, "bf16", 5, 5, 3, "draft")  # (V, dtype, B, T, index of the setting, mode)


def make_parents(shape, b, t, seed=0):
    """int32 (B, T): chain (i - 1), star (0), binary ((i - 1) // 2), or a random forest: a random earlier node, one node in five
    absent (-1; its descendants hang on it and are never reached)"""
    i = torch.arange(t)
    if shape == "chain":
        row = i - 1
    elif shape == "star":
        row = torch.where(i > 0, torch.zeros_like(i), -torch.ones_like(i))
    elif shape == "binary":
        row = torch.where(i > 0, (i - 1) // 2, -torch.ones_like(i))
    else:
        g = torch.Generator().manual_seed(seed)
        r = (torch.rand(b, t, generator=g) * i.clamp_min(1)).long().clamp_max((i - 1).clamp_min(0))
        r = torch.where(torch.rand(b, t, generator=g) < 0.2, -torch.ones_like(r), r)
        r[:, 0] = -1
        return r.int()
    return row.int().expand(b, t).contiguous()


def case_seed(v, dtype, b, t):
    return 1000003 * v + 101 * list(DTYPES).index(dtype) + 7 * b + 13 * t


def shape_of(b, t, j):
    return SHAPES[(j + b + TS.index(t) if t in TS else j) % len(SHAPES)]


def make_tensors(v, dtype, b, t, setting, seed, shape, device="cpu"):
    """-> (logits (B, T, V), draft (B, T, V), tokens (B, T) int64, parents (B, T) int32, (u_acc (B, T), u_res (B,))), made from
    `seed` on the CPU whatever the device; the tokens are drawn (and planted) under `setting`"""
    from flash_attention_annotated_amd.utils import generation as G
    top_k, top_p, temperature = setting
    logits = C.make_logits(b * t, v, dtype, seed).view(b, t, v)
    g = torch.Generator().manual_seed(seed + 1)
    draft = (logits.float() + torch.randn(b, t, v, generator=g)).to(DTYPES[dtype])
    r = torch.rand(b, t, generator=g)
    u = (torch.rand(b, t, generator=g).to(device), torch.rand(b, generator=g).to(device))
    parents = make_parents(shape, b, t, seed + 2)
    pc = parents.long().clamp_min(0)
    q, _ = G._kept_probs(draft.reshape(b * t, v).double(), top_k, top_p, temperature)
    q = q.view(b, t, v)[torch.arange(b)[:, None], pc].reshape(b * t, v)  # the row of the parent
    tokens = ((q.cumsum(dim=1) > r.double().view(-1, 1)) & (q > 0)).int().argmax(dim=1)
    k = torch.arange(b * t)
    above = logits[torch.arange(b)[:, None], pc].reshape(b * t, v).float().argmax(dim=1)
    tokens = torch.where(k % 7 == 2, above, tokens)
    tokens = torch.where(k % 17 == 5, torch.full_like(tokens, -1), tokens)
    tokens = torch.where(k % 23 == 7, torch.full_like(tokens, v), tokens).view(b, t)
    return logits.to(device), draft.to(device), tokens.to(device), parents.to(device), u


def oracles(logits, draft, tokens, parents, u, setting, mode):
    """(fp32 oracle's, fp64 oracle's) results with stats="positions": (tokens, num_generated, path, path_len, p_tok, q_tok,
    visited, accepted, margin, m_rows).  The fp64 oracle starts from the fp32 s: the division is part of the contract, not of the
    rounding under test."""
    from flash_attention_annotated_amd.utils import generation as G
    top_k, top_p, temperature = setting
    d64 = scaled(draft, temperature).double() if mode == "draft" else None
    r64 = G.sample_speculative_tree_ref(scaled(logits, temperature).double(), d64, tokens, parents, top_k, top_p, 1.0, u, stats="positions")
    r32 = G.sample_speculative_tree_ref(logits.float(), draft.float() if mode == "draft" else None, tokens, parents, top_k, top_p,
                                        temperature, u, stats="positions")
    return r32, r64


_CASES = {}


def make_case(v, dtype, b, t, j, mode, device="cpu"):
    """-> dict(logits, draft, tokens, parents, u, setting, shape, r32, r64) of setting j of a (V, dtype, B, T) block in a mode,
    computed once per session and device.  Both modes share the tensors."""
    key = (v, dtype, b, t, j, mode, device)
    if key not in _CASES:
        setting, shape = settings(v)[j], shape_of(b, t, j)
        tensors = make_tensors(v, dtype, b, t, setting, case_seed(v, dtype, b, t) + 1000 * (j + 1), shape, device)
        r32, r64 = oracles(*tensors, setting, mode)
        _CASES[key] = dict(zip(("logits", "draft", "tokens", "parents", "u"), tensors), setting=setting, shape=shape, r32=r32, r64=r64)
    return _CASES[key]


def blocks(v):
    """[(B, T, j, mode)] of a (V, dtype) case"""
    return [(b, t, j, mode) for b in BS for t in TS for j in range(len(settings(v))) for mode in MODES]


def same_result(a, b):
    """(B,) bool: two results (tokens, num_generated, path, path_len, ...) agree in all four; behind num_generated both hold 0"""
    return ((a[0] == b[0]).all(dim=1) & (a[1] == b[1]) & (a[2] == b[2]).all(dim=1) & (a[3] == b[3]))


def check_oracles(v, dtype, which, device="cpu"):
    """The condition an exact comparison rests on, over the blocks `which` of a (V, dtype): boundary sequences (by the fp64
    oracle) are within the cap, and on every other sequence the fp32 oracle gives the fp64 oracle's tokens, num_generated, path
    and path_len.  -> (sequences, left out, kinds), kinds = [a leaf reached, nothing accepted, stopped in between] counted over
    the blocks with T = 13"""
    seqs = left_out = 0
    kinds = [0, 0, 0]
    disagree = []
    for b, t, j, mode in which:
        c = make_case(v, dtype, b, t, j, mode, device)
        r32, r64 = c["r32"], c["r64"]
        compared = r64[8] > C.tol(v)
        seqs, left_out = seqs + b, left_out + int((~compared).sum())
        if not bool(same_result(r32, r64)[compared].all()):
            disagree.append((v, dtype, b, t, c["setting"], mode, c["shape"]))
        if t == 13:
            n = r64[1]
            last = r64[2].long().gather(1, (n - 1)[:, None])[:, 0]
            leaf = (c["parents"].long() != last[:, None]).all(dim=1)
            kinds[0] += int((leaf & (n > 1)).sum())
            kinds[1] += int((n == 1).sum())
            kinds[2] += int((~leaf & (n > 1)).sum())
    assert left_out <= CAP * seqs, ("boundary sequences above the cap", v, dtype, left_out, seqs)
    assert not disagree, ("oracles disagree", disagree)
    return seqs, left_out, kinds
