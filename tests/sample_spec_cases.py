"""The inputs of the speculative-sampling tests (tests/test_sample_spec_ref.py on the CPU, tests/test_sample_spec_gpu.py on the
device): the seeded grid, its tensors, and the rule that says which sequences may be left out of an exact comparison.

Target logits are sample_cases.make_logits rows; draft logits are target + N(0, 1), cast to the dtype.  Draft tokens are drawn
from the draft's filtered distribution (inverse CDF of seeded uniforms), and some are planted by their flat position
i = b * S + t: the target row's argmax (i % 7 == 2), a token outside the draft's kept set where there is one (i % 11 == 3), the
token -1 (i % 17 == 5) and the token V (i % 23 == 7).

A *boundary sequence* has, in the fp64 oracle, a margin (utils.generation.sample_speculative_ref: top-p sums of the rows up to
the first rejection, acceptance tests relative to max(p, q), the sum of the residual weights against 0, the resample's
cumulative weights against u_res times their total) of at most sample_cases.tol(V), and is left out of exact comparison.  Boundary sequences may be at most 2 % of the sequences of a (V, dtype) case, checked before
anything is compared."""
import torch

import sample_cases as C

VS = (1, 7, 16, 203, 4096, 4099, 32000)
V_WIDE = 131072 + 8  # one case: WIDE
SS = (0, 1, 4)
BS = (1, 5, 64)
DTYPES = C.DTYPES
CAP = 0.02
WIDE = (V_WIDE, "bf16", 5, 4, 3)  # (V, dtype, B, S, index of the setting)


def settings(v):
    """[(top_k, top_p, temperature)]"""
    return [(1, 0.0, 1.0), (0, 0.0, 1.0), (0, 0.9, 1.0), (50, 0.9, 0.7), (50, 0.1, 2.5), (2, 1.0, 0.7), (v + 3, 0.9, 1.0)]


def case_seed(v, dtype, b, s):
    return 1000003 * v + 101 * list(DTYPES).index(dtype) + 7 * b + 13 * s


def scaled(logits, temperature):
    """s in fp32, the one division the contract names, of a (B, S, V) block"""
    return C.scaled(logits.reshape(-1, logits.shape[-1]), temperature).view(logits.shape)


def make_tensors(v, dtype, b, s, setting, seed, device="cpu"):
    """-> (logits (B, S + 1, V), draft (B, S, V), tokens (B, S) int64, (u_acc, u_res)), made from `seed` on the CPU whatever
    the device; the draft tokens are drawn (and planted) under `setting`"""
    from flash_attention_annotated_amd.utils import generation as G
    top_k, top_p, temperature = setting
    logits = C.make_logits(b * (s + 1), v, dtype, seed).view(b, s + 1, v)
    g = torch.Generator().manual_seed(seed + 1)
    draft = (logits[:, :s].float() + torch.randn(b, s, v, generator=g)).to(DTYPES[dtype])
    r = torch.rand(b, s, generator=g)
    u = (torch.rand(b, s, generator=g).to(device), torch.rand(b, generator=g).to(device))
    logits, draft = logits.to(device), draft.to(device)
    tokens = torch.zeros(b, s, dtype=torch.int64, device=device)
    if s > 0:
        q, _ = G._kept_probs(draft.reshape(b * s, v).double(), top_k, top_p, temperature)
        tokens = ((q.cumsum(dim=1) > r.to(device).double().view(-1, 1)) & (q > 0)).int().argmax(dim=1)
        i = torch.arange(b * s, device=device)
        tokens = torch.where(i % 7 == 2, logits[:, :s].reshape(b * s, v).float().argmax(dim=1), tokens)
        outside = (q == 0)
        tokens = torch.where((i % 11 == 3) & outside.any(dim=1), outside.int().argmax(dim=1), tokens)
        tokens = torch.where(i % 17 == 5, torch.full_like(tokens, -1), tokens)
        tokens = torch.where(i % 23 == 7, torch.full_like(tokens, v), tokens).view(b, s)
    return logits, draft, tokens, u


def oracles(logits, draft, tokens, u, setting):
    """(fp32 oracle's, fp64 oracle's) (tokens, num_generated, p_tok, q_tok, accepted, margin); the fp64 oracle's are followed by
    the two per-position margins (B, S): of the top-p sums of a position's two rows, and of its acceptance test.  The fp64
    oracle starts from the fp32 s: the division is part of the contract, not of the rounding under test."""
    from flash_attention_annotated_amd.utils import generation as G
    top_k, top_p, temperature = setting
    r64 = G.sample_speculative_ref(scaled(logits, temperature).double(), scaled(draft, temperature).double(), tokens, top_k, top_p,
                                   1.0, u, stats="positions")
    r32 = G.sample_speculative_ref(logits.float(), draft.float(), tokens, top_k, top_p, temperature, u, stats=True)
    return r32, r64


_CASES = {}


def make_case(v, dtype, b, s, j, device="cpu"):
    """-> dict(logits, draft, tokens, u, setting, r32, r64): the tensors of setting j of a (V, dtype, B, S) block and the two
    oracles' results, computed once per session and device"""
    key = (v, dtype, b, s, j, device)
    if key not in _CASES:
        setting = settings(v)[j]
        logits, draft, tokens, u = make_tensors(v, dtype, b, s, setting, case_seed(v, dtype, b, s) + 1000 * (j + 1), device)
        r32, r64 = oracles(logits, draft, tokens, u, setting)
        _CASES[key] = dict(logits=logits, draft=draft, tokens=tokens, u=u, setting=setting, r32=r32, r64=r64)
    return _CASES[key]


def blocks(v, bs=BS):
    """[(B, S, j)] of a (V, dtype) case"""
    return [(b, s, j) for b in bs for s in SS for j in range(len(settings(v)))]


def same_up_to_n(a, num_a, b, num_b):
    """(B,) bool: the two results agree on num_generated and on the tokens up to the first rejected position"""
    cols = torch.arange(a.shape[1], device=a.device)[None, :] < num_a[:, None]
    return (num_a == num_b) & ((a == b) | ~cols).all(dim=1)


def check_oracles(v, dtype, which, device="cpu"):
    """The condition an exact comparison rests on, over the blocks `which` of a (V, dtype): boundary sequences (by the fp64
    oracle) are within the cap, and on every other sequence the fp32 oracle gives the fp64 oracle's tokens up to n_b and its
    num_generated.  -> (sequences, left out, kinds), kinds = [all accepted, rejected at 0, rejected in between] counted over the
    blocks with S = 4"""
    seqs = left_out = 0
    kinds = [0, 0, 0]
    disagree = []
    for b, s, j in which:
        c = make_case(v, dtype, b, s, j, device)
        t32, n32 = c["r32"][:2]
        t64, n64, margin = c["r64"][0], c["r64"][1], c["r64"][5]
        compared = margin > C.tol(v)
        seqs, left_out = seqs + b, left_out + int((~compared).sum())
        if not bool(same_up_to_n(t32, n32, t64, n64)[compared].all()):
            disagree.append((v, dtype, b, s, c["setting"]))
        if s == 4:
            kinds[0] += int((n64 == s + 1).sum())
            kinds[1] += int((n64 == 1).sum())
            kinds[2] += int(((n64 > 1) & (n64 <= s)).sum())
    assert left_out <= CAP * seqs, ("boundary sequences above the cap", v, dtype, left_out, seqs)
    assert not disagree, ("oracles disagree", disagree)
    return seqs, left_out, kinds
