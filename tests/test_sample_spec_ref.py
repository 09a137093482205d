"""CPU tests of the oracle of speculative sampling (utils.generation.sample_speculative_ref, the contract of
include/fa_spec_sample.h) and of the inputs of tests/sample_spec_cases.py: the condition the exact comparisons of
tests/test_sample_spec_gpu.py rest on, and the properties of the rule itself."""
import pytest
import torch

import sample_cases as C
import sample_spec_cases as SC
from flash_attention_annotated_amd.utils import generation as G


@pytest.mark.parametrize("dtype", list(SC.DTYPES))
@pytest.mark.parametrize("v", SC.VS)
def test_boundary_sequences_are_within_the_cap_and_the_oracles_agree(v, dtype):
    """All blocks of a (V, dtype): the cap is asserted first, over the whole case.  Every case set holds all three kinds of
    sequence."""
    bs = SC.BS
    seqs, left_out, kinds = SC.check_oracles(v, dtype, SC.blocks(v))
    assert seqs == sum(bs) * len(SC.SS) * 7
    assert all(k > 0 for k in kinds), ("all accepted / rejected at 0 / rejected in between", kinds)


def test_no_draft_tokens_is_the_draw_under_the_filters_top_k_rule():
    """S = 0: the token of p_0.  With top_k >= V or 0 that is sample_ref; with ties at the k-th value the filter's rule keeps
    them all, which is sample_ref on the filtered logits."""
    x = C.make_logits(9, 203, "bf16", 5)
    x[:, 100:110] = x.max(dim=1, keepdim=True).values  # ten ties with the maximum
    u = C.make_uniforms(9, 5)
    none = torch.zeros(9, 0, 203, dtype=x.dtype), torch.zeros(9, 0, dtype=torch.int64), torch.zeros(9, 0)
    for top_k, top_p, t in ((0, 0.0, 1.0), (0, 0.9, 0.7), (300, 0.5, 1.0), (3, 0.0, 1.0), (1, 0.0, 1.0), (5, 0.8, 2.5)):
        tokens, num = G.sample_speculative_ref(x[:, None].double(), none[0].double(), none[1], top_k, top_p, t, (none[2], u))
        filtered = G.filter_ref(C.scaled(x, t).double(), top_k, 0.0)
        want = G.sample_ref(filtered, 0, top_p, 1.0, u)
        assert tokens.shape == (9, 1) and torch.equal(tokens[:, 0], want) and num.tolist() == [1] * 9, (top_k, top_p, t)
    # top_k == 1 takes no shortcut: of 11 tied maxima any may be drawn, not the first alone
    tokens, _ = G.sample_speculative_ref(x[:1, None].double().expand(64, 1, 203), none[0][:1].double().expand(64, 0, 203),
                                         none[1][:1].expand(64, 0), 1, 0.0, 1.0, (torch.zeros(64, 0), (torch.arange(64) + 0.5) / 64))
    assert len(set(tokens[:, 0].tolist())) == 11


def test_a_draft_equal_to_the_target_accepts_everything():
    c = SC.make_case(203, "fp32", 5, 4, 3)
    x = c["logits"]
    q, _ = G._kept_probs(x[:, :4].reshape(20, 203).double(), 50, 0.9, 0.7)
    tokens = q.argmax(dim=1).view(5, 4)
    u = (torch.full((5, 4), 0.999), c["u"][1])
    out, num, p_tok, q_tok, accepted, _ = G.sample_speculative_ref(x, x[:, :4], tokens, 50, 0.9, 0.7, u, stats=True)
    assert num.tolist() == [5] * 5 and accepted.all() and torch.equal(out[:, :4], tokens) and torch.equal(p_tok, q_tok)
    # ... and a token out of range rejects even then; with no residual weight the token comes from p_n
    tokens[1, 2], tokens[3, 0] = -1, 203
    out, num, p_tok, q_tok, accepted, _ = G.sample_speculative_ref(x, x[:, :4], tokens, 50, 0.9, 0.7, u, stats=True)
    assert num.tolist() == [5, 3, 5, 1, 5] and accepted[1].tolist() == [1, 1, 0, 1] and p_tok[1, 2] == 0 and q_tok[3, 0] == 0
    want = G.sample_ref(G.filter_ref(C.scaled(torch.stack([x[1, 2], x[3, 0]]), 0.7), 50, 0.0), 0, 0.9, 1.0, u[1][[1, 3]])
    assert out[1, 2] == want[0] and out[3, 0] == want[1] and out[1, 3] == tokens[1, 3] and out[1, 4] == 0


def test_a_token_outside_the_drafts_kept_set_is_accepted():
    c = SC.make_case(4099, "bf16", 5, 4, 2)
    planted = torch.arange(20).view(5, 4) % 11 == 3
    _, _, p_tok, q_tok, accepted, _ = c["r64"][:6]
    assert planted.sum() == 2 and (q_tok[planted] == 0).all() and accepted[planted].all()


def test_the_resampled_token_is_written_per_row():
    """Two sequences that reject at different positions: the reference's `tokens[:, n] = resample` puts the token resampled
    for sequence 0 over a token sequence 1 accepted"""
    v = 16
    x = torch.zeros(2, 3, v)
    d = torch.zeros(2, 2, v)
    x[0, :, 3] = 9.0  # sequence 0: the target wants 3, the draft says 5 at position 0: rejected at 0, resampled to 3
    d[0, :, 5] = 9.0
    x[1, :, 8] = 9.0  # sequence 1: target and draft say 8 twice: all accepted, column 2 is drawn from p_2: 11
    d[1, :, 8] = 9.0
    x[1, 2, 8], x[1, 2, 11] = 0.0, 9.0
    tokens = torch.tensor([[5, 5], [8, 8]])
    u = (torch.full((2, 2), 0.5), torch.full((2,), 0.5))
    out, num = G.sample_speculative_ref(x, d, tokens, 0, 0.0, 1.0, u)
    assert num.tolist() == [1, 3] and out.tolist() == [[3, 5, 0], [8, 8, 11]]
    column_write = torch.cat([tokens, tokens.new_zeros(2, 1)], dim=1)
    column_write[:, num - 1] = torch.tensor([3, 11])
    assert column_write.tolist() == [[3, 5, 11], [3, 8, 11]]  # sequence 1 would emit 3, 8, 11: a token nobody sampled for it


def test_the_first_emitted_token_follows_the_target_distribution():
    """What the algorithm exists for, at V = 7, S = 1: whatever the draft, the first emitted token is distributed as p_0.  40000
    sequences of one (target, draft) pair over the uniforms of 4 seeds; Pearson's statistic against p_0 has 6 degrees of freedom,
    and 27.86 is its 0.9999 quantile."""
    v, n = 7, 10000
    g = torch.Generator().manual_seed(2211)
    x = torch.randn(1, 2, v, generator=g).double() * 1.5
    d = (x[:, :1] + torch.randn(1, 1, v, generator=g).double() * 1.5)
    p0 = torch.softmax(x[0, 0], dim=0)
    q0 = torch.softmax(d[0, 0], dim=0)
    assert (p0 - q0).abs().max() > 0.1  # (a draft worth rejecting)
    count = torch.zeros(v, dtype=torch.float64)
    accepted_all = 0
    for seed in range(4):
        gs = torch.Generator().manual_seed(seed)
        tokens = torch.multinomial(q0, n, replacement=True, generator=gs).view(n, 1)
        u = (torch.rand(n, 1, generator=gs), torch.rand(n, generator=gs))
        out, num = G.sample_speculative_ref(x.expand(n, 2, v), d.expand(n, 1, v), tokens, 0, 0.0, 1.0, u)
        count += torch.bincount(out[:, 0], minlength=v).double()
        accepted_all += int((num == 2).sum())
    expected = 4 * n * p0
    chi2 = float(((count - expected) ** 2 / expected).sum())
    assert chi2 <= 27.86, (chi2, count, expected)
    assert 0.2 < accepted_all / (4 * n) < 0.95  # both branches ran


def test_cpu_tensors_take_the_oracle_and_the_names_are_exported():
    c = SC.make_case(203, "fp32", 5, 4, 3)
    tokens, num = G.sample_speculative(c["logits"], c["draft"], c["tokens"].int(), 50, 0.9, 0.7, u=c["u"])
    assert tokens.dtype == torch.int32 and tokens.shape == (5, 5) and num.dtype == torch.int64
    assert torch.equal(tokens.long(), c["r32"][0]) and torch.equal(num, c["r32"][1])
    a = G.sample_speculative(c["logits"], c["draft"], c["tokens"], 0, 0.9, generator=torch.Generator().manual_seed(3))
    b = G.sample_speculative(c["logits"], c["draft"], c["tokens"], 0, 0.9, generator=torch.Generator().manual_seed(3))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert "sample_speculative" in G.__all__ and "sample_speculative_ref" in G.__all__
