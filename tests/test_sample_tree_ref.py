"""CPU tests of the oracle of tree-shaped speculative sampling (utils.generation.sample_speculative_tree_ref, the contract of
include/fa_tree_sample.h) and of the inputs of tests/sample_tree_cases.py: the condition the exact comparisons of
tests/test_sample_tree_gpu.py rest on, and the properties of the rule itself."""
import pytest
import torch

import sample_cases as C
import sample_spec_cases as SC
import sample_tree_cases as TC
from flash_attention_annotated_amd.utils import generation as G


@pytest.mark.parametrize("dtype", list(TC.DTYPES))
@pytest.mark.parametrize("v", TC.VS)
def test_boundary_sequences_are_within_the_cap_and_the_oracles_agree(v, dtype):
    """All blocks of a (V, dtype), both modes: the cap is asserted first, over the whole case.  Every case set holds walks that
    reach a leaf, that accept nothing and that stop in between."""
    seqs, left_out, kinds = TC.check_oracles(v, dtype, TC.blocks(v))
    assert seqs == sum(TC.BS) * len(TC.TS) * 7 * 2
    assert all(k > 0 for k in kinds) or v == 1, ("a leaf reached / nothing accepted / stopped in between", kinds)


def test_the_wide_case_is_within_the_cap():
    v, dtype, b, t, j, mode = TC.WIDE
    tensors = TC.make_tensors(v, dtype, b, t, TC.settings(v)[j], 131, "binary")
    r32, r64 = TC.oracles(*tensors, TC.settings(v)[j], mode)
    assert int((r64[8] <= C.tol(v)).sum()) <= TC.CAP * b and bool(TC.same_result(r32, r64).all())


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_a_chain_shaped_tree_is_the_chain_verification(dtype):
    """parents = -1, 0, 1, ...: node i is position i - 1 of the chain, with its uniform.  Tokens up to num_generated and
    num_generated are sample_speculative_ref's exactly, in both precisions: what fixes c_1 = 1 and the round-0 test."""
    for v, b, s, j in ((203, 5, 4, 3), (4099, 5, 4, 2), (16, 64, 4, 1), (7, 64, 1, 4), (203, 5, 0, 3)):
        c = SC.make_case(v, dtype, b, s, j)
        x, d, tokens, (u_acc, u_res) = c["logits"], c["draft"], c["tokens"], c["u"]
        pad = lambda a, fill: torch.cat([torch.full_like(a[:, :1], fill) if s else a.new_full((b, 1) + a.shape[2:], fill), a], dim=1)
        d_tree = torch.cat([d, torch.zeros(b, 1, v, dtype=d.dtype)], dim=1)  # (the row of the last node: no child reads it)
        parents = TC.make_parents("chain", b, s + 1)
        for cast in (torch.float32, torch.float64):
            want = G.sample_speculative_ref(x.to(cast), d.to(cast), tokens, *c["setting"], (u_acc, u_res))
            got = G.sample_speculative_tree_ref(x.to(cast), d_tree.to(cast), pad(tokens, 0), parents, *c["setting"], (pad(u_acc, 0.5), u_res))
            assert torch.equal(got[1], want[1]) and bool(SC.same_up_to_n(got[0], got[1], want[0], want[1]).all()), (v, s, cast)
            rows = torch.arange(b)
            assert torch.equal(got[0][rows, got[1] - 1], want[0][rows, want[1] - 1])  # (the drawn token itself)
            assert torch.equal(got[2], torch.where(torch.arange(s + 1)[None] < got[1][:, None], torch.arange(s + 1)[None], 0).int())


def test_one_node_is_the_draw():
    """T = 1: the token of P_0 under the filter's top-k rule, which with top_k >= V or 0 is sample_ref; in both modes."""
    x = C.make_logits(9, 203, "bf16", 5)
    u = C.make_uniforms(9, 5)
    none = torch.zeros(9, 1, dtype=torch.int64), torch.full((9, 1), -1, dtype=torch.int32), torch.zeros(9, 1)
    for top_k, top_p, t in ((0, 0.0, 1.0), (0, 0.9, 0.7), (300, 0.5, 1.0), (3, 0.0, 1.0), (5, 0.8, 2.5)):
        want = G.sample_ref(G.filter_ref(C.scaled(x, t).double(), top_k, 0.0), 0, top_p, 1.0, u)
        for draft in (None, x[:, None].double()):
            tokens, num, path, path_len = G.sample_speculative_tree_ref(x[:, None].double(), draft, none[0], none[1], top_k, top_p, t, (none[2], u))
            assert torch.equal(tokens[:, 0], want) and num.tolist() == [1] * 9 and path.tolist() == [[0]] * 9 and path_len.tolist() == [1] * 9


def _small(v=16, b=1, t=6):
    g = torch.Generator().manual_seed(v)
    return torch.randn(b, t, v, generator=g).double() * 2, torch.randn(b, t, v, generator=g).double() * 2


def test_absent_nodes_are_never_visited_and_the_path_is_a_parent_chain():
    for mode in TC.MODES:
        for seed in range(8):
            x, d, tokens, parents, u = TC.make_tensors(203, "fp32", 5, 13, (0, 0.0, 1.0), 50 + seed, "forest")
            out = G.sample_speculative_tree_ref(x, d if mode == "draft" else None, tokens, parents, 0, 0.0, 1.0, u, stats=True)
            _, num, path, path_len, _, _, visited, accepted, _ = out
            absent = parents < 0
            absent[:, 0] = False
            assert absent.any() and not visited[absent].any() and not visited[:, 0].any()
            for b in range(5):
                p = path[b, :int(path_len[b])].tolist()
                assert p[0] == 0 and p == sorted(set(p)) and all(int(parents[b, c]) == a for a, c in zip(p, p[1:]))
                assert path[b, int(path_len[b]):].eq(0).all() and int(num[b]) == int(path_len[b])
                assert accepted[b].nonzero()[:, 0].tolist() == p[1:] and (visited[b] >= accepted[b]).all()
                reachable = [i for i in range(1, 13) if int(parents[b, i]) in p and 0 <= int(parents[b, i]) < i]
                assert set(visited[b].nonzero()[:, 0].tolist()) <= set(reachable)


def test_a_token_out_of_range_is_rejected_and_the_walk_goes_on_to_the_next_sibling():
    x, d = _small()
    parents = torch.tensor([[-1, 0, 0, 0, 2, 2]], dtype=torch.int32)
    best = x[0].argmax(dim=1)
    tokens = torch.tensor([[0, -1, int(best[0]), 3, 16, int(best[2])]])
    u = (torch.zeros(1, 6), torch.tensor([0.5]))  # u = 0 accepts every token in range while weight is left
    for draft in (d, None):
        out = G.sample_speculative_tree_ref(x, draft, tokens, parents, 0, 0.0, 1.0, u, stats=True)
        assert out[2][0].tolist() == [0, 2, 5, 0, 0, 0] and int(out[3]) == 3 and out[0][0, :2].tolist() == [int(best[0]), int(best[2])]
        assert int(out[1]) == 3 and out[6][0].tolist() == [0, 1, 1, 0, 1, 1] and out[7][0].tolist() == [0, 0, 1, 0, 0, 1]
        assert out[4][0, 1] == 0 and out[5][0, 4] == 0 and out[0][0, 3:].eq(0).all()
    # a draft equal to the target leaves no residual weight after a rejection: the siblings behind it are not tried
    out = G.sample_speculative_tree_ref(x, x, tokens, parents, 0, 0.0, 1.0, u, stats=True)
    assert out[6][0].tolist() == [0, 1, 0, 0, 0, 0] and int(out[3]) == 1


def test_a_draft_equal_to_the_target_accepts_the_first_child_of_every_level():
    c = TC.make_case(203, "fp32", 5, 13, 3, "draft")
    x, parents = c["logits"], TC.make_parents("binary", 5, 13)
    q, _ = G._kept_probs(x.reshape(65, 203).double(), 50, 0.9, 0.7)
    tokens = q.view(5, 13, 203)[torch.arange(5)[:, None], parents.long().clamp_min(0)].argmax(dim=2)
    u = (torch.full((5, 13), 0.999), c["u"][1])
    out = G.sample_speculative_tree_ref(x, x, tokens, parents, 50, 0.9, 0.7, u, stats=True)
    assert out[2][:, :4].tolist() == [[0, 1, 3, 7]] * 5 and out[3].tolist() == [4] * 5 and torch.equal(out[4], out[5])
    assert out[6].sum(dim=1).tolist() == [3] * 5  # no sibling was tried


def test_the_second_of_two_equal_siblings_is_rejected_in_the_one_hot_mode():
    x, _ = _small()
    parents = torch.tensor([[-1, 0, 0, 0, -1, -1]], dtype=torch.int32)
    second = int(x[0, 0].topk(2).indices[1])
    tokens = torch.tensor([[0, second, second, second, 0, 0]])
    p = torch.softmax(x[0, 0], dim=0)
    u = (torch.tensor([[0.0, float(p[second]) * 1.5, 0.0, 0.0, 0.0, 0.0]]), torch.tensor([0.3]))  # rejected once; u = 0 would accept
    out = G.sample_speculative_tree_ref(x, None, tokens, parents, 0, 0.0, 1.0, u, stats=True)
    assert out[6][0].tolist() == [0, 1, 1, 1, 0, 0] and not out[7].any() and int(out[3]) == 1 and int(out[0][0, 0]) != second
    # ... and the draw follows the row without that token
    rest = p.clone()
    rest[second] = 0
    want = int(((rest.cumsum(0) > 0.3 * rest.sum()) & (rest > 0)).int().argmax())
    assert int(out[0][0, 0]) == want


@pytest.mark.parametrize("mode", TC.MODES)
@pytest.mark.parametrize("v", [7, 16])
def test_the_first_emitted_token_follows_the_target_distribution(v, mode):
    """What the rule exists for: a root with 3 children, whatever the draft, emits a first token distributed as P_0.  40000
    sequences of one (target, draft) pair over the uniforms of 4 seeds; the children are drawn independently from Q (draft
    mode) or are the 3 likeliest tokens of the draft (one-hot).  Pearson's statistic against P_0 has V - 1 degrees of freedom;
    27.86 and 44.26 are the 0.9999 quantiles for 6 and 15, the significance of the chain's test.  A wrong c recurrence, or an
    acceptance test that forgets R, fails it."""
    n = 10000
    g = torch.Generator().manual_seed(2211 + v)
    x = torch.randn(1, 4, v, generator=g).double() * 1.5
    d = x + torch.randn(1, 4, v, generator=g).double() * 1.5
    p0, q0 = torch.softmax(x[0, 0], dim=0), torch.softmax(d[0, 0], dim=0)
    assert (p0 - q0).abs().max() > 0.1  # (a draft worth rejecting)
    parents = torch.tensor([[-1, 0, 0, 0]], dtype=torch.int32).expand(n, 4)
    count = torch.zeros(v, dtype=torch.float64)
    lens = torch.zeros(3)
    for seed in range(4):
        gs = torch.Generator().manual_seed(seed)
        if mode == "draft":
            kids = torch.multinomial(q0, 3 * n, replacement=True, generator=gs).view(n, 3)
        else:
            kids = q0.topk(3).indices.expand(n, 3)
        tokens = torch.cat([torch.zeros(n, 1, dtype=torch.int64), kids], dim=1)
        u = (torch.rand(n, 4, generator=gs), torch.rand(n, generator=gs))
        out = G.sample_speculative_tree_ref(x.expand(n, 4, v), d.expand(n, 4, v) if mode == "draft" else None, tokens, parents, 0, 0.0,
                                            1.0, u, stats=True)
        count += torch.bincount(out[0][:, 0], minlength=v).double()
        lens += torch.stack([(out[3] == 1).sum(), (out[3] == 2).sum(), ((out[6].sum(dim=1) > 1)).sum()])
    expected = 4 * n * p0
    chi2 = float(((count - expected) ** 2 / expected).sum())
    assert chi2 <= {7: 27.86, 16: 44.26}[v], (chi2, count, expected)
    assert all(k > 400 for k in lens.tolist()), lens  # all rejected, one accepted, a later round ran


def test_cpu_tensors_take_the_oracle_and_the_names_are_exported():
    c = TC.make_case(203, "fp32", 5, 13, 3, "draft")
    out = G.sample_speculative_tree(c["logits"], c["draft"], c["tokens"].int(), c["parents"], 50, 0.9, 0.7, u=c["u"])
    assert len(out) == 4 and out[0].dtype == torch.int32 and out[0].shape == (5, 13) and out[1].dtype == torch.int64
    assert out[2].dtype == torch.int32 and out[3].dtype == torch.int32
    assert all(torch.equal(a.long(), b.long()) for a, b in zip(out, c["r32"][:4]))
    assert len(G.sample_speculative_tree(c["logits"], None, c["tokens"], c["parents"], 0, 0.9, stats=True,
                                         generator=torch.Generator().manual_seed(3))) == 8
    with pytest.raises(ValueError):
        G.sample_speculative_tree(c["logits"].expand(5, 13, 203)[:, :1].expand(5, 65, 203), None, c["tokens"], c["parents"])
    assert "sample_speculative_tree" in G.__all__ and "sample_speculative_tree_ref" in G.__all__
    import flash_attention_annotated_amd.utils as utils
    assert "sample_speculative_tree" in utils.__doc__
