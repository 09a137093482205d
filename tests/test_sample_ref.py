"""CPU tests of flash_attention_annotated_amd.utils.generation: the reference's names and signatures, InferenceParams, the oracle
(sample_ref, filter_ref, uniform_ref) on hand-made rows, the CPU path of `sample` and of the modify_logits_* functions, and the
condition the seeded grid of tests/test_sample_gpu.py rests on: on its inputs, the fp32 oracle and the fp64 oracle agree on every
row that is no boundary row, and boundary rows stay within the cap (tests/sample_cases.py)."""
import dataclasses
import inspect
import math

import pytest
import torch

import sample_cases as C
from flash_attention_annotated_amd.utils import generation as G

INF = float("inf")


def row(*values, dtype=torch.float32):
    return torch.tensor([values], dtype=dtype)


def u_of(*values):
    return torch.tensor(values, dtype=torch.float32)


def test_signatures_are_the_references():
    def sig(fn):
        return tuple((p.name, p.default, p.kind.name) for p in inspect.signature(fn).parameters.values())
    empty, pos, kw = inspect.Parameter.empty, "POSITIONAL_OR_KEYWORD", "KEYWORD_ONLY"
    assert sig(G.modify_logits_for_top_k_filtering) == (("logits", empty, pos), ("top_k", empty, pos))
    assert sig(G.modify_logits_for_top_p_filtering) == (("logits", empty, pos), ("top_p", empty, pos))
    assert sig(G.sample) == (("logits", empty, pos), ("top_k", 1, pos), ("top_p", 0.0, pos), ("temperature", 1.0, pos),
                             ("generator", None, kw), ("u", None, kw))
    fields = [(f.name, f.type, f.default if f.default is not dataclasses.MISSING else None) for f in dataclasses.fields(G.InferenceParams)]
    assert [f[0] for f in fields] == ["max_seqlen", "max_batch_size", "seqlen_offset", "batch_size_offset", "key_value_memory_dict",
                                      "lengths_per_sample"]
    assert [f[2] for f in fields] == [None, None, 0, 0, None, None]
    assert sig(G.InferenceParams.reset) == (("self", empty, pos), ("max_seqlen", empty, pos), ("max_batch_size", empty, pos))
    with pytest.raises(AssertionError, match="top-p should be in"):
        G.sample(torch.zeros(1, 4), top_k=0, top_p=1.5)


def test_inference_params_reset():
    p = G.InferenceParams(max_seqlen=128, max_batch_size=4)
    assert p.key_value_memory_dict == {} and p.lengths_per_sample is None and p.seqlen_offset == 0 == p.batch_size_offset
    p.seqlen_offset, p.batch_size_offset, p.lengths_per_sample = 17, 2, torch.tensor([3, 4, 5, 6])
    p.key_value_memory_dict[0] = "kept"
    p.reset(256, 8)
    assert (p.max_seqlen, p.max_batch_size, p.seqlen_offset, p.batch_size_offset) == (256, 8, 0, 2)
    assert p.lengths_per_sample.tolist() == [0, 0, 0, 0] and p.key_value_memory_dict == {0: "kept"}
    G.InferenceParams(1, 1).reset(2, 2)  # (without lengths_per_sample)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_top_k_ties_go_to_the_lower_index(dtype):
    x = row(1.0, 3.0, 2.0, 3.0, 2.0, 2.0, 0.0, dtype=dtype)  # the two 3s, then the 2s at 2, 4, 5
    # top_k = 3: {1, 3, 2}.  p = e^3, e^3, e^2 over z: u just below p_1 + p_2(=index 2) picks 2, above it 3
    z = 2 * math.exp(3) + math.exp(2)
    edge = (math.exp(3) + math.exp(2)) / z
    token, kept, mass, _ = G.sample_ref(x.expand(4, 7), 3, 0.0, 1.0, u_of(0.0, edge - 1e-3, edge + 1e-3, 0.999), stats=True)
    assert token.tolist() == [1, 2, 3, 3] and kept.tolist() == [3] * 4 and torch.allclose(mass, torch.ones(4, dtype=dtype))
    # top_k = 4: index 4 joins, 5 does not: the last u falls on 4 and never on 5
    token = G.sample_ref(x.expand(2, 7), 4, 0.0, 1.0, u_of(0.9999, 0.0))
    assert token.tolist() == [4, 1]
    # the filter keeps every 2
    assert G.filter_ref(x, 3, 0.0).tolist() == [[-INF, 3.0, 2.0, 3.0, 2.0, 2.0, -INF]]
    assert G.filter_ref(x, 1, 0.0).tolist() == [[-INF, 3.0, -INF, 3.0, -INF, -INF, -INF]]
    assert G.filter_ref(x, 7, 0.0).tolist() == x.tolist() and G.filter_ref(x, 0, 0.0).tolist() == x.tolist()


def test_greedy_is_the_lowest_index_of_the_maxima():
    x = torch.tensor([[0.0, 5.0, 5.0, 1.0], [7.0, 7.0, 7.0, 7.0], [-INF, -INF, -INF, -INF], [-1.0, -0.0, 0.0, -2.0]])
    assert G.sample_ref(x, 1, 0.0, 1.0, torch.zeros(4)).tolist() == [1, 0, 0, 1]
    assert G.sample(x).tolist() == [1, 0, 0, 1]  # the CPU path, the reference's defaults


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_top_p(dtype):
    p = torch.tensor([[0.05, 0.4, 0.05, 0.3, 0.2]], dtype=dtype)
    x = p.log()
    # ascending (p, -index): 2 (0.05), 0 (0.05), 4, 3, 1.  top_p = 0.92: cumulative <= 0.08 leaves: index 2 only
    token, kept, mass, margin = G.sample_ref(x.expand(3, 5), 0, 0.92, 1.0, u_of(0.0, 0.5, 0.9999), stats=True)
    assert kept.tolist() == [4, 4, 4] and torch.allclose(mass, torch.full((3,), 0.95, dtype=dtype))
    assert token.tolist() == [0, 3, 4]  # 0.05, 0.45 | 0.75 | 0.95 of 0.95
    assert torch.all(margin[:2] > 1e-3) and margin[2] < 2e-4  # (the last u is 1e-4 below the total)
    assert G.filter_ref(x, 0, 0.92)[0].isinf().tolist() == [False, False, True, False, False]
    # top_p = 0.85: cumulative <= 0.15 leaves 2 and 0; 0.5: 2, 0, 4 (0.3) leave, 3 (0.6) stays
    assert G.filter_ref(x, 0, 0.85)[0].isinf().tolist() == [True, False, True, False, False]
    assert G.filter_ref(x, 0, 0.5)[0].isinf().tolist() == [True, False, True, False, True]
    # top_p -> 0+: only the largest entry stays, however small top_p is
    for tiny in (1e-3, 1e-10, 1e-30):
        token, kept, mass, _ = G.sample_ref(x, 0, tiny, 1.0, u_of(0.9999), stats=True)
        assert token.tolist() == [1] and kept.tolist() == [1] and abs(mass.item() - 0.4) < 1e-6
    # of equal largest entries the lower index stays
    assert G.filter_ref(torch.zeros(1, 4, dtype=dtype), 0, 1e-10).tolist() == [[0.0, -INF, -INF, -INF]]
    # top_p 0 and 1 filter nothing
    for none in (0.0, 1.0):
        assert G.sample_ref(x, 0, none, 1.0, u_of(0.0), stats=True)[1].tolist() == [5]
    # top-k first, top-p within it: top_k = 3 leaves {1, 3, 4} with p = 4/9, 3/9, 2/9; top_p = 0.7: 2/9 <= 0.3 leaves
    token, kept, mass, _ = G.sample_ref(x, 3, 0.7, 1.0, u_of(0.99), stats=True)
    assert token.tolist() == [3] and kept.tolist() == [2] and abs(mass.item() - 7 / 9) < 1e-6


def test_draw_walks_in_index_order():
    x = torch.tensor([[0.1, 0.2, 0.3, 0.4]]).log()
    u = u_of(0.0, 0.0999, 0.1001, 0.2999, 0.3001, 0.5999, 0.6001, 1.0 - 2.0 ** -24)
    assert G.sample_ref(x.expand(8, 4), 0, 0.0, 1.0, u).tolist() == [0, 0, 1, 1, 2, 2, 3, 3]
    # a temperature: p^(1/T) renormalised
    t = G.sample_ref(x.expand(2, 4), 0, 0.0, 0.5, u_of(0.0334, 0.0332))  # p^2 / sum: 1/30, 4/30, ...
    assert t.tolist() == [1, 0]


def test_minus_infinity_and_one_column():
    x = torch.tensor([[-INF, 0.0, -INF, 0.0, -INF]])
    u = u_of(0.0, 0.4999, 0.5001, 1.0 - 2.0 ** -24)
    for top_k in (0, 2, 4, 5, 9):  # (4: two -inf entries are candidates, and are never drawn)
        assert G.sample_ref(x.expand(4, 5), top_k, 0.0, 1.0, u).tolist() == [1, 1, 3, 3], top_k
    token, kept, mass, _ = G.sample_ref(x, 4, 0.0, 1.0, u_of(0.7), stats=True)
    assert kept.tolist() == [4] and mass.tolist() == [1.0]
    assert G.sample_ref(x, 4, 0.5, 1.0, u_of(0.7), stats=True)[1].tolist() == [1]  # top-p removes the p = 0 entries and index 3
    nothing = torch.full((2, 3), -INF)
    token, kept, mass, _ = G.sample_ref(nothing, 0, 0.9, 1.0, u_of(0.3, 0.9), stats=True)
    assert token.tolist() == [0, 0] and kept.tolist() == [0, 0] and mass.tolist() == [0.0, 0.0]
    assert G.filter_ref(nothing, 2, 0.9).tolist() == nothing.tolist()
    one = torch.tensor([[3.0], [-2.0]])
    for top_k, top_p in ((0, 0.0), (1, 0.0), (2, 0.5), (0, 0.9)):
        assert G.sample_ref(one, top_k, top_p, 0.7, u_of(0.0, 0.999)).tolist() == [0, 0]
    assert G.filter_ref(one, 1, 0.5).tolist() == one.tolist()


def test_uniform_ref():
    u = G.uniform_ref(1234, 5678, 4096)
    assert u.dtype == torch.float32 and u.min() >= 0.0 and u.max() < 1.0 and 0.45 < u.mean() < 0.55
    assert len(set(u.tolist())) > 4000
    assert not torch.equal(u, G.uniform_ref(1234, 5679, 4096)) and not torch.equal(u, G.uniform_ref(1235, 5678, 4096))
    assert torch.equal(u, G.uniform_ref(1234 - (1 << 64), 5678, 4096))  # (an int64 seed is its 64 bits)
    assert torch.equal(u[:7], G.uniform_ref(1234, 5678, 7))


def test_cpu_paths():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(6, 33, generator=g).to(torch.bfloat16)
    u = torch.rand(6, generator=g)
    assert torch.equal(G.sample(x, 5, 0.9, 0.7, u=u), G.sample_ref(x, 5, 0.9, 0.7, u))
    a = G.sample(x, 0, 0.9, generator=torch.Generator().manual_seed(1))
    assert torch.equal(a, G.sample(x, 0, 0.9, generator=torch.Generator().manual_seed(1))) and a.dtype == torch.int64 and a.shape == (6,)
    y = x.clone()
    assert G.modify_logits_for_top_k_filtering(y, 4) is None
    assert torch.equal(y, G.filter_ref(x, 4, 0.0)) and (~y.isinf()).sum(dim=1).min() >= 4
    y = x.clone()
    G.modify_logits_for_top_p_filtering(y, 0.6)
    assert torch.equal(y, G.filter_ref(x, 0, 0.6)) and y.isinf().any()
    for top_p in (0.0, -1.0, 1.0, 2.0):  # the reference's early returns
        y = x.clone()
        G.modify_logits_for_top_p_filtering(y, top_p)
        assert torch.equal(y, x)
    with pytest.raises(RuntimeError):
        G.modify_logits_for_top_k_filtering(x.clone(), 34)
    y = x.clone().view(2, 3, 33)  # (..., vocab)
    G.modify_logits_for_top_k_filtering(y, 4)
    assert torch.equal(y.view(6, 33), G.filter_ref(x, 4, 0.0))


WIDE = 32000  # from this V on the CPU takes the blocks of 1 and 5 rows; the block of 64 is held to the same condition on the
# device, by test_sample_gpu.py::test_oracles_agree_on_the_wide_blocks, which runs no kernel: the fp64 oracle of 64 x 131080 with
# all 72 settings is minutes of sorting on a CPU


@pytest.mark.parametrize("dtype", list(C.DTYPES))
@pytest.mark.parametrize("v", C.VS)
def test_fp32_oracle_agrees_with_fp64_outside_boundary_rows(v, dtype):
    """What the exact comparison on the device rests on, on the very inputs it uses and the full product of the settings:
    boundary rows (by the fp64 oracle) are within the cap of the rows of the case, and on every other row the fp32 oracle gives
    the fp64 oracle's token, count and mass."""
    bs = C.BS if v < WIDE else C.BS[:2]
    rows, _ = C.check_oracles(v, dtype, bs)
    assert rows == sum(bs) * 72 == sum(bs) * len(C.settings(v))  # 216 (B, top_k, top_p, temperature) per (V, dtype) with all of BS
