"""GPU tests of the fused verification of speculative sampling (csrc/fa_spec_sample.hip through utils.generation): exact agreement
with the oracle on the seeded grid and on every form of tests/sample_spec_plan_universe.py, outside boundary sequences
(tests/sample_spec_cases.py); strides, token dtypes, -inf rows, the generator, repeat calls, graph capture and torch.compile."""
import pytest
import torch

import sample_cases as C
import sample_spec_cases as SC
import sample_spec_plan_universe as U
from flash_attention_annotated_amd.utils import generation as G

pytestmark = pytest.mark.gpu
DEV = "cuda"


def placed(x, shift=0, pad=0):
    """x (B, S, V) on the device with its base `shift` elements off a 256-byte boundary and a position stride of V + pad"""
    b, s, v = x.shape
    buf = torch.full((b * s * (v + pad) + shift + 128,), 7.0, dtype=x.dtype, device=DEV)
    rows = buf[shift:shift + b * s * (v + pad)].view(b, s, v + pad)[:, :, :v]
    rows.copy_(x)
    return rows


def compare(logits, draft, tokens, u, setting, r32, r64, tally, what):
    """one call against the oracles' results; tally = [sequences, left out]"""
    top_k, top_p, temperature = setting
    v, s = logits.shape[2], tokens.shape[1]
    out, num, p_tok, q_tok, accepted = G._sample_speculative(logits, draft, tokens, top_k, top_p, temperature, u[0], u[1], None, True)
    assert out.dtype == tokens.dtype and out.shape == (logits.shape[0], s + 1) and num.dtype == torch.int64
    t64, n64, p64, q64, a64, margin, m_rows, m_acc = r64
    compared = margin > C.tol(v)
    tally[0] += logits.shape[0]
    tally[1] += int((~compared).sum())
    assert bool(SC.same_up_to_n(r32[0], r32[1], t64, n64)[compared].all()), ("oracles disagree", what)
    same = SC.same_up_to_n(out.long(), num, t64, n64)
    assert bool(same[compared].all()), (what, out[compared & ~same], num[compared & ~same], t64[compared & ~same], n64[compared & ~same])
    if s > 0:
        # every position of every sequence, before and after the first rejection, whose own comparisons are clear: P and Q rest on
        # the top-p sums of the position's two rows, the flag on those and on its acceptance test
        clear = m_rows > C.tol(v)
        assert torch.allclose(p_tok[clear].double(), p64[clear], rtol=1e-5, atol=0), what
        assert torch.allclose(q_tok[clear].double(), q64[clear], rtol=1e-5, atol=0), what
        sure = clear & (m_acc > C.tol(v))
        assert torch.equal(accepted[sure], a64[sure]), what
    return out, num


@pytest.mark.parametrize("dtype", list(SC.DTYPES))
@pytest.mark.parametrize("v", SC.VS)
def test_grid_agrees_exactly_with_the_oracle(v, dtype):
    """B x S x settings of a (V, dtype): 63 calls.  The cap on boundary sequences is asserted first, over the whole case."""
    seqs, left_out, kinds = SC.check_oracles(v, dtype, SC.blocks(v), DEV)
    assert seqs == 70 * 3 * 7 and all(k > 0 for k in kinds), (seqs, kinds)
    tally = [0, 0]
    for b, s, j in SC.blocks(v):
        c = SC.make_case(v, dtype, b, s, j, DEV)
        compare(c["logits"], c["draft"], c["tokens"], c["u"], c["setting"], c["r32"], c["r64"], tally, (v, dtype, b, s, c["setting"]))
    assert tally == [seqs, left_out]


def test_the_wide_case():
    v, dtype, b, s, j = SC.WIDE
    setting = SC.settings(v)[j]
    logits, draft, tokens, u = SC.make_tensors(v, dtype, b, s, setting, 131, DEV)
    r32, r64 = SC.oracles(logits, draft, tokens, u, setting)
    left_out = int((r64[5] <= C.tol(v)).sum())
    assert left_out <= SC.CAP * b, ("boundary sequences above the cap", left_out, b)  # (of 5 sequences: none)
    tally = [0, 0]
    compare(logits, draft, tokens, u, setting, r32, r64, tally, SC.WIDE)
    assert tally == [b, left_out]
    plan = G._plan_sample_speculative(logits, draft, tokens, *setting)
    assert plan["threads"] == 1024 and plan["index_passes"] == 2 and plan["key_passes"] == 3 and plan["cw"] == 8


def test_every_form_of_the_universe_agrees_with_the_oracle():
    tally = [0, 0]
    for n, c in enumerate(U.CASES):
        setting = (c.top_k, c.top_p, c.temperature)
        x0, d0, tokens, u = SC.make_tensors(c.v, c.dtype, c.b, c.s, setting, 77 + n, DEV)
        x, d = placed(x0, c.shift, c.pad), placed(d0, c.draft_shift, c.pad)
        plan = U.Plan(**G._plan_sample_speculative(x, d, tokens, *setting))
        assert plan == U.plan(c.b, c.s, c.v, c.dtype, c.top_k, c.top_p, c.temperature, x.data_ptr(), d.data_ptr(),
                              (x.stride(0), x.stride(1)), (d.stride(0), d.stride(1))), c.name
        assert plan == U.case_plan(c), c.name
        r32, r64 = SC.oracles(x, d, tokens, u, setting)
        compare(x, d, tokens, u, setting, r32, r64, tally, c.name)
    assert tally[1] <= SC.CAP * tally[0], tally
    assert set().union(*(U.kernels_of(U.case_plan(c)) for c in U.CASES)) == U.KERNELS


def test_strided_views_and_both_token_dtypes():
    """Batch and position strides of views into wider tensors (every other sequence, the last positions of a longer block),
    a misaligned base, int32 and int64 drafts with a batch stride of their own: the results are those of the dense copies"""
    setting = (40, 0.9, 0.7)
    for v, shift in ((4096, 0), (4099, 1)):
        x0, d0, tokens0, u = SC.make_tensors(v, "bf16", 6, 7, setting, 900 + v, DEV)
        x, d, tokens = placed(x0, shift)[::2, 3:], placed(d0, shift)[::2, 3:], tokens0[::2, 3:]
        assert not x.is_contiguous() and tokens.stride(0) == 14
        ua = (u[0][::2, 3:].contiguous(), u[1][::2].contiguous())
        r32, r64 = SC.oracles(x, d, tokens, ua, setting)
        out, num = compare(x, d, tokens, ua, setting, r32, r64, [0, 0], (v, shift))
        dense = G.sample_speculative(x.contiguous(), d.contiguous(), tokens.contiguous(), *setting, u=ua)
        assert torch.equal(out, dense[0]) and torch.equal(num, dense[1])
        out32, num32 = G.sample_speculative(x, d, tokens.int(), *setting, u=ua)
        assert out32.dtype == torch.int32 and torch.equal(out32.long(), out) and torch.equal(num32, num)
    empty = G.sample_speculative(x[:0], d[:0], tokens[:0], *setting)
    assert empty[0].shape == (0, 5) and empty[1].shape == (0,)


def test_minus_infinity_entries_and_rows():
    inf = float("inf")
    setting = (30, 0.9, 0.7)
    for dtype, v in (("bf16", 4096), ("fp32", 4099)):
        x, d, tokens, u = SC.make_tensors(v, dtype, 8, 3, setting, 600 + v, DEV)
        g = torch.Generator().manual_seed(v)
        x[(torch.rand(8, 4, v, generator=g) < 0.3).to(DEV)] = -inf
        d[(torch.rand(8, 3, v, generator=g) < 0.3).to(DEV)] = -inf
        x[2, 1, :] = -inf  # a target row of nothing but -inf: P = 0, rejected unless Q = 0 too; the token drawn there is 0
        d[4, 0, :] = -inf  # a draft row of nothing but -inf: Q = 0, accepted
        x[5, :, :] = -inf
        d[5, :, :] = -inf  # P = Q = 0: accepted to the end, and the draw of column S gives 0
        tokens[5] = torch.tensor([1, 2, 3])
        for st in (setting, (0, 0.0, 1.0)):
            r32, r64 = SC.oracles(x, d, tokens, u, st)
            tally = [0, 0]
            out, num = compare(x, d, tokens, u, st, r32, r64, tally, (dtype, v, st))
            assert tally[1] <= 1 and out[5].tolist() == [1, 2, 3, 0] and int(num[5]) == 4
            ok = num > 0
            chosen = x[torch.arange(8, device=DEV), num - 1].gather(1, out[torch.arange(8, device=DEV), num - 1][:, None])[:, 0]
            finite = ~x[torch.arange(8, device=DEV), num - 1].isinf().all(dim=1)
            assert not chosen[finite & ok].isinf().any(), "-inf is never drawn while the row has a finite entry"


def test_the_generator_reproduces_and_repeat_calls_are_bit_equal():
    setting = (40, 0.9, 0.8)
    x, d, tokens, u = SC.make_tensors(4096, "bf16", 64, 4, setting, 5, DEV)
    first = G._sample_speculative(x, d, tokens, *setting, u[0], u[1], None, True)
    for _ in range(3):
        again = G._sample_speculative(x, d, tokens, *setting, u[0], u[1], None, True)
        assert all(torch.equal(a, b) for a, b in zip(first, again))
    torch.manual_seed(99)
    a, a2 = G.sample_speculative(x, d, tokens, *setting), G.sample_speculative(x, d, tokens, *setting)
    torch.manual_seed(99)
    b = G.sample_speculative(x, d, tokens, *setting)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and not (torch.equal(a[0], a2[0]) and torch.equal(a[1], a2[1]))
    # an explicit generator: (seed, offset) are what it gives next, the uniforms are uniform_ref's, the result the oracle's
    g = torch.Generator(device=DEV).manual_seed(7)
    state = torch.randint(-(1 << 62), 1 << 62, (2,), generator=torch.Generator(device=DEV).manual_seed(7), device=DEV, dtype=torch.int64)
    out, num = G.sample_speculative(x, d, tokens, *setting, generator=g)
    un = G.uniform_ref(int(state[0]), int(state[1]), 64 * 4 + 64, DEV)
    ur = (un[:256].view(64, 4), un[256:])
    r32, r64 = SC.oracles(x, d, tokens, ur, setting)
    compared = r64[5] > C.tol(4096)
    assert compared.sum() >= 60 and bool(SC.same_up_to_n(out, num, r64[0], r64[1])[compared].all())


def test_graph_capture_and_replay():
    setting = (50, 0.9, 0.7)
    x, d, tokens, u = SC.make_tensors(4096, "bf16", 8, 4, setting, 41, DEV)
    G.sample_speculative(x, d, tokens, *setting, u=u)  # (warm up outside the capture)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            out, num = G.sample_speculative(x, d, tokens, *setting, u=u)
    for seed in (42, 43):
        x2, d2, t2, u2 = SC.make_tensors(4096, "bf16", 8, 4, setting, seed, DEV)
        x.copy_(x2), d.copy_(d2), tokens.copy_(t2), u[0].copy_(u2[0]), u[1].copy_(u2[1])
        graph.replay()
        torch.cuda.synchronize()
        want = G.sample_speculative(x, d, tokens, *setting, u=u)
        assert torch.equal(out, want[0]) and torch.equal(num, want[1])


def test_torch_compile_fullgraph():
    setting = (50, 0.9, 0.7)
    x, d, tokens, u = SC.make_tensors(4096, "fp32", 4, 2, setting, 51, DEV)

    def step(logits, draft, tokens, u_acc, u_res):
        return G.sample_speculative(logits * 1.0, draft, tokens, *setting, u=(u_acc, u_res))

    out, num = torch.compile(step, fullgraph=True)(x, d, tokens, u[0], u[1])
    want = G.sample_speculative(x, d, tokens, *setting, u=u)
    assert torch.equal(out, want[0]) and torch.equal(num, want[1])

    def drawn(logits, draft, tokens):
        return G.sample_speculative(logits, draft, tokens, 0, 0.0, 2.5), G.sample_speculative(logits, draft, tokens, 0, 0.0, 2.5)

    (a, na), (b, nb) = torch.compile(drawn, fullgraph=True)(x[:1].expand(64, 3, 4096), d[:1].expand(64, 2, 4096), tokens[:1].expand(64, 2))
    assert a.shape == b.shape == (64, 3) and not (torch.equal(a, b) and torch.equal(na, nb))  # two draws: the pair is an input
