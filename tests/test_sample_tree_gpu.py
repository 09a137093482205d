"""GPU tests of the fused acceptance walk over a tree of draft tokens (csrc/fa_tree_sample.hip through utils.generation): exact
agreement with the oracle on the seeded grid and on every form of tests/sample_tree_plan_universe.py, outside boundary sequences
(tests/sample_tree_cases.py); a chain-shaped tree against sample_speculative, strides, token dtypes, -inf rows, the generator,
repeat calls, graph capture, torch.compile and one verify step end to end."""
import pytest
import torch

import sample_cases as C
import sample_spec_cases as SC
import sample_tree_cases as TC
import sample_tree_plan_universe as U
from flash_attention_annotated_amd.utils import generation as G

pytestmark = pytest.mark.gpu
DEV = "cuda"


def placed(x, shift=0, pad=0):
    """x (B, T, V) on the device with its base `shift` elements off a 256-byte boundary and a node stride of V + pad"""
    b, t, v = x.shape
    buf = torch.full((b * t * (v + pad) + shift + 128,), 7.0, dtype=x.dtype, device=DEV)
    rows = buf[shift:shift + b * t * (v + pad)].view(b, t, v + pad)[:, :, :v]
    rows.copy_(x)
    return rows


def compare(logits, draft, tokens, parents, u, setting, mode, r32, r64, tally, what):
    """one call against the oracles' results; tally = [sequences, left out]"""
    top_k, top_p, temperature = setting
    b, t, v = logits.shape
    out = G._sample_speculative_tree(logits, draft if mode == "draft" else None, tokens, parents, top_k, top_p, temperature, u[0], u[1],
                                     None, True)
    assert out[0].dtype == tokens.dtype and out[0].shape == (b, t) and out[1].dtype == torch.int64 and out[2].dtype == torch.int32
    assert out[2].shape == (b, t) and out[3].dtype == torch.int32 and torch.equal(out[1], out[3].long())
    margin, m_rows = r64[8], r64[9]
    compared = margin > C.tol(v)
    tally[0] += b
    tally[1] += int((~compared).sum())
    assert bool(TC.same_result(r32, r64)[compared].all()), ("oracles disagree", what)
    got = (out[0].long(), out[1], out[2], out[3])
    same = TC.same_result(got, (r64[0].long(),) + tuple(r64[1:4]))
    assert bool(same[compared].all()), (what, [x[compared & ~same] for x in got], [x[compared & ~same] for x in r64[:4]])
    # every node whose parent's rows have clear top-p sums: P and Q rest on those alone; the flags on the whole walk
    clear = m_rows > C.tol(v)
    assert torch.allclose(out[4][clear].double(), r64[4][clear], rtol=1e-5, atol=0), what
    assert torch.allclose(out[5][clear].double(), r64[5][clear], rtol=1e-5, atol=0), what
    assert torch.equal(out[6][compared], r64[6][compared]) and torch.equal(out[7][compared], r64[7][compared]), what
    return out


@pytest.mark.parametrize("dtype", list(TC.DTYPES))
@pytest.mark.parametrize("v", TC.VS)
def test_grid_agrees_exactly_with_the_oracle(v, dtype):
    """B x T x settings x modes of a (V, dtype): 140 calls.  The cap on boundary sequences is asserted first, over the whole
    case."""
    seqs, left_out, kinds = TC.check_oracles(v, dtype, TC.blocks(v), DEV)
    assert seqs == 6 * 5 * 7 * 2 and (all(k > 0 for k in kinds) or v == 1), (seqs, kinds)
    tally = [0, 0]
    for b, t, j, mode in TC.blocks(v):
        c = TC.make_case(v, dtype, b, t, j, mode, DEV)
        compare(c["logits"], c["draft"], c["tokens"], c["parents"], c["u"], c["setting"], mode, c["r32"], c["r64"], tally,
                (v, dtype, b, t, c["setting"], mode, c["shape"]))
    assert tally == [seqs, left_out]
    plan = G._plan_sample_speculative_tree(c["logits"], c["draft"], c["tokens"], c["parents"], *c["setting"])
    cw = 1 if v % 8 else 16 // c["logits"].element_size()  # (odd V: the element form)
    assert plan["cw"] == cw and plan["threads"] == (256 if v // cw <= 1024 else 1024)
    assert plan["threads"] == {4096: 256, 32000: 1024}.get(v, plan["threads"])


def test_the_wide_case():
    v, dtype, b, t, j, mode = TC.WIDE
    setting = TC.settings(v)[j]
    tensors = TC.make_tensors(v, dtype, b, t, setting, 131, "binary", DEV)
    r32, r64 = TC.oracles(*tensors, setting, mode)
    left_out = int((r64[8] <= C.tol(v)).sum())
    assert left_out <= TC.CAP * b, ("boundary sequences above the cap", left_out, b)  # (of 5 sequences: none)
    tally = [0, 0]
    compare(*tensors, setting, mode, r32, r64, tally, TC.WIDE)
    assert tally == [b, left_out]
    plan = G._plan_sample_speculative_tree(*tensors[:4], *setting)
    assert plan["threads"] == 1024 and plan["index_passes"] == 2 and plan["key_passes"] == 3 and plan["cw"] == 8


def test_every_form_of_the_universe_agrees_with_the_oracle():
    tally = [0, 0]
    for n, c in enumerate(U.CASES):
        setting = (c.top_k, c.top_p, c.temperature)
        x0, d0, tokens, parents, u = TC.make_tensors(c.v, c.dtype, c.b, c.t, setting, 77 + n, c.shape, DEV)
        x, d = placed(x0, c.shift, c.pad), placed(d0, c.draft_shift, c.pad)
        plan = U.Plan(**G._plan_sample_speculative_tree(x, d if c.mode == "draft" else None, tokens, parents, *setting))
        assert plan == U.plan(c.b, c.t, c.v, c.dtype, c.mode, c.top_k, c.top_p, c.temperature, x.data_ptr(), d.data_ptr(),
                              (x.stride(0), x.stride(1)), (d.stride(0), d.stride(1))), c.name
        assert plan == U.case_plan(c), c.name
        r32, r64 = TC.oracles(x, d, tokens, parents, u, setting, c.mode)
        compare(x, d, tokens, parents, u, setting, c.mode, r32, r64, tally, c.name)
    assert tally[1] <= TC.CAP * tally[0], tally
    assert set().union(*(U.kernels_of(U.case_plan(c)) for c in U.CASES)) == U.KERNELS


@pytest.mark.parametrize("dtype", list(SC.DTYPES))
def test_a_chain_shaped_tree_is_bit_equal_to_the_chain_verification(dtype):
    """parents = -1, 0, 1, ...: every sequence, boundary or not, gives sample_speculative's num_generated and its tokens up to
    there (behind them the chain leaves the drafts and the tree writes 0), in both access forms and workgroup sizes."""
    for v, b, s, j in ((4096, 64, 4, 3), (4099, 5, 4, 2), (32000, 5, 4, 4), (203, 64, 1, 1), (7, 64, 4, 5), (4096, 5, 0, 3)):
        c = SC.make_case(v, dtype, b, s, j, DEV)
        x, d, tokens, (u_acc, u_res) = c["logits"], c["draft"], c["tokens"], c["u"]
        want = G.sample_speculative(x, d, tokens, *c["setting"], u=(u_acc, u_res))
        d_tree = torch.cat([d, torch.zeros(b, 1, v, dtype=d.dtype, device=DEV)], dim=1)
        t_tree = torch.cat([torch.zeros(b, 1, dtype=tokens.dtype, device=DEV), tokens], dim=1)
        u_tree = torch.cat([torch.zeros(b, 1, device=DEV), u_acc], dim=1)
        parents = TC.make_parents("chain", b, s + 1).to(DEV)
        got = G.sample_speculative_tree(x, d_tree, t_tree, parents, *c["setting"], u=(u_tree, u_res))
        assert torch.equal(got[1], want[1]), (v, s)
        valid = torch.arange(s + 1, device=DEV)[None, :] < want[1][:, None]
        assert torch.equal(got[0][valid], want[0][valid]) and not got[0][~valid].any(), (v, s)
        assert torch.equal(got[2], torch.where(valid, torch.arange(s + 1, device=DEV)[None, :], 0).int())


def test_strided_views_and_both_token_dtypes():
    """Batch and node strides of views into wider tensors (every other sequence), a misaligned base, int32 and int64 tokens and
    parents with a batch stride of their own: the results are those of the dense copies"""
    setting = (40, 0.9, 0.7)
    for v, shift, mode in ((4096, 0, "draft"), (4099, 1, "draft"), (4096, 0, "onehot")):
        x0, d0, tokens0, parents0, u = TC.make_tensors(v, "bf16", 6, 13, setting, 900 + v, "forest", DEV)
        x, d, tokens, parents = placed(x0, shift)[::2], placed(d0, shift)[::2], tokens0[::2], parents0[::2]
        assert not x.is_contiguous() and tokens.stride(0) == 26 and parents.stride(0) == 26
        ua = (u[0][::2].contiguous(), u[1][::2].contiguous())
        r32, r64 = TC.oracles(x, d, tokens, parents, ua, setting, mode)
        out = compare(x, d, tokens, parents, ua, setting, mode, r32, r64, [0, 0], (v, shift, mode))
        dr = d if mode == "draft" else None
        dense = G.sample_speculative_tree(x.contiguous(), None if dr is None else dr.contiguous(), tokens.contiguous(), parents.contiguous(),
                                          *setting, u=ua, stats=True)
        assert all(torch.equal(a, b) for a, b in zip(out, dense))
        out32 = G.sample_speculative_tree(x, dr, tokens.int(), parents.long(), *setting, u=ua)
        assert out32[0].dtype == torch.int32 and torch.equal(out32[0].long(), out[0]) and torch.equal(out32[2], out[2])
    empty = G.sample_speculative_tree(x[:0], None, tokens[:0], parents[:0], *setting)
    assert empty[0].shape == (0, 13) and empty[1].shape == (0,) and empty[2].shape == (0, 13) and empty[3].shape == (0,)


def test_minus_infinity_entries_and_rows():
    inf = float("inf")
    setting = (30, 0.9, 0.7)
    rows = torch.arange(8, device=DEV)
    for dtype, v, mode in (("bf16", 4096, "draft"), ("fp32", 4099, "draft"), ("bf16", 4096, "onehot")):
        x, d, tokens, parents, u = TC.make_tensors(v, dtype, 8, 5, setting, 600 + v, "binary", DEV)
        g = torch.Generator().manual_seed(v)
        x[(torch.rand(8, 5, v, generator=g) < 0.3).to(DEV)] = -inf
        d[(torch.rand(8, 5, v, generator=g) < 0.3).to(DEV)] = -inf
        x[2, 0, :] = -inf  # a target row of nothing but -inf at the root: P = 0, and the token drawn there is 0
        d[4, 0, :] = -inf  # a draft row of nothing but -inf: Q = 0, the first child in range is accepted
        x[5, :, :] = -inf
        d[5, :, :] = -inf  # P = Q = 0: the first child of every level is accepted, and the draw at the leaf gives 0
        tokens[5] = torch.tensor([0, 1, 2, 3, 4])
        for st in (setting, (0, 0.0, 1.0)):
            r32, r64 = TC.oracles(x, d, tokens, parents, u, st, mode)
            tally = [0, 0]
            out = compare(x, d, tokens, parents, u, st, mode, r32, r64, tally, (dtype, v, st, mode))
            assert tally[1] <= 1
            if mode == "draft":
                assert out[2][5].tolist() == [0, 1, 3, 0, 0] and out[0][5].tolist() == [1, 3, 0, 0, 0] and int(out[1][5]) == 3
            else:
                assert int(out[1][5]) == 1 and int(out[0][5, 0]) == 0  # (nothing has weight: nothing is accepted)
            last = out[2].long().gather(1, (out[1] - 1)[:, None])[:, 0]
            row = x[rows, last]
            chosen = row.gather(1, out[0][rows, out[1] - 1][:, None])[:, 0]
            finite = ~row.isinf().all(dim=1)
            assert not chosen[finite].isinf().any(), "-inf is never drawn while the row has a finite entry"


def test_the_generator_reproduces_and_repeat_calls_are_bit_equal():
    setting = (40, 0.9, 0.8)
    for mode in TC.MODES:
        x, d, tokens, parents, u = TC.make_tensors(4096, "bf16", 64, 13, setting, 5, "binary", DEV)
        dr = d if mode == "draft" else None
        first = G._sample_speculative_tree(x, dr, tokens, parents, *setting, u[0], u[1], None, True)
        for _ in range(3):
            again = G._sample_speculative_tree(x, dr, tokens, parents, *setting, u[0], u[1], None, True)
            assert all(torch.equal(a, b) for a, b in zip(first, again))
        torch.manual_seed(99)
        a, a2 = G.sample_speculative_tree(x, dr, tokens, parents, *setting), G.sample_speculative_tree(x, dr, tokens, parents, *setting)
        torch.manual_seed(99)
        b = G.sample_speculative_tree(x, dr, tokens, parents, *setting)
        assert all(torch.equal(p, q) for p, q in zip(a, b)) and not all(torch.equal(p, q) for p, q in zip(a, a2))
        # an explicit generator: (seed, offset) are what it gives next, the uniforms are uniform_ref's, the result the oracle's
        g = torch.Generator(device=DEV).manual_seed(7)
        state = torch.randint(-(1 << 62), 1 << 62, (2,), generator=torch.Generator(device=DEV).manual_seed(7), device=DEV, dtype=torch.int64)
        out = G.sample_speculative_tree(x, dr, tokens, parents, *setting, generator=g)
        un = G.uniform_ref(int(state[0]), int(state[1]), 64 * 13 + 64, DEV)
        ur = (un[:64 * 13].view(64, 13), un[64 * 13:])
        r32, r64 = TC.oracles(x, d, tokens, parents, ur, setting, mode)
        compared = r64[8] > C.tol(4096)
        assert compared.sum() >= 60 and bool(TC.same_result((out[0].long(),) + tuple(out[1:]), r64)[compared].all())


def test_graph_capture_and_replay():
    """... with a replay after parents, tokens_draft, the logits and the uniforms were overwritten in place"""
    setting = (50, 0.9, 0.7)
    for mode in TC.MODES:
        x, d, tokens, parents, u = TC.make_tensors(4096, "bf16", 8, 13, setting, 41, "binary", DEV)
        dr = d if mode == "draft" else None
        G.sample_speculative_tree(x, dr, tokens, parents, *setting, u=u)  # (warm up outside the capture)
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=stream):
                out = G.sample_speculative_tree(x, dr, tokens, parents, *setting, u=u)
        for seed, shape in ((42, "forest"), (43, "star")):
            x2, d2, t2, p2, u2 = TC.make_tensors(4096, "bf16", 8, 13, setting, seed, shape, DEV)
            x.copy_(x2), d.copy_(d2), tokens.copy_(t2), parents.copy_(p2), u[0].copy_(u2[0]), u[1].copy_(u2[1])
            graph.replay()
            torch.cuda.synchronize()
            want = G.sample_speculative_tree(x, dr, tokens, parents, *setting, u=u)
            assert all(torch.equal(a, b) for a, b in zip(out, want))


def test_torch_compile_fullgraph():
    setting = (50, 0.9, 0.7)
    x, d, tokens, parents, u = TC.make_tensors(4096, "fp32", 4, 5, setting, 51, "binary", DEV)

    def step(logits, draft, tokens, parents, u_acc, u_res):
        return G.sample_speculative_tree(logits * 1.0, draft, tokens, parents, *setting, u=(u_acc, u_res))

    out = torch.compile(step, fullgraph=True)(x, d, tokens, parents, u[0], u[1])
    want = G.sample_speculative_tree(x, d, tokens, parents, *setting, u=u)
    assert len(out) == 4 and all(torch.equal(a, b) for a, b in zip(out, want))

    def drawn(logits, tokens, parents):
        return G.sample_speculative_tree(logits, None, tokens, parents, 0, 0.0, 2.5), G.sample_speculative_tree(logits, None, tokens, parents, 0, 0.0, 2.5)

    a, b = torch.compile(drawn, fullgraph=True)(x[:1].expand(64, 5, 4096), tokens[:1].expand(64, 5), parents[:1].expand(64, 5))
    assert a[0].shape == b[0].shape == (64, 5) and not all(torch.equal(p, q) for p, q in zip(a, b))  # two draws: the pair is an input


def test_tree_verify_step_end_to_end():
    """append -> flash_attn_with_kvcache_tree -> logits from a fixed random projection -> sample_speculative_tree ->
    kvcache_keep_tree_path_(path, path_len) -> a one-token decode: bit-equal to the decode on a cache that only ever received
    the accepted chain."""
    from flash_attention_annotated_amd import hopper_interface as fa3
    torch.manual_seed(61)
    B, H, HK, D, T, CAP, V = 2, 8, 2, 64, 13, 512, 203
    bf = torch.bfloat16
    prefix = torch.tensor([40, 100], dtype=torch.int32, device=DEV)
    k0, v0 = torch.randn(B, CAP, HK, D, device=DEV).to(bf), torch.randn(B, CAP, HK, D, device=DEV).to(bf)
    for b in range(B):  # only the prefix is filled
        k0[b, int(prefix[b]):], v0[b, int(prefix[b]):] = 0, 0
    kd, vd = torch.randn(B, T, HK, D, device=DEV).to(bf), torch.randn(B, T, HK, D, device=DEV).to(bf)
    q, q1 = torch.randn(B, T, H, D, device=DEV).to(bf), torch.randn(B, 1, H, D, device=DEV).to(bf)
    parents = TC.make_parents("binary", B, T).to(DEV)
    head = (torch.randn(H * D, V, device=DEV) * 0.5).to(bf)
    kc, vc = k0.clone(), v0.clone()
    fa3.flash_attn_with_kvcache(q, kc, vc, k=kd, v=vd, cache_seqlens=prefix)  # (the append; its output is not used)
    hidden = fa3.flash_attn_with_kvcache_tree(q, kc, vc, fa3.tree_mask_from_parents(parents), cache_seqlens=prefix + T)
    logits = hidden.reshape(B, T, H * D) @ head * 8.0
    tokens = logits.float().argmax(dim=2).gather(1, parents.long().clamp_min(0))  # the likeliest token under the parent: accepted
    tokens[:, 2::2] = V  # ... and the second child of every node out of range: never
    u = (torch.full((B, T), 0.5, device=DEV), torch.rand(B, device=DEV))
    out, num, path, path_len = G.sample_speculative_tree(logits, None, tokens, parents, 1, 0.0, 1.0, u=u)
    assert path[:, :4].tolist() == [[0, 1, 3, 7]] * B and path_len.tolist() == [4] * B and num.tolist() == [4] * B
    assert torch.equal(out[:, :3], tokens[:, [1, 3, 7]]) and torch.equal(out[:, 3], logits[:, 7].float().argmax(dim=1))
    new = fa3.kvcache_keep_tree_path_(kc, vc, prefix, path, path_len)
    assert torch.equal(new, prefix + path_len)
    step = fa3.flash_attn_with_kvcache(q1, kc, vc, cache_seqlens=new)
    kr, vr = k0.clone(), v0.clone()  # the cache that only ever received the accepted chain
    for b in range(B):
        s, n = int(prefix[b]), int(path_len[b])
        kr[b, s:s + n], vr[b, s:s + n] = kd[b, path[b, :n].long()], vd[b, path[b, :n].long()]
    want = fa3.flash_attn_with_kvcache(q1, kr, vr, cache_seqlens=new)
    assert torch.equal(step, want)
