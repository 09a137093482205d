"""The copy path of the binding (csrc/torch_binding.cpp): aligned_or_copy() copies any operand whose base is not 16-byte
aligned or whose strides are no multiples of 8, computes into a temporary where the caller's out / dq / dk / dv is such a view,
and copies the result back.  One case per entry point -- dense and varlen forward, dense and varlen backward,
flash_attn_2_cuda.fwd_kvcache (q / out / k_new / v_new) and torch.ops.flash_attn_3.fwd -- with a "misaligned" layout of
tests/layouts.py (4 spare columns, or a base 4 elements off) on one operand at a time: the result is bit-equal to the contiguous
call's, lies in the tensor the caller passed, and the sentinels around it are intact.  The KV cache itself is never copied: a
misaligned cache raises (cache_aligned), which launches nothing.  Misaligned views only ever reach the binding here, never the
C ABI.
The forward routes that share that path (FwdArgs -> fill_fwd_params, OutPath) have a case each below the cache step: ragged
queries over a 16-bit cache (fwd_kvcache_ragged), the fp8-cache read (fa_fwd_kv8), the MLA read (fa_fwd_qv8),
fwd_kvcache_sparse over both cache types, and the cute forward with a sink and with block lists.  There q, qv and o take
both misaligned layouts in turn; fwd_kvcache_sparse and cute_fwd take no out, so their out is compared only."""
import pytest
import torch

import layouts as L

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, SQ, SK, H, HK, D = 2, 70, 130, 4, 2, 64
LENS_Q, LENS_K = (33, 37), (70, 60)
MIS = L.MISALIGNED_LAYOUTS


def _rand(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(torch.bfloat16)


def _same(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


def _cases(names, outputs):
    """[(operand that is misaligned, layout)]: every input and every output of the entry point, both misaligned layouts in turn
    (the names in `outputs` get both layouts each: the newer cases list q and qv there too)."""
    return [(n, MIS[i % 2]) for i, n in enumerate(names + outputs)] + [(n, MIS[(i + 1) % 2]) for i, n in enumerate(outputs)]


def _run(call, t, outputs, which, layout):
    """call(ops) -> results in the order of `outputs`; ops: the inputs of t, and the outputs as tensors to fill (or None).  Runs it
    contiguous with the binding's own outputs, then with `which` misaligned, and compares."""
    ops = {n: x.to(DEV) for n, x in t.items()}
    ops.update({n: None for n in outputs})
    want = call(ops)
    placed = {}
    for n, x in t.items():
        placed[n] = L.place_input(x, layout if n == which else "contiguous", DEV)
    outs = {n: L.place_output(outputs[n], torch.bfloat16, layout if n == which else "padded", DEV) for n in outputs}
    assert not L.aligned((placed.get(which) or outs[which]).view)
    ops = {n: p.view for n, p in placed.items()}
    ops.update({n: p.view for n, p in outs.items()})
    got = call(ops)
    for n, g, w in zip(outputs, got, want):
        assert g.data_ptr() == outs[n].view.data_ptr() and g.stride() == outs[n].view.stride(), f"{n} is not the caller's tensor"
        assert outs[n].intact(), f"sentinels around {n} were overwritten"
        assert _same(g, w), f"{n} differs from the contiguous call with {which} {layout}"
    for g, w in zip(got[len(outputs):], want[len(outputs):]):  # (softmax_lse; out where the entry point takes none to fill)
        assert _same(g, w) if g.dtype == torch.bfloat16 else torch.equal(g, w)
    for n, p in placed.items():
        assert p.holds(t[n]) and p.intact(), f"input {n} was written"


DENSE = dict(q=(B, SQ, H, D), k=(B, SK, HK, D), v=(B, SK, HK, D))
RAGGED = dict(q=(sum(LENS_Q), H, D), k=(sum(LENS_K), HK, D), v=(sum(LENS_K), HK, D))


def _cu(lens):
    return torch.tensor([0, lens[0], lens[0] + lens[1]], dtype=torch.int32, device=DEV)


@pytest.mark.parametrize("which,layout", _cases(["q", "k", "v"], ["o"]))
def test_dense_forward(which, layout):
    from flash_attention_annotated_amd import flash_attn_2_cuda
    t = {n: _rand(*s, seed=i) for i, (n, s) in enumerate(DENSE.items())}
    call = lambda o: flash_attn_2_cuda.fwd(o["q"], o["k"], o["v"], o["o"], None, 0.0, D ** -0.5, True, -1, -1, 0.0, False, None)[:2]  # noqa: E731
    _run(call, t, dict(o=DENSE["q"]), which, layout)


@pytest.mark.parametrize("which,layout", _cases(["q", "k", "v"], ["o"]))
def test_varlen_forward(which, layout):
    from flash_attention_annotated_amd import flash_attn_2_cuda
    t = {n: _rand(*s, seed=i) for i, (n, s) in enumerate(RAGGED.items())}
    call = lambda o: flash_attn_2_cuda.varlen_fwd(o["q"], o["k"], o["v"], o["o"], _cu(LENS_Q), _cu(LENS_K), None, None, None, None,  # noqa: E731
                                                  max(LENS_Q), max(LENS_K), 0.0, D ** -0.5, False, True, -1, -1, 0.0, False, None)[:2]
    _run(call, t, dict(o=RAGGED["q"]), which, layout)


@pytest.mark.parametrize("which,layout", _cases(["q", "k", "v"], ["o"]))
def test_fa3_forward(which, layout):
    from flash_attention_annotated_amd import flash_attn_3_ops  # noqa: F401
    t = {n: _rand(*s, seed=i) for i, (n, s) in enumerate(DENSE.items())}
    call = lambda o: torch.ops.flash_attn_3.fwd(o["q"], o["k"], o["v"], None, None, None, o["o"], None, None, None, None, None, None, None,  # noqa: E731
                                                None, None, None, None, None, None, None, None, None, D ** -0.5, True, -1, -1, 0, 0.0, True,
                                                None, 1, None, 0)[:2]
    _run(call, t, dict(o=DENSE["q"]), which, layout)


def _with_forward(t, fwd):
    out, lse = fwd({n: x.to(DEV) for n, x in t.items()})
    return dict(t, o=out.cpu(), do=_rand(*out.shape, seed=9)), lse


@pytest.mark.parametrize("which,layout", _cases(["do", "q", "k", "v", "o"], ["dq", "dk", "dv"]))
def test_dense_backward(which, layout):
    from flash_attention_annotated_amd import flash_attn_2_cuda
    t = {n: _rand(*s, seed=i) for i, (n, s) in enumerate(DENSE.items())}
    t, lse = _with_forward(t, lambda o: flash_attn_2_cuda.fwd(o["q"], o["k"], o["v"], None, None, 0.0, D ** -0.5, True, -1, -1, 0.0, False,
                                                              None)[:2])
    call = lambda o: flash_attn_2_cuda.bwd(o["do"], o["q"], o["k"], o["v"], o["o"], lse, o["dq"], o["dk"], o["dv"], None, 0.0, D ** -0.5,  # noqa: E731
                                           True, -1, -1, 0.0, False, None, None)[:3]
    _run(call, t, dict(dq=DENSE["q"], dk=DENSE["k"], dv=DENSE["v"]), which, layout)


@pytest.mark.parametrize("which,layout", _cases(["do", "q", "k", "v", "o"], ["dq", "dk", "dv"]))
def test_varlen_backward(which, layout):
    from flash_attention_annotated_amd import flash_attn_2_cuda
    t = {n: _rand(*s, seed=i) for i, (n, s) in enumerate(RAGGED.items())}
    t, lse = _with_forward(t, lambda o: flash_attn_2_cuda.varlen_fwd(o["q"], o["k"], o["v"], None, _cu(LENS_Q), _cu(LENS_K), None, None, None,
                                                                     None, max(LENS_Q), max(LENS_K), 0.0, D ** -0.5, False, True, -1, -1,
                                                                     0.0, False, None)[:2])
    call = lambda o: flash_attn_2_cuda.varlen_bwd(o["do"], o["q"], o["k"], o["v"], o["o"], lse, o["dq"], o["dk"], o["dv"], _cu(LENS_Q),  # noqa: E731
                                                  _cu(LENS_K), None, max(LENS_Q), max(LENS_K), 0.0, D ** -0.5, False, True, -1, -1, 0.0,
                                                  False, None, None)[:3]
    _run(call, t, dict(dq=RAGGED["q"], dk=RAGGED["k"], dv=RAGGED["v"]), which, layout)


NEW, FILL = 3, (40, 100)   # rows appended per entry, fill levels in front of them


def _kvcache(o, kc, vc):
    from flash_attention_annotated_amd import flash_attn_2_cuda
    fill = torch.tensor(FILL, dtype=torch.int32, device=DEV)
    return flash_attn_2_cuda.fwd_kvcache(o["q"], kc, vc, o["k_new"], o["v_new"], fill, None, None, None, None, None, None, o["o"], D ** -0.5,
                                         True, -1, -1, 0.0, True, 1)


@pytest.mark.parametrize("which,layout", _cases(["q", "k_new", "v_new"], ["o"]))
def test_kvcache_step(which, layout):
    """q / k_new / v_new / out are copied; the caches of both runs hold the same rows afterwards."""
    t = dict(q=_rand(B, NEW, H, D, seed=0), k_new=_rand(B, NEW, HK, D, seed=1), v_new=_rand(B, NEW, HK, D, seed=2))
    caches = []

    def call(o):
        kc, vc = _rand(B, SK, HK, D, seed=3).to(DEV), _rand(B, SK, HK, D, seed=4).to(DEV)
        caches.append((kc, vc))
        return _kvcache(o, kc, vc)
    _run(call, t, dict(o=(B, NEW, H, D)), which, layout)
    assert _same(caches[0][0], caches[1][0]) and _same(caches[0][1], caches[1][1])
    for bi, n in enumerate(FILL):
        assert _same(caches[1][0][bi, n:n + NEW].cpu(), t["k_new"][bi]) and _same(caches[1][1][bi, n:n + NEW].cpu(), t["v_new"][bi])


F8 = torch.float8_e4m3fn
DV = 256                     # the latent / V head dim of the MLA shape


def _cache(d=D, hk=HK, sk=SK, seed=3, dtype=torch.bfloat16):
    """An aligned KV cache on the device (never misaligned here: it is never copied)."""
    return _rand(B, sk, hk, d, seed=seed).to(dtype).to(DEV)


def _descales(hk=HK):
    return dict(k_descale=torch.tensor([0.5, 2.0, 1.0, 0.25], device=DEV)[:B * hk].view(B, hk),
                v_descale=torch.tensor([2.0, 0.5, 0.25, 1.0], device=DEV)[:B * hk].view(B, hk))


def _fa3_fwd(o, k, v, **kw):
    from flash_attention_annotated_amd import flash_attn_3_ops  # noqa: F401
    return torch.ops.flash_attn_3.fwd(o["q"], k, v, q_v=o.get("qv"), out=o["o"], softmax_scale=D ** -0.5, is_causal=True, **kw)[:2]


@pytest.mark.parametrize("which,layout", _cases([], ["q", "o"]))
def test_ragged_queries_over_cache(which, layout):
    """fwd_kvcache_ragged: ragged q (3 and 5 rows) over a batched 16-bit cache with its fill levels."""
    lens = (3, 5)
    t = dict(q=_rand(sum(lens), H, D, seed=0))
    k, v, fill = _cache(seed=3), _cache(seed=4), torch.tensor(FILL, dtype=torch.int32, device=DEV)
    call = lambda o: _fa3_fwd(o, k, v, cu_seqlens_q=_cu(lens), seqused_k=fill, max_seqlen_q=max(lens))  # noqa: E731
    _run(call, t, dict(o=(sum(lens), H, D)), which, layout)


@pytest.mark.parametrize("which,layout", _cases([], ["q", "o"]))
def test_fp8_cache_read(which, layout):
    """fwd_kv8 (fa_fwd_kv8): 16-bit q over an e4m3 cache with both descales."""
    t = dict(q=_rand(B, NEW, H, D, seed=0))
    k, v, fill = _cache(seed=3, dtype=F8), _cache(seed=4, dtype=F8), torch.tensor(FILL, dtype=torch.int32, device=DEV)
    call = lambda o: _fa3_fwd(o, k, v, seqused_k=fill, **_descales())  # noqa: E731
    _run(call, t, dict(o=(B, NEW, H, D)), which, layout)


@pytest.mark.parametrize("which,layout", _cases([], ["q", "qv", "o"]))
def test_mla_read(which, layout):
    """fwd_qv8 (fa_fwd_qv8): q (.., 64) and qv (.., 256) over an e4m3 k (.., 64) / v (.., 256) of one kv head."""
    t = dict(q=_rand(B, 1, H, D, seed=0), qv=_rand(B, 1, H, DV, seed=1))
    k, v = _cache(hk=1, seed=3, dtype=F8), _cache(d=DV, hk=1, seed=4, dtype=F8)
    call = lambda o: _fa3_fwd(o, k, v, **_descales(hk=1))  # noqa: E731
    _run(call, t, dict(o=(B, 1, H, DV)), which, layout)


@pytest.mark.parametrize("which,layout", _cases([], ["q"]))
@pytest.mark.parametrize("dtype", [torch.bfloat16, F8], ids=["16bit", "e4m3"])
def test_kvcache_sparse(dtype, which, layout):
    """fwd_kvcache_sparse (fa_fwd_sparse_kv): blocks 0 and 2 of the three 64-key blocks of the cache, one list for every kv head."""
    from flash_attention_annotated_amd import flash_attn_3_ops  # noqa: F401
    t = dict(q=_rand(B, NEW, H, D, seed=0))
    k, v = _cache(sk=192, seed=3, dtype=dtype), _cache(sk=192, seed=4, dtype=dtype)
    cnt, idx = torch.tensor([[2]], dtype=torch.int32, device=DEV), torch.tensor([[[0, 2]]], dtype=torch.int32, device=DEV)
    kw = _descales() if dtype == F8 else {}
    call = lambda o: torch.ops.flash_attn_3.fwd_kvcache_sparse(o["q"], k, v, cnt, idx, 64, softmax_scale=D ** -0.5, is_causal=True, **kw)  # noqa: E731
    _run(call, t, {}, which, layout)


@pytest.mark.parametrize("which,layout", _cases(["k", "v"], ["q"]))
def test_cute_forward_with_sink(which, layout):
    """cute_fwd under the positional list of cute_interface.py: the dense route of fa3_fwd_core with a learnable sink."""
    from flash_attention_annotated_amd import _lib
    t = {n: _rand(*s, seed=i) for i, (n, s) in enumerate(DENSE.items())}
    sink = _rand(H, seed=7).to(DEV)
    call = lambda o: _lib.binding().cute_fwd(o["q"], o["k"], o["v"], None, None, None, None, None, None, None, D ** -0.5, True, -1, -1,  # noqa: E731
                                             sink, 0.0, 1, None)
    _run(call, t, {}, which, layout)


@pytest.mark.parametrize("which,layout", _cases(["k", "v"], ["q", "o"]))
def test_cute_block_sparse_forward(which, layout):
    """cute_fwd_block_sparse under the positional list of cute_interface.py (+ out): one mask list for every batch entry and head
    that names both 128-key blocks of the one 128-row block, so every row has its answer."""
    from flash_attention_annotated_amd import _lib
    t = {n: _rand(*s, seed=i) for i, (n, s) in enumerate(DENSE.items())}
    cnt = torch.tensor([[[2]]], dtype=torch.int32, device=DEV)
    idx = torch.tensor([[[[0, 1]]]], dtype=torch.int32, device=DEV)
    call = lambda o: _lib.binding().cute_fwd_block_sparse(o["q"], o["k"], o["v"], D ** -0.5, True, -1, -1, None, 0.0, 1, None, None,  # noqa: E731
                                                          cnt, idx, o["o"])
    _run(call, t, dict(o=DENSE["q"]), which, layout)


@pytest.mark.parametrize("layout", MIS)
@pytest.mark.parametrize("which", ["k", "v"])
def test_misaligned_cache_is_refused(which, layout):
    """The cache operands are never copied -- an append has to land in the caller's memory: cache_aligned raises."""
    ops = dict(q=_rand(B, NEW, H, D, seed=0).to(DEV), k_new=None, v_new=None, o=None)
    caches = {n: L.place_input(_rand(B, SK, HK, D, seed=3 + i), layout if n == which else "contiguous", DEV) for i, n in enumerate("kv")}
    with pytest.raises(RuntimeError, match="the KV cache must be 16-byte aligned"):
        _kvcache(ops, caches["k"].view, caches["v"].view)
