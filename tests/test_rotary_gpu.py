"""GPU tests of the rotary embedding layer (flash_attention_annotated_amd.layers.rotary over csrc/fa_rotary_emb.hip).

Expectation: apply_rotary_emb_torch on fp32 copies of the inputs, rows whose position is outside the tables passed through
(cos = 1, sin = 0).  The kernel does this arithmetic in fp32 and rounds once, so what remains is the order of one multiply-add:
  * 16-bit types: EVERY element within 1 ulp of the storage type at the expected value (the count of elements that are not
    bit-equal to the rounded expectation is printed);
  * fp32: |err| <= 2^-22 (|x0 c| + |x1 s|);
  * untouched columns and rows bit-equal to what they held;
  * gradients: the conjugate launch, the same bounds against autograd through the fp32 expectation.
"""
import pytest
import torch

from flash_attention_annotated_amd.layers import rotary
from flash_attention_annotated_amd.layers.rotary import (RotaryEmbedding, apply_rotary_emb, apply_rotary_emb_kv_,
                                                         apply_rotary_emb_qkv_, apply_rotary_emb_torch)

pytestmark = pytest.mark.gpu
DEV = "cuda"
MANT = {torch.bfloat16: 7, torch.float16: 10}
EMIN = {torch.bfloat16: -126, torch.float16: -14}


def make_tables(seqlen_ro, rd, dtype, seed=0):
    g = torch.Generator(device="cpu").manual_seed(1000 + seed)
    ang = torch.rand(seqlen_ro, rd // 2, generator=g) * 6.2831853
    return torch.cos(ang).to(dtype).to(DEV), torch.sin(ang).to(dtype).to(DEV)


def randn(*shape, dtype, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(*shape, generator=g).to(dtype).to(DEV)


def row_tables(cos, sin, offsets, b, s):
    """fp32 (b, s, rotary_dim / 2) tables of positions offsets[b] + i; outside [0, seqlen_ro): cos = 1, sin = 0."""
    off = offsets.long() if isinstance(offsets, torch.Tensor) else torch.full((b,), offsets, dtype=torch.long, device=cos.device)
    pos = off[:, None] + torch.arange(s, device=cos.device)[None]
    valid = ((pos >= 0) & (pos < cos.shape[0]))[..., None]
    idx = pos.clamp(0, cos.shape[0] - 1)
    one, zero = torch.ones((), device=cos.device), torch.zeros((), device=cos.device)
    return torch.where(valid, cos.float()[idx], one), torch.where(valid, sin.float()[idx], zero)


def expected(x, cos, sin, offsets=0, interleaved=False, conjugate=False):
    """fp32 expectation of a dense (b, s, h, d) call."""
    c, s = row_tables(cos, sin, offsets, x.shape[0], x.shape[1])
    return apply_rotary_emb_torch(x.float(), c, -s if conjugate else s, interleaved)


def _wide(t, interleaved):
    t = t.repeat_interleave(2, dim=-1) if interleaved else torch.cat((t, t), dim=-1)
    return t.unsqueeze(-2)


def _magnitude(xf, c, s, interleaved):
    rd = 2 * c.shape[-1]
    head = xf[..., :rd]
    m = head.abs() * _wide(c, interleaved).abs() + rotary.rotate_half(head, interleaved).abs() * _wide(s, interleaved).abs()
    return torch.cat((m, xf[..., rd:].abs()), dim=-1)


def check(got, want, what, mag=None):
    """got: the kernel's tensor; want: the fp32 expectation of the same shape."""
    assert got.shape == want.shape, what
    if got.dtype == torch.float32:
        err = (got - want).abs()
        bound = 2.0 ** -22 * mag
        print(f"{what}: fp32 max err {err.max().item():.3e}, largest err / bound {(err / bound.clamp_min(1e-30)).max().item():.3f}")
        assert bool((err <= bound).all()), what
        return
    exp = torch.frexp(want.abs())[1] - 1  # floor(log2 |want|)
    ulp = torch.exp2((exp.clamp_min(EMIN[got.dtype]) - MANT[got.dtype]).float())
    err = (got.float() - want).abs()
    differ = int((got != want.to(got.dtype)).sum())
    print(f"{what}: {differ} of {got.numel()} elements not bit-equal to the rounded expectation, max err {(err / ulp).max().item():.3f} ulp")
    assert bool((err <= ulp).all()), what


def run_dense(dtype, b, s, h, d, rd, interleaved, inplace, offsets=0, seqlen_ro=None, seed=0):
    """Forward and gradient of one dense apply_rotary_emb call against the expectation."""
    x = randn(b, s, h, d, dtype=dtype, seed=seed)
    cos, sin = make_tables(seqlen_ro or s + 8, rd, dtype, seed)
    want = expected(x, cos, sin, offsets, interleaved)
    mag = _magnitude(x.float(), *row_tables(cos, sin, offsets, b, s), interleaved) if dtype == torch.float32 else None
    xin = x.clone().requires_grad_(True)
    arg = xin * 1 if inplace else xin  # (in place on a leaf that requires grad is autograd's own refusal)
    held = arg.detach().clone()
    out = apply_rotary_emb(arg, cos, sin, interleaved=interleaved, inplace=inplace, seqlen_offsets=offsets)
    tag = f"d{d} rd{rd} il{int(interleaved)} inplace{int(inplace)} {str(dtype)[6:]}"
    check(out.detach(), want, f"fwd {tag}", mag)
    assert torch.equal(out.detach()[..., rd:], x[..., rd:])  # columns past rotary_dim: copied / left alone
    if inplace:
        assert out.data_ptr() == arg.data_ptr()
    else:
        assert torch.equal(arg.detach(), held)
    g = randn(b, s, h, d, dtype=dtype, seed=seed + 77)
    gheld = g.clone()
    (dx,) = torch.autograd.grad(out, xin, g)
    xf = x.float().requires_grad_(True)
    (dx_want,) = torch.autograd.grad(expected(xf, cos, sin, offsets, interleaved), xf, gheld.float())
    gmag = _magnitude(gheld.float(), *row_tables(cos, sin, offsets, b, s), interleaved) if dtype == torch.float32 else None
    check(dx, dx_want, f"bwd {tag}", gmag)
    return out


DENSE = [(64, 64), (128, 128), (128, 64), (128, 48), (128, 16), (256, 256), (96, 48), (40, 20), (72, 72)]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("inplace", [False, True], ids=["new", "inplace"])
@pytest.mark.parametrize("interleaved", [False, True], ids=["half", "il"])
@pytest.mark.parametrize("d,rd", DENSE)
def test_dense(d, rd, interleaved, inplace, dtype):
    run_dense(dtype, 2, 37, 3, d, rd, interleaved, inplace)


@pytest.mark.parametrize("inplace", [False, True], ids=["new", "inplace"])
@pytest.mark.parametrize("interleaved", [False, True], ids=["half", "il"])
@pytest.mark.parametrize("rd", [64, 32, 6])
def test_dense_fp32(rd, interleaved, inplace):
    run_dense(torch.float32, 2, 37, 3, 64, rd, interleaved, inplace)


@pytest.mark.parametrize("interleaved", [False, True], ids=["half", "il"])
@pytest.mark.parametrize("h,d,rd", [(1, 64, 64), (33, 64, 64), (1, 128, 64), (33, 128, 64), (33, 96, 48), (33, 40, 20)])
def test_head_walk(h, d, rd, interleaved):
    """One head: most lanes idle.  33 heads: the lanes wrap around the row (and, at d96, change their slot as they do)."""
    for inplace in (False, True):
        run_dense(torch.bfloat16, 2, 19, h, d, rd, interleaved, inplace)


def test_fp32_tables_for_16_bit_x():
    x = randn(2, 21, 3, 64, dtype=torch.bfloat16)
    cos, sin = make_tables(32, 32, torch.float32)
    for il in (False, True):
        out = apply_rotary_emb(x, cos, sin, interleaved=il)
        check(out, expected(x, cos, sin, 0, il), f"fp32 tables il{int(il)}")


OFFSETS = {
    "zero": lambda: 0,
    "int5": lambda: 5,
    "int32": lambda: torch.tensor([3, 11], dtype=torch.int32, device=DEV),
    "int64": lambda: torch.tensor([9, 0], dtype=torch.int64, device=DEV),
    "past_the_tables": lambda: torch.tensor([30, 2], dtype=torch.int32, device=DEV),  # rows 15.. of sequence 0 at >= 45
    "negative": lambda: torch.tensor([4, -7], dtype=torch.int64, device=DEV),         # rows 0..6 of sequence 1 below 0
    "all_outside": lambda: torch.tensor([1 << 40, -(1 << 40)], dtype=torch.int64, device=DEV),
}


@pytest.mark.parametrize("inplace", [False, True], ids=["new", "inplace"])
@pytest.mark.parametrize("d,rd", [(128, 64), (40, 20)], ids=["vector", "element"])
@pytest.mark.parametrize("kind", sorted(OFFSETS))
def test_offsets(kind, d, rd, inplace):
    """Rows whose position lies outside the tables come back unchanged, the others rotated.  The tables are ordinary
    allocations of exactly seqlen_ro rows: nothing is read past them."""
    b, s, h, seqlen_ro = 2, 37, 3, 45
    offsets = OFFSETS[kind]()
    for il in (False, True):
        out = run_dense(torch.bfloat16, b, s, h, d, rd, il, inplace, offsets=offsets, seqlen_ro=seqlen_ro, seed=3).detach()
        x = randn(b, s, h, d, dtype=torch.bfloat16, seed=3)
        if isinstance(offsets, torch.Tensor):
            pos = offsets.long()[:, None] + torch.arange(s, device=DEV)[None]
            outside = (pos < 0) | (pos >= seqlen_ro)
            assert torch.equal(out[outside], x[outside])
            if kind in ("past_the_tables", "negative"):
                assert bool(outside.any()) and not bool(outside.all())
                assert not torch.equal(out[~outside], x[~outside])


def test_int_offset_past_the_tables_is_refused():
    x = randn(1, 8, 2, 64, dtype=torch.bfloat16)
    cos, sin = make_tables(10, 64, torch.bfloat16)
    with pytest.raises(RuntimeError, match="seqlen_ro"):
        apply_rotary_emb(x, cos, sin, seqlen_offsets=3)
    with pytest.raises(RuntimeError, match="seqlen_ro must be >= seqlen"):
        apply_rotary_emb(x, cos[:7], sin[:7])


@pytest.mark.parametrize("interleaved", [False, True], ids=["half", "il"])
def test_strides(interleaved):
    b, s, h, d, rd = 2, 37, 3, 64, 32
    cos, sin = make_tables(s, rd, torch.bfloat16)
    # x a slice of a packed tensor, out a tensor of its own (vector path, strided rows)
    qkv = randn(b, s, 3, h, d, dtype=torch.bfloat16, seed=5)
    held = qkv.clone()
    out = apply_rotary_emb(qkv[:, :, 0], cos, sin, interleaved=interleaved)
    check(out, expected(held[:, :, 0], cos, sin, 0, interleaved), "x = qkv[:, :, 0]")
    assert out.is_contiguous() and torch.equal(qkv, held)
    # ... and in place: k and v bit-unchanged
    apply_rotary_emb(qkv[:, :, 0], cos, sin, interleaved=interleaved, inplace=True)
    check(qkv[:, :, 0], expected(held[:, :, 0], cos, sin, 0, interleaved), "x = qkv[:, :, 0] in place")
    assert torch.equal(qkv[:, :, 1:], held[:, :, 1:])
    # last stride 2 (element path)
    wide = randn(b, s, h, 2 * d, dtype=torch.bfloat16, seed=6)
    held = wide.clone()
    view = wide[..., ::2]
    out = apply_rotary_emb(view, cos, sin, interleaved=interleaved)
    check(out, expected(held[..., ::2], cos, sin, 0, interleaved), "x = [..., ::2]")
    apply_rotary_emb(view, cos, sin, interleaved=interleaved, inplace=True)
    check(wide[..., ::2], expected(held[..., ::2], cos, sin, 0, interleaved), "x = [..., ::2] in place")
    assert torch.equal(wide[..., 1::2], held[..., 1::2])
    # a 16-bit row base that is 8-byte but not 16-byte aligned (element path)
    flat = randn(b * s * h * d + 4, dtype=torch.bfloat16, seed=7)
    held = flat.clone()
    off4 = flat[4:].view(b, s, h, d)
    assert off4.data_ptr() % 16 == 8
    out = apply_rotary_emb(off4, cos, sin, interleaved=interleaved)
    check(out, expected(held[4:].view(b, s, h, d), cos, sin, 0, interleaved), "base % 16 == 8")
    apply_rotary_emb(off4, cos, sin, interleaved=interleaved, inplace=True)
    check(off4, expected(held[4:].view(b, s, h, d), cos, sin, 0, interleaved), "base % 16 == 8 in place")
    assert torch.equal(flat[:4], held[:4])


@pytest.mark.parametrize("inplace", [False, True], ids=["new", "inplace"])
@pytest.mark.parametrize("d,rd", [(128, 64), (40, 20)], ids=["vector", "element"])
@pytest.mark.parametrize("interleaved", [False, True], ids=["half", "il"])
def test_varlen(interleaved, d, rd, inplace):
    lens, h, pad = [0, 1, 17, 33], 3, 5
    total = sum(lens)
    cu = torch.tensor([0, 0, 1, 18, 51], dtype=torch.int32, device=DEV)
    offsets = torch.tensor([7, 40, 0, 12], dtype=torch.int32, device=DEV)  # 12 + 33 = 45: the last row sits at the last position
    x = randn(total + pad, h, d, dtype=torch.bfloat16, seed=11)  # `pad` rows past cu_seqlens[-1]
    cos, sin = make_tables(45, rd, torch.bfloat16)
    xin = x.clone().requires_grad_(True)
    arg = xin * 1 if inplace else xin
    out = apply_rotary_emb(arg, cos, sin, interleaved=interleaved, inplace=inplace, seqlen_offsets=offsets, cu_seqlens=cu, max_seqlen=33)
    g = randn(total + pad, h, d, dtype=torch.bfloat16, seed=12)
    gheld = g.clone()
    (dx,) = torch.autograd.grad(out, xin, g)
    start = 0
    for i, n in enumerate(lens):
        if n:
            rows = slice(start, start + n)
            check(out.detach()[rows][None], expected(x[rows][None], cos, sin, offsets[i:i + 1], interleaved), f"varlen seq {i}")
            check(dx[rows][None], expected(gheld[rows][None], cos, sin, offsets[i:i + 1], interleaved, conjugate=True), f"varlen seq {i} bwd")
        start += n
    if inplace:  # rows past cu_seqlens[-1]: not touched (out of place they are whatever the new tensor held)
        assert torch.equal(out.detach()[total:], x[total:])
        assert torch.equal(dx[total:], gheld[total:])


def _packed_expectation(qkv, cos, sin, cos_k, sin_k, il, hq, offsets, conjugate=False):
    ck, sk = (cos, sin) if cos_k is None else (cos_k, sin_k)
    if qkv.dim() == 5:
        q, k, v = qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2]
    else:
        hk = (qkv.shape[2] - hq) // 2
        q, k, v = qkv[:, :, :hq], qkv[:, :, hq:hq + hk], qkv[:, :, hq + hk:]
    q, k = expected(q, cos, sin, offsets, il, conjugate), expected(k, ck, sk, offsets, il, conjugate)
    return torch.stack([q, k, v.float()], dim=2) if qkv.dim() == 5 else torch.cat([q, k, v.float()], dim=2)


@pytest.mark.parametrize("own_k_tables", [False, True], ids=["one_launch", "cos_k"])
@pytest.mark.parametrize("gqa", [False, True], ids=["3hd", "gqa"])
@pytest.mark.parametrize("interleaved", [False, True], ids=["half", "il"])
def test_qkv(interleaved, gqa, own_k_tables):
    b, s, d = 2, 19, 64
    shape, hq = ((b, s, 6 + 2 * 2, d), 6) if gqa else ((b, s, 3, 4, d), None)
    qkv = randn(*shape, dtype=torch.bfloat16, seed=21)
    cos, sin = make_tables(s + 4, d, torch.bfloat16, 1)
    cos_k, sin_k = make_tables(s + 4, d, torch.bfloat16, 2) if own_k_tables else (None, None)
    offsets = torch.tensor([0, 4], dtype=torch.int32, device=DEV)
    leaf = qkv.clone().requires_grad_(True)
    arg = leaf * 1
    out = apply_rotary_emb_qkv_(arg, cos, sin, cos_k, sin_k, interleaved=interleaved, seqlen_offsets=offsets, num_heads_q=hq)
    assert out.data_ptr() == arg.data_ptr()
    check(out.detach(), _packed_expectation(qkv, cos, sin, cos_k, sin_k, interleaved, hq, offsets), "qkv fwd")
    v = (lambda t: t[:, :, 2]) if not gqa else (lambda t: t[:, :, 8:])
    assert torch.equal(v(out.detach()), v(qkv))  # V bit-unchanged
    g = randn(*shape, dtype=torch.bfloat16, seed=22)
    gheld = g.clone()
    (dqkv,) = torch.autograd.grad(out, leaf, g)
    check(dqkv, _packed_expectation(gheld, cos, sin, cos_k, sin_k, interleaved, hq, offsets, conjugate=True), "qkv bwd")
    assert torch.equal(v(dqkv), v(gheld))


def test_qkv_one_launch_without_k_tables(monkeypatch):
    calls = []
    real = rotary.apply_rotary
    monkeypatch.setattr(rotary, "apply_rotary", lambda x, *a, **kw: calls.append(tuple(x.shape)) or real(x, *a, **kw))
    cos, sin = make_tables(19, 64, torch.bfloat16)
    apply_rotary_emb_qkv_(randn(2, 19, 3, 4, 64, dtype=torch.bfloat16), cos, sin)
    apply_rotary_emb_qkv_(randn(2, 19, 10, 64, dtype=torch.bfloat16), cos, sin, num_heads_q=6)
    assert calls == [(2, 19, 8, 64), (2, 19, 8, 64)]
    del calls[:]
    apply_rotary_emb_qkv_(randn(2, 19, 3, 4, 64, dtype=torch.bfloat16), cos, sin, cos, sin)
    assert calls == [(2, 19, 4, 64), (2, 19, 4, 64)]


@pytest.mark.parametrize("interleaved", [False, True], ids=["half", "il"])
def test_kv(interleaved):
    b, s, h, d = 2, 19, 2, 64
    kv = randn(b, s, 2, h, d, dtype=torch.float16, seed=31)
    cos, sin = make_tables(s + 3, 32, torch.float16)
    leaf = kv.clone().requires_grad_(True)
    out = apply_rotary_emb_kv_(leaf * 1, cos, sin, interleaved=interleaved, seqlen_offsets=3)
    check(out.detach()[:, :, 0], expected(kv[:, :, 0], cos, sin, 3, interleaved), "kv fwd")
    assert torch.equal(out.detach()[:, :, 1], kv[:, :, 1])
    g = randn(b, s, 2, h, d, dtype=torch.float16, seed=32)
    gheld = g.clone()
    (dkv,) = torch.autograd.grad(out, leaf, g)
    check(dkv[:, :, 0], expected(gheld[:, :, 0], cos, sin, 3, interleaved, conjugate=True), "kv bwd")
    assert torch.equal(dkv[:, :, 1], gheld[:, :, 1])


@pytest.mark.parametrize("scale_base", [None, 512])
@pytest.mark.parametrize("interleaved", [False, True], ids=["half", "il"])
def test_rotary_embedding_module(interleaved, scale_base):
    b, s, h, d, rd = 2, 19, 4, 64, 32
    m = RotaryEmbedding(rd, interleaved=interleaved, scale_base=scale_base, device=DEV)
    qkv = randn(b, s, 3, h, d, dtype=torch.bfloat16, seed=41)
    out = m(qkv.clone(), seqlen_offset=2)
    assert m._cos_cached.shape == (s + 2, rd // 2) and m._cos_cached.dtype == torch.bfloat16
    ck, sk = (m._cos_k_cached, m._sin_k_cached) if scale_base else (None, None)
    assert (ck is not None) == (scale_base is not None)
    check(out, _packed_expectation(qkv, m._cos_cached, m._sin_cached, ck, sk, interleaved, None, 2), "module qkv")
    # q + kv, a tensor offset with max_seqlen
    q, kv = randn(b, s, h, d, dtype=torch.bfloat16, seed=42), randn(b, s, 2, h, d, dtype=torch.bfloat16, seed=43)
    offsets = torch.tensor([5, 0], dtype=torch.int32, device=DEV)
    q_out, kv_out = m(q.clone(), kv.clone(), seqlen_offset=offsets, max_seqlen=s + 9)
    assert m._cos_cached.shape[0] == s + 9
    ck, sk = (m._cos_k_cached, m._sin_k_cached) if scale_base else (m._cos_cached, m._sin_cached)
    check(q_out, expected(q, m._cos_cached, m._sin_cached, offsets, interleaved), "module q")
    check(kv_out[:, :, 0], expected(kv[:, :, 0], ck, sk, offsets, interleaved), "module k")
    assert torch.equal(kv_out[:, :, 1], kv[:, :, 1])
    # the GQA form
    g = randn(b, s, 6 + 2 * 2, d, dtype=torch.bfloat16, seed=44)
    out = m(g.clone(), num_heads_q=6)
    ck, sk = (m._cos_k_cached, m._sin_k_cached) if scale_base else (None, None)
    check(out, _packed_expectation(g, m._cos_cached, m._sin_cached, ck, sk, interleaved, 6, 0), "module gqa")


@pytest.mark.parametrize("rotary_fraction", [1.0, 0.5])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_reference_rule(dtype, rotary_fraction):
    """The reference's own inequality at its own shape (tests/test_rotary.py:60-96): against the torch path,
    rtol = 1e-3, atol = 2 max|(ref + 0.3 - 0.3) - ref|, outputs and gradients."""
    b, s, h, d = 32, 217, 4, 128
    rd = int(rotary_fraction * d)
    torch.manual_seed(42)
    x = torch.randn(b, s, h, d, dtype=dtype, device=DEV, requires_grad=True)
    x_pt = x.detach().clone().requires_grad_()
    ang = torch.rand(s, rd // 2, device=DEV) * 2 * torch.pi
    cos, sin = torch.cos(ang).to(dtype), torch.sin(ang).to(dtype)
    out = apply_rotary_emb(x, cos, sin)
    out_pt = apply_rotary_emb_torch(x_pt.float(), cos.float(), sin.float()).to(dtype)
    g = torch.randn_like(out)
    out.backward(g)
    out_pt.backward(g.clone())
    assert torch.equal(x, x_pt)
    atol = ((out_pt + 0.3 - 0.3) - out_pt).abs().max().item()
    assert torch.allclose(out, out_pt, rtol=1e-3, atol=2 * atol)
    atol = ((x_pt.grad + 0.3 - 0.3) - x_pt.grad).abs().max().item()
    assert torch.allclose(x.grad, x_pt.grad, rtol=1e-3, atol=2 * atol)


@pytest.mark.parametrize("interleaved", [False, True], ids=["half", "il"])
def test_agrees_with_the_cache_append(interleaved):
    """The keys flash_attn_with_kvcache(k=, rotary_cos=, ...) writes into a 16-bit cache against apply_rotary_emb on the same k:
    1 ulp, and -- the two share fa::rotary_slot_to -- expected bit-equal (printed)."""
    from flash_attention_annotated_amd import hopper_interface
    b, s_new, cap, h, hk, d, rd = 2, 3, 128, 4, 2, 128, 64
    q = randn(b, s_new, h, d, dtype=torch.bfloat16, seed=51)
    k, v = randn(b, s_new, hk, d, dtype=torch.bfloat16, seed=52), randn(b, s_new, hk, d, dtype=torch.bfloat16, seed=53)
    kc, vc = torch.zeros(b, cap, hk, d, dtype=torch.bfloat16, device=DEV), torch.zeros(b, cap, hk, d, dtype=torch.bfloat16, device=DEV)
    lens = torch.tensor([17, 100], dtype=torch.int32, device=DEV)
    cos, sin = make_tables(cap, rd, torch.bfloat16)
    hopper_interface.flash_attn_with_kvcache(q, kc, vc, k=k, v=v, rotary_cos=cos, rotary_sin=sin, cache_seqlens=lens,
                                             rotary_interleaved=interleaved, causal=True)
    ours = apply_rotary_emb(k, cos, sin, interleaved=interleaved, seqlen_offsets=lens)
    written = torch.stack([kc[i, int(n):int(n) + s_new] for i, n in enumerate(lens.tolist())])
    print(f"cache append vs layer, interleaved={interleaved}: bit-equal = {torch.equal(written, ours)}")
    check(written, ours.float(), "cache append vs layer")
    check(ours, expected(k, cos, sin, lens, interleaved), "layer vs expectation")


def test_tensor_of_2_31_elements():
    """bf16 (1, 65552, 128, 256) = 2^31 + 2^19 elements, in place: 64-bit row bases.  The first and the last 16 rows."""
    s, h, d = 65552, 128, 256
    x = torch.empty(1, s, h, d, dtype=torch.bfloat16, device=DEV)
    assert x.numel() > 1 << 31
    first, last = randn(1, 16, h, d, dtype=torch.bfloat16, seed=61), randn(1, 16, h, d, dtype=torch.bfloat16, seed=62)
    x[:, :16], x[:, -16:] = first, last
    cos, sin = make_tables(s, d, torch.bfloat16)
    apply_rotary_emb(x, cos, sin, inplace=True)
    check(x[:, :16], expected(first, cos, sin, 0), "2^31: first rows")
    check(x[:, -16:], expected(last, cos, sin, s - 16), "2^31: last rows")


def test_hip_graph_replay_sees_new_offsets():
    b, s, h, d = 2, 19, 3, 128
    x = randn(b, s, h, d, dtype=torch.bfloat16, seed=71)
    cos, sin = make_tables(64, 64, torch.bfloat16)
    offsets = torch.tensor([0, 7], dtype=torch.int32, device=DEV)
    out = torch.empty_like(x)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        out.copy_(apply_rotary_emb(x, cos, sin, seqlen_offsets=offsets))  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out.copy_(apply_rotary_emb(x, cos, sin, seqlen_offsets=offsets))
    graph.replay()
    check(out, expected(x, cos, sin, offsets), "graph replay")
    new = torch.tensor([30, 44], dtype=torch.int32, device=DEV)
    offsets.copy_(new)
    graph.replay()
    torch.cuda.synchronize()
    check(out, expected(x, cos, sin, new), "graph replay after new offsets")
    assert not torch.equal(out, apply_rotary_emb(x, cos, sin, seqlen_offsets=torch.tensor([0, 7], dtype=torch.int32, device=DEV)))


def test_compile_fullgraph():
    b, s, h, d = 2, 19, 4, 64
    cos, sin = make_tables(s + 4, 32, torch.bfloat16)
    offsets = torch.tensor([0, 4], dtype=torch.int32, device=DEV)

    def f(x):
        return apply_rotary_emb(x, cos, sin, interleaved=True, seqlen_offsets=offsets)

    def f_qkv(qkv):
        return apply_rotary_emb_qkv_(qkv * 1, cos, sin, seqlen_offsets=2)

    for fn, shape, want in ((f, (b, s, h, d), lambda t, conj: expected(t, cos, sin, offsets, True, conj)),
                            (f_qkv, (b, s, 3, h, d), lambda t, conj: _packed_expectation(t, cos, sin, None, None, False, None, 2, conj))):
        x = randn(*shape, dtype=torch.bfloat16, seed=81)
        g = randn(*shape, dtype=torch.bfloat16, seed=82)
        leaf = x.clone().requires_grad_(True)
        out = torch.compile(fn, backend="aot_eager", fullgraph=True)(leaf)
        (dx,) = torch.autograd.grad(out, leaf, g.clone())
        check(out.detach(), want(x, False), f"compiled {fn.__name__}")
        check(dx, want(g, True), f"compiled {fn.__name__} bwd")
