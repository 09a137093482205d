"""GPU tests of every launch form of csrc/fa_act.hip: each cell of tests/act_plan_universe.py (forward / backward x plain /
gated x dtype width x 16-byte accesses or elements) is run at the widths of its boundaries, the plan of the very tensors is
asserted, and the whole output is held to the oracle with the first and last column of every body, tail and slab checked by
name; then the walks over row blocks and slabs past their grid caps, and the dbias partial rows.

Which case reaches which kernel: vec cells run act_fwd_kernel<8> / act_bwd_kernel<8> (bf16) and <4> (fp32), element cells
<1> in both dtypes; plain backward cells ask for dbias and run act_dbias_reduce_kernel.

Not run here: the element tail of the 16-byte kernels with more than one row.  The binding allocates outputs with a pitch of
H, so with M > 1 a width with a tail takes the element kernel; the tail of act_*_kernel<8 | 4> is reached with M = 1, and its
walk over row blocks and its dbias partial rows only by C-ABI callers with padded pitches."""
import pytest
import torch

import act_plan_universe as U

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPE = {"bf16": torch.bfloat16, "fp32": torch.float32}
RTOL = {"bf16": 2.0 ** -7, "fp32": 2.0 ** -18}


def A():
    from flash_attention_annotated_amd.ops import activations
    return activations


def rows_of(m, h, dtype, vec, gen, halves=1):
    """(m, halves * h) values in a buffer whose pitch is whole 16 bytes and whose base is aligned (vec), or a view one element
    into a buffer of the bare width plus one: every row at another phase"""
    es = torch.empty((), dtype=dtype).element_size()
    cw = 16 // es
    if vec:
        pitch = halves * (-(-h // cw) * cw)
        buf = torch.randn(m, pitch, generator=gen).to(dtype).to(DEV)
        return [buf[:, i * (pitch // halves):i * (pitch // halves) + h] for i in range(halves)]
    buf = torch.randn(m, halves * h + 1, generator=gen).to(dtype).to(DEV)
    return [buf[:, 1 + i * h:1 + (i + 1) * h] for i in range(halves)]


def check(name, ours, ref, dtype, h, cw):
    assert ours.shape == ref.shape
    tol = RTOL[dtype]
    scale = ref.abs().max().item() + 1e-30
    for where, col in U.named_columns(h, cw).items():
        assert torch.allclose(ours[:, col].double(), ref[:, col], rtol=tol, atol=tol * scale), f"{name}: {where} (column {col})"
    assert torch.allclose(ours.double(), ref, rtol=tol, atol=tol * scale), name


@pytest.mark.parametrize("cell", U.CELLS, ids=lambda c: f"{c.direction}-{'gated' if c.gated else 'plain'}-{c.dtype}-{'vec' if c.vec else 'elem'}")
def test_cell(cell):
    a = A()
    dtype = DTYPE[cell.dtype]
    cw = U.cw_of(cell.dtype, cell.vec)
    code = a.SILU if cell.gated else a.GELU_TANH
    gen = torch.Generator().manual_seed(U.CELLS.index(cell))
    for h in U.widths(cw):
        # the outputs are allocated with a pitch of H elements: with more than one row, 16-byte accesses need H % cw == 0, and
        # the element tail of the 16-byte kernels is reached by one-row calls (and by C-ABI callers with padded pitches)
        m = 37 if h % cw == 0 else 1
        packed = cell.gated and m > 1
        want = U.plan(cell.direction, m, h, cell.dtype, cell.vec)
        if cell.gated:
            up, gate = rows_of(m, h, dtype, cell.vec, gen, halves=2)
            bias = None
        else:
            (gate,), up = rows_of(m, h, dtype, cell.vec, gen), None
            bias = torch.randn(-(-h // 4) * 4 + 4, generator=gen).to(DEV)[:h]  # (fp32 at an aligned base)
        x64 = gate.double() if bias is None else gate.double() + bias.double()
        if cell.direction == "fwd":
            got = a._plan_forward(gate, up, bias, code)
            assert U.Plan(**got) == want, (h, got)
            out = a._act_fwd(gate, up, bias, code)
            ref = a._apply(x64, code) * (1 if up is None else up.double())
            check(f"H{h} out", out, ref, cell.dtype, h, cw)
            continue
        (d,) = rows_of(m, h, dtype, cell.vec, gen)
        got = a._plan_backward(d, gate, up, bias, code, not cell.gated, True, packed)
        assert U.Plan(**got) == want, (h, got)
        dpre, dup, dbias, out = a._act_bwd(d, gate, up, bias, code, not cell.gated, True, packed)
        check(f"H{h} recomputed out", out, a._apply(x64, code) * (1 if up is None else up.double()), cell.dtype, h, cw)
        if cell.gated:  # one packed gradient [dup | dgate], or two tensors
            ref = a.gated_act_grad_ref(d.double(), torch.cat([up, gate], dim=-1).double(), code)
            check(f"H{h} dup", dpre[:, :h] if packed else dup, ref[:, :h], cell.dtype, h, cw)
            check(f"H{h} dgate", dpre[:, h:] if packed else dpre, ref[:, h:], cell.dtype, h, cw)
        else:
            ref, rb = a.act_grad_ref(d.double(), gate.double(), code, bias.double())
            check(f"H{h} dpre", dpre, ref, cell.dtype, h, cw)
            check(f"H{h} dbias", dbias[None], rb[None], "fp32", h, cw)  # (37 rows: two partial rows)


def test_packed_gradient_is_an_element_form_unless_its_halves_are_aligned():
    """the packed (M, 2H) gradient the binding allocates has a pitch of 2H elements: 16-byte accesses need H * esize % 16 == 0"""
    a = A()
    gen = torch.Generator().manual_seed(50)
    for h, cw in ((4096, 8), (203, 1), (204, 1), (208, 8)):
        x12 = torch.randn(37, 2 * h, generator=gen).to(torch.bfloat16).to(DEV)
        d = torch.randn(37, h, generator=gen).to(torch.bfloat16).to(DEV)
        assert a._plan_backward(d, x12[:, h:], x12[:, :h], None, a.SILU, False, False, True)["cw"] == cw, h
        assert a._plan_forward(x12[:, h:], x12[:, :h], None, a.SILU)["cw"] == cw, h


@pytest.mark.parametrize("w", U.WALKS, ids=[w.name for w in U.WALKS])
def test_walk(w):
    """a grid cap exceeded: the rows (or slabs) beyond the grid are walked, and in the backward every partial row of dbias
    holds the sums of all the row blocks of its workgroup"""
    a = A()
    dtype = DTYPE[w.dtype]
    items, extent = U.cap_exceeded(w)
    assert items > extent
    gen = torch.Generator(device=DEV).manual_seed(60)
    off = 0 if w.vec else 1
    x = torch.empty(w.m, w.h + off, dtype=dtype, device=DEV).normal_(generator=gen)[:, off:]
    bias = torch.randn(w.h + 4, device=DEV)[:w.h]
    want = U.plan(w.direction, w.m, w.h, w.dtype, w.vec)
    if w.direction == "fwd":
        assert U.Plan(**a._plan_forward(x, None, bias, a.GELU_TANH)) == want
        out = a._act_fwd(x, None, bias, a.GELU_TANH)
        ref = a.act_ref(x.double(), a.GELU_TANH, bias.double())
        assert torch.allclose(out.double(), ref, rtol=RTOL[w.dtype], atol=RTOL[w.dtype])
        return
    d = torch.empty(w.m, w.h + off, dtype=dtype, device=DEV).normal_(generator=gen)[:, off:]
    assert U.Plan(**a._plan_backward(d, x, None, bias, a.GELU_TANH, True, False, False)) == want
    dpre, _, dbias, _ = a._act_bwd(d, x, None, bias, a.GELU_TANH, True, False, False)
    ref, rb = a.act_grad_ref(d.double(), x.double(), a.GELU_TANH, bias.double())
    assert torch.allclose(dpre.double(), ref, rtol=RTOL[w.dtype], atol=RTOL[w.dtype])
    spread = d.double().abs().sum(dim=0)  # (|gelu'| <= 1.13, and near its zero the error of a term is relative to dout, not to the term)
    assert ((dbias.double() - rb).abs() <= 2.0 ** -18 * spread + 1e-30).all()
