"""CPU self-test of tests/layouts.py: every layout, for 1- and 2-byte elements, on the three operand ranks (dense, ragged, page
pool) -- values round-trip, the view is non-contiguous with last stride 1, the alignment answer is the binding's rule, the
elements of a view do not overlap, the view lies in the interior with the promised slack and NaN / sentinel around it; and the
mixed assignments give no two same-shaped operands of a universe case one stride triple."""
import math

import pytest
import torch

import bwd_plan_universe
import kv8_plan_universe
import layouts as L
import plan_universe

DTYPES = {1: torch.float8_e4m3fn, 2: torch.bfloat16}
SHAPES = {"dense": (2, 5, 3, 16), "ragged": (7, 3, 16), "pool": (3, 4, 2, 32)}
NONCONTIGUOUS = L.ALIGNED_LAYOUTS + L.MISALIGNED_LAYOUTS


def _values(shape, dtype):
    n = math.prod(shape)
    return (torch.arange(n, dtype=torch.float32) % 200 - 100).view(shape).to(dtype)


@pytest.mark.parametrize("itemsize", (1, 2))
@pytest.mark.parametrize("rank", SHAPES)
@pytest.mark.parametrize("layout", NONCONTIGUOUS)
def test_layout(layout, rank, itemsize):
    shape, dtype = SHAPES[rank], DTYPES[itemsize]
    x = _values(shape, dtype)
    slack = L.call_slack([shape], itemsize)
    p = L.place_input(x, layout, slack=slack)
    n = x.numel()
    # values round-trip, bit for bit
    assert p.view.shape == x.shape and p.holds(x) and torch.equal(p.view.contiguous().view(torch.uint8), x.view(torch.uint8))
    # non-contiguous (or, for the moved base, off its boundary) with last stride 1
    assert p.view.stride(-1) == 1
    assert not p.view.is_contiguous() or layout == "misaligned_base"
    # the binding's alignment rule accepts the aligned layouts and refuses the others; an fp8 cache asks 16 bytes of both
    assert L.aligned(p.view) == (layout in L.ALIGNED_LAYOUTS)
    if len(shape) == 4:  # (a cache is 4-D)
        assert L.cache_aligned(p.view, 16, 16 if itemsize == 1 else 8) == (layout in L.ALIGNED_LAYOUTS)
    if layout in L.ALIGNED_LAYOUTS:
        assert all(s * itemsize % 16 == 0 for s in p.view.stride()[:-1]) and p.view.data_ptr() % 16 == 0
    # the elements of the view do not overlap and stay inside the allocation, slack in front and behind
    at = torch.arange(p.buf.numel()).as_strided(p.shape, p.strides, p.offset).flatten()
    assert at.unique().numel() == n
    assert int(at.min()) >= n and p.buf.numel() - 1 - int(at.max()) >= max(n, slack)
    # NaN everywhere else; intact() notices one changed element in front of, inside (a gap) and behind the view
    outside = torch.ones(p.buf.numel(), dtype=torch.bool)
    outside[at] = False
    assert (p.bits[outside] == L.NAN_BITS[itemsize]).all() and p.intact()
    assert torch.tensor([L.NAN_BITS[itemsize]], dtype=L.INT[itemsize]).view(dtype).float().isnan().all()
    gaps = outside.clone()
    gaps[:int(at.min())] = False
    gaps[int(at.max()):] = False
    spots = [0, p.buf.numel() - 1] + ([int(gaps.nonzero()[0])] if gaps.any() else [])
    assert gaps.any() or layout in ("bhsd", "misaligned_base")  # (a permutation has no gaps)
    for spot in spots:
        keep = p.bits[spot].clone()
        p.bits[spot] = 1
        assert not p.intact()
        p.bits[spot] = keep
    assert p.intact()


@pytest.mark.parametrize("itemsize", (1, 2))
def test_output_placement(itemsize):
    """An output allocation holds the byte 0xA5 throughout; a store into the view leaves it intact, one outside does not."""
    p = L.place_output(SHAPES["dense"], DTYPES[itemsize], "bhsd_padded")
    assert (p.buf.view(torch.uint8) == 0xA5).all() and p.intact()
    p.view.copy_(_values(SHAPES["dense"], DTYPES[itemsize]))
    assert p.intact() and p.holds(_values(SHAPES["dense"], DTYPES[itemsize]))
    p.bits[p.offset - 1] = 0
    assert not p.intact()


def test_contiguous_layout_is_the_plain_tensor():
    x = _values(SHAPES["dense"], torch.bfloat16)
    p = L.place_input(x, "contiguous")
    assert p.view.is_contiguous() and p.buf.numel() == x.numel() and p.holds(x) and p.intact()


def test_call_slack_bounds_every_stride_mix():
    """The docstring's argument on numbers: the largest offset any mix of the layouts' strides gives an index of the call."""
    shapes = [(2, 300, 4, 64), (2, 715, 2, 64), (2, 715, 2, 256)]
    slack = L.call_slack(shapes)
    worst = [0, 0, 0]
    for shape in shapes:
        for layout in L.ALIGNED_LAYOUTS + ("contiguous",):
            worst = [max(w, s) for w, s in zip(worst, L.geometry(shape, 2, layout)[2][:3])]
    B, S, H, D = 2, 715, 4, 256
    assert (B - 1) * worst[0] + (S - 1) * worst[1] + (H - 1) * worst[2] + D - 1 < slack


def _universe_shapes():
    """{operand: shape} per universe case (one element type is enough: the strides do not depend on a 16-bit type)."""
    out = []
    for _, _, _, c in plan_universe.cases():
        dv = c.get("dv", c["d"])
        out.append(dict(q=(c["b"], c["sq"], c["h"], c["d"]), k=(c["b"], c["sk"], c["hk"], c["d"]), v=(c["b"], c["sk"], c["hk"], dv),
                        o=(c["b"], c["sq"], c["h"], dv), qv=(c["b"], c["sq"], c["h"], dv)))
    for _, _, _, c in kv8_plan_universe.cases():
        dv = c.get("dv", c["d"])
        out.append(dict(q=(c["b"], c["sq"], c["h"], c["d"]), k=(c["b"], c["cap"], c["hk"], c["d"]), v=(c["b"], c["cap"], c["hk"], dv),
                        o=(c["b"], c["sq"], c["h"], dv), qv=(c["b"], c["sq"], c["h"], dv)))
    for _, c in bwd_plan_universe.CASES.values():
        dv = c.get("dv", c["d"])
        lq, lk = ((sum(c["lens_q"]),), (sum(c["lens_k"]),)) if "lens_q" in c else ((c["b"], c["sq"]), (c["b"], c["sk"]))
        q, k, v, o = (*lq, c["h"], c["d"]), (*lk, c["hk"], c["d"]), (*lk, c["hk"], dv), (*lq, c["h"], dv)
        out.append(dict(q=q, k=k, v=v, o=o, do=o, dq=q, dk=k, dv=v))
    return out


def test_mixed_assignments():
    assert len(L.ASSIGNMENTS) >= 2
    for a in L.ASSIGNMENTS:
        assert all(name in L.ALIGNED_LAYOUTS for name in a.values())
        assert a["k_pages"].startswith("padded") and a["v_pages"].startswith("padded")
        for group in L.SAME_SHAPE_GROUPS:
            assert len({a[n] for n in group}) == len(group), f"{group}: a layout twice"
    for name in L.ASSIGNMENTS[0]:
        if not name.endswith("_pages"):  # every operand gets a padded and a bhsd layout
            assert {a[name][:4] for a in L.ASSIGNMENTS} == {"padd", "bhsd"}, name
    # on the universes' own shapes: no two operands of a call share a stride triple, none has the contiguous one
    for shapes in _universe_shapes():
        for a in L.ASSIGNMENTS:
            for itemsize in (1, 2):
                triples = {n: L.geometry(s, itemsize, a[n])[2] for n, s in shapes.items()}
                for group in (("q", "k", "v", "o", "qv"), ("q", "k", "v", "o", "do", "dq", "dk", "dv")):
                    got = [triples[n][:-1] for n in group if n in triples]
                    if len(got) == len(group):
                        assert len(set(got)) == len(got), (shapes, triples)
                for n, s in shapes.items():
                    assert triples[n] != L.geometry(s, itemsize, "contiguous")[2]
