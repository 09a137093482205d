"""CPU tests of tests/dropout_norm_oracle.py, the oracle tests/test_dropout_norm_forms_gpu.py holds csrc/fa_dropout_norm.hip to:
the decision hash on words computed by hand, its structure (distinct words, the 8-bit grid, the upper row word, the stream),
and the fp64 backward against torch's autograd of the fp64 forward.  No device, no library."""
import pytest
import torch

import dropout_norm_oracle as O
import dropout_norm_plan_universe as U

# (seed, offset, row, stream, group) -> (seed mix, row key, the word of the group), worked out with plain integers from the
# constants of csrc/fa_rowwise.h and csrc/fa_dropout_norm.hip.  The first is the chain of zeros: mix 0, key lowbias32(0) = 0, word
# lowbias32(0x165667B1)
WORDS = [
    ((0, 0, 0, 0, 0), (0x00000000, 0x00000000, 0x7EC30957)),
    ((1, 0, 0, 0, 0), (0x2C19FDDE, 0x0E47C35C, 0xE35B8823)),
    ((0x123456789ABCDEF0, 7, 5, 1, 3), (0x1DA9848E, 0xAEA4510A, 0x103B5C4B)),
    ((-3, 1 << 40, (1 << 32) + 9, 0, 8191), (0x1D5D706B, 0x0A03038E, 0xA54BA294)),  # (a negative int64 seed, a row past 2^32)
    ((20261021, 4, 36, 1, 65), (0x1464A480, 0xE9D0309C, 0x547DCB17)),
]


@pytest.mark.parametrize("where,want", WORDS)
def test_hand_computed_words(where, want):
    seed, offset, row, stream, g = where
    mix, key, word = want
    assert O.seed_mix(seed, offset) == mix
    assert int(O.row_key(mix, torch.tensor([row]), stream)) == key
    assert int(O.group_bytes(torch.tensor([key]), torch.tensor([g]))) == word
    for p in (0.05, 0.17, 0.5, 0.9):  # byte i of the word decides column 4 g + i, at every width that ends inside the group
        for n in range(4 * g + 1, 4 * g + 5):
            mask = O.mask_ref(seed, offset, 1, n, stream, p, row0=row)
            assert mask.dtype == torch.uint8 and mask.shape == (1, n)
            assert mask[0, 4 * g:].tolist() == [int(((word >> (8 * i)) & 255) <= int(255.0 * (1.0 - p))) for i in range(n - 4 * g)]


def test_mul32_is_the_product_mod_2_32():
    x = torch.tensor([0, 1, 0xFFFF, 0x10000, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF, 0x9E3779B1])
    for c in (0x7FEB352D, 0x846CA68B, 0x85EBCA77, 0xFFFFFFFF):
        assert O._mul32(x, c).tolist() == [(v * c) & 0xFFFFFFFF for v in x.tolist()]


def test_groups_of_a_key_have_distinct_words():
    g = torch.arange(1 << 16)
    for key in (0, 0xAEA4510A):
        assert torch.unique(O.group_bytes(torch.tensor([key]), g)).numel() == 1 << 16


@pytest.mark.parametrize("p", [0.05, 0.17, 0.5, 0.9])
def test_kept_fraction_is_on_the_8_bit_grid(p):
    """2^20 decisions: a deviation of 0.0005 at most"""
    kept = O.mask_ref(11, 5, 1024, 1024, 0, p).float().mean().item()
    assert abs(kept - (int(255 * (1 - p)) + 1) / 256) < 0.002


def test_upper_row_word_and_stream_enter_the_key():
    for r in (0, 7, 12345):
        a, b = (O.mask_ref(3, 9, 1, 1024, 0, 0.5, row0=row) for row in (r, r + (1 << 32)))
        assert not torch.equal(a, b)
        assert not torch.equal(a, O.mask_ref(3, 9, 1, 1024, 1, 0.5, row0=r))
    # rows of one call are rows of the whole: row0 only moves the window
    assert torch.equal(O.mask_ref(3, 9, 40, 37, 1, 0.17)[33:], O.mask_ref(3, 9, 7, 37, 1, 0.17, row0=33))
    m0, m1 = O.mask_ref(3, 9, 64, 1024, 0, 0.5), O.mask_ref(3, 9, 64, 1024, 1, 0.5)
    assert not torch.equal(m0[:, 4:], m1[:, :-4]) and not torch.equal(m0[:, :-4], m1[:, 4:])  # nor a stream 0 shifted by a group


@pytest.mark.parametrize("rms", [False, True], ids=["ln", "rms"])
@pytest.mark.parametrize("form", U.FORMS)
def test_backward_is_the_autograd_of_the_forward(form, rms):
    m, n, p = 5, 12, 0.5
    g = torch.Generator().manual_seed(U.FORMS.index(form))
    rand = lambda *shape: torch.randn(*shape, generator=g, dtype=torch.float64).requires_grad_(True)  # noqa: E731
    x0, w0, b0, res = rand(m, n), rand(n), rand(n), rand(m, n) if form != "two_weights_no_x1_no_res" else None
    x1 = rand(m, n) if form == "parallel" else None
    w1, b1 = (rand(n), rand(n)) if U.two_weights(U.CASES[0]._replace(form=form)) else (None, None)
    rowscale = torch.rand(m, generator=g, dtype=torch.float64) + 0.5 if form == "scaled" else None
    colscale = rand(n) if form == "scaled" else None
    keep0, keep1 = O.mask_ref(1, 2, m, n, 0, p), O.mask_ref(1, 2, m, n, 1, p) if x1 is not None else None
    f = O.forward_ref(x0, w0, b0, x1, res, w1, b1, rowscale, colscale, p, keep0, keep1, rms=rms)
    dz0, dz1, dx = (torch.randn(m, n, generator=g, dtype=torch.float64) for _ in range(3))
    loss = (f["z0"] * dz0).sum() + (f["x"] * dx).sum() + ((f["z1"] * dz1).sum() if w1 is not None else 0.0)
    leaves = dict(dx0=x0, dx1=x1, dresidual=res, dw0=w0, db0=b0, dw1=w1, db1=b1, dcolscale=colscale)
    leaves = {k: v for k, v in leaves.items() if v is not None}
    want = dict(zip(leaves, torch.autograd.grad(loss, list(leaves.values()))))
    with torch.no_grad():
        got = O.backward_ref(f["x"], None if rms else f["mu"], f["rsigma"], dz0, w0, dz1 if w1 is not None else None, w1, dx, x0,
                             rowscale, colscale, p, keep0, keep1, has_x1=x1 is not None, rms=rms)
    for name, w in want.items():
        assert (got[name] - w).abs().max() <= 1e-12 * w.abs().max(), name
    assert got["dx1"] is None or x1 is not None
    # the terms bound what they are the terms of
    for name, t in (("dresidual", "t"), ("dx0", "t_dx0"), ("dw0", "t_dw0"), ("db0", "t_db0")):
        assert bool((got[name].abs() <= got[t] * (1 + 1e-12)).all()), name
