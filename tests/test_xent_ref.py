"""CPU tests of the fused cross-entropy's oracle (ops/triton/cross_entropy.py: cross_entropy_ref, cross_entropy_grad_ref) and of
the collective step of a vocabulary split (_finish_split).  No library and no device: tests/test_xent_gpu.py holds the kernels
to this oracle."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn.functional as F

from flash_attention_annotated_amd.ops.triton.cross_entropy import _finish_split, cross_entropy_grad_ref, cross_entropy_ref

M, N, CUT = 37, 203, 96
CASES = [(0.0, 1.0, 0.0), (0.1, 0.7, 1e-2), (0.9, 1.0, 0.0)]  # (smoothing, logit_scale, lse_square_scale)
TOL = 1e-12


def _problem():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(M, N, dtype=torch.float64, generator=g) * 2
    y = torch.randint(0, N, (M,), generator=g)
    y[::7] = -100
    d = torch.randn(M, dtype=torch.float64, generator=g)
    return x, y, d


def _torch_loss(x, y, s, scale, z):
    lse = torch.logsumexp(x * scale, dim=1)
    return F.cross_entropy(x * scale, y, label_smoothing=s, reduction="none") + (z * lse.square()).masked_fill(y == -100, 0.0)


def _split_partials(x, y, s, scale):
    """The two ranks' (losses, lse) with split set, columns [0, CUT) and [CUT, N)."""
    out = []
    for start, stop in ((0, CUT), (CUT, N)):
        losses, z_losses, lse = cross_entropy_ref(x[:, start:stop], y, label_smoothing=s, logit_scale=scale, lse_square_scale=1.0,
                                                  class_start_idx=start, total_classes=N, split=True)
        assert not z_losses.any()  # (a split leaves the z-loss to the global lse)
        out.append((losses, lse))
    return out


@pytest.mark.parametrize("s,scale,z", CASES)
def test_ref_matches_torch(s, scale, z):
    x, y, d = _problem()
    xr = x.clone().requires_grad_(True)
    losses, z_losses, lse = cross_entropy_ref(xr, y, label_smoothing=s, logit_scale=scale, lse_square_scale=z)
    xt = x.clone().requires_grad_(True)
    want = _torch_loss(xt, y, s, scale, z)
    assert losses.dtype == torch.float64
    assert (losses - want).abs().max().item() <= TOL
    assert (lse - torch.logsumexp(x * scale, dim=1)).abs().max().item() <= TOL
    assert (z_losses - (z * lse.square()).masked_fill(y == -100, 0.0)).abs().max().item() <= TOL
    assert not losses[::7].any() and not z_losses[::7].any() and not z_losses.requires_grad
    (g_want,) = torch.autograd.grad(want, xt, d, retain_graph=True)
    (g_ref,) = torch.autograd.grad(losses, xr, d)
    assert (g_ref - g_want).abs().max().item() <= TOL
    g_formula = cross_entropy_grad_ref(x, y, lse.detach(), d, label_smoothing=s, logit_scale=scale, lse_square_scale=z)
    assert (g_formula - g_want).abs().max().item() <= TOL
    assert not g_formula[::7].any()
    # an expanded scalar, the gradient of losses.sum()
    g_sum = cross_entropy_grad_ref(x, y, lse.detach(), torch.ones((), dtype=torch.float64).expand(M), label_smoothing=s,
                                   logit_scale=scale, lse_square_scale=z)
    (g_sum_want,) = torch.autograd.grad(want.sum(), xt)
    assert (g_sum - g_sum_want).abs().max().item() <= TOL


def test_ref_ignored_rows_hold_anything():
    """NaN in an ignored row: zero loss, zero gradient, the other rows untouched."""
    x, y, d = _problem()
    clean = cross_entropy_ref(x, y, label_smoothing=0.1)
    x[::7] = float("nan")
    losses, z_losses, lse = cross_entropy_ref(x, y, label_smoothing=0.1)
    assert torch.equal(losses, clean[0]) and not losses[::7].any()
    g = cross_entropy_grad_ref(x, y, lse, d, label_smoothing=0.1)
    assert not g[::7].any() and not g.isnan().any()


def test_ref_label_outside_the_columns():
    x, y, _ = _problem()
    y = y.clone()
    y[1], y[2] = N + 5, N
    for s in (0.0, 0.1):
        losses, _, lse = cross_entropy_ref(x, y, label_smoothing=s, total_classes=2 * N)
        want = s * (lse - x.sum(dim=1) / (2 * N))
        assert (losses[1:3] - want[1:3]).abs().max().item() <= TOL


def test_ref_precomputed_lse():
    x, y, _ = _problem()
    losses, _, lse = cross_entropy_ref(x, y, lse_square_scale=1e-2)
    again, _, lse_again = cross_entropy_ref(x, y, precomputed_lse=lse, lse_square_scale=1e-2)
    assert torch.equal(losses, again) and lse_again is not None and torch.equal(lse, lse_again)


@pytest.mark.parametrize("s,scale,z", CASES)
def test_split_in_two_equals_unsplit(s, scale, z):
    x, y, d = _problem()
    whole, whole_z, whole_lse = cross_entropy_ref(x, y, label_smoothing=s, logit_scale=scale, lse_square_scale=z)
    (l0, lse0), (l1, lse1) = _split_partials(x, y, s, scale)
    lse = torch.logsumexp(torch.stack([lse0, lse1]), dim=0)
    z_losses = (z * lse.square()).masked_fill(y == -100, 0.0)
    losses = (l0 + l1 + lse).masked_fill(y == -100, 0.0) + z_losses
    assert (losses - whole).abs().max().item() <= TOL
    assert (lse - whole_lse).abs().max().item() <= TOL
    # the same through _finish_split without a group: the stacked partials stand in for the collectives
    got, got_z, got_lse = _finish_split(torch.stack([l0, l1]), torch.stack([lse0, lse1]), y, z, -100, None)
    assert (got - whole).abs().max().item() <= TOL and (got_z - whole_z).abs().max().item() <= TOL
    assert (got_lse - whole_lse).abs().max().item() <= TOL
    # the backward of each half from the global lse is the half of the whole gradient
    g_whole = cross_entropy_grad_ref(x, y, whole_lse, d, label_smoothing=s, logit_scale=scale, lse_square_scale=z)
    for start, stop in ((0, CUT), (CUT, N)):
        g = cross_entropy_grad_ref(x[:, start:stop], y, got_lse, d, label_smoothing=s, logit_scale=scale, lse_square_scale=z,
                                   class_start_idx=start, total_classes=N)
        assert (g - g_whole[:, start:stop]).abs().max().item() <= TOL


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _worker(rank, world, port):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        x, y, _ = _problem()  # every rank builds the same problem and keeps its columns
        for s, scale, z in CASES:
            whole, whole_z, whole_lse = cross_entropy_ref(x, y, label_smoothing=s, logit_scale=scale, lse_square_scale=z)
            losses, lse = _split_partials(x, y, s, scale)[rank]
            mine = losses.clone()
            got, got_z, got_lse = _finish_split(losses, lse, y, z, -100, dist.group.WORLD)
            assert torch.equal(losses, mine)  # (the partials are the caller's)
            assert (got - whole).abs().max().item() <= TOL, (rank, s, scale, z)
            assert (got_z - whole_z).abs().max().item() <= TOL
            assert (got_lse - whole_lse).abs().max().item() <= TOL
        dist.barrier()
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(120)
def test_finish_split_two_ranks_gloo():
    world = 2
    mp.spawn(_worker, args=(world, _free_port()), nprocs=world, join=True)
