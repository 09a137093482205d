"""GPU test of the `X_plan` entries csrc/torch_binding.cpp makes of each row operator's X_impl (def_row_op; sample_plan by hand):
one call each at the smallest valid shape (one row of 8 bf16 columns; the GEMM 8 x 8 x 8), nothing launched.  The dict has the
fields of the operator's plan struct in the order of its _lib mirror, with the values the C `fa_*_plan` entry gives for the same
call filled by hand (dummy addresses: a plan reads no memory).  And the two behaviours without a row: the GEMM has a plan, the
others refuse.  tests/test_row_binding.py holds the signatures; the forms tests hold the plans of every launch form."""
import functools

import pytest
import torch

from flash_attention_annotated_amd import _lib

pytestmark = pytest.mark.gpu

DEV = "cuda"
ADDR = 0x10000
N = 8
BF16 = _lib.FA_DTYPE_BF16
ACT = _lib.FA_ACT_SILU


def rows(m=1, n=N, dtype=torch.bfloat16):
    return torch.zeros(m, n, dtype=dtype, device=DEV)


def vec(n, dtype=torch.float32):
    return torch.zeros(n, dtype=dtype, device=DEV)


def fill(p, addresses, **fields):
    for name in addresses.split():
        setattr(p, name, ADDR)
    for name, value in fields.items():
        setattr(p, name, value)
    return p


def with_workspace(p, workspace_bytes):
    p.workspace_bytes = workspace_bytes(p)
    p.workspace = ADDR if p.workspace_bytes else 0
    return p


@functools.lru_cache(None)
def cases():
    """name -> (the binding call's arguments, the C entry point, its params filled as the binding fills them, the plan mirror)"""
    lib = _lib.load()
    weight, labels = vec(N, torch.bfloat16), vec(1, torch.int64)
    return {
        "norm_fwd": (
            (rows(), weight, None, None, None, rows(), None, 1e-5, False, False), lib.fa_norm_fwd_plan,
            fill(_lib.new_norm_fwd_params(), "x y weight mean rstd", M=1, N=N, x_row_stride=N, y_row_stride=N, eps=1e-5), _lib.FaNormPlan),
        "norm_bwd": (
            (rows(), rows(), weight, None, vec(1), vec(1), None, None, False, False, False, BF16, False), lib.fa_norm_bwd_plan,
            with_workspace(fill(_lib.new_norm_bwd_params(), "x dy weight mean rstd dx dw", M=1, N=N, x_row_stride=N, dy_row_stride=N,
                                dx_row_stride=N, dresidual_in_row_stride=N, y_row_stride=N), lib.fa_norm_bwd_workspace_bytes), _lib.FaNormPlan),
        "dropout_norm_fwd": (
            (rows(), None, None, weight, None, None, None, None, None, 0.0, 1e-5, False, False, False, False), lib.fa_dropout_norm_fwd_plan,
            fill(_lib.new_dropout_norm_fwd_params(), "x0 z0 weight0 mu rsigma", M=1, N=N, x0_row_stride=N, z0_row_stride=N, z1_row_stride=N,
                 x_row_stride=N, eps=1e-5), _lib.FaDropoutNormPlan),
        "dropout_norm_bwd": (
            (rows(), None, None, rows(), None, vec(1), vec(1), weight, None, None, None, vec(2, torch.int64), 0.0, False, False, False,
             False, BF16), lib.fa_dropout_norm_bwd_plan,
            with_workspace(fill(_lib.new_dropout_norm_bwd_params(), "dz0 x weight0 mu rsigma dx0 dw0", M=1, N=N, dz0_row_stride=N,
                                x_row_stride=N, dx0_row_stride=N, dx1_row_stride=N, dresidual_row_stride=N),
                           lib.fa_dropout_norm_bwd_workspace_bytes), _lib.FaDropoutNormPlan),
        "xent_fwd": (
            (rows(), labels, None, 0.0, 1.0, 0.0, -100, 0, N, False), lib.fa_xent_fwd_plan,
            fill(_lib.new_xent_fwd_params(), "logits labels losses lse z_losses", M=1, N=N, logits_row_stride=N, total_classes=N),
            _lib.FaXentPlan),
        "xent_bwd": (
            (vec(1), rows(), labels, vec(1), rows(), 0.0, 1.0, 0.0, -100, 0, N), lib.fa_xent_bwd_plan,
            fill(_lib.new_xent_bwd_params(), "logits labels lse dloss", dlogits=ADDR + (1 << 32), M=1, N=N, logits_row_stride=N,
                 dlogits_row_stride=N, dloss_stride=1, total_classes=N), _lib.FaXentPlan),
        "act_fwd": (
            (rows(), None, None, ACT), lib.fa_act_fwd_plan,
            fill(_lib.new_act_fwd_params(), "pre out", M=1, H=N, activation=ACT, pre_row_stride=N, out_row_stride=N), _lib.FaActPlan),
        "act_bwd": (
            (rows(), rows(), None, None, ACT, False, False, False), lib.fa_act_bwd_plan,
            fill(_lib.new_act_bwd_params(), "pre dout dpre", M=1, H=N, activation=ACT, pre_row_stride=N, dout_row_stride=N,
                 dpre_row_stride=N, out_row_stride=N), _lib.FaActPlan),
        "gemm_act_fwd": (
            (rows(N), rows(N), None, ACT, False), lib.fa_gemm_act_fwd_plan,
            fill(_lib.new_gemm_act_fwd_params(), "x weight out", M=N, N=N, K=N, activation=ACT, x_row_stride=N, weight_row_stride=N,
                 out_row_stride=N, act_input_row_stride=N), _lib.FaGemmActPlan),
        "gemm_act_dgrad": (
            (rows(N), rows(N), rows(N), ACT, False), lib.fa_gemm_act_dgrad_plan,
            fill(_lib.new_gemm_act_dgrad_params(), "grad_out weight act_input grad_in", M=N, N=N, K=N, activation=ACT,
                 grad_out_row_stride=N, weight_row_stride=N, act_input_row_stride=N, grad_in_row_stride=N), _lib.FaGemmActPlan),
        "sample": (
            (rows(), 3, 0.9, 1.0, False, False), lib.fa_sample_plan,
            fill(_lib.new_sample_params(), "logits token u", B=1, V=N, logits_row_stride=N, top_k=3, top_p=0.9), _lib.FaSampleForm),
    }


@pytest.mark.parametrize("name", ["norm_fwd", "norm_bwd", "dropout_norm_fwd", "dropout_norm_bwd", "xent_fwd", "xent_bwd", "act_fwd",
                                  "act_bwd", "gemm_act_fwd", "gemm_act_dgrad", "sample"])
def test_plan_entry_returns_the_c_plan_of_the_call(name):
    args, c_plan, params, mirror = cases()[name]
    got = getattr(_lib.binding(), name + "_plan")(*args)
    assert list(got) == [field for field, _ in mirror._fields_]
    want = mirror()
    assert c_plan(params, want) == 0
    assert got == {field: getattr(want, field) for field, _ in mirror._fields_}


def test_gemm_plan_without_a_row_is_a_plan():
    fields = [field for field, _ in _lib.FaGemmActPlan._fields_]
    got = _lib.binding().gemm_act_fwd_plan(rows(0), rows(N), None, ACT, False)
    assert list(got) == fields and got["grid_x"] == 0 and got["dgrad"] == 0  # (no tiles: tests/test_gemm_act_plan.py)
    got = _lib.binding().gemm_act_dgrad_plan(rows(0), rows(N), rows(0), ACT, True)
    assert list(got) == fields and got["grid_x"] == 0 and got["dgrad"] == 1


def test_norm_plan_without_a_row_is_refused():
    with pytest.raises(RuntimeError, match="layer_norm: a plan needs at least one row"):
        _lib.binding().norm_fwd_plan(rows(0), vec(N, torch.bfloat16), None, None, None, rows(0), None, 1e-5, False, False)
