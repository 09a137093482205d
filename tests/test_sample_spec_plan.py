"""CPU tests of fa_spec_sample_plan (include/fa_spec_sample.h) against tests/sample_spec_plan_universe.py: cw from the dtype and the
alignment of both logits tensors, the two workgroup sizes, which selections run, key and index passes, and the two grids.  No
device: the plan is the host function the launch itself consumes."""
import pytest

import sample_spec_plan_universe as U
from flash_attention_annotated_amd import _lib

DT = {"bf16": _lib.FA_DTYPE_BF16, "fp16": _lib.FA_DTYPE_FP16, "fp32": _lib.FA_DTYPE_FP32}


def c_plan(b, s, v, dtype, top_k=1, top_p=0.0, temperature=1.0, address=0x10000, draft_address=0x20000, strides=None, draft_strides=None):
    lib = _lib.load()
    p = _lib.new_spec_sample_params()
    for name in ("tokens_draft", "u_acc", "u_res", "workspace", "tokens", "num_generated"):
        setattr(p, name, 0x10000)
    p.logits, p.logits_draft = address, draft_address
    p.logits_dtype, p.B, p.S, p.V, p.top_k, p.top_p, p.temperature = DT[dtype], b, s, v, top_k, top_p, temperature
    p.logits_batch_stride, p.logits_pos_stride = ((s + 1) * v, v) if strides is None else strides
    p.draft_batch_stride, p.draft_pos_stride = (s * v, v) if draft_strides is None else draft_strides
    p.tokens_draft_batch_stride = s
    p.workspace_bytes = lib.fa_spec_sample_workspace_size(b, s)
    form = _lib.FaSpecSampleForm()
    assert lib.fa_spec_sample_plan(p, form) == 0
    return U.Plan(*(getattr(form, f) for f in U.Plan._fields))


@pytest.mark.parametrize("case", U.CASES, ids=[c.name for c in U.CASES])
def test_the_plan_of_every_case_of_the_universe(case):
    es = U.ESIZE[case.dtype]
    strides = ((case.s + 1) * (case.v + case.pad), case.v + case.pad)
    draft_strides = (case.s * (case.v + case.pad), case.v + case.pad)
    got = c_plan(case.b, case.s, case.v, case.dtype, case.top_k, case.top_p, case.temperature, 0x10000 + case.shift * es,
                 0x20000 + case.draft_shift * es, strides, draft_strides)
    assert got == U.case_plan(case)


@pytest.mark.parametrize("dtype", list(DT))
def test_both_sides_of_every_boundary(dtype):
    es = U.ESIZE[dtype]
    cw = 16 // es
    for kw in (
        dict(b=3, s=2, v=1024 * cw), dict(b=3, s=2, v=1024 * cw + cw),        # the workgroup size, 16-byte form
        dict(b=3, s=2, v=1024, address=0x10000 + es), dict(b=3, s=2, v=1025),  # ... and by elements
        dict(b=3, s=2, v=cw * 50), dict(b=3, s=2, v=cw * 50 + 1),              # the row length in bytes
        dict(b=3, s=2, v=4096, address=0x10000 + es), dict(b=3, s=2, v=4096, draft_address=0x20000 + es),
        dict(b=3, s=0, v=4096, draft_address=0x20000 + es),                    # no draft rows: its base does not count
        dict(b=3, s=2, v=4096, strides=(3 * 4096 + 1, 4096)), dict(b=1, s=2, v=4096, strides=(3 * 4096 + 1, 4096)),
        dict(b=3, s=2, v=4096, strides=(3 * 4100, 4097)), dict(b=3, s=0, v=4096, strides=(4096, 4097)),
        dict(b=3, s=2, v=4096, draft_strides=(2 * 4096 + 1, 4096)), dict(b=1, s=2, v=4096, draft_strides=(2 * 4096 + 1, 4096)),
        dict(b=3, s=2, v=4096, draft_strides=(2 * 4104, 4097)), dict(b=3, s=1, v=4096, draft_strides=(4096, 4097)),
        dict(b=3, s=2, v=208, top_k=0), dict(b=3, s=2, v=208, top_k=1), dict(b=3, s=2, v=208, top_k=207), dict(b=3, s=2, v=208, top_k=208),
        dict(b=3, s=2, v=208, top_p=0.0), dict(b=3, s=2, v=208, top_p=0.5), dict(b=3, s=2, v=208, top_p=1.0),
        dict(b=3, s=2, v=208, temperature=0.7),
        dict(b=3, s=2, v=1), dict(b=3, s=2, v=2), dict(b=3, s=2, v=2048), dict(b=3, s=2, v=2049),  # index bits and passes
        dict(b=1, s=1, v=(1 << 22) + 8), dict(b=1, s=1, v=(1 << 23) + 8),                          # fraction bits
        dict(b=21845, s=2, v=8), dict(b=21846, s=2, v=8), dict(b=65535, s=0, v=8), dict(b=65536, s=0, v=8),  # the grids
    ):
        assert c_plan(dtype=dtype, **kw) == U.plan(dtype=dtype, **kw), kw


def test_the_forms_differ_where_they_should():
    assert c_plan(3, 2, 4096, "bf16").cw == 8 and c_plan(3, 2, 4096, "fp32").cw == 4 and c_plan(3, 2, 4099, "bf16").cw == 1
    assert c_plan(3, 2, 4096, "bf16", draft_address=0x20002).cw == 1 and c_plan(3, 0, 4096, "bf16", draft_address=0x20002).cw == 8
    assert c_plan(3, 2, 4096, "bf16", top_k=1).topk == 1  # the filter's rule: no greedy shortcut
    p = c_plan(70000, 4, 8, "bf16", top_k=3)
    assert (p.grid_a, p.grid_b, p.k) == (65535, 65535, 3)
