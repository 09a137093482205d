"""CPU tests of fa_tree_sample_plan (include/fa_tree_sample.h) against tests/sample_tree_plan_universe.py: cw from the dtype and the
alignment of the logits tensors that are given, the two workgroup sizes, the mode, which selections run, key and index passes,
and the two grids.  No device: the plan is the host function the launch itself consumes."""
import pytest

import sample_tree_plan_universe as U
from flash_attention_annotated_amd import _lib

DT = {"bf16": _lib.FA_DTYPE_BF16, "fp16": _lib.FA_DTYPE_FP16, "fp32": _lib.FA_DTYPE_FP32}


def c_plan(b, t, v, dtype, mode="draft", top_k=1, top_p=0.0, temperature=1.0, address=0x10000, draft_address=0x20000, strides=None,
           draft_strides=None):
    lib = _lib.load()
    p = _lib.new_tree_sample_params()
    for name in ("tokens_draft", "parents", "u_acc", "u_res", "workspace", "path", "path_len", "tokens", "num_generated"):
        setattr(p, name, 0x10000)
    p.logits, p.logits_draft = address, draft_address if mode == "draft" else 0
    p.logits_dtype, p.B, p.T, p.V, p.top_k, p.top_p, p.temperature = DT[dtype], b, t, v, top_k, top_p, temperature
    p.logits_batch_stride, p.logits_node_stride = (t * v, v) if strides is None else strides
    p.draft_batch_stride, p.draft_node_stride = (t * v, v) if draft_strides is None else draft_strides
    p.tokens_draft_batch_stride = p.parents_batch_stride = t
    p.workspace_bytes = lib.fa_tree_sample_workspace_size(b, t)
    form = _lib.FaTreeSampleForm()
    assert lib.fa_tree_sample_plan(p, form) == 0
    return U.Plan(*(getattr(form, f) for f in U.Plan._fields))


@pytest.mark.parametrize("case", U.CASES, ids=[c.name for c in U.CASES])
def test_the_plan_of_every_case_of_the_universe(case):
    es = U.ESIZE[case.dtype]
    strides = (case.t * (case.v + case.pad), case.v + case.pad)
    got = c_plan(case.b, case.t, case.v, case.dtype, case.mode, case.top_k, case.top_p, case.temperature, 0x10000 + case.shift * es,
                 0x20000 + case.draft_shift * es, strides, strides)
    assert got == U.case_plan(case)


@pytest.mark.parametrize("mode", ["draft", "onehot"])
@pytest.mark.parametrize("dtype", list(DT))
def test_both_sides_of_every_boundary(dtype, mode):
    es = U.ESIZE[dtype]
    cw = 16 // es
    for kw in (
        dict(b=3, t=5, v=1024 * cw), dict(b=3, t=5, v=1024 * cw + cw),        # the workgroup size, 16-byte form
        dict(b=3, t=5, v=1024, address=0x10000 + es), dict(b=3, t=5, v=1025),  # ... and by elements
        dict(b=3, t=5, v=cw * 50), dict(b=3, t=5, v=cw * 50 + 1),              # the row length in bytes
        dict(b=3, t=5, v=4096, address=0x10000 + es), dict(b=3, t=5, v=4096, draft_address=0x20000 + es),
        dict(b=3, t=5, v=4096, strides=(5 * 4096 + 1, 4096)), dict(b=1, t=5, v=4096, strides=(5 * 4096 + 1, 4096)),
        dict(b=3, t=5, v=4096, strides=(5 * 4104, 4097)), dict(b=3, t=1, v=4096, strides=(4096, 4097)),
        dict(b=3, t=5, v=4096, draft_strides=(5 * 4096 + 1, 4096)), dict(b=1, t=5, v=4096, draft_strides=(5 * 4096 + 1, 4096)),
        dict(b=3, t=5, v=4096, draft_strides=(5 * 4104, 4097)), dict(b=3, t=1, v=4096, draft_strides=(4096, 4097)),
        dict(b=3, t=5, v=208, top_k=0), dict(b=3, t=5, v=208, top_k=1), dict(b=3, t=5, v=208, top_k=207), dict(b=3, t=5, v=208, top_k=208),
        dict(b=3, t=5, v=208, top_p=0.0), dict(b=3, t=5, v=208, top_p=0.5), dict(b=3, t=5, v=208, top_p=1.0),
        dict(b=3, t=5, v=208, temperature=0.7),
        dict(b=3, t=5, v=1), dict(b=3, t=5, v=2), dict(b=3, t=5, v=2048), dict(b=3, t=5, v=2049),  # index bits and passes
        dict(b=1, t=2, v=(1 << 22) + 8), dict(b=1, t=2, v=(1 << 23) + 8),                          # fraction bits
        dict(b=21845, t=3, v=8), dict(b=21846, t=3, v=8), dict(b=65535, t=1, v=8), dict(b=65536, t=1, v=8),  # the grids
        dict(b=2, t=1, v=8), dict(b=2, t=64, v=8),                                                  # the node counts
    ):
        assert c_plan(dtype=dtype, mode=mode, **kw) == U.plan(dtype=dtype, mode=mode, **kw), kw


def test_the_forms_differ_where_they_should():
    assert c_plan(3, 5, 4096, "bf16").cw == 8 and c_plan(3, 5, 4096, "fp32").cw == 4 and c_plan(3, 5, 4099, "bf16").cw == 1
    assert c_plan(3, 5, 4096, "bf16", draft_address=0x20002).cw == 1 and c_plan(3, 5, 4096, "bf16", "onehot", draft_address=0x20002).cw == 8
    assert c_plan(3, 5, 4096, "bf16").drafts == 1 and c_plan(3, 5, 4096, "bf16", "onehot").drafts == 0
    assert c_plan(3, 5, 4096, "bf16", top_k=1).topk == 1  # the filter's rule: no greedy shortcut
    assert c_plan(3, 5, 4096, "bf16").threads == 256 and c_plan(3, 5, 32000, "bf16").threads == 1024
    p = c_plan(70000, 4, 8, "bf16", top_k=3)
    assert (p.grid_a, p.grid_b, p.k) == (65535, 65535, 3)
