"""CPU test of how csrc/torch_binding.cpp registers the row operators: every `X` has an `X_plan` with the very same arguments
(names, types, order) that returns a dict.  def_row_op gives this by construction, since both are made of one X_impl; this keeps
a later hand-written m.def from breaking it.  tests/test_row_binding_gpu.py holds what the `X_plan` entries return."""
import pytest

from flash_attention_annotated_amd import _lib

ROW_OPS = ("norm_fwd", "norm_bwd", "dropout_norm_fwd", "dropout_norm_bwd", "xent_fwd", "xent_bwd", "act_fwd", "act_bwd",
           "gemm_act_fwd", "gemm_act_dgrad")


def signature(name):
    """(arguments, return type) of the pybind signature line, the name removed"""
    line = getattr(_lib.binding(), name).__doc__.splitlines()[0]
    assert line.startswith(name + "("), line
    arguments, returns = line[len(name):].rsplit(" -> ", 1)
    return arguments, returns


@pytest.mark.parametrize("name", ROW_OPS)
def test_plan_entry_takes_the_arguments_of_the_launch(name):
    arguments, returns = signature(name)
    assert signature(name + "_plan") == (arguments, "dict")
    assert returns != "dict" and "arg0" not in arguments  # (every argument is named)
