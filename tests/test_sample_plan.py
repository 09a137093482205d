"""CPU tests of fa_sample_plan (include/fa_sample.h) against tests/sample_plan_universe.py: cw from dtype and alignment, the two
workgroup sizes, which phases run, the bits and passes of the two descents, the fixed-point scale and the grid cap, each on both
sides of its boundary.  Dummy addresses, nothing dereferenced, no device; tests/test_sample_gpu.py runs U.CASES on the kernels."""
import pytest

import sample_plan_universe as U
from flash_attention_annotated_amd import _lib

ADDR = 0x10000
OK, NULLP, BAD_SHAPE = 0, -1, -5
CODE = {"bf16": _lib.FA_DTYPE_BF16, "fp16": _lib.FA_DTYPE_FP16, "fp32": _lib.FA_DTYPE_FP32}


def params(b, v, dtype="bf16", top_k=1, top_p=0.0, temperature=1.0, mode=U.DRAW, address=ADDR, stride=None):
    p = _lib.new_sample_params()
    p.logits, p.token = address, ADDR
    if mode == U.DRAW and top_k != 1:
        p.u = ADDR
    p.B, p.V, p.logits_row_stride, p.logits_dtype = b, v, v if stride is None else stride, CODE[dtype]
    p.mode, p.top_k, p.top_p, p.temperature = mode, top_k, top_p, temperature
    return p


def both(*args, **kw):
    """the library's plan, after it was held to the universe's"""
    form = _lib.FaSampleForm()
    st = _lib.load().fa_sample_plan(params(*args, **kw), form)
    assert st == OK, st
    got = U.Plan(*(getattr(form, f) for f in U.Plan._fields))
    assert got == U.plan(*args, **kw), (args, kw)
    return got


@pytest.mark.parametrize("dtype", ["bf16", "fp16", "fp32"])
def test_cw_is_from_dtype_and_alignment(dtype):
    es, cw = U.ESIZE[dtype], 16 // U.ESIZE[dtype]
    v = 64 * cw
    assert both(4, v, dtype).cw == cw
    assert both(4, v + cw, dtype).cw == cw and both(4, v + cw - 1, dtype).cw == 1 and both(4, v + 1, dtype).cw == 1
    assert both(4, v, dtype, address=ADDR + es).cw == 1 and both(4, v, dtype, address=ADDR + 16).cw == cw
    assert both(4, v, dtype, stride=v + cw).cw == cw and both(4, v, dtype, stride=v + 1).cw == 1
    assert both(1, v, dtype, stride=v + 1).cw == cw  # one row: the pitch says nothing
    assert both(4, v, dtype, stride=0, top_k=5).cw == cw


def test_threads_by_accesses():
    for dtype, cw in (("bf16", 8), ("fp32", 4)):
        assert both(2, 1024 * cw, dtype).threads == 256 and both(2, 1025 * cw, dtype).threads == 1024
        assert both(2, 1024, dtype, address=ADDR + 4).threads == 256 and both(2, 1025, dtype).threads == 1024
    assert both(2, 1, "bf16").threads == 256 and both(1, (1 << 31) - 1, "bf16").threads == 1024


def test_phases():
    v = 4096
    for mode in (U.DRAW, U.FILTER):
        for top_k in (0, 1, 2, v - 1, v, v + 3):
            for top_p in (0.0, 0.1, 1.0):
                p = both(3, v, "bf16", top_k, top_p, mode=mode)
                greedy = mode == U.DRAW and top_k == 1
                assert p.greedy == int(greedy) and p.draw == int(mode == U.DRAW and not greedy)
                assert p.topk == int(not greedy and (2 if mode == U.DRAW else 1) <= top_k < v) and p.k == (top_k if p.topk else 0)
                assert p.topp == int(not greedy and top_p == 0.1)
    assert both(3, 1, "bf16", 2, 0.5).topk == 0 and both(3, 2, "bf16", 2, 0.5).topk == 0 and both(3, 3, "bf16", 2, 0.5).topk == 1
    assert both(3, 8, "bf16", 1, 0.0, mode=U.FILTER).topk == 1


def test_key_and_index_bits():
    assert [both(2, 4096, d, 5).key_bits for d in ("bf16", "fp16", "fp32")] == [16, 19, 32]
    assert [both(2, 4096, d, 5).key_passes for d in ("bf16", "fp16", "fp32")] == [2, 2, 3]
    assert [both(2, 4096, d, 5, temperature=0.7).key_bits for d in ("bf16", "fp16", "fp32")] == [32, 32, 32]
    for v, bits, passes in ((1, 1, 1), (2, 1, 1), (3, 2, 1), (2048, 11, 1), (2049, 12, 2), (1 << 22, 22, 2), ((1 << 22) + 1, 23, 3),
                            ((1 << 31) - 1, 31, 3)):
        p = both(1, v, "bf16", 0)
        assert (p.index_bits, p.index_passes) == (bits, passes), v


def test_fixed_point_scale_and_grid():
    for v, frac in ((1, 40), (1 << 22, 40), ((1 << 22) + 1, 39), (1 << 23, 39), ((1 << 31) - 1, 31)):
        assert both(1, v, "bf16", 0).frac_bits == frac, v
    for b, grid in ((1, 1), (65535, 65535), (65536, 65535), (1 << 31, 65535)):
        assert both(b, 8, "bf16", 0).grid_x == grid


@pytest.mark.parametrize("c", U.CASES, ids=[c.name for c in U.CASES])
def test_gpu_cases_take_the_form_their_name_says(c):
    p = both(c.b, c.v, c.dtype, c.top_k, c.top_p, c.temperature, c.mode, ADDR + c.shift * U.ESIZE[c.dtype], c.v + c.pad)
    assert p == U.case_plan(c)
    words = c.name
    if ", 16 bytes" in words or "stays on 16 bytes" in words:
        assert p.cw > 1
    if "elements" in words or "off 16 bytes" in words or "no multiple of 16 bytes" in words:
        assert p.cw == 1
    if "small workgroup" in words or words.endswith("1024 accesses") or words.endswith("elements 1024"):
        assert p.threads == 256 and c.v // p.cw == 1024
    if "large workgroup" in words or words.endswith("1025 accesses") or words.endswith("elements 1025"):
        assert p.threads == 1024 and c.v // p.cw == 1025
    if "index bits" in words:
        assert p.index_bits == int(words.split()[1]) and p.index_passes == {"one": 1, "two": 2, "three": 3}[words.split()[4]]
    if "more rows than workgroups" in words:
        assert c.b > p.grid_x == U.MAX_GRID
    if "top_k = V - 1" in words:
        assert p.topk == 1
    if "top_k = V is" in words:
        assert p.topk == 0


def test_plan_validates_first():
    lib = _lib.load()
    form = _lib.FaSampleForm(cw=-7)
    assert lib.fa_sample_plan(None, form) == NULLP
    assert lib.fa_sample_plan(params(3, 0), form) == BAD_SHAPE
    assert form.cw == -7  # untouched
    assert lib.fa_sample_plan(params(3, 8), None) == NULLP
