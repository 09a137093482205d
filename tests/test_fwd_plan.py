"""CPU tests of the forward routing: fa_fwd_plan_name() names the kernel plan_fwd() (csrc/fa_fwd_api.hip) picks -- family,
template shape and forms, block_m, split-KV, fp8 expansion, 256-column calls.  One row per branch of the routing, on a
device of 256 CUs; tests/test_persistent_gpu.py and the GPU suite check that the named kernels compute the right thing."""
import ctypes
import re
import threading

import pytest

from flash_attention_annotated_amd import _lib
from plan_universe import FORMS, FP8_CASE, FP8_FORM, UNIVERSE

ADDR = 0x10000  # an aligned dummy address: nothing is dereferenced


def _params(b=2, h=16, h_k=None, sq=4096, sk=None, d=128, d_v=0, dtype=_lib.FA_DTYPE_BF16, **fields):
    """Dense contiguous (b, s, h, d) tensors; a dummy workspace large enough for any split or fp8 expansion."""
    h_k, sk, dv = h_k or h, sk or sq, d_v or d
    p = _lib.new_params()
    for f in ("q", "k", "v", "o", "softmax_lse", "workspace"):
        setattr(p, f, ADDR)
    p.workspace_bytes = 1 << 40
    p.b, p.seqlen_q, p.seqlen_k, p.h, p.h_k, p.d, p.d_v, p.dtype = b, sq, sk, h, h_k, d, d_v, dtype
    for t, rows, heads, width in (("q", sq, h, d), ("k", sk, h_k, d), ("v", sk, h_k, dv), ("o", sq, h, dv)):
        setattr(p, f"{t}_head_stride", width)
        setattr(p, f"{t}_row_stride", heads * width)
        setattr(p, f"{t}_batch_stride", rows * heads * width)
    p.softmax_scale = d ** -0.5
    p.window_size_left = p.window_size_right = -1
    for k, v in fields.items():
        setattr(p, k, v)
    return p


def _paged(**kw):
    return _params(block_table=ADDR, page_block_size=256, block_table_batch_stride=16, **kw)


def _qv(d=64, d_v=512, **kw):
    return _params(d=d, d_v=d_v, qv=ADDR, qv_head_stride=d, qv_row_stride=16 * d, qv_batch_stride=4096 * 16 * d, **kw)


FP8 = _lib.FA_DTYPE_FP8_E4M3
ROWS = [  # (id, params, persist mode, plan name)
    ("c2", _params(b=4, sq=8192), 0,
     "fwd_kernel_w64 D=128 DEFF=128 waves=4 PERSIST block_m=256 splits=1"),
    ("c2_handover", _params(b=4, sq=8192), -1,
     "fwd_kernel_w64 D=128 DEFF=128 waves=4 block_m=256 splits=1"),
    ("c3", _params(b=4, sq=16384, is_causal=1), 0,
     "fwd_kernel_w64 D=128 DEFF=128 waves=4 PERSIST block_m=256 splits=1"),
    ("d96", _params(d=96), 0,
     "fwd_kernel_w64 D=128 DEFF=96 waves=4 block_m=256 splits=1"),
    ("d64_short_causal", _params(b=16, sq=1024, d=64, is_causal=1), 0,
     "fwd_kernel D=64 waves=4 block_m=128 splits=1"),
    ("d64", _params(h=32, sq=8192, d=64), 0,
     "fwd_kernel_w64 D=64 DEFF=64 waves=4 block_m=256 splits=1"),
    ("decode", _params(b=8, h=32, h_k=8, sq=1, sk=8192), 0,
     "fwd_kernel D=128 waves=4 block_m=128 splits=4"),
    ("d128_paged", _paged(), 0,
     "fwd_kernel D=128 waves=8 block_m=256 splits=1"),
    ("d128_softcap", _params(b=4, softcap=30.0), 0,
     "fwd_kernel_d256 W=128 waves=4 SOFTCAP block_m=128 splits=1"),
    ("d64_alibi", _params(d=64, alibi_slopes=ADDR), 0,
     "fwd_kernel_d256 W=64 waves=4 ALIBI block_m=128 splits=1"),
    ("d128_softcap_alibi", _params(softcap=30.0, alibi_slopes=ADDR), 0,
     "fwd_kernel_w64 D=128 DEFF=128 waves=4 SOFTCAP block_m=256 splits=1"),
    ("d192", _params(d=192), 0,
     "fwd_kernel_d256 W=192 waves=4 block_m=128 splits=1"),
    ("d256_paged", _paged(d=256), 0,
     "fwd_kernel D=256 waves=4 block_m=128 splits=1"),
    ("d192_dv128", _params(d=192, d_v=128), 0,
     "fwd_kernel_d256 W=192 waves=4 block_m=128 splits=1"),
    ("d128_chunk", _params(attention_chunk=1024), 0,
     "fwd_kernel D=128 waves=8 EXTRA block_m=256 splits=1"),
    ("d128_dropout", _params(p_dropout=0.1, rng_state=ADDR), 0,
     "fwd_kernel D=128 waves=8 DROPOUT block_m=256 splits=1"),
    ("c5_fp8", _params(b=4, sq=8192, dtype=FP8), 0,
     "fwd_kernel_fp8 D=128 waves=4 block_m=256 splits=1"),
    ("fp8_d64", _params(d=64, dtype=FP8), 0,
     "fwd_kernel_w64 D=64 DEFF=64 waves=4 block_m=256 splits=1 fp8_expand"),
    ("qv_dv512", _qv(), 0,
     "fwd_kernel_qv DVT=512 waves=4 block_m=128 splits=1"),
    ("dv512_columns", _params(d=64, d_v=512), 0,
     "fwd_kernel_d256 W=256 waves=4 block_m=128 splits=1 cols=2"),
    ("dv384_paged", _paged(d=64, d_v=384), 0,
     "fwd_kernel_qv DVT=512 waves=4 block_m=128 splits=1"),
    # softcap beside a split-KV plan (or beside ALiBi) stays in the 256-row kernel: the capped widths of fwd_kernel_d256 do not split
    ("d64_softcap_alibi_split", _params(b=1, h=4, sq=512, sk=4096, d=64, softcap=30.0, alibi_slopes=ADDR), 0,
     "fwd_kernel_w64 D=64 DEFF=64 waves=4 SOFTCAP block_m=256 splits=16"),
    ("d128_softcap_split", _params(b=1, h=4, sq=512, sk=4096, softcap=30.0), 0,
     "fwd_kernel_w64 D=128 DEFF=128 waves=4 SOFTCAP block_m=256 splits=16"),
    ("d64_softcap", _params(d=64, softcap=30.0), 0,
     "fwd_kernel_d256 W=64 waves=4 SOFTCAP block_m=128 splits=1"),
    ("d64_softcap_causal_short", _params(d=64, sq=2048, softcap=30.0, is_causal=1), 0,
     "fwd_kernel D=64 waves=4 SOFTCAP block_m=128 splits=2"),  # (512 work items: the 4-wave shape still splits)
    ("d96_softcap", _params(d=96, softcap=30.0), 0,
     "fwd_kernel_d256 W=96 waves=4 SOFTCAP block_m=128 splits=1"),
    ("d96_alibi", _params(d=96, alibi_slopes=ADDR), 0,
     "fwd_kernel_d256 W=96 waves=4 ALIBI block_m=128 splits=1"),
    ("d160", _params(d=160), 0,
     "fwd_kernel_d256 W=160 waves=4 block_m=128 splits=1"),
    ("d256", _params(d=256), 0,
     "fwd_kernel_d256 W=256 waves=4 block_m=128 splits=1"),
    ("d64_paged", _paged(d=64), 0,
     "fwd_kernel D=64 waves=8 block_m=256 splits=1"),
    ("d256_chunk", _params(d=256, attention_chunk=1024), 0,
     "fwd_kernel D=256 waves=4 EXTRA block_m=128 splits=1"),
    ("d256_dropout", _params(d=256, p_dropout=0.1, rng_state=ADDR), 0,
     "fwd_kernel D=256 waves=4 DROPOUT block_m=128 splits=1"),
    ("qv_dv256", _qv(d_v=256), 0,
     "fwd_kernel_qv DVT=256 waves=4 block_m=128 splits=1"),
    ("qv_dv256_softcap", _qv(d_v=256, softcap=30.0), 0,
     "fwd_kernel_qv DVT=256 waves=4 SOFTCAP block_m=128 splits=1"),
    ("dv512_split_without_qv", _params(d=64, d_v=512, num_splits=3), 0,
     "fwd_kernel_qv DVT=512 waves=4 block_m=128 splits=3"),
    ("varlen", _params(cu_seqlens_q=ADDR, cu_seqlens_k=ADDR, total_q=8192, total_k=8192), 0,
     "fwd_kernel_w64 D=128 DEFF=128 waves=4 block_m=256 splits=1"),
    # fp8 at head dim 128 leaves the native kernel for each reason fp8_native() lists (paged fp8: test_fp8_paged_is_rejected)
    ("fp8_softcap", _params(dtype=FP8, softcap=30.0), 0,
     "fwd_kernel_d256 W=128 waves=4 SOFTCAP block_m=128 splits=1 fp8_expand"),
    ("fp8_left_window", _params(dtype=FP8, window_size_left=1024, window_size_right=0), 0,
     "fwd_kernel_w64 D=128 DEFF=128 waves=4 block_m=256 splits=1 fp8_expand"),
    ("fp8_alibi", _params(dtype=FP8, alibi_slopes=ADDR), 0,
     "fwd_kernel_d256 W=128 waves=4 ALIBI block_m=128 splits=1 fp8_expand"),
    ("fp8_odd_stride", _params(dtype=FP8, q_row_stride=16 * 128 + 8), 0,
     "fwd_kernel_w64 D=128 DEFF=128 waves=4 PERSIST block_m=256 splits=1 fp8_expand"),
]


@pytest.mark.parametrize("params,persist,name", [r[1:] for r in ROWS], ids=[r[0] for r in ROWS])
def test_plan_name(built_lib, params, persist, name):
    assert built_lib.fa_fwd_validate(ctypes.byref(params)) == 0
    built_lib.fa_set_persist_mode(persist)
    try:
        assert built_lib.fa_fwd_plan_name(ctypes.byref(params), 256) == name.encode()
    finally:
        built_lib.fa_set_persist_mode(0)


def test_plan_name_follows_validation(built_lib):
    p = _params()
    p.h_k = 3
    assert built_lib.fa_fwd_validate(ctypes.byref(p)) == -4
    assert built_lib.fa_fwd_plan_name(ctypes.byref(p), 256) is None
    p = _params(b=8, h=32, h_k=8, sq=1, sk=8192)  # the decode row splits: without a workspace fa_fwd refuses it
    p.workspace = None
    assert built_lib.fa_fwd_plan_name(ctypes.byref(p), 256) is None


def test_persistent_form_needs_the_cu_count(built_lib):
    """The persistent form takes chains of at least two items per CU: c2 has 2048 work items."""
    p = _params(b=4, sq=8192)
    assert b" PERSIST " in built_lib.fa_fwd_plan_name(ctypes.byref(p), 256)
    assert b" PERSIST " not in built_lib.fa_fwd_plan_name(ctypes.byref(p), 2048)
    assert b" PERSIST " not in built_lib.fa_fwd_plan_name(ctypes.byref(p), 0)


def test_fp8_paged_is_rejected(built_lib):
    """A paged cache is one of fp8_native()'s reasons to leave the native kernel, but fa_fwd_validate refuses fp8 on paged
    caches before any plan is launched: no plan name."""
    p = _paged(dtype=FP8)
    assert built_lib.fa_fwd_validate(ctypes.byref(p)) == -7
    assert built_lib.fa_fwd_plan_name(ctypes.byref(p), 256) is None


def test_last_plan_name_is_per_thread_and_follows_validation(built_lib):
    """fa_fwd_last_plan_name(): NULL on a thread that has not called fa_fwd, and NULL after a call that failed validation."""
    got = {}

    def fresh_thread():
        got["before"] = built_lib.fa_fwd_last_plan_name()
        p = _params()
        p.h_k = 3
        got["status"] = built_lib.fa_fwd(ctypes.byref(p), None)
        got["after_rejected"] = built_lib.fa_fwd_last_plan_name()
    t = threading.Thread(target=fresh_thread)
    t.start()
    t.join()
    assert got == {"before": None, "status": -4, "after_rejected": None}


# ---- the plan universe (tests/plan_universe.py) against the compiler -------------------------------------------------------

def _key_of_symbol(sym):
    """(element type, kernel key) of a mangled forward-kernel symbol; template arguments in declaration order."""
    if sym.startswith("_ZN2fa14fwd_kernel_fp8E"):
        return ("fp8", "fwd_kernel_fp8 D=128 waves=4")
    m = re.match(r"_ZN2fa\d+(fwd_kernel(?:_w64|_d256|_qv)?)I(DF16b|DF16_)((?:L[ib]\d+E)+)EEvNS_\d+\w+E$", sym)
    assert m, sym
    family, dt = m.group(1), {"DF16b": "bf16", "DF16_": "fp16"}[m.group(2)]
    a = [int(x) for x in re.findall(r"L[ib](\d+)E", m.group(3))]
    flag = lambda on, text: f" {text}" if on else ""
    if family == "fwd_kernel":  # <T, D, NWAVES, SOFTCAP, DROPOUT, DEFF, EXTRA>
        d, waves, softcap, dropout, deff, extra = a
        assert deff == d, sym
        return (dt, f"fwd_kernel D={d} waves={waves}" + flag(softcap, "SOFTCAP") + flag(dropout, "DROPOUT") + flag(extra, "EXTRA"))
    if family == "fwd_kernel_w64":  # <T, D, SOFTCAP, DEFF, PERSIST>
        d, softcap, deff, persist = a
        return (dt, f"fwd_kernel_w64 D={d} DEFF={deff} waves=4" + flag(softcap, "SOFTCAP") + flag(persist, "PERSIST"))
    if family == "fwd_kernel_d256":  # <T, W, SOFTCAP, ALIBI>
        w, softcap, alibi = a
        return (dt, f"fwd_kernel_d256 W={w} waves=4" + flag(softcap, "SOFTCAP") + flag(alibi, "ALIBI"))
    dvt, softcap = a  # fwd_kernel_qv<T, DVT, SOFTCAP>
    return (dt, f"fwd_kernel_qv DVT={dvt} waves=4" + flag(softcap, "SOFTCAP"))


def test_plan_universe_is_every_compiled_forward_kernel():
    """tests/plan_universe.py lists exactly the forward kernels the device code of fa_fwd_api.hip contains: a new template
    instantiation without a covering GPU case, or a row whose kernel is gone, fails here."""
    from device_asm import device_asm
    syms = re.findall(r"^\s*\.amdhsa_kernel (_ZN2fa\d+fwd_kernel\w*)$", open(device_asm("fa_fwd_api.hip")).read(), re.M)
    assert len(syms) == len(set(syms)) == 89
    compiled = {_key_of_symbol(s) for s in syms}
    assert len(compiled) == len(syms)
    assert compiled == set(UNIVERSE), (sorted(compiled - set(UNIVERSE)), sorted(set(UNIVERSE) - compiled))
    assert len(set(UNIVERSE.values())) == len(UNIVERSE)  # one GPU case per key


def _case_params(case, dtype):
    """The universe case as the bindings hand it to fa_fwd: the FA2 entry point plans its own split (none under dropout), the FA3
    one asks for one split; a paged cache of 256-key pages."""
    kw = dict(b=case["b"], h=case["h"], h_k=case["hk"], sq=case["sq"], sk=case["sk"], d=case["d"], d_v=case.get("dv", 0), dtype=dtype,
              is_causal=int(case.get("causal", False)), softcap=case.get("softcap", 0.0), attention_chunk=case.get("chunk", 0))
    kw["window_size_left"], kw["window_size_right"] = case.get("window", (-1, -1))
    kw["num_splits"] = 1 if case["api"] == "fa3" or case.get("dropout") else 0
    if case["api"] == "fa3":
        kw["flags"] = _lib.FA_FLAG_FA3_WINDOW
    if case.get("alibi"):
        kw["alibi_slopes"] = ADDR
    if case.get("dropout"):
        kw.update(p_dropout=case["dropout"], rng_state=ADDR)
    if case.get("qv"):
        kw.update(qv=ADDR, qv_head_stride=case["dv"], qv_row_stride=case["h"] * case["dv"], qv_batch_stride=case["sq"] * case["h"] * case["dv"])
    if case["api"] == "fa2_paged":
        kw.update(block_table=ADDR, page_block_size=256, block_table_batch_stride=16, sk=-(-case["sk"] // 256) * 256)
    return _params(**kw)


@pytest.mark.parametrize("form,case", list(FORMS.items()) + [(FP8_FORM, FP8_CASE)], ids=lambda x: x if isinstance(x, str) else "")
def test_universe_case_is_planned_on_its_kernel(built_lib, form, case):
    """Every GPU case of the universe is routed to its kernel key on a 256-CU device (the GPU test asserts the same on what
    really ran: this is the early warning in the build container)."""
    for dtype in ((FP8,) if form == FP8_FORM else (_lib.FA_DTYPE_BF16, _lib.FA_DTYPE_FP16)):
        p = _case_params(case, dtype)
        assert built_lib.fa_fwd_validate(ctypes.byref(p)) == 0
        name = built_lib.fa_fwd_plan_name(ctypes.byref(p), 256).decode()
        assert re.sub(r" (block_m|splits|cols)=\d+| fp8_expand", "", name) == form, name
