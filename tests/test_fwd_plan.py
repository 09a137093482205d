"""CPU tests of the forward routing: fa_fwd_plan_name() names the kernel plan_fwd() (csrc/fa_fwd_api.hip) picks -- family,
template shape and forms, block_m, split-KV, fp8 expansion, 256-column calls.  One row per branch of the routing, on a
device of 256 CUs; tests/test_persistent_gpu.py and the GPU suite check that the named kernels compute the right thing."""
import ctypes
import re
import threading

import pytest

from flash_attention_annotated_amd import _lib
import layouts
import plan_universe
from parity_helpers import plan_key, sparse_lists
from plan_universe import AUX, AUX_STRIDED, EPILOGUES, FORMS, FP8_FORM, UNIVERSE, UNREACHABLE, cases, case_id

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

FAMILY = r"_ZN2fa\d+(?:pk_|bs_)?fwd_kernel"  # fwd_kernel, fwd_kernel_w64 / _d256 / _qv / _fp8, pk_fwd_kernel, bs_fwd_kernel
TYPES = {"DF16b": "bf16", "DF16_": "fp16", "f": "fp32"}


def _key_of_symbol(sym):
    """(element type, kernel form) of a mangled forward-kernel symbol; template arguments in declaration order."""
    if sym.startswith("_ZN2fa14fwd_kernel_fp8E"):
        return ("fp8", "fwd_kernel_fp8 D=128 waves=4")
    m = re.match(r"_ZN2fa\d+((?:pk_|bs_)?fwd_kernel(?:_w64|_d256|_qv)?)I(DF16b|DF16_)((?:L[ib]\d+E)+)EEvNS_\d+\w+E$", sym)
    assert m, sym
    family, dt = m.group(1), TYPES[m.group(2)]
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
    if family in ("pk_fwd_kernel", "bs_fwd_kernel"):  # <T, D, SOFTCAP>, 4 waves each (PK_NWAVES, BS_NWAVES)
        d, softcap = a
        return (dt, f"{family} D={d} waves=4" + flag(softcap, "SOFTCAP"))
    assert family == "fwd_kernel_qv", sym
    dvt, softcap = a  # fwd_kernel_qv<T, DVT, SOFTCAP>
    return (dt, f"fwd_kernel_qv DVT={dvt} waves=4" + flag(softcap, "SOFTCAP"))


def _kernel_symbols():
    """(symbols of the forward kernel families, every other kernel symbol) of the device code of fa_fwd_api.hip."""
    from device_asm import device_asm
    syms = re.findall(r"^\s*\.amdhsa_kernel (\S+)$", open(device_asm("fa_fwd_api.hip")).read(), re.M)
    assert len(syms) == len(set(syms))
    return [s for s in syms if re.match(FAMILY, s)], [s for s in syms if not re.match(FAMILY, s)]


def test_plan_universe_is_every_compiled_forward_kernel():
    """tests/plan_universe.py lists exactly the forward kernels the device code of fa_fwd_api.hip contains -- 89 of the fwd_kernel
    families, 8 of pk_fwd_kernel, 12 of bs_fwd_kernel --, each with both epilogues: a new template instantiation without a
    covering GPU case, or a row whose kernel is gone, fails here."""
    syms, _ = _kernel_symbols()
    assert len(syms) == 89 + 8 + 12 == 109
    assert sum("pk_fwd_kernel" in s for s in syms) == 8 and sum("bs_fwd_kernel" in s for s in syms) == 12
    compiled = {_key_of_symbol(s) for s in syms}
    assert len(compiled) == len(syms)
    listed = {(dt, form) for dt, form, _ in UNIVERSE}
    assert compiled == listed, (sorted(compiled - listed), sorted(listed - compiled))
    # every instantiation has its two store paths accounted for: a GPU case each, or a rule in UNREACHABLE
    assert set(UNIVERSE) == {(dt, form, ep) for dt, form in compiled for ep in EPILOGUES}
    assert len(set(v for v in UNIVERSE.values() if not v.startswith("unreachable: "))) == len(UNIVERSE) - sum(
        v.startswith("unreachable: ") for v in UNIVERSE.values())  # one GPU case per key
    ids = [case_id(form, ep, dt) for form, ep, dt, _ in cases()]
    assert len(set(ids)) == len(ids) == len(UNIVERSE) - len({k for k in UNIVERSE if (k[1], k[2]) in UNREACHABLE})
    assert not [k for k in UNREACHABLE if k[1] in FORMS.get(k[0], {})], "a case and an UNREACHABLE rule for one key"


def _aux_of_symbol(sym):
    """(kernel name, element type or None) of a kernel outside the forward families: `_ZN12_GLOBAL__N_1<len><name>[I<T>E]...`."""
    m = re.match(r"_ZN12_GLOBAL__N_1(\d+)", sym)
    assert m, sym
    name, rest = sym[m.end():m.end() + int(m.group(1))], sym[m.end() + int(m.group(1)):]
    t = re.match(r"I(DF16b|DF16_|f)E", rest)
    assert t or rest.startswith("E"), sym  # one type argument, or no template
    return (name, TYPES[t.group(1)] if t else None)


def test_every_other_forward_kernel_is_named_in_aux():
    """The kernels of the forward device code are the universe's families plus the keys of AUX, in every element type each is
    instantiated for: a new kernel in csrc/fa_fwd_api.hip without a test that names it fails here, and so does an entry whose
    kernel is gone."""
    _, others = _kernel_symbols()
    compiled = {_aux_of_symbol(s) for s in others}
    assert len(compiled) == len(others) == 16
    listed = {(name, dt) for name, (_, types) in AUX.items() for dt in (types or (None,))}
    assert compiled == listed, (sorted(compiled - listed, key=str), sorted(listed - compiled, key=str))


@pytest.mark.parametrize("kernel", list(AUX_STRIDED))
def test_aux_strided_test_exists(kernel):
    import importlib
    assert kernel in AUX
    path, _, name = AUX_STRIDED[kernel].partition("::")
    module = importlib.import_module(path[len("tests/"):-len(".py")])
    assert callable(getattr(module, name, None)), f"{AUX_STRIDED[kernel]} does not exist"
    assert "gpu" in [m.name for m in [getattr(module, "pytestmark", None)] if m is not None]


@pytest.mark.parametrize("kernel", list(AUX))
def test_aux_test_exists(kernel):
    import importlib
    path, _, name = AUX[kernel][0].partition("::")
    assert path.startswith("tests/") and path.endswith("_gpu.py"), path
    module = importlib.import_module(path[len("tests/"):-len(".py")])
    test = getattr(module, name, None)
    assert callable(test), f"{AUX[kernel][0]} does not exist"
    marks = getattr(module, "pytestmark", None)
    assert "gpu" in [m.name for m in (marks if isinstance(marks, list) else [marks]) if m is not None]


def _case_params(case, dtype, num_splits=None):
    """The universe case as the bindings hand it to fa_fwd: the FA2 entry point plans its own split (none under dropout), the FA3
    one asks for one split, the cache entry points and the cute surface hand on their `num_splits`; a paged cache of 256-key
    pages; the FA3 cache route behind a cache_batch_idx (seqused_k + kv_batch_idx, the FA2 window rule).  `num_splits`
    overrides the entry point's (the UNREACHABLE rules)."""
    api = case["api"]
    kw = dict(b=case["b"], h=case["h"], h_k=case["hk"], sq=case["sq"], sk=case["sk"], d=case["d"], d_v=case.get("dv", 0), dtype=dtype,
              is_causal=int(case.get("causal", False)), softcap=case.get("softcap", 0.0), attention_chunk=case.get("chunk", 0))
    kw["window_size_left"], kw["window_size_right"] = case.get("window", (-1, -1))
    if api == "fa2":
        kw["num_splits"] = 1 if case.get("dropout") else 0
    elif api == "fa3":
        kw["num_splits"] = 1
    else:
        kw["num_splits"] = case.get("splits", 0 if api == "fa2_paged" else 1)
    if num_splits is not None:
        kw["num_splits"] = num_splits
    kw["flags"] = (_lib.FA_FLAG_FA3_WINDOW if api in ("fa3", "cute", "bs") else 0) | (_lib.FA_FLAG_PACK_GQA if case.get("pack") else 0)
    if case.get("alibi"):
        kw["alibi_slopes"] = ADDR
    if case.get("dropout"):
        kw.update(p_dropout=case["dropout"], rng_state=ADDR)
    if case.get("qv"):
        kw.update(qv=ADDR, qv_head_stride=case["dv"], qv_row_stride=case["h"] * case["dv"], qv_batch_stride=case["sq"] * case["h"] * case["dv"])
    if api == "fa2_paged":
        kw.update(block_table=ADDR, page_block_size=256, block_table_batch_stride=16, sk=-(-case["sk"] // 256) * 256)
    if api == "fa3_cache":
        kw.update(seqused_k=ADDR, kv_batch_idx=ADDR)
    return _params(**kw)


def _dtypes(form):
    return (("fp8", FP8),) if form == FP8_FORM else (("bf16", _lib.FA_DTYPE_BF16), ("fp16", _lib.FA_DTYPE_FP16))


PLANNED = [(form if ep == "direct" else f"{form} partial", case) for form, ep, dt, case in cases() if dt != "fp16"]


@pytest.mark.parametrize("form,case", PLANNED, ids=lambda x: x if isinstance(x, str) else "")
def test_universe_case_is_planned_on_its_kernel(built_lib, form, case):
    """Every GPU case of the universe is routed to its kernel key -- form and epilogue -- on a 256-CU device (the GPU test
    asserts the same on what really ran: this is the early warning in the build container), and keeps the shape rules of the
    table.  The pk rows are planned with FA_FLAG_PACK_GQA.  The bs rows have no fa_fwd_params plan -- fa_fwd_block_sparse
    launches its one kernel shape without plan_fwd -- so only their shape is checked here."""
    form, ep = (form[:-len(" partial")], "partial") if form.endswith(" partial") else (form, "direct")
    sq, sk = case["sq"], case["sk"]
    assert sk // 64 >= 3 and (sk % 64 != 0 or " PERSIST" in form)
    if case["api"] == "bs":
        assert ep == "direct" and sq % 128 != 0 and sk % 128 > 64
        return
    for dt, dtype in _dtypes(form):
        p = _case_params(case, dtype)
        assert built_lib.fa_fwd_validate(ctypes.byref(p)) == 0
        name = built_lib.fa_fwd_plan_name(ctypes.byref(p), 256).decode()
        assert plan_key(name, dt) == (dt, form, ep), name
        assert sq % int(re.search(r"block_m=(\d+)", name).group(1)) != 0
        splits = int(re.search(r"splits=(\d+)", name).group(1))
        if ep == "partial":  # thirds of a row block's key tiles: every part owns full tiles
            assert splits == 3 and -(-sk // 64) // splits >= 3, name


def _set_layout_strides(p, case, assignment, itemsize=2, names=("q", "k", "v", "o", "qv")):
    """The strides of the mixed assignment `assignment` (tests/layouts.py) in place of the contiguous ones."""
    a = layouts.ASSIGNMENTS[assignment]
    b, dv, paged = case["b"], case.get("dv", case["d"]), case["api"] == "fa2_paged"
    kv = (b * -(-case["sk"] // 256), 256) if paged else (b, case["sk"])
    shapes = dict(q=(b, case["sq"], case["h"], case["d"]), k=(*kv, case["hk"], case["d"]), v=(*kv, case["hk"], dv),
                  o=(b, case["sq"], case["h"], dv), qv=(b, case["sq"], case["h"], dv))
    for n in names:
        if n == "qv" and not case.get("qv"):
            continue
        key = f"{n}_pages" if paged and n in "kv" else n
        st = layouts.geometry(shapes[n], 2 if n == "o" and itemsize == 1 else itemsize, a[key])[2]
        for field, stride in zip(("batch", "row", "head"), st):
            setattr(p, f"{n}_{field}_stride", stride)


# layouts the routing legitimately moves to another form: (form, epilogue, assignment) -> (form it moves to, the rule's text).
# None today: at the universe's shapes the extent guards of persist_ok / d256_ok (32-bit offsets) hold for every layout.
LAYOUT_MOVES = {}


@pytest.mark.parametrize("assignment", range(len(layouts.ASSIGNMENTS)))
@pytest.mark.parametrize("form,case", [(f, c) for f, c in PLANNED if c["api"] != "bs"], ids=lambda x: x if isinstance(x, str) else "")
def test_universe_case_keeps_its_plan_on_strided_operands(built_lib, form, case, assignment):
    """fa_fwd_plan_name answers the same text when the strides of a universe case are those of a mixed assignment of
    tests/layouts.py (LAYOUT_MOVES lists the exceptions with their rule; tests/test_layout_parity_gpu.py runs them)."""
    form, ep = (form[:-len(" partial")], "partial") if form.endswith(" partial") else (form, "direct")
    for dt, dtype in _dtypes(form):
        p = _case_params(case, dtype)
        if dt == "fp8":  # (the bindings always hand over the descales' own strides)
            for n in "qkv":
                setattr(p, f"{n}_descale", ADDR)
                setattr(p, f"{n}_descale_batch_stride", case["hk"])
                setattr(p, f"{n}_descale_head_stride", 1)
        want = built_lib.fa_fwd_plan_name(ctypes.byref(p), 256).decode()
        _set_layout_strides(p, case, assignment, 1 if dt == "fp8" else 2)
        if dt == "fp8":  # a row-padded, a transposed and a padded transposed table, as tests/test_layout_parity_gpu.py::_descale
            for n, (bs, hs) in zip("qkv", ((case["hk"] + 3, 1), (1, case["b"] + 3), (1, case["b"] + 3))):
                setattr(p, f"{n}_descale_batch_stride", bs)
                setattr(p, f"{n}_descale_head_stride", hs)
        assert built_lib.fa_fwd_validate(ctypes.byref(p)) == 0
        name = built_lib.fa_fwd_plan_name(ctypes.byref(p), 256).decode()
        moved = LAYOUT_MOVES.get((form, ep, assignment))
        if moved:
            assert plan_key(name, dt) == (dt, moved[0], ep), name
        else:
            assert name == want, f"{want!r} on contiguous operands"


def _sparse_params(case):
    """fa_block_sparse_params of a universe block-sparse case: dummy list addresses, the strides of contiguous (b, h, nm[, nk])."""
    nm, nk = -(-case["sq"] // 128), -(-case["sk"] // 128)
    s = _lib.new_block_sparse_params()
    s.mask_block_cnt, s.mask_block_idx, s.full_block_cnt, s.full_block_idx = ADDR, ADDR + 4096, ADDR + 8192, ADDR + 12288
    for name in ("mask", "full"):
        getattr(s, f"{name}_cnt_stride")[:] = [case["h"] * nm, nm, 1, 0]
        getattr(s, f"{name}_idx_stride")[:] = [case["h"] * nm * nk, nm * nk, nk, 1]
    return s


@pytest.mark.parametrize("assignment", range(len(layouts.ASSIGNMENTS)))
@pytest.mark.parametrize("form", [f for f in FORMS if f.startswith("bs_fwd_kernel ")])
def test_block_sparse_case_validates_on_strided_operands(built_lib, form, assignment):
    """The block-sparse cases have no fa_fwd_params plan (one kernel shape): fa_fwd_block_sparse_validate accepts their params with
    the strides of each mixed assignment, as it does the contiguous ones."""
    case = FORMS[form]["direct"]
    for _, dtype in _dtypes(form):
        p = _case_params(case, dtype)
        assert built_lib.fa_fwd_block_sparse_validate(ctypes.byref(p), ctypes.byref(_sparse_params(case)), None) == 0
        _set_layout_strides(p, case, assignment)
        assert built_lib.fa_fwd_block_sparse_validate(ctypes.byref(p), ctypes.byref(_sparse_params(case)), None) == 0


@pytest.mark.parametrize("form,ep", list(UNREACHABLE), ids=[case_id(f, ep, "") for f, ep in UNREACHABLE])
def test_unreachable_epilogue_is_forbidden_by_its_rule(built_lib, form, ep):
    """Every (form, epilogue) the universe lists without a case: the form's own case, asked for num_splits = 3, does what the
    rule says (plan_universe.UNREACHABLE) -- at the C ABI, so no caller of any kind reaches the key."""
    how, rule, target = UNREACHABLE[(form, ep)]
    assert ep == "partial" and rule and (target is not None) == (how == "moves")
    case = plan_universe.FP8_CASE if form == FP8_FORM else FORMS[form]["direct"]
    for dt, dtype in _dtypes(form):
        if how == "refused":  # block lists: the split is what fa_fwd_block_sparse refuses
            for n, status in ((0, 0), (1, 0), (3, -7)):
                p = _case_params(case, dtype, num_splits=n)
                assert built_lib.fa_fwd_block_sparse_validate(ctypes.byref(p), ctypes.byref(_sparse_params(case)), None) == status
            continue
        p = _case_params(case, dtype, num_splits=3)
        assert built_lib.fa_fwd_validate(ctypes.byref(p)) == 0
        key = plan_key(built_lib.fa_fwd_plan_name(ctypes.byref(p), 256).decode(), dt)
        if how == "splits=1":
            assert key == (dt, form, "direct"), key
            p.num_splits = 0  # ... and the heuristic does not split it either
            assert plan_key(built_lib.fa_fwd_plan_name(ctypes.byref(p), 256).decode(), dt) == (dt, form, "direct")
            if dt != "fp8":  # (no partials to hold; an fp8 call outside the native kernel keeps its expansion workspace)
                assert built_lib.fa_fwd_workspace_size(ctypes.byref(p)) == 0
        else:
            assert how == "moves" and target != form and key == (dt, target, "partial"), key
            assert not UNIVERSE[key].startswith("unreachable"), key  # the partial store it lands on has a GPU case


def test_block_sparse_case_lists():
    """What the universe's block-sparse case needs of its seeded lists (plan_universe.SPARSE), under its causal mask (bottom-right
    aligned: query block m ends at key 415 + 128 m + 127): a query block that lists at least three blocks in its full list, a
    mask-list block the diagonal cuts, the ragged last key block visited where the mask leaves it keys, a query block with a
    shorter list than each of its neighbours, lists that differ inside a GQA group and between the batches, and rows without a
    visible key (the keyless-row convention: O = 0, LSE = +inf) that no other (batch, head) shares."""
    import torch
    case = plan_universe.SPARSE
    (fc, fi, mc, mi), visited = sparse_lists(case)
    b, h, nm, nk = visited.shape
    sq, sk = case["sq"], case["sk"]
    assert (nm, nk) == (3, 6) and sk % 128 != 0 and case["h"] // case["hk"] == 2
    i, j = torch.arange(sq).view(-1, 1) + sk - sq, torch.arange(sk).view(1, -1)
    ok = torch.zeros(nm * 128, nk * 128, dtype=torch.bool)
    ok[:sq, :sk] = j <= i
    real = torch.zeros_like(ok)
    real[:sq, :sk] = True
    blk = lambda t: t.view(nm, 128, nk, 128).permute(0, 2, 1, 3).reshape(nm, nk, -1)  # noqa: E731
    some, every = blk(ok).any(-1), (blk(ok) | ~blk(real)).all(-1)
    diagonal = some & ~every
    assert diagonal.sum(-1).tolist() == [2, 2, 1]
    import block_sparse_oracle as bso
    in_full = bso.block_mask_from_lists(None, None, fc, fi, b, h)
    in_mask = visited & ~in_full
    assert ((in_full & every).sum(-1) >= 3).any(), "no query block with three unmasked blocks in its full list"
    assert (in_mask & diagonal).any(), "no mask-list block on the causal diagonal"
    assert (visited[:, :, 1:, nk - 1]).any(), "the ragged last key block is never visited where the mask leaves it keys"
    n = visited.sum(-1)
    shorter = [(n[..., 0] < n[..., 1]), (n[..., 1] < n[..., 0]) & (n[..., 1] < n[..., 2]), (n[..., 2] < n[..., 1])]
    assert any(s.any() for s in shorter)
    assert (n >= 1).all() and (n <= nk - 1).all()
    assert not torch.equal(visited[:, 0], visited[:, 1]) and not torch.equal(visited[0], visited[1])
    keyless = ~(bso.dense_mask(visited, sq, sk) & ok[:sq, :sk]).any(-1)  # rows whose visited blocks the mask empties
    assert keyless.any() and not keyless.all(0).all(0).any()
