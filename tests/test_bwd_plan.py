"""CPU tests of the backward routing.  fa_bwd_plan_name() prints the kernels plan_bwd() (csrc/fa_bwd_api.hip) picks -- the
same plan fa_bwd launches from -- so that
  * tests/bwd_plan_universe.py lists exactly the backward kernels the compiled device code contains,
  * every case of the universe is planned on the kernels its row states, and
  * the shapes of the cases reach the generated loops the way the table claims (tests/bwd_run_model.py).
tests/test_bwd_plan_parity_gpu.py asserts the same plans on what really ran, and compares the gradients.

What the run model must show.  Per case whose plan has a generated loop, wherever the case's mask admits it (the reasons stand
in tests/bwd_plan_universe.py and next to the assertions); over the cases of one kernel together: everything.

    dK/dV and dQ   a generated run of length >= 3
    dK/dV and dQ   a run entered from each LDS buffer the kernel can enter from (dK/dV: both; dQ: buffer 0 -- every sweep
                   without a left window starts its run at its first key tile -- and all three behind a left window)
    dK/dV and dQ   a C++ masked tile right before a run (dQ: left window only) and a masked tile behind a run in the same
                   sweep (dQ: right behind it; dK/dV: right behind it when the last query tile is ragged)
    dK/dV and dQ   a ragged last tile (dK/dV: a wave whose 32 keys straddle seqlen_k, and a ragged last query tile where
                   seqlen_q is no multiple of 64; dQ: a last key tile of fewer than 64 keys)
    dK/dV          a run cut by the head change of a GQA group (seqlen_q a multiple of 64, no left window)
    dQ             an inactive wave (wrow >= sq)
    windows        a run limited by window_left and one limited by window_right, in both kernels
    ALiBi          no generated run at all
"""
import ctypes
import re
import threading

import pytest

import layouts
from flash_attention_annotated_amd import _lib
from bwd_plan_universe import CASES, DTYPES, LOOP_SEGMENTS, SINK_KEY, UNIVERSE, UNREACHABLE, segments, sequences
from bwd_run_model import dkdv_steps, dq_steps, neighbours, normalize_window, runs

ADDR = 0x10000  # an aligned dummy address: nothing is dereferenced
DT = {"bf16": _lib.FA_DTYPE_BF16, "fp16": _lib.FA_DTYPE_FP16}


def _params(b=2, h=4, h_k=2, sq=320, sk=462, d=128, d_v=0, dtype=_lib.FA_DTYPE_BF16, **fields):
    """Dense contiguous (b, s, h, d) tensors."""
    dv = d_v or d
    p = _lib.new_bwd_params()
    for f in ("q", "k", "v", "o", "dout", "softmax_lse", "dq", "dk", "dv", "softmax_d"):
        setattr(p, f, ADDR)
    p.b, p.seqlen_q, p.seqlen_k, p.h, p.h_k, p.d, p.d_v, p.dtype = b, sq, sk, h, h_k, d, d_v, dtype
    for t, rows, heads, width in (("q", sq, h, d), ("k", sk, h_k, d), ("v", sk, h_k, dv), ("o", sq, h, dv), ("do", sq, h, dv),
                                  ("dq", sq, h, d), ("dk", sk, h_k, d), ("dv", sk, h_k, dv)):
        setattr(p, f"{t}_head_stride", width)
        setattr(p, f"{t}_row_stride", heads * width)
        setattr(p, f"{t}_batch_stride", rows * heads * width)
    p.softmax_d_row_len = (sq + 127) // 128 * 128
    p.softmax_scale = d ** -0.5
    p.window_size_left = p.window_size_right = -1
    for k, v in fields.items():
        setattr(p, k, v)
    return p


def _case_params(case, dtype):
    """The universe case as the bindings hand it to fa_bwd."""
    kw = dict(h=case["h"], h_k=case["hk"], d=case["d"], d_v=case.get("dv", 0), dtype=dtype, is_causal=int(case.get("causal", False)),
              softcap=case.get("softcap", 0.0))
    kw["window_size_left"], kw["window_size_right"] = case.get("window", (-1, -1))
    if "lens_q" in case:
        tq, tk = sum(case["lens_q"]), sum(case["lens_k"])
        kw.update(b=len(case["lens_q"]), sq=max(case["lens_q"]), sk=max(case["lens_k"]), cu_seqlens_q=ADDR, cu_seqlens_k=ADDR,
                  total_q=tq, total_k=tk, softmax_d_row_len=tq + 128 * len(case["lens_q"]))
    else:
        kw.update(b=case["b"], sq=case["sq"], sk=case["sk"])
    if case["api"] == "fa3":
        kw["flags"] = _lib.FA_FLAG_FA3_WINDOW
    if case.get("alibi"):
        kw["alibi_slopes"] = ADDR
    if case.get("dropout"):
        kw.update(p_dropout=case["dropout"], rng_state=ADDR)
    return _params(**kw)


ROWS = [  # (id, params, plan): one row per branch of plan_bwd beside the universe's cases
    ("d32", _params(d=32), "bwd_dot LPR=8 | bwd_dkdv D=64 NB=1 DEFF=64 | bwd_dq D=64 NB=2 DEFF=64"),
    ("d72", _params(d=72), "bwd_dot LPR=16 | bwd_dkdv D=128 NB=1 DEFF=96 | bwd_dq D=128 NB=2 DEFF=96"),
    ("d104", _params(d=104), "bwd_dot LPR=16 | bwd_dkdv D=128 NB=1 DEFF=128 | bwd_dq D=128 NB=2 DEFF=128"),
    ("d96_softcap", _params(d=96, softcap=30.0),
     "bwd_dot LPR=16 | bwd_dkdv D=128 NB=1 DEFF=128 SOFTCAP | bwd_dq D=128 NB=2 DEFF=128 SOFTCAP"),
    ("d136", _params(d=136), "bwd_dot LPR=32 | bwd_dkdv D=256 NB=1 DEFF=160 PART=1 | bwd_dkdv D=256 NB=1 DEFF=160 PART=2 | "
                             "bwd_dq D=256 NB=1 DEFF=160"),
    ("d160_dropout", _params(d=160, p_dropout=0.1, rng_state=ADDR),
     "bwd_dot LPR=32 | bwd_dkdv D=256 NB=1 DEFF=256 PART=1 DROPOUT | bwd_dkdv D=256 NB=1 DEFF=256 PART=2 DROPOUT | "
     "bwd_dq D=256 NB=1 DEFF=256 DROPOUT"),
    ("d128_dv192", _params(d=128, d_v=192), "bwd_dot LPR=32 | bwd_dkdv D=256 NB=1 DEFF=192 PART=1 | "
                                            "bwd_dkdv D=256 NB=1 DEFF=192 PART=2 | bwd_dq D=256 NB=1 DEFF=192"),
    # a launch without work items has no segment
    ("no_keys", _params(sk=0, k=None, v=None, dk=None, dv=None), "bwd_dot LPR=16 | bwd_dq D=128 NB=2 DEFF=128"),
    ("no_queries", _params(sq=0), "bwd_dkdv D=128 NB=1 DEFF=128"),
    ("nothing", _params(sq=0, sk=0), ""),
]


@pytest.mark.parametrize("params,name", [r[1:] for r in ROWS], ids=[r[0] for r in ROWS])
def test_plan_name(built_lib, params, name):
    assert built_lib.fa_bwd_validate(ctypes.byref(params)) == 0
    assert built_lib.fa_bwd_plan_name(ctypes.byref(params)) == name.encode()


def test_plan_name_follows_validation(built_lib):
    p = _params()
    p.h_k = 3
    assert built_lib.fa_bwd_validate(ctypes.byref(p)) == -4
    assert built_lib.fa_bwd_plan_name(ctypes.byref(p)) is None
    assert built_lib.fa_bwd_plan_name(None) is None


def test_last_plan_name_is_per_thread_and_follows_validation(built_lib):
    """fa_bwd_last_plan_name(): NULL on a thread that has not called fa_bwd, and NULL after a call that failed validation; a call
    with neither queries nor keys launches nothing and records the empty plan."""
    got = {}

    def fresh_thread():
        got["before"] = built_lib.fa_bwd_last_plan_name()
        got["nothing"] = (built_lib.fa_bwd(ctypes.byref(_params(sq=0, sk=0)), None), built_lib.fa_bwd_last_plan_name())
        p = _params()
        p.h_k = 3
        got["status"] = built_lib.fa_bwd(ctypes.byref(p), None)
        got["after_rejected"] = built_lib.fa_bwd_last_plan_name()
    t = threading.Thread(target=fresh_thread)
    t.start()
    t.join()
    assert got == {"before": None, "nothing": (0, b""), "status": -4, "after_rejected": None}


# ---- the universe against the compiler ----------------------------------------------------------------------------------------

def _key_of_symbol(sym):
    """(element type, plan segment) of a mangled backward-kernel symbol; template arguments in declaration order."""
    if re.match(r"_ZN2fa\d+sink_grad_kernelE", sym):
        return SINK_KEY
    m = re.match(r"_ZN2fa\d+(bwd_dot_kernel|bwd_dkdv_kernel|bwd_dq_kernel)I(DF16b|DF16_)((?:L[ib]\d+E)+)EEvNS_7BParamsE$", sym)
    assert m, sym
    kernel, dt = m.group(1), {"DF16b": "bf16", "DF16_": "fp16"}[m.group(2)]
    a = [int(x) for x in re.findall(r"L[ib](\d+)E", m.group(3))]
    if kernel == "bwd_dot_kernel":  # <T, LPR>
        return (dt, f"bwd_dot LPR={a[0]}")
    d, nb, softcap, dropout, deff = a[:5]  # bwd_dkdv_kernel<T, D, NB, SOFTCAP, DROPOUT, DEFF, PART>, bwd_dq_kernel<.., DEFF>
    part = f" PART={a[5]}" if kernel == "bwd_dkdv_kernel" and a[5] else ""
    return (dt, f"{kernel[:-7]} D={d} NB={nb} DEFF={deff}{part}" + (" SOFTCAP" if softcap else "") + (" DROPOUT" if dropout else ""))


def test_universe_is_every_compiled_backward_kernel():
    """tests/bwd_plan_universe.py lists exactly the kernels the device code of fa_bwd_api.hip contains: an instantiation added
    without a covering GPU case, or a row whose kernel is gone, fails here.  Per element type: 3 bwd_dot, 18 + 2 bwd_dkdv (the
    two are UNREACHABLE: instantiated, never planned), 12 bwd_dq; plus sink_grad_kernel."""
    from device_asm import device_asm
    syms = re.findall(r"^\s*\.amdhsa_kernel (_ZN2fa\d+\w+)$", open(device_asm("fa_bwd_api.hip")).read(), re.M)
    assert len(syms) == len(set(syms))
    compiled = {_key_of_symbol(s) for s in syms}
    assert len(compiled) == len(syms)
    assert not set(UNIVERSE) & set(UNREACHABLE)
    listed = set(UNIVERSE) | set(UNREACHABLE)
    assert compiled == listed, (sorted(compiled - listed), sorted(listed - compiled))
    assert len(UNIVERSE) == 66 + 1 and len(UNREACHABLE) == 4
    for dt in DTYPES:
        count = lambda prefix: sum(1 for t, seg in UNIVERSE if t == dt and seg.startswith(prefix))  # noqa: E731
        assert (count("bwd_dot "), count("bwd_dkdv "), count("bwd_dq ")) == (3, 18, 12)
    assert all(UNIVERSE.values())  # every key names the cases that launch it


@pytest.mark.parametrize("name", list(CASES))
def test_universe_case_is_planned_on_its_plan(built_lib, name):
    """(the GPU test asserts the same on what really ran: this is the early warning in the build container)"""
    plan, case = CASES[name]
    for dt in DTYPES:
        p = _case_params(case, DT[dt])
        assert built_lib.fa_bwd_validate(ctypes.byref(p)) == 0
        assert built_lib.fa_bwd_plan_name(ctypes.byref(p)).decode() == plan


def _set_layout_strides(p, case, assignment):
    """The eight stride triples of the mixed assignment `assignment` (tests/layouts.py) in place of the contiguous ones."""
    a = layouts.ASSIGNMENTS[assignment]
    dv = case.get("dv", case["d"])
    lq, lk = ((sum(case["lens_q"]),), (sum(case["lens_k"]),)) if "lens_q" in case else ((case["b"], case["sq"]), (case["b"], case["sk"]))
    q, k, v, o = (*lq, case["h"], case["d"]), (*lk, case["hk"], case["d"]), (*lk, case["hk"], dv), (*lq, case["h"], dv)
    for n, shape in dict(q=q, k=k, v=v, o=o, do=o, dq=q, dk=k, dv=v).items():
        st = layouts.geometry(shape, 2, a[n])[2]
        for field, stride in zip(("batch", "row", "head"), st if len(shape) == 4 else (0, *st)):
            setattr(p, f"{n}_{field}_stride", stride)


# layouts plan_bwd legitimately moves to other kernels: (case, assignment) -> (plan, the rule's text).  None: plan_bwd reads no stride.
LAYOUT_MOVES = {}


@pytest.mark.parametrize("assignment", range(len(layouts.ASSIGNMENTS)))
@pytest.mark.parametrize("name", list(CASES))
def test_universe_case_keeps_its_plan_on_strided_operands(built_lib, name, assignment):
    """fa_bwd_plan_name answers the case's plan when its strides are those of a mixed assignment of tests/layouts.py."""
    plan, case = CASES[name]
    for dt in DTYPES:
        p = _case_params(case, DT[dt])
        _set_layout_strides(p, case, assignment)
        assert built_lib.fa_bwd_validate(ctypes.byref(p)) == 0
        assert built_lib.fa_bwd_plan_name(ctypes.byref(p)).decode() == LAYOUT_MOVES.get((name, assignment), (plan,))[0]


def test_every_distinct_plan_has_a_case():
    assert len({plan for plan, _ in CASES.values()}) == 13


# ---- the shapes against the run model -------------------------------------------------------------------------------------------

def _sweeps(case, plan, **kw):
    """-> ([dK/dV sweeps per sequence], [dQ sweeps per sequence]) of a case whose plan has the generated loops."""
    segs = segments(plan)
    nbk = int(re.search(r"NB=(\d)", segs[1]).group(1))
    seqs = sequences(case)
    win = normalize_window(case.get("window", (-1, -1)), case.get("causal", False), max(sk for _, sk in seqs))
    ratio = case["h"] // case["hk"]
    alibi = bool(case.get("alibi"))
    dkdv = [dkdv_steps(sq, sk, win, ratio, nbk, alibi, segs[1] in LOOP_SEGMENTS, **kw) for sq, sk in seqs if sk > 0]
    dq = [dq_steps(sq, sk, win, 2, alibi, segs[2] in LOOP_SEGMENTS) for sq, sk in seqs if sq > 0]
    return dkdv, dq, win


def _facts(case, plan, **kw):
    """What the model shows for the case: {kernel: set of facts}."""
    dkdv, dq, win = _sweeps(case, plan, **kw)
    seqs = sequences(case)
    facts = {"dkdv": set(), "dq": set()}
    for name, per_seq in (("dkdv", dkdv), ("dq", dq)):
        f = facts[name]
        for sweeps in per_seq:
            for r in runs(sweeps):
                f.add(f"enter{r.cur}")
                if r.length >= 3:
                    f.add("run3")
                if r.hi in ("head_change", "window_left", "window_right"):
                    f.add(r.hi)
                if r.lo:
                    f.add(r.lo)
            for before, _, after in neighbours(sweeps):
                if before == "masked":
                    f.add("masked_before")
                if after == "masked":
                    f.add("masked_right_behind")
            for steps in sweeps.values():
                kinds = [s.kind for s in steps]
                if "run" in kinds and "masked" in kinds[kinds.index("run"):]:
                    f.add("masked_behind")
                if name == "dq" and kinds and set(kinds) == {"skipped"}:
                    f.add("inactive_wave")
    for sq, sk in seqs:
        if sq > 0 and sk > 0:
            if sk % 32:
                facts["dkdv"].add("ragged_keys")
            if sq % 64:
                facts["dkdv"].add("ragged_queries")
            if sk % 64:
                facts["dq"].add("ragged_keys")
    return facts, win


LOOP_CASES = [n for n, (plan, case) in CASES.items() if segments(plan)[1] in LOOP_SEGMENTS and not case.get("alibi")]


@pytest.mark.parametrize("name", LOOP_CASES)
def test_run_model_of_loop_cases(name):
    plan, case = CASES[name]
    facts, win = _facts(case, plan)
    seqs = [(sq, sk) for sq, sk in sequences(case) if sq and sk]
    left = win[0] >= 0
    want_k = {"run3", "enter0", "enter1", "masked_before", "masked_behind", "ragged_keys"}
    want_q = {"run3", "enter0", "masked_right_behind", "ragged_keys", "inactive_wave"}
    if any(sq % 64 for sq, _ in seqs):       # a ragged last query tile: masked, right behind the run of the full tiles
        want_k |= {"ragged_queries", "masked_right_behind"}
    if not left and any(sq % 64 == 0 for sq, _ in seqs):  # the head's last query tile is plain: only the head change ends the run
        want_k.add("head_change")
    if left:                                 # sweeps start behind key 0: masked tiles in front of the run, entries from every slot
        want_k |= {"window_left", "window_right"}
        want_q |= {"window_left", "window_right", "enter1", "enter2", "masked_before"}
    assert want_k <= facts["dkdv"], (name, "dK/dV", sorted(want_k - facts["dkdv"]))
    assert want_q <= facts["dq"], (name, "dQ", sorted(want_q - facts["dq"]))
    if not left:  # (why the table asks for buffer 0 only there)
        assert not {"enter1", "enter2", "masked_before"} & facts["dq"]


@pytest.mark.parametrize("segment", sorted(LOOP_SEGMENTS))
def test_run_model_of_loop_kernels(segment):
    """Over the cases that launch one generated-loop kernel: every fact of the table."""
    names = [n for n in LOOP_CASES if segment in segments(CASES[n][0])]
    assert len(names) >= 2
    kernel = "dkdv" if segment.startswith("bwd_dkdv") else "dq"
    seen = set().union(*(_facts(CASES[n][1], CASES[n][0])[0][kernel] for n in names))
    want = {"dkdv": {"run3", "enter0", "enter1", "masked_before", "masked_behind", "masked_right_behind", "ragged_keys", "ragged_queries",
                     "head_change", "window_left", "window_right"},
            "dq": {"run3", "enter0", "enter1", "enter2", "masked_before", "masked_right_behind", "ragged_keys", "inactive_wave",
                   "window_left", "window_right"}}[kernel]
    assert want <= seen, (segment, sorted(want - seen))


@pytest.mark.parametrize("name", [n for n, (_, c) in CASES.items() if c.get("alibi")])
def test_run_model_alibi_never_enters_the_loop(name):
    plan, case = CASES[name]
    dkdv, dq, _ = _sweeps(case, plan)
    assert not any(runs(s) for s in dkdv + dq)
    assert segments(plan)[2] in LOOP_SEGMENTS  # the dQ instantiation has the loop
    if name == "d128_alibi":  # so has the dK/dV one, and the same shape without ALiBi enters both
        assert segments(plan)[1] in LOOP_SEGMENTS
        dkdv, dq, _ = _sweeps(dict(case, alibi=False), plan)
        assert any(runs(s) for s in dkdv) and any(runs(s) for s in dq)


def test_run_model_every_run_has_a_successor_of_its_head():
    """count = min(plain, left - 1): the tile behind a run belongs to the run's head (the loop prefetches it through the head's
    buffer descriptors), and in the aligned cases that rule, not a mask, is what ends the run."""
    for name in LOOP_CASES:
        plan, case = CASES[name]
        for sweeps in _sweeps(case, plan)[0]:
            for steps in sweeps.values():
                for i, s in enumerate(steps):
                    if s.kind == "run":
                        assert i + 1 < len(steps) and steps[i + 1].head == s.head, (name, s)
    assert "head_change" in _facts(CASES["d128"][1], CASES["d128"][0])[0]["dkdv"]
