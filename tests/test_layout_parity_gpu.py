"""Every forward and backward kernel key on strided operands: the cases of tests/plan_universe.py, tests/kv8_plan_universe.py and
tests/bwd_plan_universe.py, each run twice through the op beneath its public entry point that takes the caller's outputs --
once on contiguous operands, once on the views of a mixed assignment of tests/layouts.py (padded and (b, h, s, d)-ordered
storage, a different stride triple per operand, NaN between and around the inputs, a sentinel byte around the outputs).  Both
runs execute the same instantiation on the same values in the same order (the dropout decision is a hash of indices under one
seed), so the comparison is bitwise, not a tolerance:

    the plan text of both runs is the same and its kernel key / plan is the case's;
    torch.equal on out and softmax_lse (forward; S_dmask too under dropout), on dq / dk / dv (/ dsink) (backward);
    every element of an output allocation outside the view still holds the sentinel; every input allocation is unchanged.

No oracle is evaluated here: tests/test_plan_parity_gpu.py, tests/test_kv8_plan_parity_gpu.py and
tests/test_bwd_plan_parity_gpu.py compare the contiguous run with it.  What a layout cannot reach:
  * cute_fwd / cute_bwd (csrc/torch_binding.cpp) take no out / dq / dk / dv.  The PackGQA partial case of the cute surface runs
    through torch.ops.flash_attn_3.fwd behind an identity kv_batch_idx instead, which takes `out` and the same num_splits /
    pack_gqa and reaches the same key (asserted).  The sink backward runs cute_bwd on contiguous operands and, on the strided
    ones, the two calls cute_bwd is made of -- torch.ops.flash_attn_3.bwd (deterministic, as there) with the caller's dq / dk /
    dv, then sink_grad on its softmax_d -- so that sink_grad_kernel's neighbours write strided gradients.  The block-sparse
    cases pass the caller's `out` to cute_fwd_block_sparse.
  * page pools are padded views in both assignments (a (pages, hk, page, d) pool is a padded-family view as well).
Each case appends one JSON line (case, assignment, plan, equal) to the file FA_LAYOUT_PARITY_JSONL names
(profiles/layout_parity.jsonl holds such a run).  The two closing tests assert that the keys seen on strided operands are the
universes minus UNREACHABLE."""
import itertools
import json
import os

import pytest
import torch

import bwd_plan_universe as bwdu
import kv8_plan_universe as kv8u
import layouts as L
import plan_universe as fwdu
import test_plan_parity_gpu as fwdp
from parity_helpers import FP8, kernel_key, last_bwd_plan, last_plan, sparse_lists
from test_kv8_kvcache_gpu import Case as Kv8Case
from test_qv8_kvcache_gpu import Case as Qv8Case

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp8": FP8}
ASSIGN = range(len(L.ASSIGNMENTS))
JSONL = "FA_LAYOUT_PARITY_JSONL"
SEEN_FWD, SEEN_KV8, SEEN_BWD = set(), set(), set()  # kernel keys launched on strided operands in this session


def _emit(cid, assignment, plan, equal):
    line = json.dumps(dict(case=cid, assignment=assignment, plan=plan, equal=bool(equal)))
    print(line)
    if os.environ.get(JSONL):
        with open(os.environ[JSONL], "a") as f:
            f.write(line + "\n")


def _place(t, names, assignment, slack):
    """{name: Placed} of the CPU tensors t[name] under the assignment's layouts."""
    return {n: L.place_input(t[n], L.ASSIGNMENTS[assignment][names[n]], DEV, slack) for n in names if n in t}


def _descale(x, kind):
    """A (b, hk) fp32 table with other strides: 0 a row-padded view, 1 a transposed one, 2 both."""
    b, hk = x.shape
    big = torch.full((hk + 2, b + 3) if kind else (b + 2, hk + 3), float("nan"))
    view = big[1:hk + 1, 2:b + 2].t() if kind == 1 else big[:hk, :b].t() if kind == 2 else big[1:b + 1, 1:hk + 1]
    view.copy_(x)
    big = big.to(DEV)
    return big.as_strided(view.shape, view.stride(), view.storage_offset())


def _same(a, b):
    """Bitwise equality of two tensors of one type (NaN-safe)."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if not a.is_floating_point():
        return torch.equal(a, b)
    return torch.equal(a.contiguous().view(L.INT[a.element_size()]), b.contiguous().view(L.INT[b.element_size()]))


def _untouched(placed, t):
    for n, p in placed.items():
        assert p.holds(t[n]) and p.intact(), f"input {n} ({p.layout}) was written"


# ---- forward: tests/plan_universe.py ------------------------------------------------------------------------------------------

def _fwd_call(case, ops, out, seed):
    """The op beneath the case's entry point -> (out, lse, extra tensors to compare)."""
    import flash_attention_annotated_amd  # noqa: F401
    from flash_attention_annotated_amd import _lib, flash_attn_2_cuda, flash_attn_3_ops  # noqa: F401
    api, q, k, v = case["api"], ops["q"], ops["k"], ops["v"]
    causal, (wl, wr), softcap = case.get("causal", False), case.get("window", (-1, -1)), case.get("softcap", 0.0)
    b, d = q.shape[0], q.shape[-1]
    if api in ("fa3", "fa3_cache", "cute"):
        qv = ops.get("qv")
        scale = (d + (qv.shape[-1] if qv is not None else 0)) ** -0.5
        cache = api != "fa3"  # (any cache argument takes the KV-cache route: an identity kv_batch_idx over full caches)
        seqused = torch.full((b,), case["sk"], dtype=torch.int32, device=DEV) if cache else None
        idx = torch.arange(b, dtype=torch.int32, device=DEV) if cache else None
        o, lse, *_ = torch.ops.flash_attn_3.fwd(
            q, k, v, None, None, qv, out, None, None, None, None, seqused, None, None, None, idx, None, None, None, None,
            ops.get("q_descale"), ops.get("k_descale"), ops.get("v_descale"), scale, causal, wl, wr, case.get("chunk", 0), softcap,
            True, None, case["splits"] if cache else 1, case.get("pack"), 0)
        return o, lse, []
    scale = d ** -0.5
    if api == "bs":
        o, lse = _lib.binding().cute_fwd_block_sparse(q, k, v, scale, causal, -1, -1, None, softcap, 1, *ops["lists"], out=out)
        return o, lse, []
    if api == "fa2_paged":
        o, lse = flash_attn_2_cuda.fwd_kvcache(q, k, v, None, None, ops["seqlens"], None, None, None, None, ops["table"], None, out, scale,
                                               causal, wl, wr, softcap, True, case.get("splits", 0))
        return o, lse, []
    if api == "fa2_cache":
        o, lse = flash_attn_2_cuda.fwd_kvcache(q, k, v, None, None, None, None, None, None, None, None, ops.get("slopes"), out, scale,
                                               causal, wl, wr, softcap, True, case["splits"])
        return o, lse, []
    assert api == "fa2", api
    p_drop = case.get("dropout", 0.0)
    torch.manual_seed(seed)  # (the binding draws the dropout (seed, offset) from the default generator)
    o, lse, S, rng = flash_attn_2_cuda.fwd(q, k, v, out, ops.get("slopes"), p_drop, scale, causal, wl, wr, softcap, p_drop > 0, None)
    return o, lse, [S, rng]


def _fwd_operands(case, dtype, seed):
    """-> (CPU tensors by operand name, {operand: key of the assignment}, small device tensors both runs share)."""
    t = fwdp._inputs(case, dtype, seed)
    if dtype == FP8:
        t.update({n: t[n].to(FP8) for n in "qkv"})
    names = dict(q="q", k="k", v="v", qv="qv")
    shared = {}
    if case["api"] == "fa2_paged":
        t["k"], table = fwdp._paged(t["k"], seed)
        t["v"], _ = fwdp._paged(t["v"], seed)
        names.update(k="k_pages", v="v_pages")
        shared.update(table=table.to(DEV), seqlens=torch.tensor([case["sk"] - 115 * (i % 2) for i in range(case["b"])], dtype=torch.int32,
                                                                 device=DEV))
    if case["api"] == "bs":
        shared["lists"] = [x.to(DEV) for x in sparse_lists(case)[0]]
    if "slopes" in t:
        shared["slopes"] = t.pop("slopes").to(DEV)
    return t, names, shared


@pytest.mark.parametrize("assignment", ASSIGN)
@pytest.mark.parametrize("form,ep,dt,case", fwdp.CASES, ids=[fwdu.case_id(f, ep, dt) for f, ep, dt, _ in fwdp.CASES])
def test_fwd_layout_parity(form, ep, dt, case, assignment):
    dtype = DTYPES[dt]
    seed = sum(ord(c) for c in form + ep + dt)
    t, names, shared = _fwd_operands(case, dtype, seed)
    desc = {n: t.pop(n) for n in ("q_descale", "k_descale", "v_descale") if n in t}
    out_shape = (*t["q"].shape[:-1], t["v"].shape[-1])
    out_dtype = torch.bfloat16 if dtype == FP8 else dtype

    ops = {n: x.to(DEV) for n, x in t.items()}
    ops.update(shared, **{n: x.to(DEV) for n, x in desc.items()})
    out0, lse0, extra0 = _fwd_call(case, ops, None, seed)
    plan0 = last_plan()
    assert kernel_key(plan0, dtype) == (dt, form, ep), f"contiguous run planned {plan0!r}"

    slack = L.call_slack([x.shape for x in t.values()] + [out_shape], 1 if dtype == FP8 else 2)
    placed = _place(t, names, assignment, slack)
    out = L.place_output(out_shape, out_dtype, L.ASSIGNMENTS[assignment]["o"], DEV, slack)
    ops = {n: p.view for n, p in placed.items()}
    ops.update(shared, **{n: _descale(x, (i + assignment) % 3) for i, (n, x) in enumerate(desc.items())})
    out1, lse1, extra1 = _fwd_call(case, ops, out.view, seed)
    plan1 = last_plan()
    SEEN_FWD.add(kernel_key(plan1, dtype))

    equal = _same(out1, out0) and _same(lse1, lse0) and all(_same(a, b) for a, b in zip(extra1, extra0))
    _emit(fwdu.case_id(form, ep, dt), assignment, plan1, equal)
    assert plan1 == plan0, f"strided operands planned {plan1!r}, contiguous ones {plan0!r}"
    assert out1.data_ptr() == out.view.data_ptr() and out1.stride() == out.view.stride(), "the result is not in the caller's out"
    assert out.view.stride() != placed["q"].view.stride() and not out.view.is_contiguous()
    assert out.intact(), "sentinels around the caller's out were overwritten"
    _untouched(placed, t)
    assert _same(out1, out0), f"out differs from the contiguous run in {int((out1 != out0).sum())} elements"
    assert _same(lse1, lse0), "softmax_lse differs from the contiguous run"
    assert equal, "S_dmask / rng_state differ from the contiguous run"


# ---- forward over an fp8 KV cache: tests/kv8_plan_universe.py -----------------------------------------------------------------

def _kv8_call(c, case, ops, out):
    qv = ops.get("qv")
    scale = (c.q.shape[-1] + (qv.shape[-1] if qv is not None else 0)) ** -0.5
    o, lse, *_ = torch.ops.flash_attn_3.fwd(
        ops["q"], ops["k"], ops["v"], None, None, qv, out, None, None, None, None, ops["lens"], None, None, None, None, None, None, None,
        None, None, ops["k_descale"], ops["v_descale"], scale, c.causal, c.window[0], c.window[1], 0, c.softcap, True, None,
        case["splits"], None, 0)
    return o, lse


KV8_CASES = kv8u.cases()


@pytest.mark.parametrize("assignment", ASSIGN)
@pytest.mark.parametrize("form,ep,dt,case", KV8_CASES, ids=[kv8u.case_id(f, ep, dt) for f, ep, dt, _ in KV8_CASES])
def test_kv8_layout_parity(form, ep, dt, case, assignment):
    import flash_attention_annotated_amd  # noqa: F401
    from flash_attention_annotated_amd import flash_attn_3_ops  # noqa: F401
    kernel, dtype = case["kernel"], DTYPES[dt]
    seed = sum(ord(ch) for ch in form + ep + dt)
    kw = dict(dtype=dtype, b=case["b"], sq=case["sq"], h=case["h"], hk=case["hk"], d=case["d"], cap=case["cap"], lens=case["lens"],
              causal=case["causal"], softcap=case.get("softcap", 0.0), seed=seed)
    c = Kv8Case(**kw) if kernel == "kv8" else Qv8Case(dv=case["dv"], **kw)
    t = dict(q=c.q, k=c.k8, v=c.v8)
    if getattr(c, "qv", None) is not None:
        t["qv"] = c.qv
    out_shape = (*c.q.shape[:-1], c.v8.shape[-1])
    lens = c.lens.to(DEV)

    ops = {n: x.to(DEV) for n, x in t.items()}
    ops.update(lens=lens, k_descale=c.kdesc.to(DEV), v_descale=c.vdesc.to(DEV))
    out0, lse0 = _kv8_call(c, case, ops, None)
    plan0 = last_plan()
    assert kernel_key(plan0, dtype) == (dt, form, ep), f"contiguous run planned {plan0!r}"

    # (the cache's strides are bytes with pad 16, a 16-bit operand's elements with pad 8: every allocation gets the slack of the wider)
    names = dict(q="q", k="k", v="v", qv="qv")
    shapes = [x.shape for x in t.values()] + [out_shape]
    placed = {n: L.place_input(x, L.ASSIGNMENTS[assignment][names[n]], DEV, L.call_slack(shapes, 1)) for n, x in t.items()}
    for n in "kv":
        assert L.cache_aligned(placed[n].view, 16, 16)
    out = L.place_output(out_shape, dtype, L.ASSIGNMENTS[assignment]["o"], DEV, L.call_slack(shapes, 1))
    ops = {n: p.view for n, p in placed.items()}
    ops.update(lens=lens, k_descale=_descale(c.kdesc, assignment % 3), v_descale=_descale(c.vdesc, (assignment + 1) % 3))
    out1, lse1 = _kv8_call(c, case, ops, out.view)
    plan1 = last_plan()
    SEEN_KV8.add(kernel_key(plan1, dtype))

    equal = _same(out1, out0) and _same(lse1, lse0)
    _emit(kv8u.case_id(form, ep, dt), assignment, plan1, equal)
    assert plan1 == plan0, f"strided operands planned {plan1!r}, contiguous ones {plan0!r}"
    assert out1.data_ptr() == out.view.data_ptr() and out1.stride() == out.view.stride(), "the result is not in the caller's out"
    assert out.view.stride() != placed["q"].view.stride() and not out.view.is_contiguous()
    assert out.intact(), "sentinels around the caller's out were overwritten"
    _untouched(placed, t)
    assert _same(out1, out0), f"out differs from the contiguous run in {int((out1 != out0).sum())} elements"
    assert _same(lse1, lse0), "softmax_lse differs from the contiguous run"


# ---- backward: tests/bwd_plan_universe.py -------------------------------------------------------------------------------------

def _cu(lens):
    return torch.tensor([0] + list(itertools.accumulate(lens)), dtype=torch.int32, device=DEV)


def _bwd_forward(case, ops, seed):
    """One contiguous forward -> (out, lse, rng_state or None)."""
    from flash_attention_annotated_amd import _lib, flash_attn_2_cuda
    q, k, v = ops["q"], ops["k"], ops["v"]
    causal, (wl, wr), scale = case.get("causal", False), case.get("window", (-1, -1)), q.shape[-1] ** -0.5
    if case["api"] == "fa3":
        out, lse, *_ = torch.ops.flash_attn_3.fwd(q, k, v, None, None, None, None, None, None, None, None, None, None, None, None, None,
                                                  None, None, None, None, None, None, None, scale, causal, wl, wr, 0, 0.0, True, None, 1,
                                                  None, 0)
        return out, lse, None
    if case["api"] == "cute":
        out, lse = _lib.binding().cute_fwd(q, k, v, None, None, None, None, None, None, None, scale, causal, -1, -1, ops["sink"], 0.0, 1, None)
        return out, lse, None
    if case["api"] == "fa2_varlen":
        out, lse, _, _ = flash_attn_2_cuda.varlen_fwd(q, k, v, None, ops["cu_q"], ops["cu_k"], None, None, None, None, max(case["lens_q"]),
                                                      max(case["lens_k"]), 0.0, scale, False, causal, wl, wr, 0.0, False, None)
        return out, lse, None
    p_drop = case.get("dropout", 0.0)
    torch.manual_seed(seed)
    out, lse, _, rng = flash_attn_2_cuda.fwd(q, k, v, None, ops.get("slopes"), p_drop, scale, causal, wl, wr, case.get("softcap", 0.0),
                                             False, None)
    return out, lse, rng if p_drop else None


def _bwd_call(case, ops, lse, rng, grads):
    """The backward op of the case's surface on ops (do / q / k / v / o) -> (dq, dk, dv, dsink or None); grads = (dq, dk, dv) or None."""
    from flash_attention_annotated_amd import _lib, flash_attn_2_cuda
    do, q, k, v, o = (ops[n] for n in ("do", "q", "k", "v", "o"))
    dq, dk, dv = grads if grads is not None else (None, None, None)
    causal, (wl, wr), scale = case.get("causal", False), case.get("window", (-1, -1)), q.shape[-1] ** -0.5
    if case["api"] == "fa3":
        r = torch.ops.flash_attn_3.bwd(do, q, k, v, o, lse, dq, dk, dv, None, None, None, None, None, None, scale, causal, wl, wr, 0.0,
                                       False, 0)
        return r[0], r[1], r[2], None
    if case["api"] == "cute" and grads is None:  # (cute_bwd allocates its gradients itself)
        return _lib.binding().cute_bwd(do, q, k, v, o, lse, None, None, None, None, scale, causal, -1, -1, 0.0, ops["sink"])
    if case["api"] == "cute":  # the two calls cute_bwd makes, with the caller's gradients: fa3_bwd (deterministic), then the sink's gradient
        r = torch.ops.flash_attn_3.bwd(do, q, k, v, o, lse, dq, dk, dv, None, None, None, None, None, None, scale, causal, -1, -1, 0.0,
                                       True, 0)
        dsink = _lib.binding().sink_grad(lse, r[3], ops["sink"], None, None, q.shape[0], q.shape[1]).to(ops["sink"].dtype)
        return r[0], r[1], r[2], dsink
    if case["api"] == "fa2_varlen":
        r = flash_attn_2_cuda.varlen_bwd(do, q, k, v, o, lse, dq, dk, dv, ops["cu_q"], ops["cu_k"], None, max(case["lens_q"]),
                                         max(case["lens_k"]), 0.0, scale, False, causal, wl, wr, 0.0, False, None, None)
        return r[0], r[1], r[2], None
    r = flash_attn_2_cuda.bwd(do, q, k, v, o, lse, dq, dk, dv, ops.get("slopes"), case.get("dropout", 0.0), scale, causal, wl, wr,
                              case.get("softcap", 0.0), False, None, rng)
    return r[0], r[1], r[2], None


BWD_PARAMS = [(name, dt) for name in bwdu.CASES for dt in bwdu.DTYPES]


@pytest.mark.parametrize("assignment", ASSIGN)
@pytest.mark.parametrize("name,dt", BWD_PARAMS, ids=[bwdu.case_id(n, dt) for n, dt in BWD_PARAMS])
def test_bwd_layout_parity(name, dt, assignment):
    import flash_attention_annotated_amd  # noqa: F401
    from flash_attention_annotated_amd import flash_attn_3_ops  # noqa: F401
    import test_bwd_plan_parity_gpu as bwdp
    want_plan, case = bwdu.CASES[name]
    seed = sum(ord(c) for c in name + dt)
    t = bwdp._inputs(case, DTYPES[dt], seed)
    t["do"] = t.pop("g")
    shared = {n: t.pop(n).to(DEV) for n in ("slopes", "sink") if n in t}
    if "lens_q" in case:
        shared.update(cu_q=_cu(case["lens_q"]), cu_k=_cu(case["lens_k"]))

    ops = {n: x.to(DEV) for n, x in t.items()}
    ops.update(shared)
    out, lse, rng = _bwd_forward(case, ops, seed)
    ops["o"], t["o"] = out, out.cpu()
    got0 = _bwd_call(case, ops, lse, rng, None)
    plan0 = last_bwd_plan()
    assert plan0 == want_plan, f"contiguous run planned {plan0!r}"

    a = L.ASSIGNMENTS[assignment]
    slack = L.call_slack([x.shape for x in t.values()])
    placed = _place(t, {n: n for n in ("do", "q", "k", "v", "o")}, assignment, slack)
    grads = [L.place_output(t[n].shape, t[n].dtype, a["d" + n], DEV, slack) for n in "qkv"]
    ops = {n: p.view for n, p in placed.items()}
    ops.update(shared)
    got1 = _bwd_call(case, ops, lse, rng, [g.view for g in grads])
    plan1 = last_bwd_plan()
    SEEN_BWD.update((dt, seg) for seg in bwdu.segments(plan1))
    if case.get("sink"):
        SEEN_BWD.add(bwdu.SINK_KEY)  # (launched behind fa_bwd whenever a sink is given; dsink below is what observes it)

    same = [_same(x, y) for x, y in zip(got1[:3], got0[:3])]
    equal = all(same) and (got0[3] is None or _same(got1[3], got0[3]))
    _emit(bwdu.case_id(name, dt), assignment, plan1, equal)
    assert plan1 == plan0, f"strided operands planned {plan1!r}, contiguous ones {plan0!r}"
    strides = [p.view.stride() for p in placed.values()] + [g.view.stride() for g in grads]
    for i, j in itertools.combinations(range(len(strides)), 2):  # (k / v / dk / dv and q / o / do / dq: one shape each)
        assert strides[i][:-1] != strides[j][:-1], "two operands of the call share a stride triple"
    for n, g, r in zip("qkv", grads, got1):
        assert r.data_ptr() == g.view.data_ptr() and r.stride() == g.view.stride(), f"d{n} is not the caller's tensor"
        assert g.intact(), f"sentinels around the caller's d{n} were overwritten"
    _untouched(placed, t)
    for n, ok in zip("qkv", same):
        assert ok, f"d{n} differs from the contiguous run"
    if case.get("sink"):
        assert got0[3] is not None and _same(got1[3], got0[3]), "dsink differs from the contiguous run"


# ---- the append and rotary kernels of a KV-cache step: plan_universe.AUX_STRIDED ----------------------------------------------

AUX_CAP, AUX_FILL, AUX_ROTARY = 200, (40, 100), 32   # cache rows per entry, fill levels in front of the append, rotary_dim
AUX_Q, AUX_NEW = (5, 3), (4, 7)                      # ragged step: query rows and new rows per sequence (dense: 5 and 4 for both)


def _aux_step(ragged, interleaved, ops, kc, vc, out):
    """One KV-cache step with an append and rotary: q rotated into a temporary (rotary_kernel / rotary_varlen_kernel read q through
    its strides), k_new rotated and k_new / v_new written into the caches (kvcache_append_kernel / kvcache_append_varlen_kernel
    read the new rows and write the caches through theirs) -> (out, lse)."""
    from flash_attention_annotated_amd import flash_attn_2_cuda, flash_attn_3_ops  # noqa: F401
    fill = torch.tensor(AUX_FILL, dtype=torch.int32, device=DEV)
    scale = ops["q"].shape[-1] ** -0.5
    if not ragged:
        return flash_attn_2_cuda.fwd_kvcache(ops["q"], kc, vc, ops["k"], ops["v"], fill, ops["cos"], ops["sin"], None, None, None, None, out,
                                             scale, True, -1, -1, 0.0, interleaved, 1)
    o, lse, *_ = torch.ops.flash_attn_3.fwd(
        ops["q"], kc, vc, ops["k"], ops["v"], None, out, _cu(AUX_Q), None, _cu(AUX_NEW), None, fill, max(AUX_Q), None, None, None, None,
        ops["cos"], ops["sin"], None, None, None, None, scale, True, -1, -1, 0, 0.0, interleaved, None, 1, None, 0)
    return o, lse


@pytest.mark.parametrize("assignment", ASSIGN)
@pytest.mark.parametrize("interleaved", [True, False], ids=["interleaved", "halves"])
@pytest.mark.parametrize("ragged", [False, True], ids=["dense", "ragged"])
def test_aux_layout_parity(ragged, interleaved, assignment):
    """kvcache_append_kernel + rotary_kernel (dense step, flash_attn_2_cuda.fwd_kvcache) and kvcache_append_varlen_kernel +
    rotary_varlen_kernel (ragged step, torch.ops.flash_attn_3.fwd) with strided q / k_new / v_new / out and padded cache views:
    out, softmax_lse and every row of both caches are bit-equal to the contiguous call's, the sentinels around the caches and
    out are intact, the inputs untouched.  bf16 under the first assignment, fp16 under the second."""
    a, dtype = L.ASSIGNMENTS[assignment], (torch.bfloat16, torch.float16)[assignment]
    g = torch.Generator().manual_seed(17 + 2 * ragged + interleaved)
    b, h, hk, d = 2, 4, 2, 64
    lead_q, lead_n = ((sum(AUX_Q),), (sum(AUX_NEW),)) if ragged else ((b, AUX_Q[0]), (b, AUX_NEW[0]))
    t = dict(q=torch.randn(*lead_q, h, d, generator=g).to(dtype), k=torch.randn(*lead_n, hk, d, generator=g).to(dtype),
             v=torch.randn(*lead_n, hk, d, generator=g).to(dtype))
    cache = {n: torch.randn(b, AUX_CAP, hk, d, generator=g).to(dtype) for n in "kv"}
    angle = torch.rand(AUX_CAP, AUX_ROTARY // 2, generator=g) * 6.28
    shared = dict(cos=angle.cos().to(dtype).to(DEV), sin=angle.sin().to(dtype).to(DEV))

    ops = {n: x.to(DEV) for n, x in t.items()}
    ops.update(shared)
    kc0, vc0 = cache["k"].to(DEV), cache["v"].to(DEV)
    out0, lse0 = _aux_step(ragged, interleaved, ops, kc0, vc0, None)
    appended = [(bi, n, n + (AUX_NEW[bi] if ragged else AUX_NEW[0])) for bi, n in enumerate(AUX_FILL)]
    for bi, lo, hi in appended:  # the contiguous call did append and rotate: the rows differ from what the cache held
        assert not _same(kc0[bi, lo:hi].cpu(), cache["k"][bi, lo:hi]) and not _same(vc0[bi, lo:hi].cpu(), cache["v"][bi, lo:hi])

    shapes = [x.shape for x in t.values()] + [cache["k"].shape]
    slack = L.call_slack(shapes)
    placed = _place(t, dict(q="q", k="k", v="v"), assignment, slack)
    pools = {n: L.place_output(cache[n].shape, dtype, a[n + "_pages"], DEV, slack) for n in "kv"}
    for n in "kv":
        pools[n].view.copy_(cache[n])
        assert L.cache_aligned(pools[n].view) and not pools[n].view.is_contiguous()
    out = L.place_output(t["q"].shape, dtype, a["o"], DEV, slack)
    ops = {n: p.view for n, p in placed.items()}
    ops.update(shared)
    out1, lse1 = _aux_step(ragged, interleaved, ops, pools["k"].view, pools["v"].view, out.view)

    assert out1.data_ptr() == out.view.data_ptr() and out.intact(), "out is not the caller's tensor, or its sentinels were overwritten"
    assert pools["k"].intact() and pools["v"].intact(), "sentinels around a cache view were overwritten"
    _untouched(placed, t)
    assert _same(pools["k"].view, kc0) and _same(pools["v"].view, vc0), "the caches differ from the contiguous call's"
    assert _same(out1, out0) and _same(lse1, lse0), "out / softmax_lse differ from the contiguous call's"


# ---- coverage -----------------------------------------------------------------------------------------------------------------

def _subset(request):
    return request.config.option.keyword or any("::" in a for a in request.config.args)


def test_every_forward_key_ran_strided(request):
    """The forward keys launched on strided operands are both universes minus the unreachable epilogues and the hook-only forms."""
    if _subset(request):
        pytest.skip("a subset of the cases was selected: the coverage assertion needs the whole file")
    want = {key for key in fwdu.UNIVERSE if key not in fwdu.HOOK_ONLY and (key[1], key[2]) not in fwdu.UNREACHABLE}
    assert SEEN_FWD == want, f"never launched: {sorted(want - SEEN_FWD)}; outside the universe: {sorted(SEEN_FWD - want)}"
    want = {key for key in kv8u.UNIVERSE if (key[1], key[2]) not in kv8u.UNREACHABLE}
    assert SEEN_KV8 == want, f"never launched: {sorted(want - SEEN_KV8)}; outside the universe: {sorted(SEEN_KV8 - want)}"


def test_every_backward_key_ran_strided(request):
    """The backward kernels launched on strided operands are the universe."""
    if _subset(request):
        pytest.skip("a subset of the cases was selected: the coverage assertion needs the whole file")
    want = set(bwdu.UNIVERSE)
    assert SEEN_BWD == want, f"never launched: {sorted(want - SEEN_BWD)}; outside the universe: {sorted(SEEN_BWD - want)}"
