"""Plan-keyed parity of the forward units over an fp8 (e4m3) KV cache: one case per kernel key of tests/kv8_plan_universe.py --
every instantiation of kv8_fwd_kernel (csrc/fa_fwd_kv8_api.hip) and qv8_fwd_kernel (csrc/fa_fwd_qv8_api.hip), in both 16-bit
query types, with both store paths: "direct" (splits=1) and "partial" (fp32 partials in the workspace + fa_fwd_combine).  Each
case runs hopper_interface.flash_attn_with_kvcache, asserts through fa_fwd_last_plan_name() that exactly its kernel and
epilogue ran, and compares out and softmax_lse with the oracle the way tests/test_kv8_kvcache_gpu.py and
tests/test_qv8_kvcache_gpu.py do (their Case classes build the cache and the oracle's legs here; bounds justified there):

    reference   the unchanged oracle.attention_ref (qv= for qv8), fed the cache dequantised on the CPU: e4m3 -> fp32 exactly,
                times the descale of the (batch, kv head); the low-precision leg `pt` in q's dtype
    out         |out - ref|max <= 3 |pt - ref|max + 1e-5
    LSE         the same finite pattern; within 1e-3 (kv8), below 2e-3 (qv8)

Partial cases also assert the result types, that every element is finite, and agreement with the num_splits = 1 result of the
same inputs under the same bounds.  The last test asserts that the keys seen in the session are the whole universe.

test_split_edge runs the partial epilogue at its edges (kv8_plan_universe.EDGES; the geometry each case promises is asserted
on the CPU by tests/test_kv8_plan.py): ragged queries dense and paged, both page-lookup paths, cache_batch_idx, leftpad_k, a
part emptied by the mask, keyless rows inside a processed tile, several row blocks -- each with num_splits = 3 against the oracle
and against its own num_splits = 1 run, with the plan of both asserted.

Per-tile ratios, recorded and not asserted: every universe case prints the worst err / bound of its own inequality per (batch,
head, 32-row slice) as one JSON line; with FA_KV8_PARITY_JSONL=<path> set the line is appended to that file
(profiles/kv8_plan_parity.jsonl holds such a run).  As in tests/test_plan_parity_gpu.py a ratio above 1 in a tile is no finding
by itself: the asserted bound takes its two maxima anywhere in the tensor."""
import math

import pytest
import torch

from kv8_plan_universe import EDGE_SPLITS, UNIVERSE, UNREACHABLE, case_id, cases, edge_cases
from parity_helpers import Tiles, _emit, kernel_key, last_plan
from test_kv8_kvcache_gpu import Case as Kv8Case
from test_qv8_kvcache_gpu import Case as Qv8Case

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
LSE_TOL = {"kv8": 1e-3, "qv8": 2e-3}
JSONL = "FA_KV8_PARITY_JSONL"

CASES = cases()
EDGE_CASES = edge_cases()
SEEN = set()  # kernel keys launched by the universe cases of this session


def _lse_ok(kernel, err):
    """tests/test_kv8_kvcache_gpu.py: allclose(atol=1e-3); tests/test_qv8_kvcache_gpu.py: err < 2e-3."""
    return err <= LSE_TOL[kernel] if kernel == "kv8" else err < LSE_TOL[kernel]


def _check(kernel, out, lse, ref, ref_lse, pt, what, tiles=None):
    """The two files' bounds on (out, lse) in the oracle's layout (b, sq, h, d) / (b, h, sq)."""
    out, lse, ref = out.float().cpu(), lse.float().cpu(), ref.float()
    if tiles is not None:
        tiles.add(out, ref, pt, 3, 1e-5)
    err = (out - ref).abs().max().item()
    bound = 3 * (pt.float() - ref).abs().max().item() + 1e-5
    fin = torch.isfinite(ref_lse)
    same = torch.equal(torch.isfinite(lse), fin)
    lerr = (lse[fin] - ref_lse[fin]).abs().max().item() if same and fin.any() else float("nan" if not same else 0.0)
    print(f"{what}: out err {err:.3e} bound {bound:.3e}; lse err {lerr:.3e}")
    assert math.isfinite(err) and err <= bound, f"{what}: out err {err:.3e} > bound {bound:.3e}"
    assert same, f"{what}: lse finite pattern differs"
    assert _lse_ok(kernel, lerr), f"{what}: lse err {lerr:.3e}"
    return bound


def _check_against_unsplit(kernel, o3, l3, o1, l1, bound, what):
    """The split result against the num_splits = 1 result of the same inputs: the out bound of the oracle comparison, the LSE
    tolerance on the finite entries, the same entries infinite with the same sign."""
    o3, l3, o1, l1 = o3.float().cpu(), l3.float().cpu(), o1.float().cpu(), l1.float().cpu()
    err = (o3 - o1).abs().max().item()
    fin = torch.isfinite(l1)
    assert math.isfinite(err) and err <= bound, f"{what}: |split - unsplit| {err:.3e} > bound {bound:.3e}"
    assert torch.equal(torch.isfinite(l3), fin) and torch.equal(l3[~fin], l1[~fin]), f"{what}: lse infinities differ from the unsplit run"
    lerr = (l3[fin] - l1[fin]).abs().max().item() if fin.any() else 0.0
    print(f"{what}: |split - unsplit| out {err:.3e} lse {lerr:.3e}")
    assert _lse_ok(kernel, lerr), f"{what}: |lse split - unsplit| {lerr:.3e}"


def _run_entry(c, num_splits):
    """hopper_interface.flash_attn_with_kvcache on the Case's tensors -> (out, lse, plan)."""
    from flash_attention_annotated_amd import hopper_interface as fa3
    qv = getattr(c, "qv", None)
    out, lse, *_ = fa3.flash_attn_with_kvcache(c.q.to(DEV), c._phys(c.k8), c._phys(c.v8), qv=None if qv is None else qv.to(DEV),
                                               cache_seqlens=c.lens.to(DEV), k_descale=c.kdesc.to(DEV), v_descale=c.vdesc.to(DEV),
                                               causal=c.causal, window_size=c.window, softcap=c.softcap, num_splits=num_splits,
                                               return_softmax_lse=True)
    return out, lse, last_plan()


@pytest.mark.parametrize("form,ep,dt,case", CASES, ids=[case_id(f, ep, dt) for f, ep, dt, _ in CASES])
def test_kv8_plan_parity(form, ep, dt, case):
    kernel, dtype = case["kernel"], DTYPES[dt]
    seed = sum(ord(ch) for ch in form + ep + dt)
    kw = dict(dtype=dtype, b=case["b"], sq=case["sq"], h=case["h"], hk=case["hk"], d=case["d"], cap=case["cap"], lens=case["lens"],
              causal=case["causal"], softcap=case.get("softcap", 0.0), seed=seed)
    c = Kv8Case(**kw) if kernel == "kv8" else Qv8Case(dv=case["dv"], **kw)
    out, lse, plan = _run_entry(c, case["splits"])
    key = kernel_key(plan, dtype)
    SEEN.add(key)
    assert key == (dt, form, ep), f"planned {plan!r}: the case no longer reaches {(form, ep)!r} -- add a case for the kernel it left"
    what, tiles = f"{form} {ep} {dt}", Tiles()
    try:
        if ep == "partial":
            assert out.dtype == dtype and lse.dtype == torch.float32
            assert torch.isfinite(out).all() and torch.isfinite(lse).all(), f"{what}: non-finite elements in the merged result"
        ref, ref_lse, pt = c.reference()
        bound = _check(kernel, out, lse, ref, ref_lse, pt, what, tiles)
        if ep == "partial":
            o1, l1, plan1 = _run_entry(c, 1)
            assert kernel_key(plan1, dtype) == (dt, form, "direct"), plan1
            _check_against_unsplit(kernel, out, lse, o1, l1, bound, what)
    finally:
        _emit(case_id(form, ep, dt), plan, tiles, env=JSONL)


def _edge_plan(kernel, c, splits):
    if kernel == "kv8":
        return f"kv8_fwd_kernel D={64 if c.d <= 64 else 128} waves=4{' SOFTCAP' if c.softcap > 0 else ''} block_m=128 splits={splits}"
    return f"qv8_fwd_kernel DVT={c.dvt} waves=4{' SOFTCAP' if c.softcap > 0 else ''} block_m=32 splits={splits}"


@pytest.mark.parametrize("name,kernel,dt,kw", EDGE_CASES, ids=[f"{n}-{k}-{dt}" for n, k, dt, _ in EDGE_CASES])
def test_split_edge(name, kernel, dt, kw):
    """The partial epilogue at one of its edges (kv8_plan_universe.EDGES): num_splits = 3 against the oracle and against the
    num_splits = 1 run of the same inputs, both under the files' bounds; the plan of both runs is asserted.  Ragged queries are
    compared on their used rows; what the rows past seqused_q hold is printed.  Rows the oracle finds keyless hold O = 0 and
    LSE = +inf, split and unsplit."""
    c = (Kv8Case if kernel == "kv8" else Qv8Case)(dtype=DTYPES[dt], **kw)
    run = c.run_kv8 if kernel == "kv8" else c.run_qv8
    ref, ref_lse, pt = c.reference()
    what = f"{name} {kernel} {dt}"
    o3, l3, plan3 = run(num_splits=EDGE_SPLITS)
    o1, l1, plan1 = run(num_splits=1)
    assert plan3 == _edge_plan(kernel, c, EDGE_SPLITS) and plan1 == _edge_plan(kernel, c, 1), (plan3, plan1)
    assert o3.dtype == c.dtype and l3.dtype == torch.float32 and o3.shape == o1.shape and l3.shape == l1.shape
    if c.cu_q is not None:  # rows of the ragged batch no sequence uses
        used = torch.zeros(o3.shape[0], dtype=torch.bool)
        for i in range(c.b):
            used[int(c.cu_q[i]): int(c.cu_q[i]) + int(c.seqused_q[i])] = True
        assert (~used).any() and used.any()
        for label, o, l in (("split", o3, l3), ("unsplit", o1, l1)):
            po, pl = o[~used].float(), l[:, ~used]
            print(f"{what}: rows past seqused_q after the {label} call: out finite {bool(torch.isfinite(po).all())} "
                  f"|out|max {po.abs().nan_to_num(nan=float('inf')).max().item():.3e} lse {pl.flatten().tolist()[:4]}")
    s3, sl3 = c.select(o3, l3)
    s1, sl1 = c.select(o1, l1)
    assert torch.isfinite(s3.float()).all(), f"{what}: non-finite elements in the merged result"
    bound = _check(kernel, s3, sl3, ref, ref_lse, pt, f"{what} splits={EDGE_SPLITS}")
    _check(kernel, s1, sl1, ref, ref_lse, pt, f"{what} splits=1")
    _check_against_unsplit(kernel, s3, sl3, s1, sl1, bound, what)
    keyless = torch.isinf(ref_lse)  # (b, h, sq)
    if name == "keyless-rows":
        assert keyless.any() and not keyless.all()
    for o, l in ((s3, sl3), (s1, sl1)):
        assert torch.isposinf(l.float()[keyless]).all() and (o.float().transpose(1, 2)[keyless] == 0).all(), f"{what}: keyless rows"


def test_every_kv8_kernel_key_ran(request):
    """The kernel keys the universe cases launched are the universe minus the unreachable epilogues."""
    if request.config.option.keyword or any("::" in a for a in request.config.args):
        pytest.skip("a subset of the cases was selected: the coverage assertion needs the whole file")
    want = {key for key in UNIVERSE if (key[1], key[2]) not in UNREACHABLE}
    assert SEEN == want, f"never launched: {sorted(want - SEEN)}; outside the universe: {sorted(SEEN - want)}"
