"""Plan-keyed parity: one case per forward kernel key of tests/plan_universe.py -- every template instantiation the launch
tables of csrc/fa_fwd_api.hip can reach (the fwd_kernel families, pk_fwd_kernel, bs_fwd_kernel), in both 16-bit types, plus the
native fp8 kernel, each with the store paths it can take: "direct" (splits=1) and "partial" (split-KV partials + the merge).
Each case runs the public entry point a user would call, asserts through fa_fwd_last_plan_name() that exactly its kernel and
epilogue ran -- a routing change that moves the case to another kernel fails here and asks for a case for the old one -- and
compares out and softmax_lse with the oracle:

    |out - out_ref|max <= rtol |out_pt - out_ref|max + 2 |(out_ref + 0.3 - 0.3) - out_ref|max,  rtol 2, 3 with softcap
                                                                             (hopper/test_flash_attn.py:193-194, 223)
    LSE: the same finite pattern, |lse - lse_ref|max <= 2e-3 (5e-3 for fp8 inputs, as tests/test_full_size_gpu.py)

Cases with `rows="sampled"` evaluate the oracle on one row of every 32-row wave slice of the first, a middle and the last
m-block (parity_helpers._check_rows, the FA2 bound of tests/test_full_size_gpu.py).  The block-sparse cases use the oracle,
the bound (2 |out_pt - out_ref|max + 1e-5) and the keyless-row convention (O = 0, LSE = +inf) of tests/test_block_sparse_gpu.py.
Partial cases also assert the result's type and that every element of it is finite.  Nothing here touches
fa_set_default_variant / fa_set_persist_mode: this file tests what the library itself picks.  The last test asserts that the
kernel keys seen in the session are the whole universe minus UNREACHABLE.

Per-tile ratios, recorded and not asserted: every case also computes err / bound of its own inequality per (batch, head,
32-row slice) -- the smallest wave slice of any forward kernel; a sampled row stands for its slice -- and prints the worst as one
JSON line; with FA_FWD_PARITY_JSONL=<path> set the line is appended to that file (profiles/fwd_plan_parity.jsonl is the
place for such a run).  The whole-tensor bound above takes its two maxima anywhere in the tensor; per tile the reference's
factor 2 has no margin on the forward (an emulation of the kernels' arithmetic on the CPU -- online softmax over 64-key tiles,
P rounded to the input type, fp32 accumulation -- reaches a ratio of exactly 1.00 on a bf16 causal sq = sk = 300 problem), so a ratio above 1
in the file is no finding by itself."""
import math
import re

import pytest
import torch

import block_sparse_oracle as bso
from oracle import attention_ref as oracle
from parity_helpers import FP8, SLICE, Tiles, _check_rows, _emit, causal_bias, kernel_key, last_plan, sparse_lists, wave_slice_rows
from plan_universe import FORMS, HOOK_ONLY, UNIVERSE, UNREACHABLE, case_id, cases

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp8": FP8}
PAGE = 256  # (the FA2 entry point's page rule)

CASES = cases()
SEEN = set()  # kernel keys launched by the cases of this session


def _inputs(case, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    b, h, hk, sq, sk, d = (case[n] for n in ("b", "h", "hk", "sq", "sk", "d"))
    dv = case.get("dv", d)
    store = torch.bfloat16 if dtype == FP8 else dtype
    t = {"q": torch.randn(b, sq, h, d, generator=g).to(store), "k": torch.randn(b, sk, hk, d, generator=g).to(store),
         "v": torch.randn(b, sk, hk, dv, generator=g).to(store)}
    if dtype == FP8:  # values an e4m3 tensor holds, descales rand * 2 per (batch, kv head) (hopper/test_flash_attn.py:135-147)
        t = {n: x.to(FP8).to(store) for n, x in t.items()}
        t.update({f"{n}_descale": torch.rand(b, hk, generator=g) * 2 for n in "qkv"})
    if case.get("qv"):
        t["qv"] = torch.randn(b, sq, h, dv, generator=g).to(store)
    if case.get("alibi"):
        t["slopes"] = torch.rand(b, h, generator=g) * 0.1
    return t


def _paged(x, seed):
    """(b, sk, hk, d) -> (pages, PAGE, hk, d) behind a shuffled block table."""
    b, sk = x.shape[:2]
    npg = -(-sk // PAGE)
    table = torch.randperm(b * npg, generator=torch.Generator().manual_seed(seed)).view(b, npg).to(torch.int32)
    padded = torch.zeros(b, npg * PAGE, *x.shape[2:], dtype=x.dtype)
    padded[:, :sk] = x
    pages = torch.empty(b * npg, PAGE, *x.shape[2:], dtype=x.dtype)
    pages[table.flatten().long()] = padded.view(b * npg, PAGE, *x.shape[2:])
    return pages, table


def _run(case, dtype, t, seed):
    """-> (out, lse, oracle keyword arguments the run adds: the dropout keep-mask)."""
    import flash_attention_annotated_amd as fa
    from flash_attention_annotated_amd import cute_interface as cute
    from flash_attention_annotated_amd import hopper_interface as fa3
    dev = {n: (x.to(FP8) if dtype == FP8 and n in "qkv" else x).to(DEV) for n, x in t.items()}
    api, b, sk = case["api"], case["b"], case["sk"]
    mask = dict(causal=case.get("causal", False), window_size=case.get("window", (-1, -1)), softcap=case.get("softcap", 0.0))
    if api == "fa3":
        extra = {n: dev[n] for n in ("qv", "q_descale", "k_descale", "v_descale") if n in dev}
        out, lse = fa3.flash_attn_func(dev["q"], dev["k"], dev["v"], attention_chunk=case.get("chunk", 0), return_attn_probs=True,
                                       pack_gqa=case.get("pack"), **mask, **extra)
        return out, lse, {}
    if api == "fa3_cache":  # (any cache argument takes the KV-cache route: an identity cache_batch_idx over full caches)
        out, lse, *_ = fa3.flash_attn_with_kvcache(dev["q"], dev["k"], dev["v"], qv=dev.get("qv"),
                                                   cache_seqlens=torch.full((b,), sk, dtype=torch.int32, device=DEV),
                                                   cache_batch_idx=torch.arange(b, dtype=torch.int32, device=DEV),
                                                   num_splits=case["splits"], pack_gqa=case.get("pack"), return_softmax_lse=True, **mask)
        return out, lse, {}
    if api in ("cute", "bs"):
        left, right = case.get("window", (None, None))
        lists = {}
        if api == "bs":
            names = ("full_block_cnt", "full_block_idx", "mask_block_cnt", "mask_block_idx")
            lists = {n: x.to(DEV) for n, x in zip(names, case["block_lists"])}
        out, lse = cute.flash_attn_func(dev["q"], dev["k"], dev["v"], causal=mask["causal"], window_size=(left, right),
                                        softcap=mask["softcap"], num_splits=case.get("splits", 1), pack_gqa=case.get("pack"), **lists)
        return out, lse, {}
    if api == "fa2_paged":
        kc, table = _paged(t["k"], seed)
        vc, _ = _paged(t["v"], seed)
        out, lse = fa.flash_attn_with_kvcache(dev["q"], kc.to(DEV), vc.to(DEV), cache_seqlens=case["seqlens"].to(DEV),
                                              block_table=table.to(DEV), num_splits=case.get("splits", 0),
                                              return_softmax_lse=True, **mask)
        return out, lse, {}
    if api == "fa2_cache":  # q / k / v as they are: the dense routing with the caller's num_splits
        out, lse = fa.flash_attn_with_kvcache(dev["q"], dev["k"], dev["v"], alibi_slopes=dev.get("slopes"),
                                              num_splits=case["splits"], return_softmax_lse=True, **mask)
        return out, lse, {}
    assert api == "fa2", api
    p_drop = case.get("dropout", 0.0)
    torch.manual_seed(seed)
    out, lse, S = fa.flash_attn_func(dev["q"], dev["k"], dev["v"], p_drop, alibi_slopes=dev.get("slopes"), return_attn_probs=True,
                                     **mask)
    if p_drop == 0.0:
        return out, lse, {}
    # the sign of S_dmask is the dropout decision (tests/test_dropout_gpu.py): the oracle runs with the kernel's keep-mask
    S = oracle.convert_flash_attn_S_to_softmax(S.cpu(), case["sq"], case["sk"], None, None, causal=mask["causal"],
                                               window_size=mask["window_size"])
    return out, lse, dict(dropout_p=p_drop, dropout_mask=S >= 0)


def _check(out, lse, out_ref, out_pt, lse_ref, fp8, rtol, atol, what, tiles, batch=0):
    """The file's bound on (out, lse) against (out_ref, out_pt, lse_ref); atol None = 2 |(out_ref + 0.3 - 0.3) - out_ref|max."""
    out, out_ref = out.float().cpu(), out_ref.float()
    tiles.add(out, out_ref, out_pt, rtol, atol, batch=batch)
    err = (out - out_ref).abs().max().item()
    bound = rtol * (out_pt.float() - out_ref).abs().max().item() + (2 * (out_ref + 0.3 - 0.3 - out_ref).abs().max().item() if atol is None else atol)
    lse, fin = lse.float().cpu(), torch.isfinite(lse_ref)
    same = torch.equal(torch.isfinite(lse), fin)
    lerr = (lse[fin] - lse_ref[fin]).abs().max().item() if same and fin.any() else float("nan" if not same else 0.0)
    print(f"{what}: out err {err:.3e} bound {bound:.3e}; lse err {lerr:.3e}")
    assert math.isfinite(err) and err <= bound, f"{what}: out err {err:.3e} > bound {bound:.3e}"
    assert same, f"{what}: lse finite pattern differs"
    assert lerr <= (5e-3 if fp8 else 2e-3), f"{what}: lse err {lerr:.3e}"


def _compare(out, lse, q, k, v, okw, fp8, rtol, what, tiles, batch=0):
    out_ref, _, lse_ref = oracle.attention_ref(q, k, v, return_lse=True, **okw)
    out_pt, _ = oracle.attention_ref(q, k, v, upcast=False, reorder_ops=True, intermediate_dtype=FP8 if fp8 else None, **okw)
    _check(out, lse, out_ref, out_pt, lse_ref, fp8, rtol, None, what, tiles, batch)


def _compare_block_sparse(out, lse, t, case, what, tiles):
    """Oracle, bound and keyless-row convention of tests/test_block_sparse_gpu.py."""
    kw = dict(causal=case.get("causal", False), softcap=case.get("softcap", 0.0))
    ref, lse_ref = bso.attention_block_sparse_ref(t["q"], t["k"], t["v"], *case["block_lists"], **kw)
    pt, _ = bso.attention_block_sparse_ref(t["q"], t["k"], t["v"], *case["block_lists"], upcast=False, reorder_ops=True, **kw)
    _check(out, lse, ref, pt, lse_ref, False, 2, 1e-5, what, tiles)
    keyless = torch.isinf(lse_ref)                                      # (b, h, sq): rows whose visited blocks the mask empties
    assert keyless.any() and not keyless.all()
    assert torch.isposinf(lse.cpu()[keyless]).all() and (out.cpu().transpose(1, 2)[keyless] == 0).all()


@pytest.mark.parametrize("form,ep,dt,case", CASES, ids=[case_id(f, ep, dt) for f, ep, dt, _ in CASES])
def test_plan_parity(form, ep, dt, case):
    dtype, fp8 = DTYPES[dt], dt == "fp8"
    case = dict(case)
    seed = sum(ord(c) for c in form + ep + dt)
    b, sq, sk = case["b"], case["sq"], case["sk"]
    if case["api"] == "fa2_paged":
        case["seqlens"] = torch.tensor([sk - 115 * (i % 2) for i in range(b)], dtype=torch.int32)
    if case["api"] == "bs":
        case["block_lists"], _ = sparse_lists(case)
    t = _inputs(case, dtype, seed)
    out, lse, okw = _run(case, dtype, t, seed)
    plan = last_plan()
    key = kernel_key(plan, dtype)
    SEEN.add(key)
    assert key == (dt, form, ep), f"planned {plan!r}: the case no longer reaches {(form, ep)!r} -- add a case for the kernel it left"
    block_m = int(re.search(r"block_m=(\d+)", plan).group(1))
    assert sq % block_m != 0 and (sk % 64 != 0 or "PERSIST" in form)
    if ep == "partial":
        assert out.dtype == (torch.bfloat16 if fp8 else dtype) and lse.dtype == torch.float32
        assert torch.isfinite(out).all(), f"{form} {dt}: non-finite elements in the merged result"

    okw.update(softcap=case.get("softcap", 0.0), attention_chunk=case.get("chunk", 0), window_size=case.get("window", (-1, -1)))
    okw.update({n: t[n] for n in ("qv", "q_descale", "k_descale", "v_descale") if n in t})
    causal = case.get("causal", False)
    bias = oracle.attn_bias_from_alibi_slopes(t["slopes"], sq, sk, causal=False) if "slopes" in t else None  # (b, h, sq, sk)
    rtol = 3 if case.get("softcap") else 2
    what, tiles = f"{form} {ep} {dt}", Tiles()
    try:
        if case["api"] == "bs":
            _compare_block_sparse(out, lse, t, case, what, tiles)
        elif case.get("rows") == "sampled":
            rows = wave_slice_rows(sq, block_m, seed)
            assert len({r // SLICE for r in rows}) == len(rows) >= 6
            for bi in sorted({0, b // 2, b - 1}):
                rb = causal_bias(rows, sq, sk) if causal else torch.zeros(1, 1, len(rows), sk)
                if bias is not None:
                    rb = rb + bias[bi:bi + 1][:, :, rows]
                _check_rows(out[bi:bi + 1, rows], lse[bi:bi + 1, :, rows], t["q"][bi:bi + 1, rows], t["k"][bi:bi + 1], t["v"][bi:bi + 1],
                            rb, f"{what} batch {bi}",
                            record=lambda o, r, p, atol, bi=bi: tiles.add(o, r, p, 2, atol, rows_per_tile=1, batch=bi))
        elif case["api"] == "fa2_paged":
            for bi in range(b):
                n = int(case["seqlens"][bi])
                _compare(out[bi:bi + 1], lse[bi:bi + 1], t["q"][bi:bi + 1], t["k"][bi:bi + 1, :n], t["v"][bi:bi + 1, :n],
                         dict(okw, causal=causal), fp8, rtol, f"{what} batch {bi}", tiles, batch=bi)
        else:
            _compare(out, lse, t["q"], t["k"], t["v"], dict(okw, causal=causal, attn_bias=bias), fp8, rtol, what, tiles)
    finally:
        _emit(case_id(form, ep, dt), plan, tiles)


def test_block_sparse_split_is_refused_by_the_cute_surface():
    """The "refused" rule of plan_universe.UNREACHABLE on the entry point itself: the universe's block-sparse case with
    num_splits = 3 raises, with num_splits = 0 it runs the direct epilogue."""
    from flash_attention_annotated_amd import cute_interface as cute
    case = dict(FORMS["bs_fwd_kernel D=64 waves=4"]["direct"])
    t = {n: x.to(DEV) for n, x in _inputs(case, torch.bfloat16, 1).items()}
    names = ("full_block_cnt", "full_block_idx", "mask_block_cnt", "mask_block_idx")
    lists = {n: x.to(DEV) for n, x in zip(names, sparse_lists(case)[0])}
    with pytest.raises(NotImplementedError, match="num_splits"):
        cute.flash_attn_func(t["q"], t["k"], t["v"], causal=True, num_splits=3, **lists)
    cute.flash_attn_func(t["q"], t["k"], t["v"], causal=True, num_splits=0, **lists)
    assert kernel_key(last_plan(), torch.bfloat16) == ("bf16", "bs_fwd_kernel D=64 waves=4", "direct")


def test_every_kernel_key_ran(request):
    """The kernel keys the cases above launched are the universe minus the unreachable epilogues and the hook-only forms."""
    if request.config.option.keyword or any("::" in a for a in request.config.args):
        pytest.skip("a subset of the cases was selected: the coverage assertion needs the whole file")
    want = {key for key in UNIVERSE if key not in HOOK_ONLY and (key[1], key[2]) not in UNREACHABLE}
    assert SEEN == want, f"never launched: {sorted(want - SEEN)}; outside the universe: {sorted(SEEN - want)}"
