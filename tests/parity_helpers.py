"""Helpers shared by the GPU parity tests (a plain module, not collected): row sampling for problems whose full attention
matrix is too costly for the CPU oracle, and the row-subset comparison of tests/test_full_size_gpu.py (bounds in its docstring).
Tiles / _emit record the per-tile err / bound ratios of the plan-keyed parity files (tests/test_plan_parity_gpu.py,
tests/test_kv8_plan_parity_gpu.py).  Also the one place that reads back which forward plan ran (fa_fwd_last_plan_name,
include/fa_fwd.h) and which backward kernels (fa_bwd_last_plan_name, include/fa_bwd.h)."""
import json
import math
import os
import re

import torch

from oracle import attention_ref as oracle

FP8 = torch.float8_e4m3fn
SLICE = 32  # rows of the smallest wave slice of any forward kernel


def last_plan():
    """Plan name of the calling thread's most recent fa_fwd launch (both compiled bindings call fa_fwd synchronously on the
    Python thread, out of the library _lib.load() returns)."""
    from flash_attention_annotated_amd import _lib
    name = _lib.load().fa_fwd_last_plan_name()
    assert name is not None, "no forward plan recorded: the entry point did not reach fa_fwd on this thread"
    return name.decode()


def last_bwd_plan():
    """Plan text of the calling thread's most recent fa_bwd launch: one segment per launched kernel."""
    from flash_attention_annotated_amd import _lib
    name = _lib.load().fa_bwd_last_plan_name()
    assert name is not None, "no backward plan recorded: the entry point did not reach fa_bwd on this thread"
    return name.decode()


def record_bwd_plan(out):
    """-> a list that receives the plan text of the backward of `out` (an output of one of the autograd Functions).  autograd
    runs the backward node of a GPU tensor on the engine's thread for that device, not on the thread that calls
    torch.autograd.grad, and fa_bwd_last_plan_name() is per thread: a hook on the node reads it there, right behind the
    node's fa_bwd."""
    seen = []
    out.grad_fn.register_hook(lambda *_: seen.append(last_bwd_plan()))
    return seen


def kernel_key(plan, dtype):
    """(element type, plan name without block_m= / splits= / cols= / fp8_expand, epilogue): one template instantiation and the
    store path the launch took in it -- "direct" for `splits=1`, "partial" (fp32 partials + the merge) for any other count.
    fp8 inputs run the native kernel ("fp8") or, expanded, the bf16 instantiations."""
    return plan_key(plan, "fp8" if dtype == FP8 else {torch.bfloat16: "bf16", torch.float16: "fp16"}[dtype])


def plan_key(plan, dt):
    """kernel_key for an element type by name ("bf16", "fp16", "fp8"): needs no tensor type, the CPU tests use it as well."""
    form = re.sub(r" (block_m|splits|cols)=\d+| fp8_expand", "", plan)
    splits = re.search(r" splits=(\d+)", plan)
    assert splits, f"{plan!r} names no split count"
    epilogue = "direct" if splits.group(1) == "1" else "partial"
    if dt == "fp8" and " fp8_expand" in plan:
        dt = "bf16"
    return (dt, form, epilogue)


def sparse_lists(case):
    """((full_cnt, full_idx, mask_cnt, mask_idx), visited) of a block-sparse case of tests/plan_universe.py: seeded lists as
    tests/test_block_sparse_gpu.py::test_random_subsets builds them, 1 .. nk - 1 visited key blocks per query block."""
    import block_sparse_oracle as bso
    nm, nk = -(-case["sq"] // bso.BLOCK), -(-case["sk"] // bso.BLOCK)
    return bso.random_lists(case["lists"], case["b"], case["h"], nm, nk, min_visited=1, max_visited=nk - 1)


def wave_slice_rows(sq, block_m, seed=0, rows_per_wave=32):
    """One random row in every `rows_per_wave`-row slice of the first, a middle and the last `block_m`-row m-block (sorted).
    32 rows is the smallest wave slice of any forward kernel (fwd_kernel_d256: 4 waves x 32 rows; a 64-row wave of the 256-row
    kernel gets two)."""
    g = torch.Generator().manual_seed(seed)
    nblocks = (sq + block_m - 1) // block_m
    rows = []
    for mb in sorted({0, nblocks // 2, nblocks - 1}):
        for lo in range(mb * block_m, min(sq, (mb + 1) * block_m), rows_per_wave):
            hi = min(sq, lo + rows_per_wave)
            rows.append(lo + int(torch.randint(0, hi - lo, (1,), generator=g)))
    return sorted(set(rows))


def sample_rows(sq, n=128, block=256, seed=0):
    """Sorted row indices: ceil(n / #blocks) random rows in every `block`-row m-block (>= n rows in total)."""
    g = torch.Generator().manual_seed(seed)
    nblocks = (sq + block - 1) // block
    per = max(1, -(-n // nblocks))
    rows = []
    for mb in range(nblocks):
        lo, hi = mb * block, min(sq, (mb + 1) * block)
        rows += (lo + torch.randperm(hi - lo, generator=g)[:per]).tolist()
    return sorted(set(rows))


def causal_bias(rows, sq, sk):
    """(1, 1, len(rows), sk): 0 where key j <= i + sk - sq (bottom-right aligned causal), -inf elsewhere."""
    i = torch.tensor(rows, dtype=torch.long).view(-1, 1)
    j = torch.arange(sk, dtype=torch.long).view(1, -1)
    return torch.where(j <= i + sk - sq, 0.0, float("-inf")).view(1, 1, len(rows), sk)


class Tiles:
    """The worst err / bound of a case per (batch, head, row slice), over every comparison the case makes."""

    def __init__(self):
        self.worst = None

    def add(self, out, ref, pt, rtol, atol, rows_per_tile=SLICE, batch=0):
        """out / ref / pt (b, rows, h, d).  atol: a number, or None = 2 |(ref + 0.3 - 0.3) - ref|max of the tile."""
        out, ref, pt = out.float().cpu(), ref.float(), pt.float()

        def tiles(x):  # (b, rows, h, d) -> (b, h, slices): max over the slice's rows and the columns
            x = x.amax(-1)
            x = torch.nn.functional.pad(x, (0, 0, 0, -x.shape[1] % rows_per_tile))
            return x.view(x.shape[0], -1, rows_per_tile, x.shape[-1]).amax(2).transpose(1, 2)
        err = tiles((out - ref).abs().nan_to_num(nan=float("inf")))
        bound = rtol * tiles((pt - ref).abs()) + (2 * tiles((ref + 0.3 - 0.3 - ref).abs()) if atol is None else atol)
        ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)  # (a tile without error has ratio 0, also at bound 0)
        at = int(ratio.argmax())
        b, h, s = (int(i) for i in torch.unravel_index(torch.tensor(at), ratio.shape))
        got = dict(ratio=float(ratio.flatten()[at]), batch=b + batch, head=h, slice=s, err=float(err[b, h, s]), bound=float(bound[b, h, s]))
        if self.worst is None or got["ratio"] > self.worst["ratio"]:
            self.worst = got


def _emit(cid, plan, tiles, env="FA_FWD_PARITY_JSONL"):
    """One JSON line for the case: printed, and appended to the file the environment variable `env` names when it is set."""
    w = tiles.worst or {}
    line = json.dumps(dict(case=cid, plan=plan, rows_per_tile=SLICE,
                           **{k: (v if not isinstance(v, float) or math.isfinite(v) else str(v)) for k, v in w.items()}))
    print(line)
    path = os.environ.get(env)
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def _check_rows(out_rows, lse_rows, q_rows, k, v, bias, what, fp8_kw=None, lse_tol=2e-3, record=None):
    """`record(out_rows, out_ref, out_pt, atol)`, when given, sees the terms of the bound before anything is asserted."""
    kw = dict(attn_bias=bias)
    if fp8_kw:
        kw.update(fp8_kw)
    out_ref, _, lse_ref = oracle.attention_ref(q_rows, k, v, return_lse=True, **kw)
    if fp8_kw:
        out_pt, _ = oracle.attention_ref(q_rows, k, v, upcast=False, reorder_ops=True, intermediate_dtype=FP8, **kw)
        atol = 2 * (out_ref.float() + 0.3 - 0.3 - out_ref.float()).abs().max().item()
    else:
        out_pt, _ = oracle.attention_ref(q_rows, k, v, upcast=False, reorder_ops=True, **kw)
        atol = 1e-5
    if record is not None:
        record(out_rows, out_ref, out_pt, atol)
    err = (out_rows.float().cpu() - out_ref.float()).abs().max().item()
    bound = 2 * (out_pt.float() - out_ref.float()).abs().max().item() + atol
    assert math.isfinite(err) and err <= bound, f"{what}: max err {err:.3e} > bound {bound:.3e}"
    fin = torch.isfinite(lse_ref)
    lse_rows = lse_rows.float().cpu()
    assert torch.equal(torch.isfinite(lse_rows), fin), f"{what}: lse inf pattern"
    lerr = (lse_rows[fin] - lse_ref[fin]).abs().max().item()
    assert lerr <= lse_tol, f"{what}: lse err {lerr:.3e}"
