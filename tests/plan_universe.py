"""The plan universe: every forward *kernel key* the launch tables of csrc/fa_fwd_api.hip can instantiate, each with the GPU
parity case that runs it (tests/test_plan_parity_gpu.py), and every other kernel of the forward device code with the GPU test
that compares it with a reference (AUX).  A plain module, imported by tests/test_fwd_plan.py (which checks the tables against
the kernel symbols of the compiled device code: a kernel added without a row here fails on the CPU) and by the parity test
(which asserts that every case launches exactly its key).  The two forward units over an fp8 (e4m3) KV cache --
csrc/fa_fwd_kv8_api.hip and csrc/fa_fwd_qv8_api.hip, with plans of their own -- and the append unit beside them have the sibling
module tests/kv8_plan_universe.py (tests/test_kv8_plan.py, tests/test_kv8_plan_parity_gpu.py).

Kernel key = (element type, kernel form, epilogue).  The form is the plan name of fa_fwd_plan_name without `block_m=`,
`splits=`, `cols=` and `fp8_expand`: one template instantiation.  The epilogue is the store path the launch takes inside it,
selected at run time: "direct" (`splits=1`: O in the output type and the LSE go to the caller's tensors) or "partial"
(`splits=` above 1: fp32 O / LSE partials go to the workspace, combine_splits_kernel merges them).  A (form, epilogue) without
a case is listed in UNREACHABLE with the rule that forbids it; tests/test_fwd_plan.py asserts each rule on the CPU.

A case is plain data: `api` is the public entry point, the rest its problem.
    "fa2"        flash_attn_func: plans its own split (none under dropout)
    "fa2_cache"  flash_attn_with_kvcache on q / k / v as they are (no cache argument): the same routing, `splits` = num_splits
    "fa2_paged"  flash_attn_with_kvcache on a paged cache, `splits` = num_splits (0 = the heuristic)
    "fa3"        the FA3-shaped flash_attn_func: never splits (its binding hands fa_fwd num_splits = 1 on the dense route)
    "fa3_cache"  the FA3-shaped flash_attn_with_kvcache behind an identity cache_batch_idx, `splits` = num_splits
    "cute"       cute_interface.flash_attn_func, `splits` = num_splits
    "bs"         cute_interface.flash_attn_func with block lists (tests/block_sparse_oracle.py:random_lists(`lists`, ...))
`pack=True` asks for PackGQA.  Every case sweeps at least three full 64-key tiles, a masked tile (causal diagonal, window edge
or chunk edge) and a ragged last tile (seqlen_k % 64 != 0; the persistent form only takes multiples of 64), with seqlen_q no
multiple of block_m; the parts of a partial case are thirds of a row block's own key tiles (split_range, csrc/fa_fwd_kernel.h):
at 12 key tiles every part owns full tiles, and under the causal mask the last part of the first rows is empty.
What decides the routing (plan_fwd):
  * FA2 dense calls split by heuristic when (m-blocks x heads x batch) <= 128 (512 for the 4-wave shape) and seqlen_k >= 512:
    the FA2-surface cases on SMALL / SHORTQ / WINDOW run split 3 ways, about 4 key tiles per split; their direct cases ask for
    num_splits = 1 ("fa2_cache", "fa2_paged") or use the FA3 surface, which routes the same problem to the same form;
  * the width-64/96/128 forms of fwd_kernel_d256 are planned without a split only, so their ALiBi cases (FA2 surface only)
    carry 72 heads x batch; the FA3 surface never splits by itself, the softcap cases use it with small batches;
  * head-dim tile 64 under a causal mask runs the 4-wave compiler-scheduled shape up to seqlen_k 2048 (up to 512 otherwise):
    the 256-row kernel and fwd_kernel_d256 W=64 need longer keys (`rows="sampled"`: the oracle is evaluated on sampled rows);
  * seqlen_q <= 128 dense runs the 4-wave compiler-scheduled shape at every head dim;
  * FA_FLAG_PACK_GQA takes GQA calls at head dims <= 128 to pk_fwd_kernel; block lists run bs_fwd_kernel (fa_fwd_block_sparse).
"""

SMALL = dict(b=2, h=4, hk=2, sq=300, sk=715, causal=True)     # GQA 2; 11 full key tiles + 11 keys
WIDE = dict(b=3, h=24, hk=8, sq=300, sk=715, causal=True)     # GQA 3; > 128 work items: no heuristic split
SHORTQ = dict(b=2, h=4, hk=2, sq=100, sk=715, causal=True)    # seqlen_q <= 128
LONG64 = dict(b=1, h=2, hk=1, sq=2100, sk=2250, causal=True)  # head dim 64 causal past seqlen_k 2048
LONG64_WIDE = dict(b=1, h=16, hk=8, sq=2100, sk=2250, causal=True, rows="sampled")
WINDOW = dict(b=2, h=4, hk=2, sq=300, sk=715, window=(400, 100))
# PackGQA, g = 3: 43 rows x 3 heads = 129 packed rows -- a tail block of one row, and edges of 32-row slices and of the 128-row
# block that cut a head group (32 = 10 * 3 + 2).  Direct: 3 full key tiles + 43 keys; partial: 12 tiles, 4 per part
PACKED = dict(b=2, h=6, hk=2, sq=43, causal=True, pack=True)
PACKED_DIRECT, PACKED_PARTIAL = dict(api="fa3", sk=235, **PACKED), dict(api="cute", sk=715, splits=3, **PACKED)
# block-sparse: 3 query blocks (the last of 44 rows) x 6 key blocks of 128 (the last of 75 keys: one full 64-key tile + 11 keys),
# causal; `lists` is the seed of block_sparse_oracle.random_lists (1 .. 5 of the 6 key blocks per query block, distinct per batch
# and head; some rows lose all their keys to the mask: O = 0, LSE = +inf).  What the seed has to give is asserted by
# tests/test_fwd_plan.py::test_block_sparse_case_lists
SPARSE = dict(api="bs", b=2, h=4, hk=2, sq=300, sk=715, causal=True, lists=6)
SOFTCAP = 5.0      # unscaled N(0, 1) scores reach |s| ~ 4: tanh(s / 5) is well off its linear part
CHUNK = 300        # attention_chunk: rows see up to 300 keys (>= 3 full tiles) that start and end inside a tile
DROPOUT = 0.17


def _split(case, direct_api, **direct_kw):
    """An FA2-surface case the heuristic splits 3 ways, and the same problem without a split through `direct_api`."""
    direct = dict(case, api=direct_api, **direct_kw)
    return dict(direct=direct, partial=case)


def _paged(**case):
    return dict(direct=dict(api="fa2_paged", splits=1, **case), partial=dict(api="fa2_paged", **case))


def _packed(d, **kw):
    return dict(direct=dict(PACKED_DIRECT, d=d, **kw), partial=dict(PACKED_PARTIAL, d=d, **kw))


def _qv(dv, **kw):
    case = dict(d=64, dv=dv, qv=True, **kw, **SMALL)
    return dict(direct=dict(api="fa3", **case), partial=dict(api="fa3_cache", splits=3, **case))


# form -> {epilogue: case}.  The case id on the GPU is "<form>[-partial]-<bf16|fp16|fp8>" (case_id).
FORMS = {
    # ---- fwd_kernel (compiler-scheduled; fa_fwd_kernel.h) ------------------------------------------------------------------
    "fwd_kernel D=64 waves=4": _split(dict(api="fa2", d=64, **SMALL), "fa3"),
    "fwd_kernel D=64 waves=4 SOFTCAP": _split(dict(api="fa2", d=64, softcap=SOFTCAP, **SMALL), "fa3"),
    "fwd_kernel D=64 waves=8": _paged(d=64, **SMALL),
    "fwd_kernel D=64 waves=8 SOFTCAP": _paged(d=64, softcap=SOFTCAP, **SMALL),
    "fwd_kernel D=64 waves=8 DROPOUT": dict(direct=dict(api="fa2", d=64, dropout=DROPOUT, **SMALL)),
    "fwd_kernel D=64 waves=8 EXTRA": dict(direct=dict(api="fa3", d=64, chunk=CHUNK, **SMALL)),
    "fwd_kernel D=64 waves=8 SOFTCAP EXTRA": dict(direct=dict(api="fa3", d=64, chunk=CHUNK, softcap=SOFTCAP, **SMALL)),
    "fwd_kernel D=128 waves=4": _split(dict(api="fa2", d=128, **SHORTQ), "fa3"),
    "fwd_kernel D=128 waves=4 SOFTCAP": _split(dict(api="fa2", d=128, softcap=SOFTCAP, **SHORTQ), "fa3"),
    "fwd_kernel D=128 waves=8": _paged(d=128, **SMALL),
    "fwd_kernel D=128 waves=8 SOFTCAP": _paged(d=128, softcap=SOFTCAP, **SMALL),
    "fwd_kernel D=128 waves=8 DROPOUT": dict(direct=dict(api="fa2", d=128, dropout=DROPOUT, **SMALL)),
    "fwd_kernel D=128 waves=8 EXTRA": dict(direct=dict(api="fa3", d=128, chunk=CHUNK, **SMALL)),
    "fwd_kernel D=128 waves=8 SOFTCAP EXTRA": dict(direct=dict(api="fa3", d=128, chunk=CHUNK, softcap=SOFTCAP, **SMALL)),
    "fwd_kernel D=256 waves=4": _split(dict(api="fa2", d=256, **SHORTQ), "fa3"),
    "fwd_kernel D=256 waves=4 SOFTCAP": _split(dict(api="fa2", d=256, softcap=SOFTCAP, **SHORTQ), "fa3"),
    "fwd_kernel D=256 waves=4 DROPOUT": dict(direct=dict(api="fa2", d=256, dropout=DROPOUT, **SMALL)),
    "fwd_kernel D=256 waves=4 EXTRA": dict(direct=dict(api="fa3", d=256, chunk=CHUNK, **SMALL)),
    "fwd_kernel D=256 waves=4 SOFTCAP EXTRA": dict(direct=dict(api="fa3", d=256, chunk=CHUNK, softcap=SOFTCAP, **SMALL)),
    # ---- fwd_kernel_w64 (256-row software-pipelined; fa_fwd_kernel_w64.h) ---------------------------------------------------
    "fwd_kernel_w64 D=64 DEFF=64 waves=4": _split(dict(api="fa2", d=64, **WINDOW), "fa2_cache", splits=1),
    "fwd_kernel_w64 D=64 DEFF=64 waves=4 SOFTCAP": _split(dict(api="fa2", d=64, softcap=SOFTCAP, alibi=True, **WINDOW),
                                                          "fa2_cache", splits=1),
    "fwd_kernel_w64 D=128 DEFF=96 waves=4": _split(dict(api="fa2", d=96, **SMALL), "fa2_cache", splits=1),
    "fwd_kernel_w64 D=128 DEFF=128 waves=4": _split(dict(api="fa2", d=128, **SMALL), "fa2_cache", splits=1),
    "fwd_kernel_w64 D=128 DEFF=128 waves=4 SOFTCAP": _split(dict(api="fa2", d=128, softcap=SOFTCAP, alibi=True, **SMALL),
                                                            "fa2_cache", splits=1),
    # more work items than CUs (a shape of tests/test_persistent_gpu.py::SHAPES; seqlen_k a multiple of 64 is the form's rule)
    "fwd_kernel_w64 D=128 DEFF=128 waves=4 PERSIST": dict(direct=dict(api="fa2", d=128, b=16, h=16, hk=4, sq=300, sk=1024,
                                                                      causal=True, rows="sampled")),
    # ---- fwd_kernel_d256 (32 rows per wave around the generated loop; fa_fwd_kernel_d256.h) --------------------------------
    "fwd_kernel_d256 W=64 waves=4 SOFTCAP": dict(direct=dict(api="fa3", d=64, softcap=SOFTCAP, **LONG64)),
    "fwd_kernel_d256 W=64 waves=4 ALIBI": dict(direct=dict(api="fa2", d=64, alibi=True, **LONG64_WIDE)),
    "fwd_kernel_d256 W=96 waves=4 SOFTCAP": dict(direct=dict(api="fa3", d=96, softcap=SOFTCAP, **SMALL)),
    "fwd_kernel_d256 W=96 waves=4 ALIBI": dict(direct=dict(api="fa2", d=96, alibi=True, **WIDE)),
    "fwd_kernel_d256 W=128 waves=4 SOFTCAP": dict(direct=dict(api="fa3", d=128, softcap=SOFTCAP, **SMALL)),
    "fwd_kernel_d256 W=128 waves=4 ALIBI": dict(direct=dict(api="fa2", d=128, alibi=True, **WIDE)),
    "fwd_kernel_d256 W=160 waves=4": dict(direct=dict(api="fa3", d=160, **SMALL)),
    "fwd_kernel_d256 W=160 waves=4 SOFTCAP": dict(direct=dict(api="fa3", d=160, softcap=SOFTCAP, **SMALL)),
    "fwd_kernel_d256 W=160 waves=4 ALIBI": dict(direct=dict(api="fa2", d=160, alibi=True, **WIDE)),
    "fwd_kernel_d256 W=192 waves=4": dict(direct=dict(api="fa3", d=192, **SMALL)),
    "fwd_kernel_d256 W=192 waves=4 SOFTCAP": dict(direct=dict(api="fa3", d=192, softcap=SOFTCAP, **SMALL)),
    "fwd_kernel_d256 W=192 waves=4 ALIBI": dict(direct=dict(api="fa2", d=192, alibi=True, **WIDE)),
    "fwd_kernel_d256 W=256 waves=4": dict(direct=dict(api="fa3", d=256, **SMALL)),
    "fwd_kernel_d256 W=256 waves=4 SOFTCAP": dict(direct=dict(api="fa3", d=256, softcap=SOFTCAP, **SMALL)),
    "fwd_kernel_d256 W=256 waves=4 ALIBI": dict(direct=dict(api="fa2", d=256, alibi=True, **WIDE)),
    # ---- fwd_kernel_qv (q/k head dim <= 64 beside a V head dim in [256, 512]; fa_fwd_kernel_qv.h) ---------------------------
    "fwd_kernel_qv DVT=256 waves=4": _qv(256),
    "fwd_kernel_qv DVT=256 waves=4 SOFTCAP": _qv(256, softcap=SOFTCAP),
    "fwd_kernel_qv DVT=512 waves=4": _qv(512),
    "fwd_kernel_qv DVT=512 waves=4 SOFTCAP": _qv(512, softcap=SOFTCAP),
    # ---- pk_fwd_kernel (PackGQA: the heads of a GQA group packed into the rows of a tile; fa_fwd_kernel_pk.h) ----------------
    "pk_fwd_kernel D=64 waves=4": _packed(64),
    "pk_fwd_kernel D=64 waves=4 SOFTCAP": _packed(64, softcap=SOFTCAP),
    "pk_fwd_kernel D=128 waves=4": _packed(128),
    "pk_fwd_kernel D=128 waves=4 SOFTCAP": _packed(128, softcap=SOFTCAP),
    # ---- bs_fwd_kernel (block-sparse, 128 x 128 blocks from lists; fa_fwd_kernel_bs.h) ---------------------------------------
    # D=256 through d = 256, not d = 192 beside d_v = 128: every column of the 256-wide tile carries data in Q.K^T and in P.V, so
    # a column the kernel drops or doubles shows in both; the narrower pair is a case of tests/test_block_sparse_gpu.py
    "bs_fwd_kernel D=64 waves=4": dict(direct=dict(d=64, **SPARSE)),
    "bs_fwd_kernel D=64 waves=4 SOFTCAP": dict(direct=dict(d=64, softcap=SOFTCAP, **SPARSE)),
    "bs_fwd_kernel D=128 waves=4": dict(direct=dict(d=128, **SPARSE)),
    "bs_fwd_kernel D=128 waves=4 SOFTCAP": dict(direct=dict(d=128, softcap=SOFTCAP, **SPARSE)),
    "bs_fwd_kernel D=256 waves=4": dict(direct=dict(d=256, **SPARSE)),
    "bs_fwd_kernel D=256 waves=4 SOFTCAP": dict(direct=dict(d=256, softcap=SOFTCAP, **SPARSE)),
}
FP8_FORM = "fwd_kernel_fp8 D=128 waves=4"
FP8_CASE = dict(api="fa3", d=128, **SMALL)
EPILOGUES = ("direct", "partial")

# (form, epilogue) no call can launch -- from Python or from the C ABI -- -> (how, rule, target).  `how` is what
# tests/test_fwd_plan.py asserts when the form's own case asks fa_fwd_plan_name for num_splits = 3:
#   "splits=1"   the plan keeps the form and answers splits=1
#   "moves"      the plan is a split plan of the form `target`, which has a partial case of its own
#   "refused"    fa_fwd_block_sparse_validate answers FA_ERR_UNSUPPORTED (and the cute surface raises: asserted on the GPU)
_DROPOUT = ("splits=1", "split_plan: `if (p->p_dropout > 0.f) return sp;` (the FA2 binding asks for num_splits = 1 as well)", None)
_EXTRA = ("splits=1", "split_plan: `if (generic_only(p)) return sp;` -- attention_chunk and a V head dim of its own never split", None)
_D256_RULE = "plan_fwd: `capped` and `d256_ok` require pl.split.splits <= 1"
_D256_TARGET = {  # the form a split call of the d256 form's case is planned on
    "fwd_kernel_d256 W=64 waves=4 SOFTCAP": "fwd_kernel_w64 D=64 DEFF=64 waves=4 SOFTCAP",
    "fwd_kernel_d256 W=64 waves=4 ALIBI": "fwd_kernel_w64 D=64 DEFF=64 waves=4",
    "fwd_kernel_d256 W=96 waves=4 SOFTCAP": "fwd_kernel_w64 D=128 DEFF=128 waves=4 SOFTCAP",
    "fwd_kernel_d256 W=96 waves=4 ALIBI": "fwd_kernel_w64 D=128 DEFF=96 waves=4",
    "fwd_kernel_d256 W=128 waves=4 SOFTCAP": "fwd_kernel_w64 D=128 DEFF=128 waves=4 SOFTCAP",
    "fwd_kernel_d256 W=128 waves=4 ALIBI": "fwd_kernel_w64 D=128 DEFF=128 waves=4",
}
UNREACHABLE = {}
for _form in FORMS:
    if " DROPOUT" in _form:
        UNREACHABLE[(_form, "partial")] = _DROPOUT
    elif " EXTRA" in _form:
        UNREACHABLE[(_form, "partial")] = _EXTRA
    elif _form.startswith("fwd_kernel_d256 "):  # (widths above 128: the compiler-scheduled shape at head-dim tile 256)
        UNREACHABLE[(_form, "partial")] = ("moves", _D256_RULE, _D256_TARGET.get(
            _form, "fwd_kernel D=256 waves=4" + (" SOFTCAP" if " SOFTCAP" in _form else "")))
    elif " PERSIST" in _form:
        UNREACHABLE[(_form, "partial")] = ("moves", "persist_ok: `pl.split.splits > 1` returns false", _form.replace(" PERSIST", ""))
    elif _form.startswith("bs_fwd_kernel "):
        UNREACHABLE[(_form, "partial")] = ("refused", "fa_fwd_block_sparse_validate: `p->num_splits > 1` is FA_ERR_UNSUPPORTED; "
                                                      "cute_interface._flash_attn_fwd_block_sparse raises NotImplementedError", None)
UNREACHABLE[(FP8_FORM, "partial")] = ("splits=1", "split_plan: `p->dtype == FA_DTYPE_FP8_E4M3` returns no split", None)
# (a `cols=2` call -- d_v above 256 without the qv kernel -- is no key of its own: plan_fwd plans its first 256 columns and
#  forces SplitPlan{1, ...}; asked for a split, the shape leaves for fwd_kernel_qv: test_fwd_plan.py::ROWS dv512_*)

# forms only the test hooks (fa_set_default_variant / fa_set_persist_mode) reach, with the test that covers them: none today --
# variant 3 and the forced persistent mode launch instantiations the library also picks by itself (rows above).
HOOK_ONLY = {}

# Every other kernel of the forward device code (csrc/fa_fwd_api.hip) -> the GPU test that compares its effect with a reference,
# and the element types it is instantiated for (None: no template).  test_fwd_plan.py checks the kernels and types against the
# symbols and that the named tests exist.  These kernels leave no plan text behind, so nothing checks mechanically that a
# named test launches its kernel: the table records where a reader finds the comparison, no more.
AUX = {
    # the split-KV merge behind every "partial" key above, in both types: it is compared with a reference only through the merged
    # attention result of those cases (tests/test_kvcache_gpu.py::test_kvcache_split_kv sweeps split counts and empty parts, bf16)
    "combine_splits_kernel": ("tests/test_plan_parity_gpu.py::test_plan_parity", ("bf16", "fp16")),
    "combine_partials_kernel": ("tests/test_combine_gpu.py::test_flash_attn_combine", ("fp32", "fp16", "bf16")),
    "kvcache_append_kernel": ("tests/test_kvcache_gpu.py::test_kvcache", ("bf16", "fp16")),
    "kvcache_append_varlen_kernel": ("tests/test_fa3_ragged_kvcache_gpu.py::test_ragged_append_rotary_both_types", ("bf16", "fp16")),
    "rotary_kernel": ("tests/test_kvcache_gpu.py::test_kvcache_rotary", ("bf16", "fp16")),
    "rotary_varlen_kernel": ("tests/test_fa3_ragged_kvcache_gpu.py::test_ragged_append_rotary_both_types", ("bf16", "fp16")),
    "sdmask_kernel": ("tests/test_dropout_gpu.py::test_dropout_output_and_grads", ("bf16", "fp16")),
    "expand_fp8_kernel": ("tests/test_fp8_fa3_gpu.py::test_fp8_expansion_path_equals_bf16_path", None),
}

# The kernels of AUX that take strides of their own for the caller's tensors -> the GPU test that runs them on strided operands
# (bit-equality with the contiguous call, sentinels around the cache views).  Beside AUX, not in it: that test compares with the
# contiguous call, not with a reference, so AUX keeps naming where the kernel's effect is compared with one.
AUX_STRIDED = {kernel: "tests/test_layout_parity_gpu.py::test_aux_layout_parity"
               for kernel in ("kvcache_append_kernel", "kvcache_append_varlen_kernel", "rotary_kernel", "rotary_varlen_kernel")}
AUX_STRIDED["combine_splits_kernel"] = "tests/test_layout_parity_gpu.py::test_fwd_layout_parity"


def case_id(form, epilogue, dtype):
    """"<form>-<type>" for the direct case (the ids this table had before it knew epilogues), "<form>-partial-<type>"."""
    return f"{form.replace(' ', '_').replace('=', '')}{'' if epilogue == 'direct' else '-' + epilogue}-{dtype}"


def cases():
    """[(form, epilogue, element type, case)] of every GPU case."""
    rows = [(form, ep, dt, by_ep[ep]) for form, by_ep in FORMS.items() for ep in EPILOGUES if ep in by_ep for dt in ("bf16", "fp16")]
    return rows + [(FP8_FORM, "direct", "fp8", FP8_CASE)]


# (element type, kernel form, epilogue) -> GPU case id, "unreachable: <rule>" or "hook-only: <test>"
UNIVERSE = {(dt, form, ep): case_id(form, ep, dt) for form, ep, dt, _ in cases()}
UNIVERSE.update({(dt, form, ep): f"unreachable: {rule}" for (form, ep), (_, rule, _) in UNREACHABLE.items()
                 for dt in (("fp8",) if form == FP8_FORM else ("bf16", "fp16"))})
UNIVERSE.update({key: f"hook-only: {test}" for key, test in HOOK_ONLY.items()})
