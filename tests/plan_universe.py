"""The plan universe: every forward *kernel key* the launch tables of csrc/fa_fwd_api.hip can instantiate, each with the GPU
parity case that runs it (tests/test_plan_parity_gpu.py).  A plain module, imported by tests/test_fwd_plan.py (which checks the
table against the kernel symbols of the compiled device code: a kernel form added without a row here fails on the CPU) and by
the parity test (which asserts that every case launches exactly its key).

Kernel key = (element type, plan name of fa_fwd_plan_name without `block_m=`, `splits=`, `cols=` and `fp8_expand`).

A case is plain data: `api` is the public entry point ("fa2" = flash_attn_func, "fa2_paged" = flash_attn_with_kvcache on a
paged cache, "fa3" = the FA3-shaped flash_attn_func), the rest its problem.  Every case sweeps at least three full 64-key
tiles, a masked tile (causal diagonal, window edge or chunk edge) and a ragged last tile (seqlen_k % 64 != 0; the persistent
form only takes multiples of 64), with seqlen_q no multiple of block_m.  What decides the routing (plan_fwd):
  * (consequence of the next rule: the FA2-surface cases on SMALL / SHORTQ / WINDOW -- plain fwd_kernel_w64, fwd_kernel waves=4,
    the paged waves=8 forms -- run split 3 ways with the merge behind them, about 4 key tiles per split; the key ignores
    `splits=`, so the unsplit epilogue of those instantiations is not required by this table -- it is left to the shape sweeps
    of tests/test_flash_attn_gpu.py and tests/test_kvcache_gpu.py)
  * FA2 dense calls split by heuristic when (m-blocks x heads x batch) <= 128 (512 for the 4-wave shape) and seqlen_k >= 512;
    the width-64/96/128 forms of fwd_kernel_d256 are planned without a split only, so their ALiBi cases (FA2 surface only)
    carry 72 heads x batch; the FA3 surface never splits by itself, the softcap cases use it with small batches;
  * head-dim tile 64 under a causal mask runs the 4-wave compiler-scheduled shape up to seqlen_k 2048 (up to 512 otherwise):
    the 256-row kernel and fwd_kernel_d256 W=64 need longer keys (`rows="sampled"`: the oracle is evaluated on sampled rows);
  * seqlen_q <= 128 dense runs the 4-wave compiler-scheduled shape at every head dim.
"""

SMALL = dict(b=2, h=4, hk=2, sq=300, sk=715, causal=True)     # GQA 2; 11 full key tiles + 11 keys
WIDE = dict(b=3, h=24, hk=8, sq=300, sk=715, causal=True)     # GQA 3; > 128 work items: no heuristic split
SHORTQ = dict(b=2, h=4, hk=2, sq=100, sk=715, causal=True)    # seqlen_q <= 128
LONG64 = dict(b=1, h=2, hk=1, sq=2100, sk=2250, causal=True)  # head dim 64 causal past seqlen_k 2048
LONG64_WIDE = dict(b=1, h=16, hk=8, sq=2100, sk=2250, causal=True, rows="sampled")
WINDOW = dict(b=2, h=4, hk=2, sq=300, sk=715, window=(400, 100))
SOFTCAP = 5.0      # unscaled N(0, 1) scores reach |s| ~ 4: tanh(s / 5) is well off its linear part
CHUNK = 300        # attention_chunk: rows see up to 300 keys (>= 3 full tiles) that start and end inside a tile
DROPOUT = 0.17

# form -> case.  The case id on the GPU is "<form>-<bf16|fp16>" (fp8: "<form>-fp8").
FORMS = {
    # ---- fwd_kernel (compiler-scheduled; fa_fwd_kernel.h) ------------------------------------------------------------------
    "fwd_kernel D=64 waves=4": dict(api="fa2", d=64, **SMALL),
    "fwd_kernel D=64 waves=4 SOFTCAP": dict(api="fa2", d=64, softcap=SOFTCAP, **SMALL),
    "fwd_kernel D=64 waves=8": dict(api="fa2_paged", d=64, **SMALL),
    "fwd_kernel D=64 waves=8 SOFTCAP": dict(api="fa2_paged", d=64, softcap=SOFTCAP, **SMALL),
    "fwd_kernel D=64 waves=8 DROPOUT": dict(api="fa2", d=64, dropout=DROPOUT, **SMALL),
    "fwd_kernel D=64 waves=8 EXTRA": dict(api="fa3", d=64, chunk=CHUNK, **SMALL),
    "fwd_kernel D=64 waves=8 SOFTCAP EXTRA": dict(api="fa3", d=64, chunk=CHUNK, softcap=SOFTCAP, **SMALL),
    "fwd_kernel D=128 waves=4": dict(api="fa2", d=128, **SHORTQ),
    "fwd_kernel D=128 waves=4 SOFTCAP": dict(api="fa2", d=128, softcap=SOFTCAP, **SHORTQ),
    "fwd_kernel D=128 waves=8": dict(api="fa2_paged", d=128, **SMALL),
    "fwd_kernel D=128 waves=8 SOFTCAP": dict(api="fa2_paged", d=128, softcap=SOFTCAP, **SMALL),
    "fwd_kernel D=128 waves=8 DROPOUT": dict(api="fa2", d=128, dropout=DROPOUT, **SMALL),
    "fwd_kernel D=128 waves=8 EXTRA": dict(api="fa3", d=128, chunk=CHUNK, **SMALL),
    "fwd_kernel D=128 waves=8 SOFTCAP EXTRA": dict(api="fa3", d=128, chunk=CHUNK, softcap=SOFTCAP, **SMALL),
    "fwd_kernel D=256 waves=4": dict(api="fa2", d=256, **SHORTQ),
    "fwd_kernel D=256 waves=4 SOFTCAP": dict(api="fa2", d=256, softcap=SOFTCAP, **SHORTQ),
    "fwd_kernel D=256 waves=4 DROPOUT": dict(api="fa2", d=256, dropout=DROPOUT, **SMALL),
    "fwd_kernel D=256 waves=4 EXTRA": dict(api="fa3", d=256, chunk=CHUNK, **SMALL),
    "fwd_kernel D=256 waves=4 SOFTCAP EXTRA": dict(api="fa3", d=256, chunk=CHUNK, softcap=SOFTCAP, **SMALL),
    # ---- fwd_kernel_w64 (256-row software-pipelined; fa_fwd_kernel_w64.h) ---------------------------------------------------
    "fwd_kernel_w64 D=64 DEFF=64 waves=4": dict(api="fa2", d=64, **WINDOW),
    "fwd_kernel_w64 D=64 DEFF=64 waves=4 SOFTCAP": dict(api="fa2", d=64, softcap=SOFTCAP, alibi=True, **WINDOW),
    "fwd_kernel_w64 D=128 DEFF=96 waves=4": dict(api="fa2", d=96, **SMALL),
    "fwd_kernel_w64 D=128 DEFF=128 waves=4": dict(api="fa2", d=128, **SMALL),
    "fwd_kernel_w64 D=128 DEFF=128 waves=4 SOFTCAP": dict(api="fa2", d=128, softcap=SOFTCAP, alibi=True, **SMALL),
    # more work items than CUs (a shape of tests/test_persistent_gpu.py::SHAPES; seqlen_k a multiple of 64 is the form's rule)
    "fwd_kernel_w64 D=128 DEFF=128 waves=4 PERSIST": dict(api="fa2", d=128, b=16, h=16, hk=4, sq=300, sk=1024, causal=True,
                                                          rows="sampled"),
    # ---- fwd_kernel_d256 (32 rows per wave around the generated loop; fa_fwd_kernel_d256.h) --------------------------------
    "fwd_kernel_d256 W=64 waves=4 SOFTCAP": dict(api="fa3", d=64, softcap=SOFTCAP, **LONG64),
    "fwd_kernel_d256 W=64 waves=4 ALIBI": dict(api="fa2", d=64, alibi=True, **LONG64_WIDE),
    "fwd_kernel_d256 W=96 waves=4 SOFTCAP": dict(api="fa3", d=96, softcap=SOFTCAP, **SMALL),
    "fwd_kernel_d256 W=96 waves=4 ALIBI": dict(api="fa2", d=96, alibi=True, **WIDE),
    "fwd_kernel_d256 W=128 waves=4 SOFTCAP": dict(api="fa3", d=128, softcap=SOFTCAP, **SMALL),
    "fwd_kernel_d256 W=128 waves=4 ALIBI": dict(api="fa2", d=128, alibi=True, **WIDE),
    "fwd_kernel_d256 W=160 waves=4": dict(api="fa3", d=160, **SMALL),
    "fwd_kernel_d256 W=160 waves=4 SOFTCAP": dict(api="fa3", d=160, softcap=SOFTCAP, **SMALL),
    "fwd_kernel_d256 W=160 waves=4 ALIBI": dict(api="fa2", d=160, alibi=True, **WIDE),
    "fwd_kernel_d256 W=192 waves=4": dict(api="fa3", d=192, **SMALL),
    "fwd_kernel_d256 W=192 waves=4 SOFTCAP": dict(api="fa3", d=192, softcap=SOFTCAP, **SMALL),
    "fwd_kernel_d256 W=192 waves=4 ALIBI": dict(api="fa2", d=192, alibi=True, **WIDE),
    "fwd_kernel_d256 W=256 waves=4": dict(api="fa3", d=256, **SMALL),
    "fwd_kernel_d256 W=256 waves=4 SOFTCAP": dict(api="fa3", d=256, softcap=SOFTCAP, **SMALL),
    "fwd_kernel_d256 W=256 waves=4 ALIBI": dict(api="fa2", d=256, alibi=True, **WIDE),
    # ---- fwd_kernel_qv (q/k head dim <= 64 beside a V head dim in [256, 512]; fa_fwd_kernel_qv.h) ---------------------------
    "fwd_kernel_qv DVT=256 waves=4": dict(api="fa3", d=64, dv=256, qv=True, **SMALL),
    "fwd_kernel_qv DVT=256 waves=4 SOFTCAP": dict(api="fa3", d=64, dv=256, qv=True, softcap=SOFTCAP, **SMALL),
    "fwd_kernel_qv DVT=512 waves=4": dict(api="fa3", d=64, dv=512, qv=True, **SMALL),
    "fwd_kernel_qv DVT=512 waves=4 SOFTCAP": dict(api="fa3", d=64, dv=512, qv=True, softcap=SOFTCAP, **SMALL),
}
FP8_FORM = "fwd_kernel_fp8 D=128 waves=4"
FP8_CASE = dict(api="fa3", d=128, **SMALL)

# forms only the test hooks (fa_set_default_variant / fa_set_persist_mode) reach, with the test that covers them: none today --
# variant 3 and the forced persistent mode launch instantiations the library also picks by itself (rows above).
HOOK_ONLY = {}


def case_id(form, dtype):
    return f"{form.replace(' ', '_').replace('=', '')}-{dtype}"


# (element type, kernel key) -> GPU case id, or "hook-only: <test>"
UNIVERSE = {(dt, form): case_id(form, dt) for form in FORMS for dt in ("bf16", "fp16")}
UNIVERSE[("fp8", FP8_FORM)] = case_id(FP8_FORM, "fp8")
UNIVERSE.update({key: f"hook-only: {test}" for key, test in HOOK_ONLY.items()})
