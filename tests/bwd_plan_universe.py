"""The backward plan universe: every kernel the launch switch of csrc/fa_bwd_api.hip (run_bwd, driven by plan_bwd) instantiates,
each with the GPU cases that launch it (tests/test_bwd_plan_parity_gpu.py).  A plain module, imported by tests/test_bwd_plan.py
(which checks the table against the kernel symbols of the compiled device code, the cases against fa_bwd_plan_name and the
shapes against tests/bwd_run_model.py) and by the parity test (which asserts after every backward that exactly the stated plan
ran).

Kernel key = (element type, one segment of the plan text of fa_bwd_plan_name): one template instantiation.
sink_grad_kernel has no element type and no segment: key ("any", "sink_grad_kernel"), launched behind the plan of the sink case.

A case is plain data.  `api`: "fa2" = flash_attn_func, "fa2_varlen" = flash_attn_varlen_func, "fa3" = the FA3-shaped
flash_attn_func, "cute" = the cute-shaped flash_attn_func (learnable sink).  Dense cases give b / h / hk / sq / sk, varlen cases
`lens_q` / `lens_k`.  Every case runs in bf16 and fp16.

Shapes: the smallest that reach the branches, chosen with the run model, not by taste.
  * ALIGNED (sq 320 = five 64-row query tiles, sk 462 = three 128-key blocks + 78 keys = seven 64-key tiles + 14 keys, causal,
    sk - sq = 142): for the instantiations with a generated loop.  seqlen_q has to be a multiple of 64 here: a run is cut by the
    head change of the GQA group (count = left - 1 < plain) only when the last query tile of the head is itself plain, i.e. full.
    dK/dV: runs of 4 from both buffers in key block 0, masked tile -> run of 3 in block 1, last block ragged;  dQ: runs of 2..6,
    masked diagonal tiles behind them, ragged last key tile, the second 256-row block has three inactive waves.
  * RAGGED (sq 330, sk 460: a sixth query tile of 10 rows, sk - sq = 130): for everything else -- the windows (a left window
    never leaves the last query tile of a key block plain, so there is no head-change cut to show) and the C++-only kernels.
  * the varlen batch has both kinds of sequence (333 x 470 ragged, 320 x 462 aligned) beside the degenerate ones.
  * UNITS (b 3, h 12, hk 6): 18 (batch, kv head) units in the dK/dV launch -- 16 dealt whole to the 8 XCDs, 2 block by block --
    and 36 (batch, head) units in the dQ launch -- 32 whole, 4 block by block (decode_block, tests/test_scheduler_map.py).
"""

ALIGNED = dict(b=2, h=4, hk=2, sq=320, sk=462, causal=True)
RAGGED = dict(b=2, h=4, hk=2, sq=330, sk=460, causal=True)
WINDOW = dict(b=2, h=4, hk=2, sq=330, sk=460, window=(200, 100))   # both sides shorter than the sequences
UNITS = dict(b=3, h=12, hk=6, sq=320, sk=462, causal=True)
# cu_seqlens_q 0 75 75 76 409 729, cu_seqlens_k 0 0 70 120 590 1052: no boundary on a multiple of 64; sequence 0 has no keys,
# sequence 1 no queries, sequence 2 one query, sequences 3 (ragged) and 4 (aligned) are long enough for generated runs
VARLEN = dict(h=4, hk=2, lens_q=(75, 0, 1, 333, 320), lens_k=(0, 70, 50, 470, 462), causal=True)
SOFTCAP = 5.0   # unscaled N(0, 1) scores reach |s| ~ 4: tanh(s / 5) is well off its linear part
DROPOUT = 0.17

DOT8, DOT16, DOT32 = "bwd_dot LPR=8", "bwd_dot LPR=16", "bwd_dot LPR=32"


def _p256(deff, flag=""):
    return " | ".join([DOT32, f"bwd_dkdv D=256 NB=1 DEFF={deff} PART=1{flag}", f"bwd_dkdv D=256 NB=1 DEFF={deff} PART=2{flag}",
                       f"bwd_dq D=256 NB=1 DEFF={deff}{flag}"])


PLAN_D64 = f"{DOT8} | bwd_dkdv D=64 NB=1 DEFF=64 | bwd_dq D=64 NB=2 DEFF=64"
PLAN_D64_ALIBI = f"{DOT8} | bwd_dkdv D=64 NB=2 DEFF=64 | bwd_dq D=64 NB=2 DEFF=64"
PLAN_D64_SOFTCAP = f"{DOT8} | bwd_dkdv D=64 NB=2 DEFF=64 SOFTCAP | bwd_dq D=64 NB=2 DEFF=64 SOFTCAP"
PLAN_D64_DROPOUT = f"{DOT8} | bwd_dkdv D=64 NB=2 DEFF=64 DROPOUT | bwd_dq D=64 NB=2 DEFF=64 DROPOUT"
PLAN_D96 = f"{DOT16} | bwd_dkdv D=128 NB=1 DEFF=96 | bwd_dq D=128 NB=2 DEFF=96"
PLAN_D128 = f"{DOT16} | bwd_dkdv D=128 NB=1 DEFF=128 | bwd_dq D=128 NB=2 DEFF=128"
PLAN_D128_SOFTCAP = f"{DOT16} | bwd_dkdv D=128 NB=1 DEFF=128 SOFTCAP | bwd_dq D=128 NB=2 DEFF=128 SOFTCAP"
PLAN_D128_DROPOUT = f"{DOT16} | bwd_dkdv D=128 NB=1 DEFF=128 DROPOUT | bwd_dq D=128 NB=2 DEFF=128 DROPOUT"
PLAN_D160, PLAN_D192, PLAN_D256 = _p256(160), _p256(192), _p256(256)
PLAN_D256_SOFTCAP, PLAN_D256_DROPOUT = _p256(256, " SOFTCAP"), _p256(256, " DROPOUT")

# case -> (plan, problem).  The first 13 are the 13 distinct plans; the rest reuse kernels through other run-time branches.
CASES = {
    "d64": (PLAN_D64, dict(api="fa2", d=64, **ALIGNED)),
    "d64_alibi": (PLAN_D64_ALIBI, dict(api="fa2", d=64, alibi=True, **RAGGED)),
    "d64_softcap": (PLAN_D64_SOFTCAP, dict(api="fa2", d=64, softcap=SOFTCAP, **RAGGED)),
    "d64_dropout": (PLAN_D64_DROPOUT, dict(api="fa2", d=64, dropout=DROPOUT, **RAGGED)),
    "d96": (PLAN_D96, dict(api="fa2", d=96, **ALIGNED)),
    "d128": (PLAN_D128, dict(api="fa2", d=128, **ALIGNED)),
    "d128_softcap": (PLAN_D128_SOFTCAP, dict(api="fa2", d=128, softcap=SOFTCAP, **RAGGED)),
    "d128_dropout": (PLAN_D128_DROPOUT, dict(api="fa2", d=128, dropout=DROPOUT, **RAGGED)),
    "d160": (PLAN_D160, dict(api="fa2", d=160, **RAGGED)),
    "d192": (PLAN_D192, dict(api="fa2", d=192, **RAGGED)),
    "d256": (PLAN_D256, dict(api="fa2", d=256, **RAGGED)),
    "d256_softcap": (PLAN_D256_SOFTCAP, dict(api="fa2", d=256, softcap=SOFTCAP, **RAGGED)),
    "d256_dropout": (PLAN_D256_DROPOUT, dict(api="fa2", d=256, dropout=DROPOUT, **RAGGED)),
    # ---- path cases ----------------------------------------------------------------------------------------------------------
    "d128_alibi": (PLAN_D128, dict(api="fa2", d=128, alibi=True, **ALIGNED)),   # the plain kernels, the loop never entered
    "window_d64": (PLAN_D64, dict(api="fa2", d=64, **WINDOW)),
    "window_d96": (PLAN_D96, dict(api="fa2", d=96, **WINDOW)),   # (the DEFF = 96 loops under both window limits)
    "window_d128": (PLAN_D128, dict(api="fa2", d=128, **WINDOW)),
    "varlen_d64": (PLAN_D64, dict(api="fa2_varlen", d=64, **VARLEN)),
    "varlen_d128": (PLAN_D128, dict(api="fa2_varlen", d=128, **VARLEN)),
    "varlen_d256": (PLAN_D256, dict(api="fa2_varlen", d=256, **VARLEN)),
    "fa3_d192_dv128": (PLAN_D192, dict(api="fa3", d=192, dv=128, **RAGGED)),
    "fa3_d64_dv256": (PLAN_D256, dict(api="fa3", d=64, dv=256, **RAGGED)),
    "sink_d128": (PLAN_D128, dict(api="cute", d=128, sink=True, **ALIGNED)),
    "units_d64": (PLAN_D64, dict(api="fa2", d=64, **UNITS)),
    "units_d128": (PLAN_D128, dict(api="fa2", d=128, **UNITS)),
}
DTYPES = ("bf16", "fp16")
SINK_KEY = ("any", "sink_grad_kernel")

# kernels the device code contains and no plan launches, with the reason: run_bwd picks the D = 64 dK/dV block count at run time
# (`pl.nbk == 1 ? <NB = 1> : <NB = 2>`), which instantiates the one-block form for the softcap and dropout switches too, where
# plan_bwd never asks for it.
UNREACHABLE = {(dt, f"bwd_dkdv D=64 NB=1 DEFF=64 {flag}"): "plan_bwd: NB = 1 at D = 64 only for the plain problem"
               for dt in DTYPES for flag in ("SOFTCAP", "DROPOUT")}


def case_id(name, dt):
    return f"{name}-{dt}"


def segments(plan):
    return plan.split(" | ")


# (element type, segment) -> the GPU case ids that launch it
UNIVERSE = {}
for _name, (_plan, _case) in CASES.items():
    for _dt in DTYPES:
        for _seg in segments(_plan):
            UNIVERSE.setdefault((_dt, _seg), []).append(case_id(_name, _dt))
        if _case.get("sink"):
            UNIVERSE.setdefault(SINK_KEY, []).append(case_id(_name, _dt))

# which instantiations carry a generated loop (fa_bwd_kernel.h: plain problems at head-dim tiles 64 / 128)
LOOP_SEGMENTS = {"bwd_dkdv D=64 NB=1 DEFF=64", "bwd_dkdv D=128 NB=1 DEFF=96", "bwd_dkdv D=128 NB=1 DEFF=128",
                 "bwd_dq D=64 NB=2 DEFF=64", "bwd_dq D=128 NB=2 DEFF=96", "bwd_dq D=128 NB=2 DEFF=128"}


def sequences(case):
    """[(sq, sk)] of the case: one pair for a dense batch, one per sequence for a varlen one."""
    return list(zip(case["lens_q"], case["lens_k"])) if "lens_q" in case else [(case["sq"], case["sk"])]
