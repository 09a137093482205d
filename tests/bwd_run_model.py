"""The per-wave tile sweep of the two backward MFMA kernels (csrc/fa_bwd_kernel.h) restated in plain Python -- a plain module,
not collected; tests/test_scheduler_map.py restates decode_block() the same way.  tests/test_bwd_plan.py uses it to show, on
the CPU, that the shapes of tests/bwd_plan_universe.py reach the generated asm loops (BwdLoop64/96/128, BwdDqLoop64/96/128)
the way the table claims: how long the runs are, from which LDS buffer they are entered, what stands before and behind them.

Both functions follow one sequence (sq queries, sk keys; a varlen batch is modelled sequence by sequence) and return
{(block, wave): [Step, ...]} in the order the wave executes.  A Step is one of
    run       `length` tiles through the generated loop, entered with LDS buffer `cur`; `lo` / `hi` say what bounds the run
    masked    one tile on the C++ path with the masks evaluated
    unmasked  one tile on the C++ path without
    skipped   one tile this wave has nothing to do for (the loads and barriers still happen)
`index` is the loop variable at the step (dK/dV: `it`, which counts the query tiles of every head of the GQA group; dQ: the
key tile `n`).  `generated` says whether the instantiation has the loop at all (plain problems at head-dim tiles 64 / 128:
NB = 1 for dK/dV, NB = 2 for dQ); ALiBi keeps the instantiation and never enters the loop.
"""
from collections import namedtuple

BM = 64       # query rows per streamed tile of bwd_dkdv_kernel
BLOCK_N = 64  # keys per streamed tile of bwd_dq_kernel
DQ_NBUF = 3   # K / V LDS slots of bwd_dq_kernel at head-dim tiles <= 128

Step = namedtuple("Step", "kind index length cur head lo hi", defaults=(1, None, None, None, None))


def normalize_window(window, causal, seqlen_k, fa3=False):
    """(window_left, window_right) as fa_bwd hands them to the kernels (csrc/fa_bwd_api.hip); seqlen_k is the batch's maximum."""
    wl, wr = window
    if causal:
        wr = 0
    if not fa3:
        if wl >= seqlen_k:
            wl = -1
        if wr >= seqlen_k:
            wr = -1
        if causal:
            wr = 0
        if wl >= 0 and wr < 0:
            wr = seqlen_k
    return wl, wr


def dkdv_steps(sq, sk, window=(-1, -1), h_ratio=1, nb=1, alibi=False, generated=True):
    """bwd_dkdv_kernel.  window: normalized."""
    wl, wr = window
    wkeys, block_k, shift = 32 * nb, 128 * nb, sk - sq
    out = {}
    for block in range((sk + block_k - 1) // block_k):
        n0 = block * block_k
        last_key = min(sk, n0 + block_k) - 1
        row_lo, row_hi = 0, sq
        if wr >= 0:
            row_lo = max(0, n0 - shift - wr)
        if wl >= 0:
            row_hi = min(sq, last_key - shift + wl + 1)
        m_min = row_lo // BM
        m_max = (row_hi + BM - 1) // BM if row_hi > row_lo else m_min
        num_m = m_max - m_min
        total_it = num_m * h_ratio
        for wave in range(4):
            key_w0 = n0 + wave * wkeys
            steps, it = [], 0
            while it < total_it:
                cur, head, row0 = it & 1, it // num_m, (m_min + it % num_m) * BM
                if generated and nb == 1:
                    left = num_m - it % num_m
                    hi_row, hi = sq - BM, "seq_end"
                    if wl >= 0 and key_w0 - (BM - 1) - shift + wl < hi_row:
                        hi_row, hi = key_w0 - (BM - 1) - shift + wl, "window_left"
                    plain = (hi_row - row0) // BM + 1 if row0 <= hi_row else 0
                    if key_w0 + wkeys > sk:
                        plain = 0
                    if wr >= 0 and key_w0 + wkeys - 1 > row0 + shift + wr:
                        plain = 0
                    count = min(plain, left - 1)  # the tile behind a run must belong to the same head
                    if left - 1 < plain:
                        hi = "head_change"
                    if count >= 2 and not alibi:
                        lo = None  # what kept the tile in front of the run off the loop
                        if it % num_m > 0 and wr >= 0 and key_w0 + wkeys - 1 > row0 - BM + shift + wr:
                            lo = "window_right"
                        steps.append(Step("run", it, count, cur, head, lo, hi))
                        it += count
                        continue
                skip = key_w0 >= sk
                if wr >= 0:
                    skip = skip or key_w0 > row0 + BM - 1 + shift + wr
                if wl >= 0:
                    skip = skip or key_w0 + wkeys - 1 < row0 + shift - wl
                need_mask = key_w0 + wkeys > sk or row0 + BM > sq
                if wr >= 0:
                    need_mask = need_mask or key_w0 + wkeys - 1 > row0 + shift + wr
                if wl >= 0:
                    need_mask = need_mask or key_w0 < row0 + BM - 1 + shift - wl
                steps.append(Step("skipped" if skip else "masked" if need_mask else "unmasked", it, 1, cur, head))
                it += 1
            out[(block, wave)] = steps
    return out


def dq_steps(sq, sk, window=(-1, -1), nb=2, alibi=False, generated=True):
    """bwd_dq_kernel; a wave with wrow >= sq is inactive: every step of it is `skipped` and it never enters the loop."""
    wl, wr = window
    wrows, block_m, shift = 32 * nb, 128 * nb, sk - sq
    out = {}
    for block in range((sq + block_m - 1) // block_m):
        row_lo = block * block_m
        row_hi = min(sq, row_lo + block_m)
        key_hi, key_lo = sk, 0
        if wr >= 0:
            key_hi = min(sk, row_hi + shift + wr)
        if wl >= 0:
            key_lo = max(0, row_lo + shift - wl)
        n_min = key_lo // BLOCK_N
        n_max = (key_hi + BLOCK_N - 1) // BLOCK_N if key_hi > 0 else 0
        for wave in range(4):
            wrow = row_lo + wave * wrows
            wave_active = wrow < sq
            steps, n = [], n_min
            while n < n_max:
                cur = (n - n_min) % DQ_NBUF
                if generated and nb == 2:
                    n_hi, hi = sk // BLOCK_N - 1, "keys_end"
                    if wr >= 0:
                        lim = wrow + shift + wr - (BLOCK_N - 1)
                        lim_n = lim // BLOCK_N if lim >= 0 else -1
                        if lim_n < n_hi:
                            n_hi, hi = lim_n, "window_right"
                    n_lo = 0
                    if wl >= 0:
                        lo_key = wrow + wrows - 1 + shift - wl
                        n_lo = (lo_key + BLOCK_N - 1) // BLOCK_N if lo_key > 0 else 0
                    count = min(n_hi, n_max - 1) - n + 1 if n_lo <= n <= n_hi else 0
                    if count >= 2 and wave_active and not alibi:
                        steps.append(Step("run", n, count, cur, None, "window_left" if n == n_lo and n_lo > 0 else None, hi))
                        n += count
                        continue
                k0 = n * BLOCK_N
                skip = not wave_active
                if wr >= 0:
                    skip = skip or k0 > wrow + wrows - 1 + shift + wr
                if wl >= 0:
                    skip = skip or k0 + BLOCK_N - 1 < wrow + shift - wl
                need_mask = k0 + BLOCK_N > sk
                if wr >= 0:
                    need_mask = need_mask or k0 + BLOCK_N - 1 > wrow + shift + wr
                if wl >= 0:
                    need_mask = need_mask or k0 < wrow + wrows - 1 + shift - wl
                steps.append(Step("skipped" if skip else "masked" if need_mask else "unmasked", n, 1, cur))
                n += 1
            out[(block, wave)] = steps
    return out


def runs(sweeps):
    return [s for steps in sweeps.values() for s in steps if s.kind == "run"]


def neighbours(sweeps):
    """[(kind of the step in front of a run or None, the run, kind of the step behind it or None)]"""
    out = []
    for steps in sweeps.values():
        for i, s in enumerate(steps):
            if s.kind == "run":
                out.append((steps[i - 1].kind if i else None, s, steps[i + 1].kind if i + 1 < len(steps) else None))
    return out
