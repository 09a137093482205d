"""The plan universe of the forward units over an fp8 (e4m3) KV cache -- csrc/fa_fwd_kv8_api.hip (kv8_fwd_kernel) and
csrc/fa_fwd_qv8_api.hip (qv8_fwd_kernel) -- and of the append unit csrc/fa_kvcache_append_kv8.hip: the sibling of
tests/plan_universe.py, which ends at the edge of csrc/fa_fwd_api.hip.  A plain module, imported by tests/test_kv8_plan.py (which
checks the table against the kernel symbols of the compiled device code, plans every case on the CPU and asserts the geometry
below) and by tests/test_kv8_plan_parity_gpu.py (which asserts that every case launches exactly its key and compares it with
the oracle).

Kernel key = (element type of q, kernel form, epilogue), as in tests/plan_universe.py: the form is what parity_helpers.plan_key
leaves of fa_fwd_kv8_plan_name / fa_fwd_qv8_plan_name (one template instantiation <T, D | DVT, SOFTCAP>), the epilogue the store
path inside it: "direct" (`splits=1`) or "partial" (fp32 partials in the workspace + fa_fwd_combine).  8 forms x 2 epilogues x
{bf16, fp16} = 32 keys, every one with a GPU case: neither plan_kv8 / plan_qv8 nor the split counts forbid one.

A case is plain data for hopper_interface.flash_attn_with_kvcache over a dense e4m3 cache of `cap` rows with the fill levels
`lens` (cache_seqlens), k_descale / v_descale (the tables of tests/test_kv8_kvcache_gpu.py: distinct powers of two per (batch,
kv head), another permutation for V) and `splits` (num_splits); the qv8 forms add qv.  What every case has, asserted by
tests/test_kv8_plan.py through replay() below:
  * at least three full 64-key tiles that no row's mask touches, a tile the causal diagonal cuts, a ragged last tile
    (fill level % 64 != 0) -- in the longest entry; fill levels that differ between the batch entries;
  * h_k = 2 and a GQA group that is no power of two; packed rows (seqlen_q x group) that are no multiple of the kernel's row
    block (128 for kv8, 32 for qv8): a second row block with a short tail, and block and 32-row wave edges that cut a head group;
  * partial cases (num_splits = 3): every part of every row block of the longest entry owns a full tile (12 and 11 key tiles:
    thirds of 4 / 4 / 4 and 4 / 4 / 3).
d = 64 and d = 128 (kv8), d_v = 256 and d_v = 512 (qv8): every column of the tile carries data.

EDGES is the edge set of the partial epilogue (tests/test_kv8_plan_parity_gpu.py::test_split_edge): keyword arguments of the
Case classes of tests/test_kv8_kvcache_gpu.py / tests/test_qv8_kvcache_gpu.py, each run with num_splits = 3 and 1."""

KV8_BLOCK_M, QV8_BLOCK_M = 128, 32   # packed rows per workgroup: fa::PK_BLOCK_M, qv8_fwd_kernel's 32
BLOCK_N = 64
SOFTCAP = 5.0      # as tests/plan_universe.py; the factor in front of the tanh is softmax_scale x the descale(s) of the (batch, kv head)
CAP = 768
DIRECT_LENS, PARTIAL_LENS = (235, 203), (715, 651)   # 3 full tiles + 43 / 11 keys; 11 full tiles + 11 keys / 10 + 11
# kv8: 43 rows x 3 heads = 129 packed rows (a tail block of one row; 32 = 10 * 3 + 2).  qv8: 7 rows x 6 heads = 42 (32 = 5 * 6 + 2)
KV8 = dict(kernel="kv8", b=2, h=6, hk=2, sq=43, causal=True, cap=CAP)
QV8 = dict(kernel="qv8", b=2, h=12, hk=2, sq=7, d=64, qv=True, causal=True, cap=CAP)
EDGE_SPLITS = 3


def _both(base, **kw):
    return dict(direct=dict(base, lens=DIRECT_LENS, splits=1, **kw), partial=dict(base, lens=PARTIAL_LENS, splits=3, **kw))


# form -> {epilogue: case}.  The case id on the GPU is "<form>[-partial]-<bf16|fp16>" (case_id).
FORMS = {
    # ---- kv8_fwd_kernel (packed_rows_fwd over the byte tile; fa_fwd_kernel_kv8.h) -------------------------------------------
    "kv8_fwd_kernel D=64 waves=4": _both(KV8, d=64),
    "kv8_fwd_kernel D=64 waves=4 SOFTCAP": _both(KV8, d=64, softcap=SOFTCAP),
    "kv8_fwd_kernel D=128 waves=4": _both(KV8, d=128),
    "kv8_fwd_kernel D=128 waves=4 SOFTCAP": _both(KV8, d=128, softcap=SOFTCAP),
    # ---- qv8_fwd_kernel (the MLA decode shape; fa_fwd_kernel_qv8.h) ----------------------------------------------------------
    "qv8_fwd_kernel DVT=256 waves=4": _both(QV8, dv=256),
    "qv8_fwd_kernel DVT=256 waves=4 SOFTCAP": _both(QV8, dv=256, softcap=SOFTCAP),
    "qv8_fwd_kernel DVT=512 waves=4": _both(QV8, dv=512),
    "qv8_fwd_kernel DVT=512 waves=4 SOFTCAP": _both(QV8, dv=512, softcap=SOFTCAP),
}
EPILOGUES = ("direct", "partial")
DTYPES = ("bf16", "fp16")

# (form, epilogue) no call can launch -> the rule that forbids it.  None: both plans take any num_splits up to the 64-key blocks
# of the capacity for every form (tests/test_kv8_plan.py plans all 32 keys and asserts that this stays empty or carries rules).
UNREACHABLE = {}

# Every other kernel of the three units -> the GPU test that compares it with a reference, and its element types.
AUX = {
    "kvcache_append_kv8_kernel": ("tests/test_kv8_append_gpu.py::test_every_16bit_value_byte_for_byte", ("bf16", "fp16")),
}


def case_id(form, epilogue, dtype):
    return f"{form.replace(' ', '_').replace('=', '')}{'' if epilogue == 'direct' else '-' + epilogue}-{dtype}"


def cases():
    """[(form, epilogue, element type, case)] of every GPU case."""
    return [(form, ep, dt, by_ep[ep]) for form, by_ep in FORMS.items() for ep in EPILOGUES if ep in by_ep for dt in DTYPES]


# (element type, kernel form, epilogue) -> GPU case id or "unreachable: <rule>"
UNIVERSE = {(dt, form, ep): case_id(form, ep, dt) for form, ep, dt, _ in cases()}
UNIVERSE.update({(dt, form, ep): f"unreachable: {rule}" for (form, ep), rule in UNREACHABLE.items() for dt in DTYPES})


def block_m(kernel):
    return {"kv8": KV8_BLOCK_M, "qv8": QV8_BLOCK_M}[kernel]


def replay(sq, sk, g, block, causal=False, window=(-1, -1), splits=1):
    """The key-range arithmetic of packed_rows_fwd (csrc/fa_fwd_kernel_pk.h) and qv8_fwd_kernel (csrc/fa_fwd_kernel_qv8.h) --
    both compute the same thing -- for one (batch, kv head): `sq` query rows over `sk` visible keys, GQA group `g`, `block`
    packed rows per workgroup.  -> one dict per row block:
        parts  [(n_min, n_max)] per split: its 64-key tiles (split_range, csrc/fa_fwd_kernel.h)
        rows   [(query row, lim_lo, lim_hi)]: the keys [lim_lo, lim_hi) each query row of the block sees (empty: keyless)"""
    wl, wr = window
    if causal:
        wr = 0
    shift, prows, out = sk - sq, sq * g, []
    for pr_lo in range(0, prows, block):
        qr_lo, qr_hi = pr_lo // g, min(prows - 1, pr_lo + block - 1) // g
        key_hi = min(sk, qr_hi + 1 + shift + wr) if wr >= 0 else sk
        key_lo = max(0, qr_lo + shift - wl) if wl >= 0 else 0
        n_min, n_max = key_lo // BLOCK_N, (-(-key_hi // BLOCK_N) if key_hi > 0 else 0)
        parts = []
        for split in range(splits):
            lo, hi = n_min, n_max
            if splits > 1:
                per = int((n_max - n_min + splits - 1) / splits)  # (C++ division truncates)
                hi = min(n_max, n_min + split * per + per)
                lo = min(n_min + split * per, hi)
            parts.append((lo, hi))
        rows = []
        for qr in range(qr_lo, qr_hi + 1):
            lim_hi = min(sk, qr + shift + wr + 1) if wr >= 0 else sk
            lim_lo = max(0, qr + shift - wl) if wl >= 0 else 0
            rows.append((qr, lim_lo, lim_hi))
        out.append(dict(parts=parts, rows=rows))
    return out


def sees(row, part):
    """Whether a row of replay() sees a key inside a part of replay()."""
    (_, lim_lo, lim_hi), (lo, hi) = row, part
    return max(lim_lo, lo * BLOCK_N) < min(lim_hi, hi * BLOCK_N)


# ---- the partial epilogue at its edges: name -> (Case keyword arguments for kv8, for qv8, element types) --------------------
# (the Case defaults: kv8 b2 sq1 h8 hk2 d128 cap320, qv8 b2 sq1 h8 hk1 d64 dv512 cap320; cap 320 = 5 key tiles)
_RAGGED = dict(b=4, sq=4, lens=(257, 100, 70, 16), cu_q=(0, 1, 1, 5, 6), seqused_q=(1, 0, 3, 1), causal=True)
_PAGED = dict(b=3, sq=3, cap=384, lens=(257, 256, 1), causal=True)  # fill levels inside a page and on a page boundary
BOTH, BF16 = ("bf16", "fp16"), ("bf16",)
EDGES = {
    # cu_seqlens_q with a sequence without queries, seqused_q shorter than one range: the (splits, total_q, h, d) / (splits, h,
    # total_q) workspace and the merge's one batch of total_q rows
    "ragged-dense": (dict(_RAGGED, seed=61), dict(_RAGGED, seed=61), BOTH),
    "ragged-page16": (dict(_RAGGED, page=16, seed=62), dict(_RAGGED, page=16, seed=62), BOTH),
    "page64": (dict(_PAGED, page=64, seed=63), dict(_PAGED, page=64, seed=63), BF16),   # one page per tile
    "page16": (dict(_PAGED, page=16, seed=64), dict(_PAGED, page=16, seed=64), BF16),   # one page per staged row
    "cache_batch_idx": (dict(b=3, sq=3, batch_idx=(2, 0, 2), lens=(257, 70, 130), causal=True, seed=65),
                        dict(b=3, sq=3, batch_idx=(2, 0, 2), lens=(257, 70, 130), causal=True, seed=65), BF16),
    "leftpad_k": (dict(sq=3, leftpad=(3, 70), lens=(40, 300), causal=True, seed=66),
                  dict(sq=3, leftpad=(3, 70), lens=(40, 300), causal=True, seed=66), BF16),
    # a part emptied by the MASK: one row block whose key tiles are 2, 3, 4 -- one per part -- under a causal left window; its
    # first rows see tiles 2 (and 3) only, its last rows tiles (3 and) 4 only, every row sees keys (test_kv8_plan.py)
    "masked-part": (dict(b=1, sq=130, h=2, hk=2, lens=(300,), causal=True, window=(40, 0), seed=67),
                    dict(b=1, sq=40, h=2, hk=2, lens=(290,), causal=True, window=(80, 0), seed=67), BOTH),
    # seqlen_q above the first entry's fill level: its first 23 query rows see no key, in a row block whose tile 0 is loaded
    # and multiplied for the rows behind them
    "keyless-rows": (dict(sq=43, h=6, hk=2, lens=(20, 257), causal=True, seed=68),
                     dict(sq=43, h=4, hk=2, lens=(20, 257), causal=True, seed=68), BF16),
    # several row blocks: 130 x 4 = 520 packed rows (five blocks of 128), 40 x 4 = 160 (five blocks of 32)
    "row-blocks": (dict(b=1, sq=130, h=8, hk=2, d=64, lens=(300,), causal=True, seed=69),
                   dict(sq=40, h=4, hk=1, lens=(300, 257), causal=True, seed=69), BF16),
}


def edge_cases():
    """[(edge name, kernel, element type, Case keyword arguments)]"""
    return [(name, kernel, dt, kw) for name, (kv8, qv8, dts) in EDGES.items() for kernel, kw in (("kv8", kv8), ("qv8", qv8))
            for dt in dts]


def edge_geometry(kernel, kw):
    """replay() per batch entry of an edge case: the Case defaults filled in, the visible keys past leftpad_k, the used
    query rows of a ragged batch."""
    b = kw.get("b", 2)
    h, hk = kw.get("h", 8), kw.get("hk", 2 if kernel == "kv8" else 1)
    lens, leftpad = kw.get("lens", (1, 257)), kw.get("leftpad", (0,) * b)
    if "cu_q" in kw:
        sqs = kw.get("seqused_q") or [kw["cu_q"][i + 1] - kw["cu_q"][i] for i in range(b)]
    else:
        sqs = (kw.get("sq", 1),) * b
    return [replay(sqs[i], max(lens[i] - leftpad[i], 0), h // hk, block_m(kernel), kw.get("causal", False), kw.get("window", (-1, -1)),
                   EDGE_SPLITS) for i in range(b)]
