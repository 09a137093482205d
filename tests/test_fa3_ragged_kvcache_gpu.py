"""GPU tests of one continuous-batching step on the FA3 surface: `flash_attn_with_kvcache(..., cu_seqlens_q=, max_seqlen_q=,
cu_seqlens_k_new=)` (hopper/flash_attn_interface.py:640-800; the reference's test_flash_attn_kvcache runs it as varlen_q=True,
hopper/test_flash_attn.py:626, 704-727, 864-919) -- ragged queries (total_q, h, d) that mix prefill chunks with single-token
decodes over a batched or paged KV cache, the new keys / values ragged as well.

Reference: oracle.attention_ref on the padded tensors with query_padding_mask / key_padding_mask (the reference's own test builds
it the same way).  Tolerances are the project's: |out - ref| <= 3 |pt - ref| + 1e-5 (tests/test_fa3_kvcache_gpu.py) and the LSE
rule of tests/parity_helpers.py (same +inf pattern, 2e-3 on the finite entries).  Cache contents are compared bit for bit.

The rotary tables of this file are not unit-norm angles but multiples of 1/8 in [-1, 1], one random pattern per position: the
rotation formula does not care, every product of a 16-bit value with such a factor is exact in fp32, and so the rotated row is the
same bit pattern whether a compiler contracts x1 c - x2 s into a fused multiply-add (the kernels) or not (the oracle) -- which
is what makes "bit for bit" a fair demand on rows that went through arithmetic."""
import pytest
import torch

from oracle import attention_ref as oracle
from parity_helpers import last_plan

pytestmark = pytest.mark.gpu
DEV = "cuda"
I32 = torch.int32


def _fa3():
    from flash_attention_annotated_amd import hopper_interface
    return hopper_interface


def _cu(lens):
    return torch.tensor([sum(lens[:i]) for i in range(len(lens) + 1)], dtype=I32)


def _tables(rows, rd, dtype, gen):
    return tuple((torch.randint(-8, 9, (rows, rd // 2), generator=gen).float() / 8).to(dtype) for _ in range(2))


class Step:
    """One step: ragged q (lens_q), a cache of capacity `cap` filled to `fills`, ragged new keys / values (lens_new).
    layout: contig | batch_idx | leftpad | page<N>."""

    def __init__(self, lens_q, fills, lens_new=None, cap=768, h=4, hk=2, d=128, dv=None, layout="contig", dtype=torch.bfloat16,
                 qv=False, rotary=None, rot_seqlens=None, seed=0):
        g = torch.Generator().manual_seed(seed)
        rnd = lambda *s: torch.randn(*s, generator=g).to(dtype)  # noqa: E731
        self.b, self.cap, self.h, self.hk, self.d, self.dv, self.layout, self.dtype = len(lens_q), cap, h, hk, d, dv or d, layout, dtype
        b, dv = self.b, self.dv
        self.lens_q, self.fills = list(lens_q), torch.tensor(fills, dtype=I32)
        self.lens_new = list(lens_new) if lens_new is not None else None
        self.cu_q = _cu(lens_q)
        self.q = rnd(sum(lens_q), h, d)
        self.qv = rnd(sum(lens_q), h, dv) if qv else None
        bc = b + 2 if layout == "batch_idx" else b
        self.kc, self.vc = rnd(bc, cap, hk, d), rnd(bc, cap, hk, dv)
        self.idx = torch.randperm(bc, generator=g)[:b].to(I32) if layout == "batch_idx" else torch.arange(b, dtype=I32)
        self.leftpad = torch.tensor([min((3 + 5 * i) % 20, fills[i]) for i in range(b)], dtype=I32) if layout == "leftpad" else None
        self.page = int(layout[4:]) if layout.startswith("page") else 0
        if self.page:
            nblk = cap // self.page
            self.table = torch.randperm(b * nblk, generator=g).to(I32).view(b, nblk)
        if self.lens_new is not None:
            self.cu_new = _cu(self.lens_new)
            self.k_new, self.v_new = rnd(sum(self.lens_new), hk, d), rnd(sum(self.lens_new), hk, dv)
        self.rotary = rotary  # (rotary_dim, interleaved)
        if rotary:
            self.cos, self.sin = _tables(cap + 512, rotary[0], dtype, g)
        self.rot = torch.tensor(rot_seqlens, dtype=I32) if rot_seqlens is not None else None

    # ---- the expected cache and the oracle ------------------------------------------------------------------------------
    def expected_cache(self):
        """(k, v) per sequence (b, cap, hk, .) after the append: a Python scatter of the (rotated) new rows; rows past the
        capacity are dropped.  Also the fill levels afterwards."""
        k_ref, v_ref = self.kc[self.idx.long()].clone(), self.vc[self.idx.long()].clone()
        total = self.fills.clone()
        if self.lens_new is not None:
            for s in range(self.b):
                lo, n, fill = int(self.cu_new[s]), self.lens_new[s], int(self.fills[s])
                rows_k, rows_v = self.k_new[lo:lo + n], self.v_new[lo:lo + n]
                if self.rotary and n:
                    pos = self.rot[s:s + 1] if self.rot is not None else self.fills[s:s + 1]
                    rows_k = oracle.apply_rotary_emb_ref(rows_k[None], self.cos, self.sin, pos, interleaved=self.rotary[1])[0]
                fit = max(0, min(n, self.cap - fill))
                k_ref[s, fill:fill + fit], v_ref[s, fill:fill + fit] = rows_k[:fit], rows_v[:fit]
                total[s] = min(fill + n, self.cap)
        return k_ref, v_ref, total

    def padded(self, x):
        out = torch.zeros(self.b, max(self.lens_q), *x.shape[1:], dtype=x.dtype)
        for s in range(self.b):
            out[s, :self.lens_q[s]] = x[int(self.cu_q[s]):int(self.cu_q[s + 1])]
        return out

    def reference(self, causal=False, window=(-1, -1), softcap=0.0, seqused_q=None):
        k_ref, v_ref, total = self.expected_cache()
        j = torch.arange(self.cap).view(1, -1)
        kmask = j < total.view(-1, 1)
        if self.leftpad is not None:
            kmask &= j >= self.leftpad.view(-1, 1)
        used_q = torch.tensor(self.lens_q if seqused_q is None else seqused_q)
        qmask = torch.arange(max(self.lens_q)).view(1, -1) < used_q.view(-1, 1)
        qp = self.padded(self.q)
        if self.rotary:  # the dense route's rule per sequence: causal / local -> row i at the old fill level (or seqlens_rotary) + i
            per_row = causal or window[0] >= 0 or window[1] >= 0
            qp = oracle.apply_rotary_emb_ref(qp, self.cos, self.sin, self.rot if self.rot is not None else self.fills,
                                             interleaved=self.rotary[1], per_row_positions=per_row)
        kw = dict(causal=causal, window_size=window, softcap=softcap, key_leftpad=self.leftpad,
                  qv=self.padded(self.qv) if self.qv is not None else None)
        ref, _, lse = oracle.attention_ref(qp, k_ref, v_ref, qmask, kmask, return_lse=True, **kw)
        pt, _ = oracle.attention_ref(qp, k_ref, v_ref, qmask, kmask, upcast=False, reorder_ops=True, **kw)
        return ref, pt, lse, qmask

    # ---- the call ---------------------------------------------------------------------------------------------------------
    def device_cache(self):
        kc, vc = self.kc.to(DEV), self.vc.to(DEV)
        if not self.page:
            return kc, vc
        flat = self.table.flatten().long().to(DEV)
        kp = torch.empty(flat.numel(), self.page, self.hk, self.d, dtype=self.dtype, device=DEV)
        vp = torch.empty(flat.numel(), self.page, self.hk, self.dv, dtype=self.dtype, device=DEV)
        kp[flat] = kc.reshape(-1, self.page, self.hk, self.d)
        vp[flat] = vc.reshape(-1, self.page, self.hk, self.dv)
        return kp, vp

    def cache_per_sequence(self, kd, vd):
        """The device cache back in (b, cap, hk, .) order of the sequences, on the host."""
        if self.page:
            flat = self.table.flatten().long().to(DEV)
            return kd[flat].reshape(self.b, self.cap, self.hk, self.d).cpu(), vd[flat].reshape(self.b, self.cap, self.hk, self.dv).cpu()
        return kd[self.idx.long().to(DEV)].cpu(), vd[self.idx.long().to(DEV)].cpu()

    def kwargs(self, causal=False, window=(-1, -1), softcap=0.0, num_splits=1, seqused_q=None):
        dev = lambda t: None if t is None else t.to(DEV)  # noqa: E731
        kw = dict(cache_seqlens=dev(self.fills), cu_seqlens_q=dev(self.cu_q), max_seqlen_q=max(self.lens_q), causal=causal,
                  window_size=window, softcap=softcap, num_splits=num_splits, return_softmax_lse=True, qv=dev(self.qv))
        if self.lens_new is not None:
            kw.update(k=dev(self.k_new), v=dev(self.v_new), cu_seqlens_k_new=dev(self.cu_new))
        if self.layout == "batch_idx":
            kw["cache_batch_idx"] = dev(self.idx)
        if self.leftpad is not None:
            kw["cache_leftpad"] = dev(self.leftpad)
        if self.page:
            kw["page_table"] = dev(self.table)
        if self.rotary:
            kw.update(rotary_cos=dev(self.cos), rotary_sin=dev(self.sin), rotary_interleaved=self.rotary[1], rotary_seqlens=dev(self.rot))
        return kw

    def call(self, kd, vd, **kw):
        args = self.kwargs(**kw)
        if "seqused_q" in kw and kw["seqused_q"] is not None:  # (not an argument of flash_attn_with_kvcache: the op itself)
            a = dict(args)
            out, lse, *_ = torch.ops.flash_attn_3.fwd(
                self.q.to(DEV), kd, vd, a.get("k"), a.get("v"), a["qv"], None, a["cu_seqlens_q"], None, a.get("cu_seqlens_k_new"),
                torch.tensor(kw["seqused_q"], dtype=I32, device=DEV), a["cache_seqlens"], a["max_seqlen_q"], None, a.get("page_table"),
                a.get("cache_batch_idx"), a.get("cache_leftpad"), a.get("rotary_cos"), a.get("rotary_sin"), a.get("rotary_seqlens"),
                None, None, None, None, a["causal"], a["window_size"][0], a["window_size"][1], 0, a["softcap"],
                a.get("rotary_interleaved", True), None, a["num_splits"], None, 0)
            return out, lse
        out, lse, *_ = _fa3().flash_attn_with_kvcache(self.q.to(DEV), kd, vd, **args)
        return out, lse


def _check(step, out, lse, ref, pt, lse_ref, qmask, what):
    total_q = int(qmask.sum())
    assert tuple(out.shape) == (sum(step.lens_q), step.h, step.dv) and tuple(lse.shape) == (step.h, sum(step.lens_q))
    rows = torch.cat([torch.arange(step.lens_q[s])[qmask[s, :step.lens_q[s]]] + int(step.cu_q[s]) for s in range(step.b)])
    assert rows.numel() == total_q
    o, r, p = out.float().cpu()[rows], ref[qmask].float(), pt[qmask].float()
    err, bound = (o - r).abs().max().item(), 3 * (p - r).abs().max().item() + 1e-5
    print(f"{what}: max err {err:.3e} bound {bound:.3e}")
    assert err == err and err <= bound, f"{what}: max err {err:.3e} > bound {bound:.3e}"
    l, lr = lse.float().cpu().t()[rows], lse_ref.permute(0, 2, 1)[qmask]  # (rows, h)
    fin = torch.isfinite(lr)
    assert torch.equal(torch.isfinite(l), fin), f"{what}: lse inf pattern"
    if fin.any():
        lerr = (l[fin] - lr[fin]).abs().max().item()
        print(f"{what}: lse err {lerr:.3e}")
        assert lerr <= 2e-3, f"{what}: lse err {lerr:.3e}"


def _check_cache(step, kd, vd):
    k_ref, v_ref, _ = step.expected_cache()
    k_got, v_got = step.cache_per_sequence(kd, vd)
    assert torch.equal(k_got, k_ref) and torch.equal(v_got, v_ref)


LENS_Q = [0, 1, 37, 300, 1, 130]          # empty, single-token decodes, prefill chunks; max_seqlen_q 300
FILLS = [100, 517, 64, 300, 0, 411]       # (a sequence that starts on an empty cache: fill 0)
LENS_NEW = [3, 1, 37, 300, 1, 0]          # new rows per sequence (one without any); fill + new <= 768

W64_128 = "fwd_kernel_w64 D=128 DEFF=128 waves=4 block_m=256 splits=1"
W64_64 = "fwd_kernel_w64 D=64 DEFF=64 waves=4 block_m=256 splits=1"
CASES = [  # (id, d, h, hk, mask, softcap, layout, append, plan)
    ("d128_gqa_causal_contig", 128, 4, 2, "causal", 0.0, "contig", True, W64_128),
    ("d128_gqa_causal_contig_noappend", 128, 4, 2, "causal", 0.0, "contig", False, W64_128),
    ("d128_mha_full_batch_idx", 128, 2, 2, "full", 0.0, "batch_idx", True, W64_128),
    ("d128_mqa_window_batch_idx_noappend", 128, 4, 1, "window", 0.0, "batch_idx", False, W64_128),
    ("d128_gqa_causal_leftpad", 128, 4, 2, "causal", 0.0, "leftpad", True, W64_128),
    ("d64_mha_window_leftpad_noappend", 64, 2, 2, "window", 0.0, "leftpad", False, W64_64),
    ("d128_gqa_softcap_contig", 128, 4, 2, "causal", 5.0, "contig", True, "fwd_kernel_d256 W=128 waves=4 SOFTCAP block_m=128 splits=1"),
    ("d64_mqa_causal_contig", 64, 4, 1, "causal", 0.0, "contig", True, "fwd_kernel D=64 waves=4 block_m=128 splits=1"),
    ("d64_gqa_full_contig_noappend", 64, 4, 2, "full", 0.0, "contig", False, W64_64),
    ("d256_gqa_causal_contig", 256, 4, 2, "causal", 0.0, "contig", True, "fwd_kernel_d256 W=256 waves=4 block_m=128 splits=1"),
    ("d256_mha_window_softcap_noappend", 256, 2, 2, "window", 5.0, "contig", False, "fwd_kernel_d256 W=256 waves=4 SOFTCAP block_m=128 splits=1"),
    ("d128_gqa_causal_page1", 128, 4, 2, "causal", 0.0, "page1", True, "fwd_kernel D=128 waves=8 block_m=256 splits=1"),
    ("d64_mqa_full_page1_noappend", 64, 4, 1, "full", 0.0, "page1", False, "fwd_kernel D=64 waves=8 block_m=256 splits=1"),
    ("d128_mha_window_page16", 128, 2, 2, "window", 0.0, "page16", True, "fwd_kernel D=128 waves=8 block_m=256 splits=1"),
    ("d256_gqa_causal_page16_noappend", 256, 4, 2, "causal", 0.0, "page16", False, "fwd_kernel D=256 waves=4 block_m=128 splits=1"),
    ("d128_gqa_causal_page64", 128, 4, 2, "causal", 0.0, "page64", True, "fwd_kernel D=128 waves=8 block_m=256 splits=1"),
    ("d128_mqa_softcap_page64_noappend", 128, 4, 1, "causal", 5.0, "page64", False, "fwd_kernel D=128 waves=8 SOFTCAP block_m=256 splits=1"),
    ("d64_gqa_causal_page256", 64, 4, 2, "causal", 0.0, "page256", True, "fwd_kernel D=64 waves=8 block_m=256 splits=1"),
    ("d128_gqa_full_page256_noappend", 128, 4, 2, "full", 0.0, "page256", False, "fwd_kernel D=128 waves=8 block_m=256 splits=1"),
]
MASKS = {"causal": (True, (-1, -1)), "full": (False, (-1, -1)), "window": (False, (120, 30))}


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_ragged_kvcache_against_oracle(case):
    name, d, h, hk, mask, softcap, layout, append, plan = case
    causal, window = MASKS[mask]
    dtype = torch.float16 if "mha" in name else torch.bfloat16
    step = Step(LENS_Q, FILLS, LENS_NEW if append else None, h=h, hk=hk, d=d, layout=layout, dtype=dtype, seed=len(name))
    kd, vd = step.device_cache()
    out, lse = step.call(kd, vd, causal=causal, window=window, softcap=softcap)
    assert last_plan() == plan
    _check(step, out, lse, *step.reference(causal, window, softcap), name)
    _check_cache(step, kd, vd)


@pytest.mark.parametrize("append", [False, True])
@pytest.mark.parametrize("mask,softcap", [("causal", 0.0), ("window", 5.0)])
def test_ragged_kvcache_qv_paged(mask, softcap, append):
    """MLA shape: d 64 beside d_v 512 with qv, pages of 64 rows, 16 query heads on one kv head."""
    causal, window = MASKS[mask]
    step = Step(LENS_Q, FILLS, LENS_NEW if append else None, h=16, hk=1, d=64, dv=512, layout="page64", qv=True, seed=5)
    kd, vd = step.device_cache()
    out, lse = step.call(kd, vd, causal=causal, window=window, softcap=softcap)
    assert last_plan() == f"fwd_kernel_qv DVT=512 waves=4{' SOFTCAP' if softcap else ''} block_m=128 splits=1"
    _check(step, out, lse, *step.reference(causal, window, softcap), f"qv {mask} append={append}")
    _check_cache(step, kd, vd)


def test_ragged_kvcache_seqused_q():
    """seqused_q: only the first rows of every sequence are queries; the rest of the ragged tensor is left alone."""
    used = [0, 1, 20, 257, 0, 130]
    step = Step(LENS_Q, FILLS, LENS_NEW, seed=9)
    kd, vd = step.device_cache()
    out, lse = step.call(kd, vd, causal=True, seqused_q=used)
    assert last_plan() == W64_128
    _check(step, out, lse, *step.reference(True, seqused_q=used), "seqused_q")


# ---- the append ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", ["contig", "batch_idx", "page16"])
@pytest.mark.parametrize("interleaved", [False, True])
@pytest.mark.parametrize("rot_seqlens", [None, [5, 700, 0, 33, 400, 1]])
def test_ragged_append_rotary_bits_and_oracle(layout, interleaved, rot_seqlens):
    """The cache after the call equals a Python scatter of the rotated rows, bit for bit (both interleave forms, seqlens_rotary),
    and the attention over it follows the oracle with q rotated by the dense route's rule."""
    step = Step(LENS_Q, FILLS, LENS_NEW, d=128, layout=layout, rotary=(64, interleaved), rot_seqlens=rot_seqlens, seed=3)
    for causal in (True, False):
        kd, vd = step.device_cache()
        out, lse = step.call(kd, vd, causal=causal)
        _check_cache(step, kd, vd)
        _check(step, out, lse, *step.reference(causal), f"rotary causal={causal}")


@pytest.mark.parametrize("lens_new", [LENS_NEW, [0] * 6], ids=["append", "empty_append"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_ragged_append_rotary_both_types(dtype, lens_new):
    """kvcache_append_varlen_kernel and rotary_varlen_kernel in both element types (the tests above rotate bf16 only) against
    plain torch: the cache equals a Python scatter of the rows rotated by oracle.apply_rotary_emb_ref, bit for bit, and the
    attention over it follows the oracle with q rotated the same way.  342 new rows and 469 query rows in 6 sequences, two
    of them without rows: no multiple of the 16 rows of a workgroup, sequences cut inside a wave's 4 rows.  `empty_append`:
    the empty input -- k_new / v_new of no rows at all: every byte of the cache stays what it was, q is still rotated, and
    the result has its shape, no non-finite element, and follows the oracle over the old fill levels."""
    step = Step(LENS_Q, FILLS, lens_new, d=128, dtype=dtype, rotary=(64, False), seed=43)
    assert (sum(LENS_Q) % 16, sum(LENS_NEW) % 16) == (5, 6)
    kd, vd = step.device_cache()
    out, lse = step.call(kd, vd, causal=True)
    assert last_plan() == W64_128
    _check_cache(step, kd, vd)
    if not sum(lens_new):
        assert step.k_new.shape[0] == 0 and torch.equal(kd.cpu(), step.kc) and torch.equal(vd.cpu(), step.vc)
        assert out.dtype == dtype and torch.isfinite(out).all()
    _check(step, out, lse, *step.reference(True), f"rotary {dtype} new rows {sum(lens_new)}")


@pytest.mark.parametrize("layout", ["contig", "page64"])
def test_ragged_append_drops_rows_past_capacity(layout):
    """Sequences whose new rows do not fit: the rows past the capacity are dropped, nothing else is touched, and the attention
    launch sees the capacity as the fill level."""
    fills = [760, 768, 64, 500, 0, 700]  # the first two overflow (8 of 20 rows fit; none of 5), the fourth ends exactly at 768
    new = [20, 5, 37, 268, 1, 0]
    step = Step(LENS_Q, fills, new, layout=layout, rotary=(32, False), seed=11)
    kd, vd = step.device_cache()
    guard_k, guard_v = kd.clone(), vd.clone()
    out, lse = step.call(kd, vd, causal=False)
    _check_cache(step, kd, vd)
    assert not torch.equal(kd, guard_k) and not torch.equal(vd, guard_v)
    _check(step, out, lse, *step.reference(False), "overflow")


@pytest.mark.parametrize("layout", ["contig", "page16"])
def test_ragged_append_equal_lengths_matches_dense_call(layout):
    """With equal lengths the ragged call leaves the same cache bits as the dense (b, s_new, h_k, d) call."""
    b, n = 4, 9
    fills = [10, 200, 0, 511]
    step = Step([n] * b, fills, [n] * b, layout=layout, rotary=(64, True), seed=13)
    kd, vd = step.device_cache()
    step.call(kd, vd, causal=True)
    kd2, vd2 = step.device_cache()
    kw = step.kwargs(causal=True)
    for key in ("cu_seqlens_q", "cu_seqlens_k_new", "max_seqlen_q"):
        kw.pop(key)
    kw.update(k=kw["k"].view(b, n, step.hk, step.d), v=kw["v"].view(b, n, step.hk, step.dv))
    _fa3().flash_attn_with_kvcache(step.q.to(DEV).view(b, n, step.h, step.d), kd2, vd2, **kw)
    assert torch.equal(kd, kd2) and torch.equal(vd, vd2)
    _check_cache(step, kd, vd)


# ---- split-KV --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout,d,dv,plan", [
    ("contig", 128, None, "fwd_kernel_w64 D=128 DEFF=128 waves=4 block_m=256 splits={}"),
    ("page64", 128, None, "fwd_kernel D=128 waves=8 block_m=256 splits={}"),
    ("page64", 64, 512, "fwd_kernel_qv DVT=512 waves=4 block_m=128 splits={}"),
])
def test_ragged_splits(layout, d, dv, plan):
    """num_splits 2 and 5 follow the oracle like num_splits 1, repeated runs are bit-identical, and sequences shorter than one
    split (fills of 0 + 1 and 3 + 3 keys: most of five splits are empty) are correct."""
    fills = [100, 517, 64, 300, 0, 3]
    new = [3, 1, 37, 300, 1, 3]
    lens_q = [0, 1, 37, 300, 1, 3]
    qv = dv is not None
    step = Step(lens_q, fills, new, h=16 if qv else 4, hk=1 if qv else 2, d=d, dv=dv, layout=layout, qv=qv, seed=21)
    ref = step.reference(True)
    for splits in (1, 2, 5):
        kd, vd = step.device_cache()
        out, lse = step.call(kd, vd, causal=True, num_splits=splits)
        assert last_plan() == plan.format(splits)
        _check(step, out, lse, *ref, f"splits={splits}")
        for _ in range(2):
            kd2, vd2 = step.device_cache()
            out2, lse2 = step.call(kd2, vd2, causal=True, num_splits=splits)
            assert torch.equal(out2, out) and torch.equal(lse2, lse)


def test_ragged_split_heuristic_runs():
    """num_splits = 0 on a decode-heavy mixed step: the heuristic splits (few row blocks) and the result follows the oracle."""
    step = Step([1, 2, 1, 3], [700, 650, 500, 767], [1, 2, 1, 1], cap=768, seed=23)
    kd, vd = step.device_cache()
    out, lse = step.call(kd, vd, causal=True, num_splits=0)
    assert int(last_plan().rsplit("splits=", 1)[1]) > 1
    _check(step, out, lse, *step.reference(True), "heuristic")


# ---- single-token route ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", ["contig", "batch_idx", "page16"])
@pytest.mark.parametrize("new_kv", ["none", "dense", "ragged"])
def test_single_token_step_is_the_dense_decode_call(layout, new_kv):
    """max_seqlen_q = 1 with total_q = batch: bit-equal to the dense flash_attn_with_kvcache call in out, LSE and cache, on the
    dense call's plan (its GQA swap and split heuristic)."""
    b, h, hk, d = 5, 8, 2, 128
    fills = [100, 517, 64, 700, 1]
    step = Step([1] * b, fills, None if new_kv == "none" else [1] * b, h=h, hk=hk, d=d, layout=layout,
                rotary=None if new_kv == "none" else (64, False), seed=31)
    dense_kw = step.kwargs(causal=True, num_splits=0)
    for key in ("cu_seqlens_q", "cu_seqlens_k_new", "max_seqlen_q"):
        dense_kw.pop(key, None)
    if new_kv != "none":
        dense_kw.update(k=dense_kw["k"].view(b, 1, hk, d), v=dense_kw["v"].view(b, 1, hk, d))
    kd_d, vd_d = step.device_cache()
    out_d, lse_d, *_ = _fa3().flash_attn_with_kvcache(step.q.to(DEV).view(b, 1, h, d), kd_d, vd_d, **dense_kw)
    plan_d = last_plan()
    ragged_kw = step.kwargs(causal=True, num_splits=0)
    if new_kv == "dense":  # new rows as (b, 1, h_k, d) beside ragged queries
        ragged_kw.pop("cu_seqlens_k_new")
        ragged_kw.update(k=dense_kw["k"], v=dense_kw["v"])
    kd, vd = step.device_cache()
    out, lse, *_ = _fa3().flash_attn_with_kvcache(step.q.to(DEV), kd, vd, **ragged_kw)
    assert last_plan() == plan_d
    assert tuple(out.shape) == (b, h, d) and tuple(lse.shape) == (h, b)
    assert torch.equal(out, out_d.view(b, h, d)) and torch.equal(lse, lse_d.view(b, h).t())
    assert torch.equal(kd, kd_d) and torch.equal(vd, vd_d)
    _check_cache(step, kd, vd)


# ---- graph capture -----------------------------------------------------------------------------------------------------------

def test_ragged_step_graph_capture():
    """One ragged append-and-attend step (rotary, paged, split) is captured and replays to the same bits: nothing on the way
    reads device data on the host."""
    step = Step(LENS_Q, FILLS, LENS_NEW, layout="page64", rotary=(64, False), seed=41)
    kd0, vd0 = step.device_cache()
    kd, vd = kd0.clone(), vd0.clone()
    kw = step.kwargs(causal=True, num_splits=2)
    q = step.q.to(DEV)
    run = lambda k, v: _fa3().flash_attn_with_kvcache(q, k, v, **kw)[:2]  # noqa: E731
    want_out, want_lse = run(kd, vd)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(kd0.clone(), vd0.clone())
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    kg, vg = kd0.clone(), vd0.clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got_out, got_lse = run(kg, vg)
    for _ in range(2):  # (the second replay appends the same rows again)
        got_out.zero_(); got_lse.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(got_out, want_out) and torch.equal(got_lse, want_lse)
        assert torch.equal(kg, kd) and torch.equal(vg, vd)


# ---- rejections ------------------------------------------------------------------------------------------------------------

def test_ragged_kvcache_rejections():
    fa3 = _fa3()
    bf = torch.bfloat16
    q = torch.randn(6, 4, 64, dtype=bf, device=DEV)
    kc = torch.randn(2, 256, 4, 64, dtype=bf, device=DEV)
    cu = torch.tensor([0, 2, 6], dtype=I32, device=DEV)
    lens = torch.tensor([5, 9], dtype=I32, device=DEV)
    f8 = torch.float8_e4m3fn
    with pytest.raises(RuntimeError, match="does not support KV-cache arguments with fp8 inputs"):
        fa3.flash_attn_with_kvcache(q.to(f8), kc.to(f8), kc.to(f8), cache_seqlens=lens, cu_seqlens_q=cu, max_seqlen_q=4)
    with pytest.raises(RuntimeError, match="does not support attention_chunk or a V headdim of its own with KV-cache"):
        fa3.flash_attn_with_kvcache(q, kc, kc, cache_seqlens=lens, cu_seqlens_q=cu, max_seqlen_q=4, attention_chunk=64)
    with pytest.raises(RuntimeError, match="does not support attention_chunk or a V headdim of its own with KV-cache"):
        fa3.flash_attn_with_kvcache(q, kc, torch.randn(2, 256, 4, 128, dtype=bf, device=DEV), cache_seqlens=lens, cu_seqlens_q=cu,
                                    max_seqlen_q=4)
    table = torch.arange(8, dtype=I32, device=DEV).view(2, 4)
    with pytest.raises(RuntimeError, match="does not support KV-cache arguments together with cu_seqlens_k"):
        torch.ops.flash_attn_3.fwd(q, kc.view(8, 64, 4, 64), kc.view(8, 64, 4, 64), cu_seqlens_q=cu, cu_seqlens_k=cu, seqused_k=lens,
                                   max_seqlen_q=4, max_seqlen_k=256, page_table=table)
    kn = torch.randn(2, 1, 4, 64, dtype=bf, device=DEV)
    with pytest.raises(RuntimeError, match="does not support cu_seqlens_k_new without cu_seqlens_q"):
        fa3.flash_attn_with_kvcache(q[:2].view(2, 1, 4, 64), kc, kc, k=kn, v=kn, cache_seqlens=lens, cu_seqlens_k_new=cu)
    with pytest.raises(RuntimeError, match="max_seqlen_q must be provided if cu_seqlens_q is provided"):
        fa3.flash_attn_with_kvcache(q, kc, kc, cache_seqlens=lens, cu_seqlens_q=cu)
    with pytest.raises(RuntimeError, match="cu_seqlens_k_new must have dtype torch.int32"):
        fa3.flash_attn_with_kvcache(q, kc, kc, k=q, v=q, cache_seqlens=lens, cu_seqlens_q=cu, cu_seqlens_k_new=cu.long(), max_seqlen_q=4)


def test_dense_query_cu_seqlens_k_new_calls_still_raise():
    """The two dense-query calls the older suites pin (tests/test_fa3_kvcache_gpu.py, tests/test_qv_gpu.py) keep their text."""
    fa3 = _fa3()
    q = torch.randn(2, 1, 4, 64, dtype=torch.bfloat16, device=DEV)
    kc = torch.randn(2, 256, 4, 64, dtype=torch.bfloat16, device=DEV)
    lens = torch.tensor([5, 9], dtype=I32, device=DEV)
    with pytest.raises(RuntimeError, match="does not support cu_seqlens_k_new"):
        fa3.flash_attn_with_kvcache(q, kc, kc, cache_seqlens=lens, cu_seqlens_k_new=lens)
    q = torch.randn(1, 8, 4, 64, dtype=torch.bfloat16, device=DEV)
    k = torch.randn(1, 8, 1, 64, dtype=torch.bfloat16, device=DEV)
    v = torch.randn(1, 8, 1, 512, dtype=torch.bfloat16, device=DEV)
    qv = torch.randn(1, 8, 4, 512, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(RuntimeError, match="does not support cu_seqlens_k_new"):
        fa3.flash_attn_with_kvcache(q, k, v, k=k, v=v, qv=qv, cache_seqlens=0,
                                    cu_seqlens_k_new=torch.zeros(2, dtype=I32, device=DEV))
