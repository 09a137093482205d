"""GPU tests of the MLA decode shape over an fp8 (e4m3) KV cache: torch.ops.flash_attn_3.fwd / flash_attn_with_kvcache with a
Float8_e4m3fn k (.., h_k, d <= 64) and v (.., h_k, d_v in [256, 512]), 16-bit q and optional qv, k_descale / v_descale --
fa_fwd_qv8 and qv8_fwd_kernel (csrc/fa_fwd_kernel_qv8.h).  The method is tests/test_kv8_kvcache_gpu.py's.

Reference: the unchanged oracle, attention_ref(..., qv=), fed the cache dequantised on the CPU -- the e4m3 values taken exactly
to fp32, times the descale of their (batch, kv head).  Bound: |out - ref| <= 3 |pt - ref| + 1e-5 with the low-precision leg
`pt` computed in q's dtype; there is no margin for quantisation.  The LSE goes under the bound tests/test_qv_gpu.py applies to
the 16-bit qv route: the same entries finite, and those within 2e-3.

Every case also runs the 16-bit qv route on the same values -- the cache expanded to q's dtype with the descales multiplied
in -- and prints both errors against the oracle (no bit equality: the summation order differs), and asserts the plan
fa_fwd_last_plan_name() names: qv8_fwd_kernel, its DVT, SOFTCAP and the epilogue.  The oracle's legs of a problem are computed
once per Case."""
import re

import pytest
import torch

from oracle import attention_ref as oracle

pytestmark = pytest.mark.gpu
DEV = "cuda"
F8 = torch.float8_e4m3fn


def _fa3():
    from flash_attention_annotated_amd import hopper_interface
    return hopper_interface


def _last_plan():
    from flash_attention_annotated_amd import _lib
    name = _lib.load().fa_fwd_last_plan_name()
    return name.decode() if name else None


def _descales(b, hk, shift):
    """Distinct powers of two per (batch, kv head): a swapped index or a K / V mix-up shows."""
    vals = torch.tensor([0.5, 1.0, 2.0, 4.0, 0.25, 8.0, 0.125, 16.0])
    idx = (torch.arange(b * hk) + shift) % len(vals)
    return vals[idx].view(b, hk).contiguous()


def _all_bytes(rows, d, seed):
    """(rows, d) uint8: every row holds the 254 non-NaN e4m3 patterns (subnormals, +-0, +-448), permuted; cut (d < 254, rotated
    per row so that every pattern occurs) or repeated to d."""
    g = torch.Generator().manual_seed(seed)
    pats = torch.tensor([x for x in range(256) if x not in (0x7F, 0xFF)], dtype=torch.uint8)
    out = torch.empty(rows, d, dtype=torch.uint8)
    for r in range(rows):
        perm = pats[torch.randperm(254, generator=g)]
        out[r] = perm.repeat((d + 253) // 254)[:d] if d > 254 else torch.roll(pats, 61 * r)[:d]
    return out


def _plan(dvt, splits=1, softcap=False):
    return f"qv8_fwd_kernel DVT={dvt} waves=4{' SOFTCAP' if softcap else ''} block_m=32 splits={splits}"


class Case:
    """One problem: the logical cache entries K (bc, cap, hk, d), V (bc, cap, hk, dv) as e4m3, laid out physically (dense /
    strided view / pages), the oracle's two legs, and the two GPU routes."""

    def __init__(self, dtype=torch.bfloat16, b=2, sq=1, h=8, hk=1, d=64, dv=512, cap=320, lens=(1, 257), page=None, batch_idx=None,
                 leftpad=None, strided=False, causal=False, window=(-1, -1), softcap=0.0, kdesc=None, vdesc=None,
                 cu_q=None, seqused_q=None, all_bytes=False, with_qv=True, seed=0):
        torch.manual_seed(seed)
        self.dtype, self.b, self.sq, self.h, self.hk, self.d, self.dv, self.cap = dtype, b, sq, h, hk, d, dv, cap
        self.causal, self.window, self.softcap, self.page = causal, window, softcap, page
        self.dvt = 256 if dv <= 256 else 512
        self.lens = torch.tensor(lens, dtype=torch.int32)
        self.batch_idx = None if batch_idx is None else torch.tensor(batch_idx, dtype=torch.int32)
        self.leftpad = None if leftpad is None else torch.tensor(leftpad, dtype=torch.int32)
        self.cu_q = None if cu_q is None else torch.tensor(cu_q, dtype=torch.int32)
        self.seqused_q = None if seqused_q is None else torch.tensor(seqused_q, dtype=torch.int32)
        bc = b if batch_idx is None else max(batch_idx) + 2
        if all_bytes:
            self.k8 = _all_bytes(bc * cap * hk, d, seed).view(bc, cap, hk, d).view(F8)
            self.v8 = _all_bytes(bc * cap * hk, dv, seed + 1).view(bc, cap, hk, dv).view(F8)
        else:
            self.k8 = torch.randn(bc, cap, hk, d).to(F8)
            self.v8 = torch.randn(bc, cap, hk, dv).to(F8)
        as_desc = lambda x, shift: (_descales(b, hk, shift) if x is None else
                                    x.float().contiguous() if torch.is_tensor(x) else torch.full((b, hk), float(x)))
        self.kdesc, self.vdesc = as_desc(kdesc, 0), as_desc(vdesc, 3)
        lead = (b, sq) if self.cu_q is None else (int(self.cu_q[-1]),)
        self.q = torch.randn(*lead, h, d).to(dtype)
        self.qv = torch.randn(*lead, h, dv).to(dtype) if with_qv else None
        self.strided = strided
        if page is not None:
            assert cap % page == 0 and batch_idx is None and leftpad is None
            nblk = cap // page
            self.table = torch.randperm(b * nblk + 3)[: b * nblk].to(torch.int32).view(b, nblk)  # more pages allocated than used
        self._ref = None

    # ---- what the oracle sees: per batch row its keys from position 0, dequantised, times the descale ----------------------
    def _logical(self, x8, desc):
        x = x8.float()
        out = torch.zeros(self.b, self.cap, self.hk, x.shape[-1])
        for i in range(self.b):
            e = i if self.batch_idx is None else int(self.batch_idx[i])
            lp = 0 if self.leftpad is None else int(self.leftpad[i])
            out[i, : self.cap - lp] = x[e, lp:]
        return out * desc[:, None, :, None]

    def valid(self):
        lp = torch.zeros_like(self.lens) if self.leftpad is None else self.leftpad
        return (self.lens - lp).clamp(min=0)

    def _used_q(self):
        return (self.cu_q[1:] - self.cu_q[:-1]) if self.seqused_q is None else self.seqused_q

    def _padded(self, x):
        """ragged rows (total_q, h, w) -> (b, sq, h, w), zero past a sequence's used rows"""
        n = self._used_q()
        out = torch.zeros(self.b, self.sq, self.h, x.shape[-1], dtype=x.dtype)
        for i in range(self.b):
            out[i, : int(n[i])] = x[int(self.cu_q[i]): int(self.cu_q[i]) + int(n[i])]
        return out

    def reference(self):
        """(ref out, ref lse, pt out) in the oracle's padded layout (b, sq, h, dv) / (b, h, sq); computed once."""
        if self._ref is not None:
            return self._ref
        kl, vl = self._logical(self.k8, self.kdesc), self._logical(self.v8, self.vdesc)
        kmask = torch.arange(self.cap).view(1, -1) < self.valid().view(-1, 1)
        if self.cu_q is None:
            qd, qvd, qmask = self.q, self.qv, None
        else:
            qd, qvd = self._padded(self.q), None if self.qv is None else self._padded(self.qv)
            qmask = torch.arange(self.sq).view(1, -1) < self._used_q().view(-1, 1)
        kw = dict(causal=self.causal, window_size=self.window, softcap=self.softcap, qv=qvd)
        ref, _, lse = oracle.attention_ref(qd, kl, vl, qmask, kmask, return_lse=True, **kw)
        if qmask is not None:  # rows past a sequence's used queries do not exist
            lse = lse.masked_fill(~qmask.view(self.b, 1, self.sq), float("inf"))
        pt = oracle.attention_ref(qd, kl.to(self.dtype), vl.to(self.dtype), qmask, kmask, upcast=False, reorder_ops=True, **kw)[0]
        self._ref = (ref, lse, pt)
        return self._ref

    def select(self, out, lse):
        """GPU results -> the oracle's padded layout (ragged queries only; unused rows zero / inf)."""
        if self.cu_q is None:
            return out, lse
        n = self._used_q()
        o = torch.zeros(self.b, self.sq, self.h, self.dv, dtype=out.dtype)
        l = torch.full((self.b, self.h, self.sq), float("inf"))
        for i in range(self.b):
            s, c = int(self.cu_q[i]), int(n[i])
            o[i, :c] = out[s: s + c]
            l[i, :, :c] = lse[:, s: s + c]
        return o, l

    # ---- physical layouts --------------------------------------------------------------------------------------------------
    def _phys(self, x):
        """x: the logical entries (bc, cap, hk, w) of any dtype -> the tensor handed to the call, on the device."""
        if x.dtype == F8:  # (indexing and strided copies as bytes)
            return self._phys(x.view(torch.uint8)).view(F8)
        x = x.to(DEV)
        w = x.shape[-1]
        if self.page is not None:
            nblk = self.cap // self.page
            pool = torch.zeros(self.b * nblk + 3, self.page, self.hk, w, dtype=x.dtype, device=DEV)
            pool[self.table.flatten().long().to(DEV)] = x[: self.b].reshape(self.b * nblk, self.page, self.hk, w)
            return pool
        if self.strided:  # head stride != w, row stride != hk * w; 16-byte aligned rows for both element sizes
            big = torch.zeros(x.shape[0], self.cap, self.hk + 1, w + 16, dtype=x.dtype, device=DEV)
            view = big[:, :, : self.hk, : w]
            view.copy_(x)
            return view
        return x.contiguous()

    def kwargs(self):
        dev = lambda t: None if t is None else t.to(DEV)
        kw = dict(seqused_k=dev(self.lens), kv_batch_idx=dev(self.batch_idx), leftpad_k=dev(self.leftpad), q_v=dev(self.qv),
                  is_causal=self.causal, window_size_left=self.window[0], window_size_right=self.window[1], softcap=self.softcap)
        if self.page is not None:
            kw["page_table"] = self.table.to(DEV)
        if self.cu_q is not None:
            kw.update(cu_seqlens_q=dev(self.cu_q), seqused_q=dev(self.seqused_q), max_seqlen_q=self.sq)
        return kw

    def run_qv8(self, num_splits=1):
        import flash_attention_annotated_amd.flash_attn_3_ops  # noqa: F401  (registers torch.ops.flash_attn_3)
        out, lse, *_ = torch.ops.flash_attn_3.fwd(self.q.to(DEV), self._phys(self.k8), self._phys(self.v8),
                                                  k_descale=self.kdesc.to(DEV), v_descale=self.vdesc.to(DEV),
                                                  num_splits=num_splits, **self.kwargs())
        plan = _last_plan()
        return out.cpu(), lse.cpu(), plan

    def run_16bit(self, num_splits=1):
        import flash_attention_annotated_amd.flash_attn_3_ops  # noqa: F401
        def expand(x8, desc):  # entry e holds batch row i's descale where the row reads it
            x = x8.float()
            for i in range(self.b):
                e = i if self.batch_idx is None else int(self.batch_idx[i])
                x[e] = x8[e].float() * desc[i][None, :, None]
            return x.to(self.dtype)
        out, lse, *_ = torch.ops.flash_attn_3.fwd(self.q.to(DEV), self._phys(expand(self.k8, self.kdesc)),
                                                  self._phys(expand(self.v8, self.vdesc)), num_splits=num_splits, **self.kwargs())
        return out.cpu(), lse.cpu()

    def check(self, num_splits=1, epilogue_splits=1, name=""):
        """Run both routes, print both errors, assert the plan and the oracle bounds for the qv8 route.  Returns (out, lse)."""
        ref, ref_lse, pt = self.reference()
        out, lse, plan = self.run_qv8(num_splits)
        want = _plan(self.dvt, epilogue_splits, self.softcap > 0)
        assert plan == want, (plan, want)
        assert out.dtype == self.dtype and tuple(out.shape) == (*self.q.shape[:-1], self.dv)
        o16, _ = self.run_16bit(1)
        o, l = self.select(out, lse)
        o16s, _ = self.select(o16, torch.zeros_like(lse))
        err8 = (o.float() - ref.float()).abs().max().item()
        err16 = (o16s.float() - ref.float()).abs().max().item()
        bound = 3 * (pt.float() - ref.float()).abs().max().item() + 1e-5
        fin = torch.isfinite(ref_lse)
        lse_err = (l[fin] - ref_lse[fin]).abs().max().item() if fin.any() else 0.0
        print(f"qv8 {name}: |qv8 - ref| = {err8:.3e}  |16-bit qv route - ref| = {err16:.3e}  bound = {bound:.3e}  "
              f"|lse - ref| = {lse_err:.3e}  plan = {plan}")
        assert err8 <= bound
        assert torch.equal(fin, torch.isfinite(l))
        assert lse_err < 2e-3
        return out, lse


# ---- decode at the base shape: b2, capacity 320 (5 tiles), fill levels [1, 257], h_k 1 ---------------------------------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_qv8_decode(dtype):
    """d 64 / d_v 512, h 16: one key in one entry, four full tiles plus a one-key tail in the other."""
    Case(dtype=dtype, h=16).check(name=f"decode {dtype}")


def test_qv8_with_kvcache_entry_point():
    """hopper_interface.flash_attn_with_kvcache reaches the same route."""
    c = Case(seed=1)
    ref, _, pt = c.reference()
    out, lse, *_ = _fa3().flash_attn_with_kvcache(c.q.to(DEV), c._phys(c.k8), c._phys(c.v8), qv=c.qv.to(DEV),
                                                  cache_seqlens=c.lens.to(DEV), k_descale=c.kdesc.to(DEV), v_descale=c.vdesc.to(DEV),
                                                  num_splits=1, return_softmax_lse=True)
    assert _last_plan() == _plan(512)
    assert out.dtype == c.dtype and tuple(out.shape) == (c.b, 1, c.h, c.dv) and tuple(lse.shape) == (c.b, c.h, 1)
    assert (out.float().cpu() - ref.float()).abs().max().item() <= 3 * (pt.float() - ref.float()).abs().max().item() + 1e-5


@pytest.mark.parametrize("d,dv", [(32, 256), (48, 320)])
def test_qv8_head_dims(d, dv):
    """d 32 / d_v 256: the DVT = 256 tile and half a K row; d 48 / d_v 320: clamped K and V columns meet zero Q / Qv columns, O
    columns past d_v are not stored."""
    Case(d=d, dv=dv, h=4, seed=d).check(name=f"d{d}/dv{dv}")


def test_qv8_without_qv():
    """qv = None at d 64 / d_v 256: the score is the K product alone."""
    Case(dv=256, with_qv=False, seed=3).check(name="no qv")


def test_qv8_two_kv_heads_distinct_descales():
    """h_k 2: four distinct (batch, kv head) descales for K, another four for V."""
    c = Case(h=8, hk=2, seed=4)
    assert len(set(c.kdesc.flatten().tolist())) == 4 and not torch.equal(c.kdesc, c.vdesc)
    c.check(name="h_k 2")


def test_qv8_two_query_rows_causal():
    """sq 2 under a causal mask; the entry with one key leaves its first query row without a visible key."""
    Case(sq=2, causal=True, seed=5).check(name="sq 2 causal")


def test_qv8_several_row_blocks():
    """sq 40 with g = 4: 160 packed rows, five 32-row blocks; the causal mask goes by query row, not packed row."""
    Case(sq=40, h=4, lens=(40, 257), causal=True, seed=6).check(name="sq 40 g 4")


def test_qv8_window():
    Case(sq=2, window=(25, 6), lens=(30, 257), seed=7).check(name="window (25, 6)")


def test_qv8_softcap():
    """softcap 20 with k_descale 4 and v_descale 2: both factors act in front of the tanh."""
    Case(softcap=20.0, kdesc=4.0, vdesc=2.0, seed=8).check(name="softcap")


def test_qv8_descales_act_in_fp32():
    """Descales that are no powers of two: folded into a 16-bit operand they would round it."""
    Case(kdesc=0.3, vdesc=1.7, seed=9).check(name="descales 0.3 / 1.7")


def test_qv8_exact_conversion_of_every_byte_pattern():
    """K and V hold all 254 non-NaN byte patterns; descales 2^-6 keep the scores in the tens."""
    Case(b=1, cap=256, lens=(256,), all_bytes=True, kdesc=2.0 ** -6, vdesc=2.0 ** -6, seed=10).check(name="all bytes")


@pytest.mark.parametrize("page", [64, 16])
def test_qv8_paged(page):
    """A shuffled page_table over more pages than are used; fill levels that end inside a page and on a page boundary."""
    Case(b=3, cap=384, lens=(257, 256, 1), page=page, seed=page).check(name=f"page {page}")


def test_qv8_cache_batch_idx():
    kd = torch.tensor([[0.5], [1.0], [0.5]])
    vd = torch.tensor([[4.0], [2.0], [4.0]])
    Case(b=3, batch_idx=(2, 0, 2), lens=(257, 70, 130), kdesc=kd, vdesc=vd, seed=11).check(name="cache_batch_idx")


def test_qv8_cache_leftpad():
    Case(leftpad=(3, 70), lens=(40, 300), seed=12).check(name="cache_leftpad")


def test_qv8_strided_cache_view():
    c = Case(strided=True, seed=13)
    v = c._phys(c.v8)
    assert v.stride(2) != c.dv and v.stride(1) != c.hk * c.dv and not v.is_contiguous()
    c.check(name="strided view")


@pytest.mark.parametrize("page", [None, 16], ids=["dense", "page16"])
def test_qv8_ragged_queries(page):
    """cu_seqlens_q = [0, 1, 1, 5, 6]: a sequence without queries; seqused_q uses 3 of the third one's 4 rows; causal."""
    Case(b=4, sq=4, lens=(257, 100, 70, 16), page=page, cu_q=(0, 1, 1, 5, 6), seqused_q=(1, 0, 3, 1), causal=True,
         seed=14).check(name=f"ragged page={page}")


def test_qv8_split_with_an_empty_part():
    """num_splits = 3 over capacity 320 (5 key blocks: parts of 2 blocks): fill level 70 leaves the third part without keys."""
    c = Case(lens=(70, 257), seed=21)
    o3, l3 = c.check(num_splits=3, epilogue_splits=3, name="splits=3")
    o1, l1 = c.check(num_splits=1, epilogue_splits=1, name="splits=1")
    ref, _, pt = c.reference()
    assert (o3.float() - o1.float()).abs().max().item() <= 3 * (pt.float() - ref.float()).abs().max().item() + 1e-5
    assert (l3 - l1).abs().max().item() < 2e-3


def test_qv8_split_heuristic():
    """num_splits = 0 at b1, capacity 1024: one group leaves the chip idle, the heuristic splits."""
    c = Case(b=1, cap=1024, lens=(1000,), seed=22)
    _, _, plan = c.run_qv8(num_splits=0)
    m = re.fullmatch(r"qv8_fwd_kernel DVT=512 waves=4 block_m=32 splits=(\d+)", plan)
    assert m and int(m.group(1)) > 1, plan
    c.check(num_splits=0, epilogue_splits=int(m.group(1)), name="heuristic")


@pytest.mark.parametrize("splits", [1, 3])
def test_qv8_row_without_a_visible_key(splits):
    """An empty cache entry: O = 0 and LSE = +inf, unsplit and through the merge."""
    c = Case(lens=(0, 257), seed=23)
    out, lse = c.check(num_splits=splits, epilogue_splits=splits, name=f"empty entry splits={splits}")
    assert torch.all(out[0] == 0) and torch.all(torch.isinf(lse[0]) & (lse[0] > 0))


# ---- stand-alone -----------------------------------------------------------------------------------------------------------------
def test_qv8_hip_graph_follows_cache_seqlens():
    """One capture of a paged decode step on a single stream, replayed after the fill levels change: equal bit for bit to the
    eager call on the new levels."""
    c = Case(cap=256, lens=(5, 9), page=64, seed=51)
    import flash_attention_annotated_amd.flash_attn_3_ops  # noqa: F401
    q, qv, k, v = c.q.to(DEV), c.qv.to(DEV), c._phys(c.k8), c._phys(c.v8)
    kd, vd, table, lens = c.kdesc.to(DEV), c.vdesc.to(DEV), c.table.to(DEV), c.lens.to(DEV)
    call = lambda: torch.ops.flash_attn_3.fwd(q, k, v, q_v=qv, seqused_k=lens, page_table=table, k_descale=kd, v_descale=vd,
                                              num_splits=1)
    call()  # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, lse, *_ = call()
    lens.copy_(torch.tensor([40, 200], dtype=torch.int32))
    graph.replay()
    torch.cuda.synchronize()
    got, got_lse = out.cpu(), lse.cpu()
    want, want_lse, *_ = call()
    assert _last_plan() == _plan(512)
    assert torch.equal(got, want.cpu()) and torch.equal(got_lse, want_lse.cpu())
    c.lens = torch.tensor([40, 200], dtype=torch.int32)
    ref, _, pt = c.reference()
    assert (got.float() - ref.float()).abs().max().item() <= 3 * (pt.float() - ref.float()).abs().max().item() + 1e-5


def test_qv8_is_deterministic():
    c = Case(sq=2, causal=True, seed=52)
    a, la, _ = c.run_qv8(num_splits=3)
    b, lb, _ = c.run_qv8(num_splits=3)
    assert torch.equal(a, b) and torch.equal(la, lb)
    a, la, _ = c.run_qv8(num_splits=1)
    b, lb, _ = c.run_qv8(num_splits=1)
    assert torch.equal(a, b) and torch.equal(la, lb)


def test_qv8_rejections():
    fa3 = _fa3()
    q = torch.randn(2, 1, 4, 64, dtype=torch.bfloat16, device=DEV)
    qv = torch.randn(2, 1, 4, 512, dtype=torch.bfloat16, device=DEV)
    kc = torch.randn(2, 256, 1, 64, device=DEV).to(F8)
    vc = torch.randn(2, 256, 1, 512, device=DEV).to(F8)
    lens = torch.tensor([5, 9], dtype=torch.int32, device=DEV)
    desc = torch.ones(2, 1, device=DEV)
    k_new = torch.randn(2, 1, 1, 64, dtype=torch.bfloat16, device=DEV)
    v_new = torch.randn(2, 1, 1, 512, dtype=torch.bfloat16, device=DEV)
    # the MLA shape is read only: new rows and rotary answer with a message of their own, with or without descales
    for kw in (dict(), dict(k_descale=desc, v_descale=desc)):
        with pytest.raises(RuntimeError, match="does not support k_new / v_new with an fp8 KV cache of the MLA shape"):
            fa3.flash_attn_with_kvcache(q, kc, vc, k=k_new, v=v_new, qv=qv, cache_seqlens=lens, **kw)
        ang = torch.rand(256, 16, device=DEV)
        with pytest.raises(RuntimeError, match="does not support rotary_cos / rotary_sin with an fp8 KV cache of the MLA shape"):
            fa3.flash_attn_with_kvcache(q, kc, vc, qv=qv, rotary_cos=torch.cos(ang).bfloat16(), rotary_sin=torch.sin(ang).bfloat16(),
                                        cache_seqlens=lens, **kw)
    with pytest.raises(RuntimeError, match="q_v must have shape"):
        fa3.flash_attn_with_kvcache(q, kc, vc, qv=qv[..., :256], cache_seqlens=lens)
    with pytest.raises(RuntimeError, match="does not support attention_chunk with an fp8 KV cache"):
        fa3.flash_attn_with_kvcache(q, kc, vc, qv=qv, cache_seqlens=lens, attention_chunk=64)
    # every pinned refusal still fires for its old call
    with pytest.raises(RuntimeError, match="does not support qv with an fp8 KV cache"):
        fa3.flash_attn_with_kvcache(q, kc, kc, qv=q, cache_seqlens=lens)
    v128 = torch.randn(2, 256, 1, 128, device=DEV).to(F8)
    with pytest.raises(RuntimeError, match="does not support a V headdim of its own with an fp8 KV cache"):
        fa3.flash_attn_with_kvcache(q, kc, v128, cache_seqlens=lens)
    with pytest.raises(RuntimeError, match="does not support qv with an fp8 KV cache"):
        fa3.flash_attn_with_kvcache(q, kc, v128, qv=qv[..., :128].contiguous(), cache_seqlens=lens)
    with pytest.raises(RuntimeError, match="does not support k_new / v_new with an fp8 KV cache: appending"):
        fa3.flash_attn_with_kvcache(q, kc, kc, k=k_new, v=k_new, cache_seqlens=lens)


def test_qv8_fake_impl_traces_the_call():
    """The meta implementation of flash_attn_3::fwd gives q's dtype and the (..., d_v) shape for this call."""
    import flash_attention_annotated_amd.flash_attn_3_ops  # noqa: F401
    q = torch.empty(2, 1, 16, 64, dtype=torch.float16, device="meta")
    qv = torch.empty(2, 1, 16, 512, dtype=torch.float16, device="meta")
    kc = torch.empty(2, 320, 1, 64, dtype=F8, device="meta")
    vc = torch.empty(2, 320, 1, 512, dtype=F8, device="meta")
    out, lse, *_ = torch.ops.flash_attn_3.fwd(q, kc, vc, q_v=qv, seqused_k=torch.empty(2, dtype=torch.int32, device="meta"))
    assert out.dtype == torch.float16 and tuple(out.shape) == (2, 1, 16, 512) and tuple(lse.shape) == (2, 16, 1)
