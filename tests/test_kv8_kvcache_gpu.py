"""GPU tests of 16-bit queries over an fp8 (e4m3) KV cache: torch.ops.flash_attn_3.fwd / hopper_interface.flash_attn_with_kvcache
with a Float8_e4m3fn k / v and k_descale / v_descale, i.e. fa_fwd_kv8 and kv8_fwd_kernel (csrc/fa_fwd_kernel_kv8.h).

Reference: the unchanged oracle, fed the cache dequantised on the CPU -- the e4m3 values taken exactly to fp32, times the descale
of their (batch, kv head).  Bound: the rule of tests/test_fa3_kvcache_gpu.py, |out - ref| <= 3 |pt - ref| + 1e-5, with the
low-precision leg `pt` computed in q's dtype.  The kernel sees exactly the values the oracle sees (the conversion is exact and
the descales are powers of two), so there is no margin for quantisation.  The LSE is fp32 arithmetic over at most 128 exact
products per score and scores of a few tens: 1e-3 absolute covers its rounding with room (fp32 eps x 128 x 50 ~ 4e-4).

Every case also runs the existing 16-bit route on the same values -- the cache expanded to q's dtype with the descales
multiplied in (exact) -- and prints both errors against the oracle, and asserts the plan fa_fwd_last_plan_name() names:
kv8_fwd_kernel, its D, SOFTCAP and the epilogue (splits=1: the kernel's own store; splits=N: N parts + the merge)."""
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
    """(rows, d) uint8: every row a permutation of the 254 non-NaN e4m3 patterns (subnormals, +-0, +-448), cut or repeated to d."""
    g = torch.Generator().manual_seed(seed)
    pats = torch.tensor([x for x in range(256) if x not in (0x7F, 0xFF)], dtype=torch.uint8)
    out = torch.empty(rows, d, dtype=torch.uint8)
    for r in range(rows):
        perm = pats[torch.randperm(254, generator=g)]
        out[r] = perm.repeat((d + 253) // 254)[:d] if d > 254 else torch.roll(perm, r)[:d]
    return out


class Case:
    """One problem: the logical cache entries (bc, cap, hk, d) as e4m3, laid out physically (dense / strided view / pages), the
    oracle's two legs, and the two GPU routes."""

    def __init__(self, dtype=torch.bfloat16, b=2, sq=1, h=8, hk=2, d=128, cap=320, lens=(1, 257), page=None, batch_idx=None,
                 leftpad=None, strided=False, causal=False, window=(-1, -1), softcap=0.0, kdesc=None, vdesc=None,
                 cu_q=None, seqused_q=None, all_bytes=False, seed=0):
        torch.manual_seed(seed)
        self.dtype, self.b, self.sq, self.h, self.hk, self.d, self.cap = dtype, b, sq, h, hk, d, cap
        self.causal, self.window, self.softcap, self.page = causal, window, softcap, page
        self.lens = torch.tensor(lens, dtype=torch.int32)
        self.batch_idx = None if batch_idx is None else torch.tensor(batch_idx, dtype=torch.int32)
        self.leftpad = None if leftpad is None else torch.tensor(leftpad, dtype=torch.int32)
        self.cu_q = None if cu_q is None else torch.tensor(cu_q, dtype=torch.int32)
        self.seqused_q = None if seqused_q is None else torch.tensor(seqused_q, dtype=torch.int32)
        bc = b if batch_idx is None else max(batch_idx) + 2
        if all_bytes:
            self.k8 = _all_bytes(bc * cap * hk, d, seed).view(bc, cap, hk, d).view(F8)
            self.v8 = _all_bytes(bc * cap * hk, d, seed + 1).view(bc, cap, hk, d).view(F8)
        else:
            self.k8 = torch.randn(bc, cap, hk, d).to(F8)
            self.v8 = torch.randn(bc, cap, hk, d).to(F8)
        as_desc = lambda x, shift: (_descales(b, hk, shift) if x is None else
                                    x.float().contiguous() if torch.is_tensor(x) else torch.full((b, hk), float(x)))
        self.kdesc, self.vdesc = as_desc(kdesc, 0), as_desc(vdesc, 3)
        if self.cu_q is None:
            self.q = torch.randn(b, sq, h, d).to(dtype)
        else:
            self.q = torch.randn(int(self.cu_q[-1]), h, d).to(dtype)
        self.strided = strided
        if page is not None:
            assert cap % page == 0 and batch_idx is None and leftpad is None
            nblk = cap // page
            total = b * nblk + 3  # more pages allocated than used
            self.table = torch.randperm(total)[: b * nblk].to(torch.int32).view(b, nblk)

    # ---- what the oracle sees: per batch row its keys from position 0, dequantised, times the descale ----------------------
    def _logical(self, x8, desc):
        b, cap = self.b, self.cap
        x = x8.float()
        out = torch.zeros(b, cap, self.hk, self.d)
        for i in range(b):
            e = i if self.batch_idx is None else int(self.batch_idx[i])
            lp = 0 if self.leftpad is None else int(self.leftpad[i])
            out[i, : cap - lp] = x[e, lp:]
        return out * desc[:, None, :, None]

    def valid(self):
        lp = torch.zeros_like(self.lens) if self.leftpad is None else self.leftpad
        return (self.lens - lp).clamp(min=0)

    def reference(self):
        """(ref out, ref lse, pt out) as lists of per-row tensors selected to the used query rows: (rows, h, d) / (h, rows)."""
        kl, vl = self._logical(self.k8, self.kdesc), self._logical(self.v8, self.vdesc)
        kmask = torch.arange(self.cap).view(1, -1) < self.valid().view(-1, 1)
        if self.cu_q is None:
            qd, qmask = self.q, None
        else:
            n = (self.cu_q[1:] - self.cu_q[:-1]) if self.seqused_q is None else self.seqused_q
            qd = torch.zeros(self.b, self.sq, self.h, self.d, dtype=self.dtype)
            qmask = torch.arange(self.sq).view(1, -1) < n.view(-1, 1)
            for i in range(self.b):
                qd[i, : int(n[i])] = self.q[int(self.cu_q[i]): int(self.cu_q[i]) + int(n[i])]
        kw = dict(causal=self.causal, window_size=self.window, softcap=self.softcap)
        ref, _, lse = oracle.attention_ref(qd, kl, vl, qmask, kmask, return_lse=True, **kw)
        if qmask is not None:  # rows past a sequence's used queries do not exist
            lse = lse.masked_fill(~qmask.view(self.b, 1, self.sq), float("inf"))
        pt = oracle.attention_ref(qd, kl.to(self.dtype), vl.to(self.dtype), qmask, kmask, upcast=False, reorder_ops=True, **kw)[0]
        return ref, lse, pt

    def select(self, out, lse):
        """GPU results -> the oracle's padded (b, sq, h, d) / (b, h, sq) layout (ragged queries only; unused rows zero / inf)."""
        if self.cu_q is None:
            return out, lse
        n = (self.cu_q[1:] - self.cu_q[:-1]) if self.seqused_q is None else self.seqused_q
        o = torch.zeros(self.b, self.sq, self.h, self.d, dtype=out.dtype)
        l = torch.full((self.b, self.h, self.sq), float("inf"))
        for i in range(self.b):
            s, c = int(self.cu_q[i]), int(n[i])
            o[i, :c] = out[s: s + c]
            l[i, :, :c] = lse[:, s: s + c]
        return o, l

    # ---- physical layouts --------------------------------------------------------------------------------------------------
    def _phys(self, x):
        """x: the logical entries (bc, cap, hk, d) of any dtype -> the tensor handed to the call, on the device."""
        if x.dtype == F8:  # (indexing and strided copies as bytes)
            return self._phys(x.view(torch.uint8)).view(F8)
        x = x.to(DEV)
        if self.page is not None:
            nblk = self.cap // self.page
            pool = torch.zeros(self.b * nblk + 3, self.page, self.hk, self.d, dtype=x.dtype, device=DEV)
            pool[self.table.flatten().long().to(DEV)] = x[: self.b].reshape(self.b * nblk, self.page, self.hk, self.d)
            return pool
        if self.strided:  # head stride != d, row stride != hk * d; 16-byte aligned rows for both element sizes
            big = torch.zeros(x.shape[0], self.cap, self.hk + 1, self.d + 16, dtype=x.dtype, device=DEV)
            view = big[:, :, : self.hk, : self.d]
            view.copy_(x)
            return view
        return x.contiguous()

    def kwargs(self, lens=None):
        dev = lambda t: None if t is None else t.to(DEV)
        kw = dict(seqused_k=dev(self.lens if lens is None else lens), kv_batch_idx=dev(self.batch_idx), leftpad_k=dev(self.leftpad),
                  is_causal=self.causal, window_size_left=self.window[0], window_size_right=self.window[1], softcap=self.softcap)
        if self.page is not None:
            kw["page_table"] = self.table.to(DEV)
        if self.cu_q is not None:
            kw.update(cu_seqlens_q=dev(self.cu_q), seqused_q=dev(self.seqused_q), max_seqlen_q=self.sq)
        return kw

    def run_kv8(self, num_splits=1, **over):
        import flash_attention_annotated_amd.flash_attn_3_ops  # noqa: F401  (registers torch.ops.flash_attn_3)
        kw = self.kwargs()
        kw.update(over)
        out, lse, *_ = torch.ops.flash_attn_3.fwd(self.q.to(DEV), self._phys(self.k8), self._phys(self.v8),
                                                  k_descale=self.kdesc.to(DEV), v_descale=self.vdesc.to(DEV),
                                                  num_splits=num_splits, **kw)
        plan = _last_plan()
        return out.cpu(), lse.cpu(), plan

    def run_16bit(self, num_splits=1):
        import flash_attention_annotated_amd.flash_attn_3_ops  # noqa: F401
        def expand(x8, desc):  # entry e holds batch row i's descale where the row reads it (exact: powers of two)
            x = x8.float()
            for i in range(self.b):
                e = i if self.batch_idx is None else int(self.batch_idx[i])
                x[e] = x8[e].float() * desc[i][None, :, None]
            return x.to(self.dtype)
        out, lse, *_ = torch.ops.flash_attn_3.fwd(self.q.to(DEV), self._phys(expand(self.k8, self.kdesc)),
                                                  self._phys(expand(self.v8, self.vdesc)), num_splits=num_splits, **self.kwargs())
        return out.cpu(), lse.cpu()

    def check(self, plan_d, num_splits=1, epilogue_splits=1, name=""):
        """Run both routes, print both errors, assert the plan and the oracle bound for the kv8 route.  Returns (out, lse)."""
        ref, ref_lse, pt = self.reference()
        out, lse, plan = self.run_kv8(num_splits)
        want = f"kv8_fwd_kernel D={plan_d} waves=4{' SOFTCAP' if self.softcap > 0 else ''} block_m=128 splits={epilogue_splits}"
        assert plan == want, (plan, want)
        o16, _ = self.run_16bit(1)
        o, l = self.select(out, lse)
        o16s, _ = self.select(o16, torch.zeros_like(lse))
        err8 = (o.float() - ref.float()).abs().max().item()
        err16 = (o16s.float() - ref.float()).abs().max().item()
        bound = 3 * (pt.float() - ref.float()).abs().max().item() + 1e-5
        print(f"kv8 {name}: |kv8 - ref| = {err8:.3e}  |16-bit route - ref| = {err16:.3e}  bound = {bound:.3e}  plan = {plan}")
        assert err8 <= bound
        finite = torch.isfinite(ref_lse)
        assert torch.equal(torch.isfinite(l), finite)
        assert torch.allclose(l[finite], ref_lse[finite], atol=1e-3, rtol=0)
        return out, lse


# ---- decode, seqlen_q = 1 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_kv8_decode(dtype):
    """b2 hq8 / hkv2 d128, capacity 320, fill levels [1, 257]: one key in one entry, four full tiles plus a one-key tail in the
    other; distinct descales per (batch, kv head), another permutation for V."""
    Case(dtype=dtype).check(128, name=f"decode {dtype}")


def test_kv8_with_kvcache_entry_point():
    """hopper_interface.flash_attn_with_kvcache reaches the same route (pack_gqa is accepted and ignored)."""
    c = Case()
    ref, _, pt = c.reference()
    out, lse, *_ = _fa3().flash_attn_with_kvcache(c.q.to(DEV), c._phys(c.k8), c._phys(c.v8), cache_seqlens=c.lens.to(DEV),
                                             k_descale=c.kdesc.to(DEV), v_descale=c.vdesc.to(DEV), num_splits=1, pack_gqa=True,
                                             return_softmax_lse=True)
    assert _last_plan() == "kv8_fwd_kernel D=128 waves=4 block_m=128 splits=1"
    assert out.dtype == c.dtype and tuple(lse.shape) == (c.b, c.h, 1)
    assert (out.float().cpu() - ref.float()).abs().max().item() <= 3 * (pt.float() - ref.float()).abs().max().item() + 1e-5


@pytest.mark.parametrize("d,tile", [(64, 64), (96, 128), (80, 128), (16, 64)])
def test_kv8_head_dims(d, tile):
    """d64; d96 and d80: a D = 128 tile partly used; d16: one 16-byte chunk of a D = 64 tile."""
    Case(d=d, seed=d).check(tile, name=f"d{d}")


@pytest.mark.parametrize("h,hk", [(4, 4), (16, 1)], ids=["mha", "mqa"])
def test_kv8_head_layouts(h, hk):
    Case(h=h, hk=hk, seed=h).check(128, name=f"h{h}/hk{hk}")


def test_kv8_exact_conversion_of_every_byte_pattern():
    """K and V hold all 254 non-NaN byte patterns (subnormals, +-0, +-448), permuted per row; d128, 256 keys.  A conversion
    that flushed subnormals, lost -0's sign or saturated would leave the oracle bound by orders of magnitude (448^2 products)."""
    Case(b=1, cap=256, lens=(256,), all_bytes=True, kdesc=2.0 ** -9, vdesc=1.0, seed=5).check(128, name="all bytes")


# ---- paged caches ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("page", [64, 128, 16, 1])
def test_kv8_paged(page):
    """A shuffled page_table over more pages than are used; fill levels that end inside a page (257; 1) and on a page
    boundary (256).  Multiples of 64 resolve one page per tile, 16 and 1 one page per staged row."""
    Case(b=3, cap=384, lens=(257, 256, 1), page=page, seed=page).check(128, name=f"page {page}")


# ---- cache selection and layout ------------------------------------------------------------------------------------------------
def test_kv8_cache_batch_idx_permutes_and_repeats():
    """Rows 0 and 2 read the same cache entry, so they share its descales (the 16-bit route expands an entry once)."""
    kd = torch.tensor([[0.5, 2.0], [1.0, 4.0], [0.5, 2.0]])
    vd = torch.tensor([[4.0, 1.0], [2.0, 0.5], [4.0, 1.0]])
    Case(b=3, batch_idx=(2, 0, 2), lens=(257, 70, 130), kdesc=kd, vdesc=vd, seed=11).check(128, name="cache_batch_idx")


def test_kv8_cache_leftpad():
    Case(b=2, leftpad=(3, 70), lens=(40, 300), seed=12).check(128, name="cache_leftpad")


def test_kv8_strided_cache_view():
    """head stride != d and row stride != h_k d (a view into a wider allocation)."""
    c = Case(d=64, strided=True, seed=13)
    k = c._phys(c.k8)
    assert k.stride(2) != c.d and k.stride(1) != c.hk * c.d and not k.is_contiguous()
    c.check(64, name="strided view")


# ---- split-KV ------------------------------------------------------------------------------------------------------------------
def test_kv8_split_with_an_empty_part():
    """num_splits = 3 over capacity 320 (5 key blocks: parts of 2 blocks): fill level 70 leaves the third part -- and at 257
    none -- without keys.  Compared with num_splits = 1 under the oracle bound."""
    c = Case(lens=(70, 257), seed=21)
    o3, l3 = c.check(128, num_splits=3, epilogue_splits=3, name="splits=3")
    o1, l1 = c.check(128, num_splits=1, epilogue_splits=1, name="splits=1")
    ref, _, pt = c.reference()
    assert (o3.float() - o1.float()).abs().max().item() <= 3 * (pt.float() - ref.float()).abs().max().item() + 1e-5
    assert torch.allclose(l3, l1, atol=1e-3, rtol=0)


def test_kv8_split_heuristic():
    """num_splits = 0 at b1, capacity 2048: one (batch, kv head) group per kv head leaves the chip idle, the heuristic splits."""
    c = Case(b=1, cap=2048, lens=(2000,), seed=22)
    ref, _, pt = c.reference()
    out, lse, plan = c.run_kv8(num_splits=0)
    m = re.fullmatch(r"kv8_fwd_kernel D=128 waves=4 block_m=128 splits=(\d+)", plan)
    assert m and int(m.group(1)) > 1, plan
    o1, _, _ = c.run_kv8(num_splits=1)
    bound = 3 * (pt.float() - ref.float()).abs().max().item() + 1e-5
    print(f"kv8 heuristic: plan = {plan}  |split - ref| = {(out.float() - ref.float()).abs().max().item():.3e}  bound = {bound:.3e}")
    assert (out.float() - ref.float()).abs().max().item() <= bound
    assert (out.float() - o1.float()).abs().max().item() <= bound


# ---- ragged queries over the cache ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("page", [None, 16], ids=["dense", "page16"])
def test_kv8_ragged_queries(page):
    """cu_seqlens_q = [0, 1, 5, 6] with seqused_q (the middle sequence uses 3 of its 4 rows), causal, left window 17."""
    c = Case(b=3, sq=4, cap=320, lens=(257, 70, 16), page=page, cu_q=(0, 1, 5, 6), seqused_q=(1, 3, 1), causal=True,
             window=(17, 0), seed=31)
    c.check(128, name=f"ragged page={page}")


def test_kv8_softcap_descale_acts_before_tanh():
    """softcap 30 with k_descale = 4: tanh(4 s / 30) 30 is far from 4 tanh(s / 30) 30 for scores of a few units."""
    Case(softcap=30.0, kdesc=4.0, vdesc=1.0, seed=41).check(128, name="softcap")


def test_kv8_empty_cache_entry_equals_16bit_route():
    c = Case(lens=(0, 257), seed=42)
    out, lse, plan = c.run_kv8()
    assert plan == "kv8_fwd_kernel D=128 waves=4 block_m=128 splits=1"
    o16, l16 = c.run_16bit()
    assert torch.equal(out[0], o16[0]) and torch.equal(lse[0], l16[0])
    assert torch.all(out[0] == 0) and torch.all(torch.isinf(lse[0]) & (lse[0] > 0))
    c.check(128, name="cache_seqlens = 0")


def test_kv8_prefill_chunk():
    """seqlen_q = 130 over 300 cached keys, causal, MHA: two row blocks per kv head, the second partial."""
    Case(b=1, sq=130, h=2, hk=2, cap=320, lens=(300,), causal=True, seed=43).check(128, name="prefill chunk")


def test_kv8_prefill_chunk_gqa_d64():
    """130 rows x 4 heads of a group = 520 packed rows: five row blocks, rows of one query row in different waves."""
    Case(b=1, sq=130, h=8, hk=2, d=64, cap=320, lens=(300,), causal=True, seed=44).check(64, name="prefill chunk gqa")


def test_kv8_hip_graph_follows_cache_seqlens():
    """One capture of a paged decode step on a single stream, three replays: the fill levels are device data the kernel reads,
    so overwriting the captured tensor in place changes what the replays compute."""
    c = Case(b=2, cap=256, lens=(5, 9), page=64, seed=51)
    import flash_attention_annotated_amd.flash_attn_3_ops  # noqa: F401
    q, k, v = c.q.to(DEV), c._phys(c.k8), c._phys(c.v8)
    kd, vd, table, lens = c.kdesc.to(DEV), c.vdesc.to(DEV), c.table.to(DEV), c.lens.to(DEV)
    call = lambda: torch.ops.flash_attn_3.fwd(q, k, v, seqused_k=lens, page_table=table, k_descale=kd, v_descale=vd, num_splits=1)
    call()  # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, lse, *_ = call()
    lens.copy_(torch.tensor([40, 200], dtype=torch.int32))
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    got, got_lse = out.cpu(), lse.cpu()
    want, want_lse, *_ = call()
    assert _last_plan() == "kv8_fwd_kernel D=128 waves=4 block_m=128 splits=1"
    assert torch.equal(got, want.cpu()) and torch.equal(got_lse, want_lse.cpu())
    c.lens = torch.tensor([40, 200], dtype=torch.int32)
    ref, _, pt = c.reference()
    assert (got.float() - ref.float()).abs().max().item() <= 3 * (pt.float() - ref.float()).abs().max().item() + 1e-5


def test_kv8_rejections():
    fa3 = _fa3()
    q = torch.randn(2, 1, 4, 64, dtype=torch.bfloat16, device=DEV)
    kc = torch.randn(2, 256, 2, 64, device=DEV).to(F8)
    lens = torch.tensor([5, 9], dtype=torch.int32, device=DEV)
    new = torch.randn(2, 1, 2, 64, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(RuntimeError, match="does not support k_new / v_new with an fp8 KV cache"):
        fa3.flash_attn_with_kvcache(q, kc, kc, k=new, v=new, cache_seqlens=lens)
    ang = torch.rand(256, 16, device=DEV)
    with pytest.raises(RuntimeError, match="does not support rotary_cos / rotary_sin with an fp8 KV cache"):
        fa3.flash_attn_with_kvcache(q, kc, kc, rotary_cos=torch.cos(ang).bfloat16(), rotary_sin=torch.sin(ang).bfloat16(),
                                    cache_seqlens=lens)
    with pytest.raises(RuntimeError, match="does not support qv with an fp8 KV cache"):
        fa3.flash_attn_with_kvcache(q, kc, kc, qv=q, cache_seqlens=lens)
    for d in (192, 72):
        qd = torch.randn(2, 1, 4, d, dtype=torch.bfloat16, device=DEV)
        kd = torch.randn(2, 256, 2, d, device=DEV).to(F8)
        with pytest.raises(RuntimeError, match=f"head_size <= 128 that is a multiple of 16, got {d}"):
            fa3.flash_attn_with_kvcache(qd, kd, kd, cache_seqlens=lens)
    vc = torch.randn(2, 256, 2, 128, device=DEV).to(F8)
    with pytest.raises(RuntimeError, match="does not support a V headdim of its own with an fp8 KV cache"):
        fa3.flash_attn_with_kvcache(q, kc, vc, cache_seqlens=lens)
    with pytest.raises(RuntimeError, match="does not support attention_chunk with an fp8 KV cache"):
        fa3.flash_attn_with_kvcache(q, kc, kc, cache_seqlens=lens, attention_chunk=64)
    # every other mixed pair keeps today's message: fp8 q beside a 16-bit cache, an fp8 K beside a 16-bit V
    k16 = torch.randn(2, 256, 2, 64, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(RuntimeError, match="query and key must have the same dtype"):
        fa3.flash_attn_with_kvcache(q.to(F8), k16, k16, cache_seqlens=lens)
    with pytest.raises(RuntimeError, match="query and key must have the same dtype"):
        fa3.flash_attn_with_kvcache(q, kc, k16, cache_seqlens=lens)


def test_kv8_fake_impl_traces_the_mixed_call():
    """The meta implementation of flash_attn_3::fwd gives out q's dtype for 16-bit q over an fp8 cache (torch.compile traces it)."""
    import flash_attention_annotated_amd.flash_attn_3_ops  # noqa: F401
    q = torch.empty(2, 1, 8, 128, dtype=torch.float16, device="meta")
    kc = torch.empty(2, 320, 2, 128, dtype=F8, device="meta")
    out, lse, *_ = torch.ops.flash_attn_3.fwd(q, kc, kc, seqused_k=torch.empty(2, dtype=torch.int32, device="meta"))
    assert out.dtype == torch.float16 and tuple(out.shape) == (2, 1, 8, 128) and tuple(lse.shape) == (2, 8, 1)
