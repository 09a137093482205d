"""GPU tests of the write half of the fp8 (e4m3) KV cache of the MLA shape: fa_kvcache_append_qv8 / kvcache_append_qv8_kernel
(csrc/fa_kvcache_append_qv8.hip) through hopper_interface.kvcache_append_fp8 -- k_cache (.., h_k, d <= 64) takes the rotated
k_pe rows, v_cache (.., h_k, d_v in [256, 512]) the latent rows -- and the two-call step: that append, then the read
(fa_fwd_qv8) on the fill levels it returns.

The method is tests/test_kv8_append_gpu.py's and its helpers are imported from there: the bytes are fixed by include/fa_fwd.h
and compared with strict equality against torch's CPU `.clamp(-448, 448).to(torch.float8_e4m3fn)`; under rotary the reference
for K is the GPU's own 16-bit append of the same K rows quantised on the CPU, where a rotated column may be one e4m3 code off
(a contracted multiply-add in one kernel and not the other) and nothing else may differ.  Placement is checked on the whole
physical buffers of both caches: spare pages, unused entries and the padding of strided views keep their bytes.  The step is
bit-equal to the read over a cache whose new rows were quantised on the CPU, and meets the bound of
tests/test_qv8_kvcache_gpu.py, unchanged: |out - ref| <= 3 |pt - ref| + 1e-5, LSE 2e-3, the oracle fed the expected cache
dequantised on the CPU."""
import pytest
import torch

from test_kv8_append_gpu import K_DESCALES, V_DESCALES, append_16bit, code_order, descales, per_seq, quantise, rotary_tables
from test_qv8_kvcache_gpu import Case, _last_plan, _plan

pytestmark = pytest.mark.gpu
DEV = "cuda"
F8 = torch.float8_e4m3fn
DIMS = [(64, 512), (32, 256), (48, 320), (16, 272)]  # (d, d_v): 272 / 8 = 34 chunks, a row that ends inside a wavefront's pass
DIM_IDS = [f"d{d}_dv{dv}" for d, dv in DIMS]


def _fa3():
    from flash_attention_annotated_amd import hopper_interface
    return hopper_interface


class Store:
    """The physical fp8 caches on the CPU as bytes -- k_big of width d, v_big of width d_v -- the tensors handed to the call,
    view(big, w), and where row r of sequence s lives in them.  dense: (entries, cap, hk, w), entry = batch_idx[s] or s; paged:
    (pages, page, hk, w) through a shuffled table with spare pages; strided: heads and columns sliced from a wider buffer."""

    def __init__(self, b, cap, hk, d, dv, page=None, batch_idx=None, strided=False, spare=2, seed=0):
        g = torch.Generator().manual_seed(seed)
        self.b, self.cap, self.hk, self.d, self.dv, self.page, self.batch_idx, self.strided = b, cap, hk, d, dv, page, batch_idx, strided
        if page is not None:
            assert cap % page == 0
            n = cap // page
            self.table = torch.randperm(b * n + 3, generator=g)[: b * n].to(torch.int32).view(b, n)
            lead = (b * n + 3, page)
        else:
            lead = ((b if batch_idx is None else max(batch_idx) + 1) + spare, cap)
        pad = (1, 16) if strided else (0, 0)
        # a byte pattern without the NaN codes, different for K and V
        self.k_big = torch.randint(0, 127, (*lead, hk + pad[0], d + pad[1]), generator=g, dtype=torch.uint8)
        self.v_big = torch.randint(128, 255, (*lead, hk + pad[0], dv + pad[1]), generator=g, dtype=torch.uint8)

    def view(self, big, w):
        return big[:, :, : self.hk, : w] if self.strided else big

    def place(self, s, r):
        if self.page is not None:
            return int(self.table[s, r // self.page]), r % self.page
        return (s if self.batch_idx is None else self.batch_idx[s]), r

    def expected(self, big, w, rows, fills):
        """rows[s]: (n_s, hk, w) uint8, written at fills[s] + i; rows at or past the capacity are dropped."""
        out = big.clone()
        v = self.view(out, w)
        for s in range(self.b):
            for i in range(rows[s].shape[0]):
                r = int(fills[s]) + i
                if r < self.cap:
                    e, rr = self.place(s, r)
                    v[e, rr] = rows[s][i]
        return out

    def kwargs(self):
        kw = {}
        if self.page is not None:
            kw["page_table"] = self.table.to(DEV)
        if self.batch_idx is not None:
            kw["cache_batch_idx"] = torch.tensor(self.batch_idx, dtype=torch.int32, device=DEV)
        return kw


def run_append(st, k_new, v_new, fills, kd, vd, lens=None, max_len=None, **kw):
    """k_new / v_new dense (b, n, hk, d / d_v), or ragged (total, hk, d / d_v) with lens.  Returns (k bytes, v bytes, new fill
    levels) of the whole physical buffers after kvcache_append_fp8."""
    k_big, v_big = st.k_big.to(DEV), st.v_big.to(DEV)
    if lens is not None:
        cu = torch.zeros(len(lens) + 1, dtype=torch.int32)
        cu[1:] = torch.cumsum(torch.tensor(lens), 0)
        kw.update(cu_seqlens_k_new=cu.to(DEV), max_seqlen_k_new=max_len)
    new_fill = _fa3().kvcache_append_fp8(st.view(k_big, st.d).view(F8), st.view(v_big, st.dv).view(F8), k_new.to(DEV), v_new.to(DEV),
                                         torch.tensor(fills, dtype=torch.int32, device=DEV), kd.to(DEV), vd.to(DEV),
                                         **st.kwargs(), **kw)
    torch.cuda.synchronize()
    assert new_fill.dtype == torch.int32 and new_fill.is_cuda
    return k_big.cpu(), v_big.cpu(), new_fill.cpu()


def check_placement(st, dtype, fills, n_new=None, lens=None, max_len=None, seed=0):
    torch.manual_seed(seed)
    b, hk = st.b, st.hk
    lead = (b, n_new) if lens is None else (sum(lens) + 2,)  # (ragged: two rows behind cu_seqlens[b] are ignored)
    k_new, v_new = (torch.randn(*lead, hk, st.d) * 3).to(dtype), (torch.randn(*lead, hk, st.dv) * 3).to(dtype)
    kd, vd = descales(b, hk, K_DESCALES), descales(b, hk, V_DESCALES, 3)
    k_got, v_got, new_fill = run_append(st, k_new, v_new, fills, kd, vd, lens=lens, max_len=max_len)
    kq = [quantise(r, kd[s]) for s, r in enumerate(per_seq(k_new, lens))]
    vq = [quantise(r, vd[s]) for s, r in enumerate(per_seq(v_new, lens))]
    assert torch.equal(k_got, st.expected(st.k_big, st.d, kq, fills))
    assert torch.equal(v_got, st.expected(st.v_big, st.dv, vq, fills))
    want_fill = [min(f + (n_new if lens is None else lens[s]), st.cap) for s, f in enumerate(fills)]
    assert new_fill.tolist() == want_fill


# ---- 1. every 16-bit value ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_every_16bit_value_byte_for_byte(dtype):
    """1024 new rows, h_k 1, d 64 / d_v 512, as 8 sequences of 128 rows: k_new holds all 65536 bit patterns once (NaNs -> 0),
    v_new a permutation of eight copies of them; a descale per sequence and tensor, the eight of tests/test_kv8_append_gpu.py,
    half powers of two: every tie, subnormal, saturation, +-0 and +-inf under exact and inexact scaling.  Every other byte of
    both caches keeps its prefill."""
    bits = torch.arange(65536, dtype=torch.int32).to(torch.int16)  # (wraps: all patterns)
    k_new = bits.view(dtype).clone()
    k_new[torch.isnan(k_new.float())] = 0
    g = torch.Generator().manual_seed(1)
    v_new = k_new.repeat(8)[torch.randperm(8 * 65536, generator=g)]
    k_new, v_new = k_new.view(8, 128, 1, 64), v_new.view(8, 128, 1, 512)
    kd, vd = K_DESCALES.view(8, 1), V_DESCALES.view(8, 1)
    fills = [3, 0, 5, 1, 0, 7, 2, 4]
    st = Store(8, 136, 1, 64, 512, spare=1, seed=2)
    k_got, v_got, new_fill = run_append(st, k_new, v_new, fills, kd, vd)
    k_want = st.expected(st.k_big, 64, [quantise(k_new[s], kd[s]) for s in range(8)], fills)
    v_want = st.expected(st.v_big, 512, [quantise(v_new[s], vd[s]) for s in range(8)], fills)
    print(f"all 16-bit values {dtype}: unequal K bytes {(k_got != k_want).sum().item()}, V bytes {(v_got != v_want).sum().item()}")
    assert torch.equal(k_got, k_want) and torch.equal(v_got, v_want)
    assert torch.equal(k_got[0, :3], st.k_big[0, :3]) and torch.equal(v_got[0, 131:], st.v_big[0, 131:]) and torch.equal(v_got[8], st.v_big[8])
    assert not torch.equal(k_got[0, 3:131], st.k_big[0, 3:131]) and not torch.equal(v_got[1, :128], st.v_big[1, :128])
    assert new_fill.tolist() == [f + 128 for f in fills]


# ---- 2. placement ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hk", [1, 2])
@pytest.mark.parametrize("d,dv", DIMS, ids=DIM_IDS)
def test_cache_batch_idx_into_a_larger_cache(d, dv, hk):
    dtype = torch.bfloat16 if hk == 1 else torch.float16
    check_placement(Store(3, 48, hk, d, dv, batch_idx=[4, 0, 2], seed=3), dtype, fills=[5, 0, 40], n_new=4, seed=3)


@pytest.mark.parametrize("hk", [1, 2])
@pytest.mark.parametrize("d,dv", DIMS, ids=DIM_IDS)
def test_strided_cache_view(d, dv, hk):
    st = Store(2, 32, hk, d, dv, strided=True, seed=4)
    v = st.view(st.v_big, dv)
    assert v.stride(2) != dv and v.stride(1) != hk * dv and not v.is_contiguous()
    check_placement(st, torch.bfloat16, fills=[0, 7], n_new=5, seed=4)


@pytest.mark.parametrize("page", [16, 64])
@pytest.mark.parametrize("hk", [1, 2])
@pytest.mark.parametrize("d,dv", DIMS, ids=DIM_IDS)
def test_paged_rows_cross_a_page_boundary(d, dv, hk, page):
    """A shuffled table with spare pages; new rows [page - 3, page + 4) and [2 page - 1, 2 page + 6) cross a boundary."""
    check_placement(Store(2, 3 * page, hk, d, dv, page=page, seed=page), torch.bfloat16, fills=[page - 3, 2 * page - 1], n_new=7, seed=page)


@pytest.mark.parametrize("page", [None, 16], ids=["dense", "page16"])
@pytest.mark.parametrize("hk", [1, 2])
@pytest.mark.parametrize("d,dv", DIMS, ids=DIM_IDS)
def test_rows_past_the_capacity_are_dropped(d, dv, hk, page):
    """Sequence 1 has room for 2 of its 6 new rows: the rest is dropped (no write past the entry / into another page) and the
    new fill level is the capacity."""
    check_placement(Store(2, 32, hk, d, dv, page=page, seed=5), torch.float16, fills=[3, 30], n_new=6, seed=5)
    check_placement(Store(3, 32, hk, d, dv, page=page, seed=6), torch.float16, fills=[3, 30, 32], lens=[6, 6, 2], max_len=6, seed=6)


@pytest.mark.parametrize("max_len", [70, 0], ids=["max_len", "search"])
@pytest.mark.parametrize("hk", [1, 2])
@pytest.mark.parametrize("d,dv", DIMS, ids=DIM_IDS)
def test_ragged_new_rows(d, dv, hk, max_len):
    """cu_seqlens_k_new with lengths (0, 1, 5, 70) in both lookup modes: an empty sequence, more rows than a workgroup's 16;
    dense entries at h_k 1, pages of 16 at h_k 2."""
    check_placement(Store(4, 96, hk, d, dv, page=None if hk == 1 else 16, seed=7), torch.bfloat16, fills=[9, 0, 14, 20],
                    lens=[0, 1, 5, 70], max_len=max_len, seed=7)


def test_more_kv_heads_than_a_pass_has_k_lanes():
    """h_k 20 at d 64 / d_v 256: 80 K slots against 64 lanes -- the K items spill into the second of the row's 10 passes."""
    check_placement(Store(2, 8, 20, 64, 256, seed=8), torch.bfloat16, fills=[1, 5], n_new=2, seed=8)


# ---- 3. rotary -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_seqlens", [False, True], ids=["at_fill", "rotary_seqlens"])
@pytest.mark.parametrize("d,dv,rd", [(64, 512, 64), (64, 512, 16), (32, 256, 32), (32, 256, 16)], ids=["d64_full", "d64_rd16", "d32_full", "d32_rd16"])
@pytest.mark.parametrize("interleaved", [True, False], ids=["interleaved", "halves"])
@pytest.mark.parametrize("form", ["dense", "ragged"])
def test_rotary(form, interleaved, d, dv, rd, with_seqlens):
    """K against the GPU's 16-bit append of the same K rows (a 16-bit cache of d_v = d: only K is rotated, the V it writes is not
    looked at) quantised on the CPU; V, never rotated, against the CPU quantisation of v_new."""
    dtype = torch.bfloat16 if interleaved else torch.float16
    b, cap, hk = 3, 40, 2
    fills = [0, 11, 30]
    lens = None if form == "dense" else [4, 0, 9]
    n_new = 5
    torch.manual_seed(rd + interleaved + d)
    lead = (b, n_new) if lens is None else (sum(lens),)
    k_new, v_new = (torch.randn(*lead, hk, d) * 2).to(dtype), (torch.randn(*lead, hk, dv) * 2).to(dtype)
    cos, sin = rotary_tables(64, rd, dtype, rd)
    rot_seqlens = [17, 3, 40] if with_seqlens else None
    kd, vd = descales(b, hk, K_DESCALES, 1), descales(b, hk, V_DESCALES, 2)
    st = Store(b, cap, hk, d, dv, spare=0, seed=8)
    rot = dict(rotary_cos=cos.to(DEV), rotary_sin=sin.to(DEV), rotary_interleaved=interleaved,
               rotary_seqlens=None if rot_seqlens is None else torch.tensor(rot_seqlens, dtype=torch.int32, device=DEV))
    k_got, v_got, _ = run_append(st, k_new, v_new, fills, kd, vd, lens=lens, max_len=None if lens is None else 0, **rot)
    k16, _ = append_16bit(k_new, torch.zeros_like(k_new), fills, cap, cos, sin, interleaved, rot_seqlens, lens)
    counts = [n_new] * b if lens is None else lens
    vq = [quantise(r, vd[s]) for s, r in enumerate(per_seq(v_new, lens))]
    assert torch.equal(v_got, st.expected(st.v_big, dv, vq, fills))
    unequal = 0
    for s, (f, n) in enumerate(zip(fills, counts)):
        kq = quantise(k16[s, f: f + n], kd[s])
        assert torch.equal(k_got[s, f: f + n, :, rd:], kq[..., rd:])
        step = (code_order(k_got[s, f: f + n, :, :rd]) - code_order(kq[..., :rd])).abs()
        unequal += int((step != 0).sum())
        assert int(step.max()) <= 1 if n else True
        assert torch.equal(k_got[s, :f], st.k_big[s, :f]) and torch.equal(k_got[s, f + n:], st.k_big[s, f + n:])
        if n:  # (the rotation happened: the rotated columns are not the quantisation of the rows as given)
            assert not torch.equal(k_got[s, f: f + n, :, :rd], quantise(per_seq(k_new, lens)[s], kd[s])[..., :rd])
    print(f"rotary {form} interleaved={interleaved} d={d} rd={rd} seqlens={with_seqlens}: {unequal} rotated bytes differ from the "
          f"quantised 16-bit append")


# ---- 4. the step: append, then read -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("page", [None, 16], ids=["dense", "page16"])
@pytest.mark.parametrize("with_qv", [True, False], ids=["qv", "no_qv"])
@pytest.mark.parametrize("n_new", [1, 3])
def test_step_append_then_read(n_new, with_qv, page):
    """b 2, h 16, h_k 1, d 64 / d_v 512, descales 0.3 / 1.7, causal with n_new query rows: fill levels 63 (the new rows end a
    64-key tile or cross its edge) and 100 (mid-tile).  kvcache_append_fp8, then flash_attn_with_kvcache on the fill levels it
    returned: out / LSE bit-equal to the same read over caches whose new rows were quantised on the CPU, and within the bound of
    tests/test_qv8_kvcache_gpu.py against the oracle on those caches dequantised."""
    c = Case(b=2, sq=n_new, h=16, hk=1, d=64, dv=512, cap=320, lens=(63, 100), page=page, causal=True, kdesc=0.3, vdesc=1.7,
             with_qv=with_qv, seed=80 + n_new)
    torch.manual_seed(81)
    k_new, v_new = torch.randn(2, n_new, 1, 64).to(c.dtype), torch.randn(2, n_new, 1, 512).to(c.dtype)
    fa3 = _fa3()
    q, kd, vd = c.q.to(DEV), c.kdesc.to(DEV), c.vdesc.to(DEV)
    read = dict(qv=None if c.qv is None else c.qv.to(DEV), k_descale=kd, v_descale=vd, causal=True, num_splits=1, return_softmax_lse=True,
                page_table=c.table.to(DEV) if page else None)
    kc, vc = c._phys(c.k8), c._phys(c.v8)
    fill = fa3.kvcache_append_fp8(kc, vc, k_new.to(DEV), v_new.to(DEV), c.lens.to(DEV), kd, vd, page_table=read["page_table"])
    out, lse, *_ = fa3.flash_attn_with_kvcache(q, kc, vc, cache_seqlens=fill, **read)
    plan = _last_plan()
    assert plan == _plan(512), plan
    assert fill.tolist() == [63 + n_new, 100 + n_new]
    # the expected caches: the new rows quantised on the CPU
    k_exp, v_exp = c.k8.view(torch.uint8).clone(), c.v8.view(torch.uint8).clone()
    for s, f in enumerate((63, 100)):
        k_exp[s, f: f + n_new] = quantise(k_new[s], c.kdesc[s])
        v_exp[s, f: f + n_new] = quantise(v_new[s], c.vdesc[s])
    c.k8, c.v8, c.lens = k_exp.view(F8), v_exp.view(F8), c.lens + n_new
    kc2, vc2 = c._phys(c.k8), c._phys(c.v8)
    assert torch.equal(kc.view(torch.uint8), kc2.view(torch.uint8)) and torch.equal(vc.view(torch.uint8), vc2.view(torch.uint8))
    out2, lse2, *_ = fa3.flash_attn_with_kvcache(q, kc2, vc2, cache_seqlens=c.lens.to(DEV), **read)
    assert torch.equal(out, out2) and torch.equal(lse, lse2)
    ref, ref_lse, pt = c.reference()
    out, lse = out.cpu(), lse.cpu()
    err = (out.float() - ref.float()).abs().max().item()
    bound = 3 * (pt.float() - ref.float()).abs().max().item() + 1e-5
    fin = torch.isfinite(ref_lse)
    lse_err = (lse[fin] - ref_lse[fin]).abs().max().item()
    print(f"qv8 step n_new={n_new} qv={with_qv} page={page}: |out - ref| = {err:.3e}  bound = {bound:.3e}  |lse - ref| = {lse_err:.3e}  "
          f"plan = {plan}")
    assert err <= bound
    assert torch.equal(fin, torch.isfinite(lse))
    assert lse_err < 2e-3


# ---- 5. graph capture ----------------------------------------------------------------------------------------------------------
def test_step_in_a_hip_graph():
    """One capture of append + read on a single stream, two replays with k_new / v_new and cache_seqlens changed in place
    between them: cache bytes, fill levels and out equal the eager calls' (no host sync, nothing baked into the capture)."""
    c = Case(b=2, h=16, hk=1, d=64, dv=512, cap=128, lens=(5, 9), kdesc=0.3, vdesc=1.7, seed=90)
    fa3 = _fa3()
    torch.manual_seed(91)
    steps = [(torch.randn(2, 1, 1, 64).bfloat16(), torch.randn(2, 1, 1, 512).bfloat16(), torch.tensor([5, 9], dtype=torch.int32)),
             (torch.randn(2, 1, 1, 64).bfloat16(), torch.randn(2, 1, 1, 512).bfloat16(), torch.tensor([63, 40], dtype=torch.int32))]
    q, qv, kd, vd = c.q.to(DEV), c.qv.to(DEV), c.kdesc.to(DEV), c.vdesc.to(DEV)

    def call(kc, vc, k_new, v_new, lens):
        fill = fa3.kvcache_append_fp8(kc, vc, k_new, v_new, lens, kd, vd)
        return fa3.flash_attn_with_kvcache(q, kc, vc, qv=qv, cache_seqlens=fill, k_descale=kd, v_descale=vd, num_splits=1), fill

    kc_e, vc_e = c._phys(c.k8), c._phys(c.v8)
    eager = [tuple(t.cpu() for t in call(kc_e, vc_e, k.to(DEV), v.to(DEV), n.to(DEV))) for k, v, n in steps]
    kc_g, vc_g = c._phys(c.k8), c._phys(c.v8)
    k_new, v_new, lens = (t.to(DEV) for t in steps[0])
    call(kc_g, vc_g, k_new, v_new, lens)  # warm-up outside the capture (writes what the first replay writes again)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, fill = call(kc_g, vc_g, k_new, v_new, lens)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), eager[0][0]) and fill.tolist() == [6, 10]
    k_new.copy_(steps[1][0]); v_new.copy_(steps[1][1]); lens.copy_(steps[1][2])
    graph.replay()
    torch.cuda.synchronize()
    assert _last_plan() == _plan(512)
    assert torch.equal(out.cpu(), eager[1][0]) and fill.tolist() == [64, 41]
    assert torch.equal(kc_g.view(torch.uint8), kc_e.view(torch.uint8)) and torch.equal(vc_g.view(torch.uint8), vc_e.view(torch.uint8))
    assert not torch.equal(vc_g.view(torch.uint8).cpu(), c.v8.view(torch.uint8))  # (rows were written)


# ---- 6. what stays refused -------------------------------------------------------------------------------------------------------
def test_only_the_head_dim_pair_is_the_mla_shape():
    """A V that differs from K in anything but this head-dim pair keeps "v must have the shape of k"; the new rows are checked
    against the two head dims; nothing is written by a refused call."""
    fa3 = _fa3()
    kc = torch.zeros(2, 64, 1, 64, device=DEV).to(F8)
    lens = torch.tensor([5, 9], dtype=torch.int32, device=DEV)
    one = torch.ones(2, 1, device=DEV)
    k_new = torch.randn(2, 1, 1, 64, dtype=torch.bfloat16, device=DEV)
    v_of = lambda w: torch.randn(2, 1, 1, w, dtype=torch.bfloat16, device=DEV)  # noqa: E731
    for shape in ((2, 64, 1, 128), (2, 64, 1, 264), (2, 64, 1, 528), (2, 32, 1, 512), (2, 64, 2, 512), (3, 64, 1, 512)):
        vc = torch.zeros(*shape, device=DEV).to(F8)
        with pytest.raises(RuntimeError, match="v must have the shape of k"):
            fa3.kvcache_append_fp8(kc, vc, k_new, v_of(shape[-1]), lens, one, one)
    k128 = torch.zeros(2, 64, 1, 128, device=DEV).to(F8)  # (head_size 128 beside 512: not the MLA shape)
    with pytest.raises(RuntimeError, match="v must have the shape of k"):
        fa3.kvcache_append_fp8(k128, torch.zeros(2, 64, 1, 512, device=DEV).to(F8), v_of(128), v_of(512), lens, one, one)
    vc = torch.zeros(2, 64, 1, 512, device=DEV).to(F8)
    with pytest.raises(RuntimeError, match=r"v_new must have shape \(batch_size, k_new.size\(1\), num_heads_k, head_size_v\)"):
        fa3.kvcache_append_fp8(kc, vc, k_new, v_of(64), lens, one, one)
    with pytest.raises(RuntimeError, match=r"k_new must have shape \(batch_size, k_new.size\(1\), num_heads_k, head_size\)"):
        fa3.kvcache_append_fp8(kc, vc, v_of(512), v_of(512), lens, one, one)
    tab = torch.rand(64, 40, device=DEV).bfloat16()  # rotary_dim 80: within d_v, above d
    with pytest.raises(RuntimeError, match="rotary_dim must be <= headdim"):
        fa3.kvcache_append_fp8(kc, vc, k_new, v_of(512), lens, one, one, rotary_cos=tab, rotary_sin=tab)
    assert torch.all(kc.view(torch.uint8) == 0) and torch.all(vc.view(torch.uint8) == 0)
    assert fa3.kvcache_append_fp8(kc, vc, k_new, v_of(512), lens, one, one).tolist() == [6, 10]
