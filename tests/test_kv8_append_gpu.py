"""GPU tests of the write half of the fp8 (e4m3) KV cache: fa_kvcache_append_kv8 / kvcache_append_kv8_kernel
(csrc/fa_kvcache_append_kv8.hip) through hopper_interface.kvcache_append_fp8 and through flash_attn_with_kvcache(k=, v=) over
a Float8_e4m3fn cache with both descales.

The bytes are fixed by include/fa_fwd.h: inv = 1.0f / descale[s, g] (fp32), y = float(x) * inv, byte =
e4m3fn_rne(clamp(y, -448, 448)).  torch's CPU `.clamp(-448, 448).to(torch.float8_e4m3fn)` is that rounding, so the bytes are
compared with strict equality; under rotary the reference is the GPU's own 16-bit append quantised on the CPU (one rotation
code for both, so equal -- but the compiler may contract a multiply-add in one kernel and not the other: a rotated column may
be one e4m3 code off, nothing else may differ).  Placement is checked on the whole physical buffer: spare pages, unused
entries and the padding of strided views keep their bytes.  End to end the bound is that of tests/test_kv8_kvcache_gpu.py,
unchanged: |out - ref| <= 3 |pt - ref| + 1e-5, LSE 1e-3, the oracle fed the expected cache dequantised on the CPU."""
import pytest
import torch

from test_kv8_kvcache_gpu import Case, _last_plan

pytestmark = pytest.mark.gpu
DEV = "cuda"
F8 = torch.float8_e4m3fn
K_DESCALES = torch.tensor([0.5, 0.37, 2.0, 3.0, 0.125, 1.7e-2, 16.0, 11.0])  # half powers of two, half not
V_DESCALES = torch.tensor([0.25, 0.41, 4.0, 5.0, 1.0, 2.3e-2, 8.0, 13.0])


def _fa3():
    from flash_attention_annotated_amd import hopper_interface
    return hopper_interface


def quantise(x, descale):
    """x: (..., h_k, d) fp16 / bf16 on the CPU, descale: (h_k,) fp32 -> the bytes of include/fa_fwd.h as uint8."""
    inv = torch.ones((), dtype=torch.float32) / descale.to(torch.float32)
    y = x.to(torch.float32) * inv[:, None]
    return y.clamp(-448.0, 448.0).to(F8).view(torch.uint8)


def descales(b, hk, table, shift=0):
    return table[(torch.arange(b * hk) + shift) % len(table)].view(b, hk).contiguous()


def code_order(u8):
    """Position of an e4m3 byte in the ordered sequence of codes: -448 ... -0, +0 ... 448 (-0 and +0 are neighbours)."""
    u = u8.to(torch.int32)
    return torch.where(u < 128, u, -(u - 128) - 1)


class Store:
    """A physical fp8 cache on the CPU as bytes, `big`, the tensor handed to the call, `view(big)`, and where row r of
    sequence s lives in that view.  dense: (entries, cap, hk, d), entry = batch_idx[s] or s; paged: (pages, page, hk, d)
    through a shuffled table with spare pages; strided: heads and columns sliced from a wider buffer."""

    def __init__(self, b, cap, hk, d, page=None, batch_idx=None, strided=False, spare=2, seed=0):
        g = torch.Generator().manual_seed(seed)
        self.b, self.cap, self.hk, self.d, self.page, self.batch_idx, self.strided = b, cap, hk, d, page, batch_idx, strided
        if page is not None:
            assert cap % page == 0
            n = cap // page
            self.table = torch.randperm(b * n + 3, generator=g)[: b * n].to(torch.int32).view(b, n)
            shape = (b * n + 3, page, hk, d)
        else:
            shape = ((b if batch_idx is None else max(batch_idx) + 1) + spare, cap, hk, d)
        if strided:
            shape = (shape[0], shape[1], hk + 1, d + 16)
        # a byte pattern without the NaN codes, different for K and V
        self.k_big = torch.randint(0, 127, shape, generator=g, dtype=torch.uint8)
        self.v_big = torch.randint(128, 255, shape, generator=g, dtype=torch.uint8)

    def view(self, big):
        return big[:, :, : self.hk, : self.d] if self.strided else big

    def place(self, s, r):
        if self.page is not None:
            return int(self.table[s, r // self.page]), r % self.page
        return (s if self.batch_idx is None else self.batch_idx[s]), r

    def expected(self, big, rows, fills):
        """rows[s]: (n_s, hk, d) uint8, written at fills[s] + i; rows at or past the capacity are dropped."""
        out = big.clone()
        v = self.view(out)
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
    """k_new / v_new dense (b, n, hk, d), or ragged (total, hk, d) with lens.  Returns (k bytes, v bytes, new fill levels) of
    the whole physical buffers after kvcache_append_fp8."""
    k_big, v_big = st.k_big.to(DEV), st.v_big.to(DEV)
    if lens is not None:
        cu = torch.zeros(len(lens) + 1, dtype=torch.int32)
        cu[1:] = torch.cumsum(torch.tensor(lens), 0)
        kw.update(cu_seqlens_k_new=cu.to(DEV), max_seqlen_k_new=max_len)
    new_fill = _fa3().kvcache_append_fp8(st.view(k_big).view(F8), st.view(v_big).view(F8), k_new.to(DEV), v_new.to(DEV),
                                         torch.tensor(fills, dtype=torch.int32, device=DEV), kd.to(DEV), vd.to(DEV),
                                         **st.kwargs(), **kw)
    torch.cuda.synchronize()
    assert new_fill.dtype == torch.int32 and new_fill.is_cuda
    return k_big.cpu(), v_big.cpu(), new_fill.cpu()


def per_seq(x, lens):
    """dense (b, n, hk, d) -> list of (n, hk, d); ragged (total, hk, d) with lens -> list of (len_s, hk, d)."""
    if lens is None:
        return list(x)
    out, at = [], 0
    for n in lens:
        out.append(x[at: at + n])
        at += n
    return out


def check_placement(st, dtype, fills, n_new=None, lens=None, max_len=None, seed=0):
    torch.manual_seed(seed)
    b, hk, d = st.b, st.hk, st.d
    shape = (b, n_new, hk, d) if lens is None else (sum(lens) + 2, hk, d)  # (ragged: two rows behind cu_seqlens[b] are ignored)
    k_new, v_new = (torch.randn(shape) * 3).to(dtype), (torch.randn(shape) * 3).to(dtype)
    kd, vd = descales(b, hk, K_DESCALES), descales(b, hk, V_DESCALES, 3)
    k_got, v_got, new_fill = run_append(st, k_new, v_new, fills, kd, vd, lens=lens, max_len=max_len)
    kq = [quantise(r, kd[s]) for s, r in enumerate(per_seq(k_new, lens))]
    vq = [quantise(r, vd[s]) for s, r in enumerate(per_seq(v_new, lens))]
    assert torch.equal(k_got, st.expected(st.k_big, kq, fills))
    assert torch.equal(v_got, st.expected(st.v_big, vq, fills))
    want_fill = [min(f + (n_new if lens is None else lens[s]), st.cap) for s, f in enumerate(fills)]
    assert new_fill.tolist() == want_fill


# ---- 1. every 16-bit value ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_every_16bit_value_byte_for_byte(dtype):
    """k_new holds all 65536 bit patterns once (1 x 64 rows x 8 kv heads x 128; NaNs -> 0), v_new a permutation of them; eight
    distinct descales per tensor, half powers of two: every tie, subnormal, saturation, +-0 and +-inf under exact and inexact
    scaling.  Rows 3 ... 66 of entry 0 are written, every other byte of both caches keeps its prefill."""
    bits = torch.arange(65536, dtype=torch.int32).to(torch.int16)  # (wraps: all patterns)
    k_new = bits.view(dtype).clone()
    k_new[torch.isnan(k_new.float())] = 0
    g = torch.Generator().manual_seed(1)
    v_new = k_new[torch.randperm(65536, generator=g)]
    k_new, v_new = k_new.view(1, 64, 8, 128), v_new.view(1, 64, 8, 128)
    kd, vd = K_DESCALES.view(1, 8), V_DESCALES.view(1, 8)
    st = Store(1, 80, 8, 128, spare=1, seed=2)
    k_got, v_got, new_fill = run_append(st, k_new, v_new, [3], kd, vd)
    k_want = st.expected(st.k_big, [quantise(k_new[0], kd[0])], [3])
    v_want = st.expected(st.v_big, [quantise(v_new[0], vd[0])], [3])
    print(f"all 16-bit values {dtype}: unequal K bytes {(k_got != k_want).sum().item()}, V bytes {(v_got != v_want).sum().item()}")
    assert torch.equal(k_got, k_want) and torch.equal(v_got, v_want)
    assert torch.equal(k_got[0, :3], st.k_big[0, :3]) and torch.equal(k_got[0, 67:], st.k_big[0, 67:]) and torch.equal(k_got[1], st.k_big[1])
    assert new_fill.tolist() == [67]


# ---- 2. placement ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_cache_batch_idx_into_a_larger_cache(dtype):
    check_placement(Store(3, 48, 2, 64, batch_idx=[4, 0, 2], seed=3), dtype, fills=[5, 0, 40], n_new=4, seed=3)


def test_strided_cache_view():
    st = Store(2, 32, 3, 64, strided=True, seed=4)
    v = st.view(st.k_big)
    assert v.stride(2) != 64 and v.stride(1) != 3 * 64 and not v.is_contiguous()
    check_placement(st, torch.bfloat16, fills=[0, 7], n_new=5, seed=4)


@pytest.mark.parametrize("page", [16, 64])
def test_paged_rows_cross_a_page_boundary(page):
    """A shuffled table with spare pages; new rows [page - 3, page + 4) and [2 page - 1, 2 page + 6) cross a boundary."""
    check_placement(Store(2, 3 * page, 2, 128, page=page, seed=page), torch.bfloat16, fills=[page - 3, 2 * page - 1], n_new=7, seed=page)


@pytest.mark.parametrize("page", [None, 16], ids=["dense", "page16"])
def test_rows_past_the_capacity_are_dropped(page):
    """Sequence 1 has room for 2 of its 6 new rows: the rest is dropped (no write past the entry / into another page) and the
    new fill level is the capacity."""
    check_placement(Store(2, 32, 2, 64, page=page, seed=5), torch.float16, fills=[3, 30], n_new=6, seed=5)
    check_placement(Store(3, 32, 2, 64, page=page, seed=6), torch.float16, fills=[3, 30, 32], lens=[6, 6, 2], max_len=6, seed=6)


@pytest.mark.parametrize("max_len", [70, 0], ids=["max_len", "search"])
@pytest.mark.parametrize("page", [None, 16], ids=["dense", "page16"])
def test_ragged_new_rows(max_len, page):
    """cu_seqlens_k_new with lengths (0, 1, 5, 70) in both lookup modes: an empty sequence, more rows than a workgroup's 16."""
    check_placement(Store(4, 96, 2, 64, page=page, seed=7), torch.bfloat16, fills=[9, 0, 14, 20], lens=[0, 1, 5, 70], max_len=max_len, seed=7)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("hk", [1, 3])
@pytest.mark.parametrize("d", [16, 64, 80, 128])
def test_head_dims_and_head_counts(d, hk, dtype):
    """d16: one chunk, half a slot; d80: an odd chunk count; h_k 1 and 3: rows of fewer items than a wavefront has lanes."""
    check_placement(Store(2, 16, hk, d, seed=d + hk), dtype, fills=[1, 9], n_new=3, seed=d + hk)
    check_placement(Store(2, 16, hk, d, seed=d + hk + 1), dtype, fills=[1, 9], lens=[2, 3], max_len=0, seed=d + hk + 1)


# ---- 3. rotary -----------------------------------------------------------------------------------------------------------------
def rotary_tables(rows, rd, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    ang = torch.rand(rows, rd // 2, generator=g) * 6.283
    return torch.cos(ang).to(dtype), torch.sin(ang).to(dtype)


def append_16bit(k_new, v_new, fills, cap, cos, sin, interleaved, rot_seqlens, lens):
    """The GPU's own 16-bit append of the same rows into a zeroed 16-bit cache (b, cap, hk, d), through the public call (its
    attention result is not looked at).  Returns the caches on the CPU."""
    dtype, hk, d, b = k_new.dtype, k_new.shape[-2], k_new.shape[-1], len(fills)
    kc = torch.zeros(b, cap, hk, d, dtype=dtype, device=DEV)
    vc = torch.zeros_like(kc)
    kw = dict(k=k_new.to(DEV), v=v_new.to(DEV), rotary_cos=cos.to(DEV), rotary_sin=sin.to(DEV), rotary_interleaved=interleaved,
              cache_seqlens=torch.tensor(fills, dtype=torch.int32, device=DEV),
              rotary_seqlens=None if rot_seqlens is None else torch.tensor(rot_seqlens, dtype=torch.int32, device=DEV))
    if lens is None:
        q = torch.zeros(b, 1, hk, d, dtype=dtype, device=DEV)
    else:  # one query row per sequence beside the ragged new rows
        q = torch.zeros(b, hk, d, dtype=dtype, device=DEV)
        cu = torch.zeros(b + 1, dtype=torch.int32)
        cu[1:] = torch.cumsum(torch.tensor(lens), 0)
        kw.update(cu_seqlens_q=torch.arange(b + 1, dtype=torch.int32, device=DEV), max_seqlen_q=1, cu_seqlens_k_new=cu.to(DEV))
    _fa3().flash_attn_with_kvcache(q, kc, vc, **kw)
    torch.cuda.synchronize()
    return kc.cpu(), vc.cpu()


def check_against_16bit_append(k_got, v_got, k16, v16, kd, vd, fills, counts, rd, k_prefill, v_prefill, name):
    """k_got / v_got: (b, cap, hk, d) bytes after the fp8 append.  Appended rows: V and the columns >= rd strictly equal to the
    quantised 16-bit cache, rotated columns at most one code apart; all other rows keep the prefill."""
    unequal = 0
    for s, (f, n) in enumerate(zip(fills, counts)):
        kq, vq = quantise(k16[s, f: f + n], kd[s]), quantise(v16[s, f: f + n], vd[s])
        assert torch.equal(v_got[s, f: f + n], vq)
        assert torch.equal(k_got[s, f: f + n, :, rd:], kq[..., rd:])
        step = (code_order(k_got[s, f: f + n, :, :rd]) - code_order(kq[..., :rd])).abs()
        unequal += int((step != 0).sum())
        assert int(step.max()) <= 1 if n else True
        assert torch.equal(k_got[s, :f], k_prefill[s, :f]) and torch.equal(k_got[s, f + n:], k_prefill[s, f + n:])
        assert torch.equal(v_got[s, :f], v_prefill[s, :f]) and torch.equal(v_got[s, f + n:], v_prefill[s, f + n:])
    print(f"rotary {name}: {unequal} rotated bytes differ from the quantised 16-bit append")


@pytest.mark.parametrize("with_seqlens", [False, True], ids=["at_fill", "rotary_seqlens"])
@pytest.mark.parametrize("rd", [64, 32], ids=["full", "partial"])
@pytest.mark.parametrize("interleaved", [True, False], ids=["interleaved", "halves"])
@pytest.mark.parametrize("form", ["dense", "ragged"])
def test_rotary(form, interleaved, rd, with_seqlens):
    dtype = torch.bfloat16 if interleaved else torch.float16
    b, cap, hk, d = 3, 40, 2, 64
    fills = [0, 11, 30]
    lens = None if form == "dense" else [4, 0, 9]
    n_new = 5
    torch.manual_seed(rd + interleaved)
    shape = (b, n_new, hk, d) if lens is None else (sum(lens), hk, d)
    k_new, v_new = (torch.randn(shape) * 2).to(dtype), (torch.randn(shape) * 2).to(dtype)
    cos, sin = rotary_tables(64, rd, dtype, rd)
    rot_seqlens = [17, 3, 40] if with_seqlens else None
    kd, vd = descales(b, hk, K_DESCALES, 1), descales(b, hk, V_DESCALES, 2)
    st = Store(b, cap, hk, d, spare=0, seed=8)
    rot = dict(rotary_cos=cos.to(DEV), rotary_sin=sin.to(DEV), rotary_interleaved=interleaved,
               rotary_seqlens=None if rot_seqlens is None else torch.tensor(rot_seqlens, dtype=torch.int32, device=DEV))
    k_got, v_got, _ = run_append(st, k_new, v_new, fills, kd, vd, lens=lens, max_len=None if lens is None else 0, **rot)
    k16, v16 = append_16bit(k_new, v_new, fills, cap, cos, sin, interleaved, rot_seqlens, lens)
    counts = [n_new] * b if lens is None else lens
    check_against_16bit_append(k_got, v_got, k16, v16, kd, vd, fills, counts, rd, st.k_big, st.v_big,
                               f"{form} interleaved={interleaved} rd={rd} seqlens={with_seqlens}")


# ---- 4. end to end -------------------------------------------------------------------------------------------------------------
def run_step(c, k_new, v_new, new_lens=None, rotary=None, **kw):
    """flash_attn_with_kvcache over c's fp8 caches with new rows.  Returns (out, lse, K bytes, V bytes) on the CPU."""
    kc, vc = c._phys(c.k8), c._phys(c.v8)
    ckw = c.kwargs()
    args = dict(k=k_new.to(DEV), v=v_new.to(DEV), cache_seqlens=ckw["seqused_k"], k_descale=c.kdesc.to(DEV), v_descale=c.vdesc.to(DEV),
                causal=c.causal, window_size=c.window, softcap=c.softcap, num_splits=1, return_softmax_lse=True,
                page_table=ckw.get("page_table"), cu_seqlens_q=ckw.get("cu_seqlens_q"), max_seqlen_q=ckw.get("max_seqlen_q"))
    if new_lens is not None:
        cu = torch.zeros(len(new_lens) + 1, dtype=torch.int32)
        cu[1:] = torch.cumsum(torch.tensor(new_lens), 0)
        args["cu_seqlens_k_new"] = cu.to(DEV)
    if rotary is not None:
        args.update(rotary_cos=rotary[0].to(DEV), rotary_sin=rotary[1].to(DEV), rotary_interleaved=rotary[2])
    args.update(kw)
    out, lse, *_ = _fa3().flash_attn_with_kvcache(c.q.to(DEV), kc, vc, **args)
    plan = _last_plan()
    assert plan is not None and plan.startswith("kv8_fwd_kernel"), plan
    return out.cpu(), lse.cpu(), kc.view(torch.uint8).cpu(), vc.view(torch.uint8).cpu(), (kc, vc, args, plan)


def check_step(c, k_new, v_new, new_lens, name):
    """No rotary: the caches must hold the expected bytes, and out / lse meet the oracle on the expected cache."""
    old = c.lens.clone()
    out, lse, k_got, v_got, (kc, vc, args, plan) = run_step(c, k_new, v_new, new_lens)
    k_exp, v_exp = c.k8.view(torch.uint8).clone(), c.v8.view(torch.uint8).clone()
    for s, (kr, vr) in enumerate(zip(per_seq(k_new, new_lens), per_seq(v_new, new_lens))):
        f, n = int(old[s]), kr.shape[0]
        k_exp[s, f: f + n] = quantise(kr, c.kdesc[s])
        v_exp[s, f: f + n] = quantise(vr, c.vdesc[s])
        c.lens[s] = f + n
    c.k8, c.v8 = k_exp.view(F8), v_exp.view(F8)
    assert torch.equal(k_got, c._phys(c.k8).view(torch.uint8).cpu()) and torch.equal(v_got, c._phys(c.v8).view(torch.uint8).cpu())
    check_outputs(c, out, lse, name, plan)
    # the stand-alone writer followed by the plain read: the same bytes, bit-identical out
    c.lens = old
    kc2, vc2 = c._phys(c.k8), c._phys(c.v8)  # (already holds the new rows: the writer overwrites them with the same bytes)
    fill = _fa3().kvcache_append_fp8(kc2, vc2, args["k"], args["v"], args["cache_seqlens"], args["k_descale"], args["v_descale"],
                                     cu_seqlens_k_new=args.get("cu_seqlens_k_new"), page_table=args.get("page_table"))
    assert torch.equal(kc2.view(torch.uint8), kc.view(torch.uint8)) and torch.equal(vc2.view(torch.uint8), vc.view(torch.uint8))
    read = {k: v for k, v in args.items() if k not in ("k", "v", "cu_seqlens_k_new", "cache_seqlens")}
    out2, lse2, *_ = _fa3().flash_attn_with_kvcache(c.q.to(DEV), kc2, vc2, cache_seqlens=fill, **read)
    assert torch.equal(out2.cpu(), out) and torch.equal(lse2.cpu(), lse)


def check_outputs(c, out, lse, name, plan):
    ref, ref_lse, pt = c.reference()
    o, l = c.select(out, lse)
    err = (o.float() - ref.float()).abs().max().item()
    bound = 3 * (pt.float() - ref.float()).abs().max().item() + 1e-5
    print(f"kv8 append {name}: |out - ref| = {err:.3e}  bound = {bound:.3e}  plan = {plan}")
    assert err <= bound
    finite = torch.isfinite(ref_lse)
    assert torch.equal(torch.isfinite(l), finite)
    assert torch.allclose(l[finite], ref_lse[finite], atol=1e-3, rtol=0)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_decode_step(dtype):
    """b 2, one new row, GQA 8 / 2, d 128: the row is quantised into the cache and attended to in the same call."""
    c = Case(dtype=dtype, b=2, h=8, hk=2, d=128, cap=320, lens=(1, 257), seed=61)
    torch.manual_seed(62)
    check_step(c, torch.randn(2, 1, 2, 128).to(dtype), torch.randn(2, 1, 2, 128).to(dtype), None, f"decode {dtype}")


def test_causal_chunk_over_pages():
    """5 new rows over a page-16 cache, fill levels 14 and 30: both chunks cross a page boundary; causal, 5 query rows."""
    c = Case(b=2, sq=5, h=4, hk=2, d=64, cap=64, lens=(14, 30), page=16, causal=True, seed=63)
    torch.manual_seed(64)
    check_step(c, torch.randn(2, 5, 2, 64).bfloat16(), torch.randn(2, 5, 2, 64).bfloat16(), None, "causal chunk page 16")


def test_ragged_mixed_step():
    """cu_seqlens_q + cu_seqlens_k_new with lengths (1, 4, 1): two decode rows around a prefill chunk, causal."""
    c = Case(b=3, sq=4, h=8, hk=2, d=128, cap=128, lens=(70, 0, 16), cu_q=(0, 1, 5, 6), causal=True, seed=65)
    torch.manual_seed(66)
    check_step(c, torch.randn(6, 2, 128).bfloat16(), torch.randn(6, 2, 128).bfloat16(), [1, 4, 1], "ragged mixed step")


def rotate_cpu(x, cos, sin, interleaved):
    """x: (h, d) of a 16-bit type at one position; cos / sin: (rd / 2,).  fp32 arithmetic, rounded to x's dtype."""
    rd = 2 * cos.numel()
    xf, c, s = x.float(), cos.float(), sin.float()
    y = xf.clone()
    if interleaved:
        x1, x2 = xf[:, 0:rd:2], xf[:, 1:rd:2]
        y[:, 0:rd:2], y[:, 1:rd:2] = x1 * c - x2 * s, x2 * c + x1 * s
    else:
        x1, x2 = xf[:, : rd // 2], xf[:, rd // 2: rd]
        y[:, : rd // 2], y[:, rd // 2: rd] = x1 * c - x2 * s, x2 * c + x1 * s
    return y.to(x.dtype)


def test_decode_step_with_rotary_and_a_window():
    """One new row per sequence, rotary over 32 of 64 columns (halves), a left window of 40 keys.  The expected cache is the
    GPU's 16-bit append quantised on the CPU (case 3's rule for the rotated columns); q is rotated on the CPU."""
    dtype, b, hk, d, cap, rd = torch.float16, 2, 2, 64, 128, 32
    c = Case(dtype=dtype, b=b, h=4, hk=hk, d=d, cap=cap, lens=(9, 100), window=(40, 0), seed=67)
    torch.manual_seed(68)
    k_new, v_new = torch.randn(b, 1, hk, d).to(dtype), torch.randn(b, 1, hk, d).to(dtype)
    cos, sin = rotary_tables(cap, rd, dtype, 69)
    fills = c.lens.tolist()
    k_prefill, v_prefill = c.k8.view(torch.uint8).clone(), c.v8.view(torch.uint8).clone()
    out, lse, k_got, v_got, (_, _, _, plan) = run_step(c, k_new, v_new, rotary=(cos, sin, False))
    k16, v16 = append_16bit(k_new, v_new, fills, cap, cos, sin, False, None, None)
    check_against_16bit_append(k_got, v_got, k16, v16, c.kdesc, c.vdesc, fills, [1] * b, rd, k_prefill, v_prefill, "end to end")
    for s, f in enumerate(fills):
        k_prefill[s, f] = quantise(k16[s, f], c.kdesc[s])
        v_prefill[s, f] = quantise(v16[s, f], c.vdesc[s])
        c.q[s, 0] = rotate_cpu(c.q[s, 0], cos[f], sin[f], False)  # (a window: row i at the old fill level + i)
    c.k8, c.v8, c.lens = k_prefill.view(F8), v_prefill.view(F8), c.lens + 1
    check_outputs(c, out, lse, "decode rotary window", plan)


def test_new_rows_need_both_descales_and_the_query_dtype():
    fa3 = _fa3()
    q = torch.randn(2, 1, 4, 64, dtype=torch.bfloat16, device=DEV)
    kc = torch.zeros(2, 64, 2, 64, device=DEV).to(F8)
    lens = torch.tensor([5, 9], dtype=torch.int32, device=DEV)
    new = torch.randn(2, 1, 2, 64, dtype=torch.bfloat16, device=DEV)
    one = torch.ones(2, 2, device=DEV)
    with pytest.raises(RuntimeError, match="does not support k_new / v_new with an fp8 KV cache"):
        fa3.flash_attn_with_kvcache(q, kc, kc, k=new, v=new, cache_seqlens=lens, k_descale=one)
    with pytest.raises(RuntimeError, match="does not support fp8 k_new / v_new with an fp8 KV cache"):
        fa3.flash_attn_with_kvcache(q, kc, kc, k=new.to(F8), v=new.to(F8), cache_seqlens=lens, k_descale=one, v_descale=one)
    with pytest.raises(RuntimeError, match="must have the same dtype as query"):
        fa3.flash_attn_with_kvcache(q, kc, kc, k=new.half(), v=new.half(), cache_seqlens=lens, k_descale=one, v_descale=one)
    assert torch.all(kc.view(torch.uint8) == 0)  # nothing was written by the refused calls


# ---- 5. graph capture ----------------------------------------------------------------------------------------------------------
def test_decode_step_in_a_hip_graph():
    """One capture of append + attention on a single stream, two replays with k_new / v_new and cache_seqlens changed in
    place between them: cache bytes and out equal the eager calls' (no host sync, nothing baked into the capture)."""
    c = Case(b=2, h=8, hk=2, d=128, cap=64, lens=(5, 9), seed=71)
    fa3 = _fa3()
    torch.manual_seed(72)
    steps = [(torch.randn(2, 1, 2, 128).bfloat16(), torch.randn(2, 1, 2, 128).bfloat16(), torch.tensor([5, 9], dtype=torch.int32)),
             (torch.randn(2, 1, 2, 128).bfloat16(), torch.randn(2, 1, 2, 128).bfloat16(), torch.tensor([6, 40], dtype=torch.int32))]
    q, kd, vd = c.q.to(DEV), c.kdesc.to(DEV), c.vdesc.to(DEV)

    def call(kc, vc, k_new, v_new, lens):
        return fa3.flash_attn_with_kvcache(q, kc, vc, k=k_new, v=v_new, cache_seqlens=lens, k_descale=kd, v_descale=vd, num_splits=1)

    kc_e, vc_e = c._phys(c.k8), c._phys(c.v8)
    eager = [call(kc_e, vc_e, k.to(DEV), v.to(DEV), n.to(DEV)).cpu() for k, v, n in steps]
    kc_g, vc_g = c._phys(c.k8), c._phys(c.v8)
    k_new, v_new, lens = (t.to(DEV) for t in steps[0])
    call(kc_g, vc_g, k_new, v_new, lens)  # warm-up outside the capture (writes what the first replay writes again)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = call(kc_g, vc_g, k_new, v_new, lens)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), eager[0])
    k_new.copy_(steps[1][0]); v_new.copy_(steps[1][1]); lens.copy_(steps[1][2])
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), eager[1])
    assert torch.equal(kc_g.view(torch.uint8), kc_e.view(torch.uint8)) and torch.equal(vc_g.view(torch.uint8), vc_e.view(torch.uint8))
    assert not torch.equal(kc_g.view(torch.uint8).cpu(), c.k8.view(torch.uint8))  # (rows were written)
