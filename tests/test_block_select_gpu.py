"""GPU tests of the block summaries and the Quest block selection (csrc/fa_block_select.hip through
hopper_interface.kvcache_block_summary_update / kvcache_select_blocks) against the torch oracles block_summary_ref /
select_blocks_ref run on the CPU.

Summaries: minimum and maximum are exact, so equality.  Selection on multiples of 1/4 in [-4, 4]: every product is a multiple of
1/16 of magnitude <= 16 and a sum of 128 * 12 of them stays below 2^15, exact in fp32, so cnt, idx and scores equal the oracle's,
ties included.  Selection on normal data: an fp32 sum of d terms, in any order, errs by at most (d - 1) 2^-24 times the sum of the
terms' magnitudes, A (first order; the oracle returns A per row).  Every case asserts the form it ran in through the plan name
(tests/block_select_plan_universe.py)."""
import pytest
import torch

import block_select_plan_universe as U
import sparse_kv_oracle
from oracle import attention_ref as oracle

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, FP, F8 = torch.bfloat16, torch.float16, torch.float8_e4m3fn
EPS = 2.0 ** -24
SENTINEL = 77.0


def _fa3():
    from flash_attention_annotated_amd import hopper_interface
    return hopper_interface


def _binding():
    from flash_attention_annotated_amd import _lib
    return _lib.binding()


def _i32(values):
    return torch.tensor(values, dtype=torch.int32)


def _dev(t):
    return None if t is None else t.to(DEV)


def _store(logical, form, spare=2, seed=0):
    """The cache a kernel sees for the logical rows (b, cap, h_k, d): dense with a permuted cache_batch_idx (form "dense"), or pages
    of int(form[1:]) rows behind a shuffled page table.  Returns (store, cache_batch_idx, page_table, slots of the summary)."""
    b, cap = logical.shape[:2]
    g = torch.Generator().manual_seed(seed)
    raw = logical.view(torch.uint8) if logical.dtype == F8 else logical
    if form == "dense":
        batch_idx = torch.randperm(b + spare, generator=g)[:b].to(torch.int32)
        store = torch.zeros((b + spare, *raw.shape[1:]), dtype=raw.dtype)
        store[batch_idx.long()] = raw
        return store.view(logical.dtype), batch_idx, None, b + spare
    page = int(form[1:])
    per = cap // page
    table = torch.randperm(b * per + spare, generator=g)[:b * per].to(torch.int32).view(b, per)
    store = torch.zeros((b * per + spare, page, *raw.shape[2:]), dtype=raw.dtype)
    store[table.flatten().long()] = raw.reshape(b * per, page, *raw.shape[2:])
    return store.view(logical.dtype), None, table, b


def _random_cache(b, cap, h_k, d, cache, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(b, cap, h_k, d, generator=g) * 3
    return x.to({"bf16": BF, "fp16": FP, "e4m3": F8}[cache])


# ---- summaries --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["dense", "p16", "p64", "p256"])
@pytest.mark.parametrize("cache", ["bf16", "fp16", "e4m3"])
def test_summary_equals_the_oracle(cache, form):
    """Every combination of cache type, cache form, B, d and h_k, at the fill levels 0, 1, B - 1, B, B + 1 and the capacity in one
    call: a rebuild into a sentinel pattern equals the oracle's, sentinel included."""
    H = _fa3()
    cases = [c for c in U.SUMMARY_CASES if c.cache == cache and c.form == form]
    assert len(cases) == 8
    for n, c in enumerate(cases):
        fills = _i32(U.fills_of(c.block))
        logical = _random_cache(len(fills), U.CAPACITY, c.h_k, c.d, cache, seed=n)
        store, batch_idx, table, slots = _store(logical, form, seed=n)
        sdt = logical.dtype if cache != "e4m3" else (BF if c.d == 128 else FP)
        max_blocks = U.CAPACITY // c.block + (1 if c.h_k == 2 else 0)  # (a summary longer than the capacity needs)
        want = torch.full((slots, max_blocks, 2, c.h_k, c.d), SENTINEL, dtype=sdt)
        H.block_summary_ref(want, store, None, fills, kv_block_size=c.block, cache_batch_idx=batch_idx, page_table=table)
        got = torch.full_like(want, SENTINEL).to(DEV)
        args = (got, store.to(DEV), None, fills.to(DEV))
        kw = dict(kv_block_size=c.block, cache_batch_idx=_dev(batch_idx), page_table=_dev(table))
        assert H.kvcache_block_summary_update(*args, **kw) is got
        plan = _binding().kvcache_block_summary_update_plan(*args, max_seqlen_new=None, **kw)
        assert plan == U.update_plan(len(fills), c.h_k, c.d, max_blocks, c.block, U.CAPACITY, cache == "e4m3", form != "dense"), plan
        assert torch.equal(got.cpu(), want), (c, (got.cpu().float() - want.float()).abs().max())
        assert (want == SENTINEL).any() and not (want == SENTINEL).all()


@pytest.mark.parametrize("cache,form", [("bf16", "p64"), ("e4m3", "p16"), ("fp16", "dense"), ("e4m3", "dense")])
def test_summary_incremental_equals_rebuild(cache, form):
    """A prefill of 200 rows, then appends of 1, 1, 70 and 1 rows (the third entry: twice as many, so that a step crosses two block
    boundaries): after every step k_summary equals a rebuild from scratch, and the blocks outside the step's range are bit for bit
    what they were."""
    H = _fa3()
    b, cap, h_k, d, B = 3, 512, 2, 128, 128
    logical = _random_cache(b, cap, h_k, d, cache, seed=9)
    store, batch_idx, table, slots = _store(logical, form, seed=9)
    kw_cpu = dict(kv_block_size=B, cache_batch_idx=batch_idx, page_table=table)
    kw = dict(kv_block_size=B, cache_batch_idx=_dev(batch_idx), page_table=_dev(table))
    store_d = store.to(DEV)
    s = torch.full((slots, cap // B, 2, h_k, d), SENTINEL, dtype=FP if cache == "fp16" else BF, device=DEV)
    fills = _i32([200, 200, 120])
    H.kvcache_block_summary_update(s, store_d, None, fills.to(DEV), max_seqlen_new=200, **kw)
    for step in (0, 1, 1, 70, 1):
        new = fills + _i32([step, step, 2 * step])
        before = s.cpu()
        H.kvcache_block_summary_update(s, store_d, fills.to(DEV), new.to(DEV), max_seqlen_new=2 * step, **kw)
        want = H.block_summary_ref(torch.full_like(before, SENTINEL), store, None, new, **kw_cpu)
        after = s.cpu()
        assert torch.equal(after, want), (step, fills.tolist())
        for i in range(b):
            slot = i if batch_idx is None else int(batch_idx[i])
            lo, hi = int(fills[i]) // B, -(-int(new[i]) // B) if new[i] > fills[i] else 0
            keep = [j for j in range(cap // B) if not lo <= j < hi]
            assert torch.equal(after[slot, keep].view(torch.int16), before[slot, keep].view(torch.int16))
        assert (after == SENTINEL).any()
        fills = new
    assert fills.tolist() == [273, 273, 266]


# ---- selection, exact -------------------------------------------------------------------------------------------------------
def _quarter_inputs(b, s_q, h, h_k, d, max_blocks, seed, distinct=6):
    """q and a valid summary of multiples of 1/4 in [-4, 4]; the blocks of a (slot, head) are copies of `distinct` summaries, so
    that equal scores -- ties at the cut -- are the rule."""
    g = torch.Generator().manual_seed(seed)
    q = (torch.randint(-16, 17, (b, s_q, h, d), generator=g).float() / 4).to(BF)
    a = torch.randint(-16, 17, (b, distinct, 2, h_k, d), generator=g).float() / 4
    proto = torch.stack((a.amin(2), a.amax(2)), 2)
    which = torch.randint(0, distinct, (b, max_blocks), generator=g)
    s = torch.stack([proto[i, which[i]] for i in range(b)]).to(BF)
    return q, s


def _tie_at_the_cut(r, fills, block, sink, local):
    """whether some (b, hk) of the oracle's result r leaves out an unforced block whose score equals a chosen unforced one's"""
    for i in range(r.cnt.shape[0]):
        n = -(-min(int(fills[i]), r.scores.shape[2] * block) // block)
        free = [j for j in range(n) if not (j < sink or j >= n - local)]
        for hk in range(r.cnt.shape[1]):
            chosen = set(r.idx[i, hk, :int(r.cnt[i, hk])].tolist())
            inside = [float(r.scores[i, hk, j]) for j in free if j in chosen]
            outside = [float(r.scores[i, hk, j]) for j in free if j not in chosen]
            if inside and outside and min(inside) == max(outside):
                return True
    return False


def _run_select(q, s, fills, c, width=None, batch_idx=None):
    H = _fa3()
    kw = dict(kv_block_size=c.block, sink_blocks=c.sink, local_blocks=c.local, group_reduce=c.reduce)
    qd, sd, fd, bd = q.to(DEV), s.to(DEV), fills.to(DEV), _dev(batch_idx)
    b, h_k, mb = q.shape[0], s.shape[3], s.shape[1]
    width = c.num_blocks if width is None else width
    cnt = torch.full((b, h_k), -7, dtype=torch.int32, device=DEV)
    idx = torch.full((b, h_k, width), -7, dtype=torch.int32, device=DEV)
    out = H.kvcache_select_blocks(qd, sd, fd, c.num_blocks, cache_batch_idx=bd, kv_block_cnt=cnt, kv_block_idx=idx, return_scores=True, **kw)
    assert out[0] is cnt and out[1] is idx
    plan = _binding().kvcache_select_blocks_plan(qd, sd, fd, c.num_blocks, c.block, c.sink, c.local, c.reduce, bd, cnt, idx, out[2])
    assert plan == U.select_plan(b, h_k, c.d, mb, c.reduce), plan
    ref = H.select_blocks_ref(q, s, fills, c.num_blocks, cache_batch_idx=batch_idx, width=width, **kw)
    PLANS.append(plan)
    return cnt.cpu(), idx.cpu(), out[2].cpu(), ref


PLANS = []  # of the calls of _run_select, in order


@pytest.mark.parametrize("reduce", ["max", "sum"])
@pytest.mark.parametrize("s_q", [1, 3])
@pytest.mark.parametrize("g", [1, 4])
@pytest.mark.parametrize("d", [64, 128])
def test_select_exact(d, g, s_q, reduce):
    """B, num_blocks and (sink, local) of the grid inside: n(b) = 0, 1, 3, 37 and max_blocks over a batch of 5, two kv heads, the
    summary slots behind a permuted cache_batch_idx.  cnt, idx and scores equal the oracle's."""
    cases = [c for c in U.SELECT_CASES if (c.d, c.g, c.s_q, c.reduce) == (d, g, s_q, reduce)]
    assert len(cases) == 18
    h_k = 2
    q, s = _quarter_inputs(5, s_q, g * h_k, h_k, d, U.SMALL_MAX_BLOCKS, seed=d + g + s_q)
    batch_idx = _i32([3, 0, 4, 1, 2])
    ties = []
    for c in cases:
        fills = _i32([max(n * c.block - c.block // 2, 0) for n in U.RAGGED_N])
        fills[-1] = U.SMALL_MAX_BLOCKS * c.block + 5  # (past the capacity: clamped)
        if c.num_blocks < c.sink + c.local:
            with pytest.raises(RuntimeError, match="num_blocks must be at least sink_blocks"):
                _fa3().kvcache_select_blocks(q.to(DEV), s.to(DEV), fills.to(DEV), c.num_blocks, kv_block_size=c.block, sink_blocks=c.sink,
                                             local_blocks=c.local, group_reduce=c.reduce)
            continue
        cnt, idx, scores, ref = _run_select(q, s, fills, c, width=c.num_blocks + 3, batch_idx=batch_idx)
        assert torch.equal(cnt, ref.cnt) and torch.equal(idx, ref.idx), c
        assert torch.equal(scores.double(), ref.scores), c
        assert cnt[:, 0].tolist() == [min(n, c.num_blocks) for n in U.RAGGED_N]
        if c.num_blocks >= U.SMALL_MAX_BLOCKS:  # at least n: the list is 0 .. n - 1
            for i, n in enumerate(U.RAGGED_N):
                assert idx[i, 1, :n].tolist() == list(range(n)) and torch.all(idx[i, 1, n:] == -1)
        ties.append(_tie_at_the_cut(ref, fills, c.block, c.sink, c.local))
    assert sum(ties) >= 3, "ties at the cut are the rule here by construction"


@pytest.mark.parametrize("c", U.LARGE_CASES, ids=lambda c: f"d{c.d}-{c.reduce}-k{c.num_blocks}")
def test_select_exact_4096_blocks(c):
    """b = 1, h_k = 1, 4096 blocks: the scoring is spread over 64 (d 128) or 32 (d 64) workgroups, the selection has 1024 threads"""
    q, s = _quarter_inputs(1, c.s_q, c.g, 1, c.d, c.max_blocks, seed=c.d + c.num_blocks, distinct=300)
    ties = []
    for fill in (4096 * c.block, 4000 * c.block - 3, 1030 * c.block):
        fills = _i32([fill])
        cnt, idx, scores, ref = _run_select(q, s, fills, c)
        assert f" split={64 if c.d == 128 else 32} " in PLANS[-1] and PLANS[-1].endswith("threads=1024")
        assert torch.equal(cnt, ref.cnt) and torch.equal(idx, ref.idx) and torch.equal(scores.double(), ref.scores), (c, fill)
        assert int(cnt) == min(c.num_blocks, -(-fill // c.block))
        ties.append(_tie_at_the_cut(ref, fills, c.block, c.sink, c.local))
    assert c.num_blocks == 4096 or any(ties), "no tie at the cut"


# ---- selection, normal data -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reduce", ["max", "sum"])
@pytest.mark.parametrize("d,dtype,max_blocks", [(128, BF, 300), (64, FP, 2000), (80, BF, 77)])
def test_select_normal_data(d, dtype, max_blocks, reduce):
    """Scores within the derived bound of the fp64 oracle, and a chosen set that is valid under the fp64 scores with that slack.
    max: fp32 U of some row r, which is within e_r = (d - 1) 2^-24 A_r of the fp64 U_r: the score lies within e_r of some row's U_r
    and, as the maximum of values each within e_r of U_r, within max_r e_r of the fp64 maximum.  sum: the rows' errors add, and
    the fp32 sum of the R = s_q g values adds (R - 1) 2^-24 sum_r |U_r| <= (R - 1) 2^-24 sum_r A_r.
    The set: with e the largest slack of a block of the (b, hk) and c the fp64 score at the cut (the K'-th largest of the unforced
    blocks, K' = K - |forced|), a chosen unforced block below c - 2 e would have displaced an unchosen one at or above c, whose
    fp32 score is larger by more than 0; likewise an unchosen one above c + 2 e."""
    torch.manual_seed(d + max_blocks)
    b, s_q, h, h_k, B, K, sink, local = 3, 2, 8, 2, 128, 24, 1, 2
    R = s_q * h // h_k
    q = torch.randn(b, s_q, h, d).to(dtype)
    a = torch.randn(b, max_blocks, 2, h_k, d)
    s = torch.stack((a.amin(2) - 0.5, a.amax(2) + 0.5), 2).to(dtype)
    fills = _i32([max_blocks * B, max_blocks * B // 2 + 17, 30 * B - 1])
    c = U.SelectCase(d, h // h_k, s_q, reduce, B, K, sink, local, max_blocks)
    cnt, idx, scores, ref = _run_select(q, s, fills, c)
    assert torch.equal(cnt, ref.cnt)
    for i in range(b):
        n = -(-int(fills[i]) // B)
        assert torch.all(scores[i, :, n:] == float("-inf"))
        forced = [j for j in range(n) if j < sink or j >= n - local]
        for hk in range(h_k):
            u32, U64, A = scores[i, hk, :n].double(), ref.U[i, hk, :, :n], ref.A[i, hk, :, :n]
            e_rows = (d - 1) * EPS * A
            if reduce == "max":
                assert torch.all(((u32[None] - U64).abs() <= e_rows).any(0)), "a score within the bound of no row"
                e = e_rows.amax(0)
            else:
                e = e_rows.sum(0) + (R - 1) * EPS * A.sum(0)
            u64 = ref.scores[i, hk, :n]
            print(f"select {reduce} d{d} ({i}, {hk}): worst |u32 - u64| / e = {((u32 - u64).abs() / e).max():.3f}")
            assert torch.all((u32 - u64).abs() <= e)
            k = int(cnt[i, hk])
            got = idx[i, hk, :k].tolist()
            assert got == sorted(set(got)) and all(0 <= j < n for j in got) and torch.all(idx[i, hk, k:] == -1)
            assert set(forced) <= set(got) and k == min(K, n)
            free = [j for j in range(n) if j not in forced]
            places = k - len(forced)
            if 0 < places < len(free):
                cut = torch.sort(u64[free], descending=True).values[places - 1]
                slack = 2 * e.amax()
                assert all(u64[j] >= cut - slack for j in got if j not in forced)
                assert all(u64[j] <= cut + slack for j in free if j not in got)


def test_select_nan_stays_inside():
    """NaN in q and in the summaries: the choice is unspecified, every index written is in [0, n) or -1, the count is K"""
    q, s = _quarter_inputs(2, 1, 4, 2, 64, 50, seed=1)
    q[0, 0, 1, 5] = float("nan")
    s[1, 7:19, 0, 1, 3] = float("nan")
    fills = _i32([50 * 128, 33 * 128 - 9])
    c = U.SelectCase(64, 2, 1, "max", 128, 9, 1, 1, 50)
    qd, sd = q.to(DEV), s.to(DEV)
    cnt, idx = _fa3().kvcache_select_blocks(qd, sd, fills.to(DEV), c.num_blocks)
    for i, n in enumerate((50, 33)):
        for hk in range(2):
            got = idx[i, hk].tolist()
            assert int(cnt[i, hk]) == 9 and got == sorted(set(got)) and 0 <= got[0] and got[-1] < n and got[0] == 0 and got[-1] == n - 1


# ---- end to end -------------------------------------------------------------------------------------------------------------
class Step:
    """hq8 / hkv2, d128, pages of 64, B = 128, a batch of 3 with fill levels in 130 .. 700, capacity 768 (6 blocks): the rows up to
    the fill level but the last lie in the cache; the last is appended by the project's append."""
    b, h, h_k, d, page, B, cap = 3, 8, 2, 128, 64, 128, 768

    def __init__(self, fp8, fills=(130, 384, 699), seed=0):
        g = torch.Generator().manual_seed(seed)
        self.fp8, self.H = fp8, _fa3()
        per = self.cap // self.page
        self.table = torch.randperm(self.b * per + 3, generator=g)[:self.b * per].to(torch.int32).view(self.b, per).to(DEV)
        self.fills = _i32(fills).to(DEV)
        self.rows_k = torch.randn(self.b, self.cap, self.h_k, self.d, generator=g).to(BF)  # what is appended, row by row
        self.rows_v = torch.randn(self.b, self.cap, self.h_k, self.d, generator=g).to(BF)
        self.q = torch.randn(self.b, 1, self.h, self.d, generator=g).to(BF).to(DEV)
        self.kdesc = torch.tensor([[0.5, 1.0], [2.0, 0.25], [1.0, 4.0]], device=DEV) if fp8 else None
        self.vdesc = torch.tensor([[1.0, 0.5], [0.25, 2.0], [4.0, 1.0]], device=DEV) if fp8 else None
        self.level = (self.fills - 1).clone()
        self.kc, self.vc = self._prefill(self.rows_k, self.kdesc), self._prefill(self.rows_v, self.vdesc)
        self.summary = torch.full((self.b, self.cap // self.B, 2, self.h_k, self.d), SENTINEL, dtype=BF, device=DEV)

    def _prefill(self, rows, desc):
        """the pool with the rows below `level` of every entry in place (an e4m3 pool: quantised by torch), zeros elsewhere"""
        filled = torch.arange(self.cap)[None, :, None, None] < self.level.cpu()[:, None, None, None]
        x = torch.where(filled, rows.float(), torch.zeros(()))
        if self.fp8:
            x = (x / desc.cpu()[:, None, :, None]).to(F8).view(torch.uint8)
        else:
            x = x.to(BF)
        pool = torch.zeros((int(self.table.max()) + 4, self.page, self.h_k, self.d), dtype=x.dtype)
        pool[self.table.flatten().long().cpu()] = x.reshape(-1, self.page, self.h_k, self.d)
        return (pool.view(F8) if self.fp8 else pool).to(DEV)

    def _append(self, k, v, level):
        if self.fp8:
            self.H.kvcache_append_fp8(self.kc, self.vc, k, v, level, self.kdesc, self.vdesc, page_table=self.table)
        else:
            q = torch.zeros((self.b, 1, self.h, self.d), dtype=BF, device=DEV)
            self.H.flash_attn_with_kvcache(q, self.kc, self.vc, k=k, v=v, cache_seqlens=level, page_table=self.table)

    def append_one(self):
        """the step's append: row level[i] of every entry; returns (old, new) fill levels"""
        old = self.level.clone()
        at = old.long().cpu()
        k = torch.stack([self.rows_k[i, at[i]] for i in range(self.b)])[:, None].to(DEV)
        v = torch.stack([self.rows_v[i, at[i]] for i in range(self.b)])[:, None].to(DEV)
        self._append(k, v, old)
        self.level = old + 1
        return old, self.level

    def logical(self):
        """(k, v) fp32 (b, cap, h_k, d): the cache as attention reads it, dequantised exactly"""
        out = []
        for pool, desc in ((self.kc, self.kdesc), (self.vc, self.vdesc)):
            raw = pool.view(torch.uint8) if self.fp8 else pool
            rows = raw[self.table.flatten().long()].view(pool.dtype).float().reshape(self.b, self.cap, self.h_k, self.d).cpu()
            out.append(rows * desc.cpu()[:, None, :, None] if self.fp8 else rows)
        return out

    def sparse(self, cnt, idx, fills):
        return self.H.flash_attn_with_kvcache_sparse(self.q, self.kc, self.vc, cnt, idx, kv_block_size=self.B, cache_seqlens=fills,
                                                     page_table=self.table, k_descale=self.kdesc, v_descale=self.vdesc,
                                                     return_softmax_lse=True)

    def check(self, out, lse, cnt, idx, fills, name):
        """the bound of tests/test_sparse_kv_gpu.py: |out - ref| <= 3 |pt - ref| + 1e-5, LSE within 1e-3, on the kernel's own lists"""
        k, v = self.logical()
        out, lse, cnt, idx, q = out.cpu(), lse.cpu(), cnt.cpu(), idx.cpu(), self.q.cpu()
        for i in range(self.b):
            ref, l_ref, vis = sparse_kv_oracle.sparse_kv_ref(q[i], k[i], v[i], int(fills[i]), cnt[i], idx[i], self.B)
            bias = torch.where(vis > 0, 0.0, float("-inf")).to(BF)[None]
            pt = oracle.attention_ref(q[i][None], k[i][None].to(BF), v[i][None].to(BF), attn_bias=bias, upcast=False, reorder_ops=True)[0][0]
            bound = 3 * (pt.float() - ref).abs().max().item() + 1e-5
            err = (out[i].float() - ref).abs().max().item()
            print(f"block_select {name} batch {i}: |out - ref| = {err:.3e}  bound = {bound:.3e}")
            assert err <= bound, (name, i, err, bound)
            assert torch.allclose(lse[i], l_ref, atol=1e-3, rtol=0), (name, i)


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "e4m3"])
def test_end_to_end_step(fp8):
    st = Step(fp8)
    H = st.H
    old, new = st.append_one()
    assert new.tolist() == [130, 384, 699]
    H.kvcache_block_summary_update(st.summary, st.kc, None, new, kv_block_size=st.B, page_table=st.table)
    k_log = st.logical()[0]
    raw = (k_log / st.kdesc.cpu()[:, None, :, None]) if fp8 else k_log  # the stored values, without the descale
    want = H.block_summary_ref(torch.full_like(st.summary.cpu(), SENTINEL), raw.to(BF), None, new.cpu(), kv_block_size=st.B)
    assert torch.equal(st.summary.cpu(), want)
    cnt, idx = H.kvcache_select_blocks(st.q, st.summary, new, 3, kv_block_size=st.B)
    assert cnt[:, 0].tolist() == [2, 3, 3] and idx.shape == (3, 2, 3)
    ref = H.select_blocks_ref(st.q.cpu(), want, new.cpu(), 3, kv_block_size=st.B)
    assert torch.equal(idx.cpu()[:, :, 0], ref.idx[:, :, 0]) and torch.all(idx[2, :, 0] == 0) and torch.all(idx[2, :, 2] == 5)
    out, lse = st.sparse(cnt, idx, new)
    st.check(out, lse, cnt, idx, new.cpu(), f"{'e4m3' if fp8 else 'bf16'} 3 blocks")
    # at least n blocks: every block is listed, in order, and the output is bit for bit that of hand-made arange lists
    cnt_all, idx_all = H.kvcache_select_blocks(st.q, st.summary, new, 6, kv_block_size=st.B, sink_blocks=0, local_blocks=0, group_reduce="sum")
    hand_cnt = torch.tensor([[2, 2], [3, 3], [6, 6]], dtype=torch.int32, device=DEV)
    hand_idx = torch.arange(6, dtype=torch.int32, device=DEV).expand(3, 2, 6).contiguous()
    assert torch.equal(cnt_all, hand_cnt)
    for i, n in enumerate((2, 3, 6)):
        assert torch.equal(idx_all[i, :, :n], hand_idx[i, :, :n]) and torch.all(idx_all[i, :, n:] == -1)
    out_all, lse_all = st.sparse(cnt_all, idx_all, new)
    out_hand, lse_hand = st.sparse(hand_cnt, hand_idx, new)
    assert torch.equal(out_all, out_hand) and torch.equal(lse_all, lse_hand)


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "e4m3"])
def test_graph_replay_after_an_append(fp8):
    """The three calls after the append, captured with the output buffers given; one more row is appended, by which entry 1 enters
    block 3; the replay equals the eager calls on the new fill levels."""
    st = Step(fp8, seed=1)
    H = st.H
    old, new = st.append_one()
    H.kvcache_block_summary_update(st.summary, st.kc, None, new, kv_block_size=st.B, page_table=st.table)
    old_buf, new_buf = old.clone(), new.clone()
    cnt = torch.zeros(3, 2, dtype=torch.int32, device=DEV)
    idx = torch.zeros(3, 2, 3, dtype=torch.int32, device=DEV)

    def step(summary, cnt, idx):
        H.kvcache_block_summary_update(summary, st.kc, old_buf, new_buf, kv_block_size=st.B, max_seqlen_new=1, page_table=st.table)
        H.kvcache_select_blocks(st.q, summary, new_buf, 3, kv_block_size=st.B, kv_block_cnt=cnt, kv_block_idx=idx)
        return st.sparse(cnt, idx, new_buf)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(st.summary.clone(), cnt.clone(), idx.clone())  # (warm-up outside the capture: allocator and lazy initialisation)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, lse = step(st.summary, cnt, idx)
    old2, new2 = st.append_one()
    assert new2.tolist() == [131, 385, 700]
    old_buf.copy_(old2), new_buf.copy_(new2)
    eager_summary = st.summary.clone()
    graph.replay()
    torch.cuda.synchronize()
    e_cnt, e_idx = torch.zeros_like(cnt), torch.zeros_like(idx)
    e_out, e_lse = step(eager_summary, e_cnt, e_idx)
    assert torch.equal(st.summary, eager_summary) and not torch.all(st.summary[1, 3] == SENTINEL)
    assert torch.equal(cnt, e_cnt) and torch.equal(idx, e_idx) and cnt[:, 0].tolist() == [2, 3, 3]
    assert torch.equal(out, e_out) and torch.equal(lse, e_lse)
    st.check(out, lse, cnt, idx, new2.cpu(), f"graph replay {'e4m3' if fp8 else 'bf16'}")


def test_torch_compile_fullgraph():
    H = _fa3()
    q, s = _quarter_inputs(2, 1, 8, 2, 128, 12, seed=3)
    logical = _random_cache(2, 512, 2, 128, "bf16", seed=3)
    fills = _i32([512, 300]).to(DEV)

    def update(summary, cache, fills):
        H.kvcache_block_summary_update(summary, cache, None, fills, kv_block_size=128)
        return summary + 0

    def select(q, summary, fills):
        return H.kvcache_select_blocks(q, summary, fills, 3, return_scores=True)

    summary = torch.full((2, 4, 2, 2, 128), SENTINEL, dtype=BF, device=DEV)
    got = torch.compile(update, backend="aot_eager", fullgraph=True)(summary, logical.to(DEV), fills)
    want = H.block_summary_ref(torch.full((2, 4, 2, 2, 128), SENTINEL, dtype=BF), logical, None, fills.cpu())
    assert torch.equal(got.cpu(), want) and torch.equal(summary.cpu(), want)
    fills = _i32([12 * 128, 700]).to(DEV)
    cnt, idx, scores = torch.compile(select, backend="aot_eager", fullgraph=True)(q.to(DEV), s.to(DEV), fills)
    ref = H.select_blocks_ref(q, s, fills.cpu(), 3)
    assert torch.equal(cnt.cpu(), ref.cnt) and torch.equal(idx.cpu(), ref.idx) and torch.equal(scores.cpu().double(), ref.scores)
