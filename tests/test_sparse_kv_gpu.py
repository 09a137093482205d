"""GPU tests of block-sparse attention over a KV cache: hopper_interface.flash_attn_with_kvcache_sparse /
torch.ops.flash_attn_3.fwd_kvcache_sparse, i.e. fa_fwd_sparse_kv and sp_fwd_kernel (csrc/fa_fwd_kernel_sp.h).

Reference: tests/sparse_kv_oracle.py (fp64 softmax over the explicit visibility of the definition), for an fp8 cache on the
cache dequantised on the CPU (e4m3 values taken exactly to fp32, times the power-of-two descale of their (batch, kv head)).
Bounds, the project's own and unchanged: |out - ref| <= 3 |pt - ref| + 1e-5 (tests/test_fa3_kvcache_gpu.py for 16-bit caches,
tests/test_kv8_kvcache_gpu.py for fp8 caches), `pt` being the project's dense oracle in q's dtype (upcast=False,
reorder_ops=True) under the same visibility; LSE within 1e-3 absolute and +inf exactly where the oracle has it
(tests/test_kv8_kvcache_gpu.py).  Every case asserts the plan fa_fwd_last_plan_name() names and emits its worst err / bound
ratio per (batch, head, row slice) as a JSON line (tests/parity_helpers.py; FA_FWD_PARITY_JSONL=<path> collects them:
profiles/sparse_kv_parity.jsonl).

Shapes: b = 2, h / h_k = 8 / 2, capacity 512, fill levels 200 and 453 (no multiples of 64).  Lists hold max_blocks =
capacity / B entries.  Out-of-range entries (at or above ceil(fill / B)) and the stale entries behind the count are always
block numbers INSIDE the capacity, and page tables map every page of the capacity: a wrong kernel computes wrong numbers, it
never reads outside an allocation.

Pruned axes of the parity grid ({bf16, fp16} x d {64, 128} x cache {16-bit, fp8} x B {64, 128} x cache form {dense +
cache_batch_idx, page 64, page 16} x query form {decode, verify, ragged} = 144 combinations): dtype x d x cache type selects
the kernel instantiation, so all 8 are kept; B only changes the walk's entry / sub-tile split, the cache form only
load_tile's addressing, the query form only the row mapping -- none of them interacts with the instantiation, so each value
of the three appears with both cache types and is otherwise spread over the 8 rows (every B x cache form pair appears)."""
import re

import pytest
import torch

from oracle import attention_ref as oracle
from parity_helpers import Tiles, _emit
import sparse_kv_oracle

pytestmark = pytest.mark.gpu
DEV = "cuda"
F8 = torch.float8_e4m3fn
B_, H, HK, CAP = 2, 8, 2, 512
FILLS = (200, 453)


def _fa3():
    from flash_attention_annotated_amd import hopper_interface
    return hopper_interface


def _last_plan():
    from flash_attention_annotated_amd import _lib
    name = _lib.load().fa_fwd_last_plan_name()
    return name.decode() if name else None


def _descales(shift):
    vals = torch.tensor([0.5, 1.0, 2.0, 4.0, 0.25, 8.0, 0.125, 16.0])
    return vals[(torch.arange(B_ * HK) + shift) % len(vals)].view(B_, HK).contiguous()


def random_lists(block, seed=0):
    """Per (batch, kv head): a random order of ALL block numbers of the capacity, the first `cnt` of them listed.  The listed
    part holds the last (partial) block of the fill level and usually blocks past it (out of range, inside the capacity); the
    tail behind the count holds the rest (stale but valid block numbers)."""
    g = torch.Generator().manual_seed(seed)
    nb = CAP // block
    cnt = torch.zeros(B_, HK, dtype=torch.int32)
    idx = torch.zeros(B_, HK, nb, dtype=torch.int32)
    for b in range(B_):
        last = (FILLS[b] - 1) // block
        for kv in range(HK):
            perm = torch.randperm(nb, generator=g).tolist()
            c = int(torch.randint(nb // 2, nb, (1,), generator=g))
            at = perm.index(last)
            if at >= c:  # the straddling block is always listed
                perm[at], perm[c - 1] = perm[c - 1], perm[at]
            cnt[b, kv], idx[b, kv] = c, torch.tensor(perm, dtype=torch.int32)
    return cnt, idx


def full_lists(block, descending=False):
    """Every block of the fill level, in order; the tail holds valid block numbers past it."""
    nb = CAP // block
    order = torch.arange(nb, dtype=torch.int32)
    cnt = torch.tensor([[-(-f // block)] * HK for f in FILLS], dtype=torch.int32)
    idx = order.view(1, 1, nb).repeat(B_, HK, 1)
    if descending:
        for b in range(B_):
            c = int(cnt[b, 0])
            idx[b, :, :c] = order[:c].flip(0)
    return cnt, idx.contiguous()


class Case:
    def __init__(self, dtype=torch.bfloat16, d=128, fp8=False, block=128, form="dense", qform="decode", lists=None, window=(-1, -1),
                 softcap=0.0, seed=0):
        torch.manual_seed(seed)
        self.dtype, self.d, self.fp8, self.block, self.form, self.qform = dtype, d, fp8, block, form, qform
        self.window, self.softcap = window, softcap
        self.causal = qform != "decode"
        self.fills = torch.tensor(FILLS, dtype=torch.int32)
        self.cnt, self.idx = lists if lists is not None else random_lists(block, seed)
        if fp8:
            self.k_store, self.v_store = torch.randn(B_, CAP, HK, d).to(F8), torch.randn(B_, CAP, HK, d).to(F8)
            self.kdesc, self.vdesc = _descales(0), _descales(3)
            self.k_log = self.k_store.float() * self.kdesc[:, None, :, None]  # dequantised on the CPU (exact)
            self.v_log = self.v_store.float() * self.vdesc[:, None, :, None]
        else:
            self.k_store, self.v_store = torch.randn(B_, CAP, HK, d).to(dtype), torch.randn(B_, CAP, HK, d).to(dtype)
            self.k_log, self.v_log = self.k_store.float(), self.v_store.float()
        if qform == "ragged":  # a decode row and a 3-row verify step
            self.cu_q, self.sq = torch.tensor([0, 1, 4], dtype=torch.int32), 3
            self.q = torch.randn(4, H, d).to(dtype)
        else:
            self.cu_q, self.sq = None, 1 if qform == "decode" else 3
            self.q = torch.randn(B_, self.sq, H, d).to(dtype)
        self.batch_idx = self.table = None
        if form == "dense":
            self.batch_idx = torch.tensor([2, 0], dtype=torch.int32)
        else:
            page = 64 if form == "p64" else 16
            self.page, nblk = page, CAP // page
            self.table = torch.randperm(B_ * nblk + 3)[: B_ * nblk].to(torch.int32).view(B_, nblk)
        self._ref = None

    def q_rows(self, b):
        return self.q[b] if self.cu_q is None else self.q[int(self.cu_q[b]): int(self.cu_q[b + 1])]

    def reference(self, cnt=None, idx=None):
        """Per batch entry (out_ref (rows, h, d), lse_ref (h, rows), out_pt (rows, h, d)); computed once per list pair."""
        own = cnt is None
        if own and self._ref is not None:
            return self._ref
        cnt, idx = (self.cnt, self.idx) if own else (cnt, idx)
        res = []
        for b in range(B_):
            q = self.q_rows(b)
            c = cnt[b if cnt.shape[0] > 1 else 0].expand(HK) if cnt.shape[1] == 1 else cnt[b if cnt.shape[0] > 1 else 0]
            i = idx[b if idx.shape[0] > 1 else 0]
            i = i.expand(HK, -1) if i.shape[0] == 1 else i
            ref, lse, vis = sparse_kv_oracle.sparse_kv_ref(q, self.k_log[b], self.v_log[b], int(self.fills[b]), c, i, self.block,
                                                           self.causal, self.window, self.softcap)
            bias = torch.where(vis > 0, 0.0, float("-inf")).to(self.dtype)[None]
            pt = oracle.attention_ref(q[None], self.k_log[b][None].to(self.dtype), self.v_log[b][None].to(self.dtype), attn_bias=bias,
                                      softcap=self.softcap, upcast=False, reorder_ops=True)[0][0]
            res.append((ref, lse, pt.float().nan_to_num(0.0)))  # (a row without a visible key: 0, as the reference leg has it)
        if own:
            self._ref = res
        return res

    def _phys(self, x):
        if x.dtype == F8:
            return self._phys(x.view(torch.uint8)).view(F8)
        x = x.to(DEV)
        if self.table is not None:
            nblk = CAP // self.page
            pool = torch.zeros(B_ * nblk + 3, self.page, HK, self.d, dtype=x.dtype, device=DEV)
            pool[self.table.flatten().long().to(DEV)] = x.reshape(B_ * nblk, self.page, HK, self.d)
            return pool
        entries = torch.zeros(4, CAP, HK, self.d, dtype=x.dtype, device=DEV)
        entries[self.batch_idx.long().to(DEV)] = x
        return entries

    def inputs(self):
        """Device tensors of one call (kept by the caller over a graph capture)."""
        dev = lambda t: None if t is None else t.to(DEV)
        kw = dict(kv_block_size=self.block, cache_seqlens=dev(self.fills), cache_batch_idx=dev(self.batch_idx), page_table=dev(self.table),
                  causal=self.causal, window_size=self.window, softcap=self.softcap, return_softmax_lse=True)
        if self.cu_q is not None:
            kw.update(cu_seqlens_q=dev(self.cu_q), max_seqlen_q=self.sq)
        if self.fp8:
            kw.update(k_descale=dev(self.kdesc), v_descale=dev(self.vdesc))
        return (self.q.to(DEV), self._phys(self.k_store), self._phys(self.v_store), self.cnt.to(DEV), self.idx.to(DEV)), kw

    def plan(self, splits=1):
        return (f"sp_fwd_kernel D={self.d} waves=4{' SOFTCAP' if self.softcap > 0 else ''} KV={'e4m3' if self.fp8 else '16'} "
                f"B={self.block} block_m=128 splits={splits}")

    def run(self, num_splits=1):
        args, kw = self.inputs()
        out, lse = _fa3().flash_attn_with_kvcache_sparse(*args, num_splits=num_splits, **kw)
        return out.cpu(), lse.cpu(), _last_plan()

    def compare(self, out, lse, name, plan, ref=None, also=None):
        """Emit the worst error ratio, then assert the bound against the oracle -- and against `also` (another run's out) within
        the same bound."""
        ref = ref or self.reference()
        tiles, worst = Tiles(), []
        for b in range(B_):
            o_ref, l_ref, o_pt = ref[b]
            rows = slice(None) if self.cu_q is None else slice(int(self.cu_q[b]), int(self.cu_q[b + 1]))
            o = out[b] if self.cu_q is None else out[rows]
            l = lse[b] if self.cu_q is None else lse[:, rows]
            tiles.add(o[None], o_ref[None], o_pt[None], 3, 1e-5, batch=b)
            bound = 3 * (o_pt - o_ref).abs().max().item() + 1e-5
            err = (o.float() - o_ref).abs().max().item()
            worst.append((b, err, bound, o, l, l_ref, rows))
        _emit(f"sparse_kv::{name}", plan, tiles)
        for b, err, bound, o, l, l_ref, rows in worst:
            print(f"sparse_kv {name} batch {b}: |out - ref| = {err:.3e}  bound = {bound:.3e}  plan = {plan}")
            assert err <= bound, (name, b, err, bound)
            finite = torch.isfinite(l_ref)
            assert torch.equal(torch.isfinite(l), finite), (name, b)
            assert torch.all(l[~finite] == float("inf"))
            assert torch.allclose(l[finite], l_ref[finite], atol=1e-3, rtol=0), (name, b)
            if also is not None:
                other = also[b] if self.cu_q is None else also[rows]
                assert (o.float() - other.float()).abs().max().item() <= bound, (name, b, "against the unsplit run")

    def check(self, name, num_splits=1, splits=1, also=None):
        out, lse, plan = self.run(num_splits)
        assert plan == self.plan(splits), (plan, self.plan(splits))
        self.compare(out, lse, name, plan, also=also)
        return out, lse


BF, FP = torch.bfloat16, torch.float16
GRID = [
    (BF, 128, False, 128, "dense", "decode"),
    (BF, 128, True, 128, "p64", "decode"),
    (FP, 64, False, 64, "p16", "verify"),
    (FP, 64, True, 64, "dense", "ragged"),
    (BF, 64, True, 128, "p16", "verify"),
    (FP, 128, False, 64, "p64", "ragged"),
    (BF, 64, False, 128, "p64", "verify"),
    (FP, 128, True, 64, "dense", "decode"),
    (BF, 128, False, 64, "dense", "verify"),
    (FP, 64, True, 128, "dense", "ragged"),
    (BF, 128, True, 64, "p16", "ragged"),
    (FP, 128, False, 128, "p16", "decode"),
]


def _gid(row):
    dtype, d, fp8, block, form, qform = row
    return f"{'bf16' if dtype == BF else 'fp16'}-d{d}-{'fp8' if fp8 else '16bit'}-B{block}-{form}-{qform}"


@pytest.mark.parametrize("row", GRID, ids=[_gid(r) for r in GRID])
def test_sparse_kv_parity(row):
    dtype, d, fp8, block, form, qform = row
    Case(dtype, d, fp8, block, form, qform, seed=GRID.index(row)).check(_gid(row))


def _list_form(name, block):
    nb = CAP // block
    if name == "ascending":
        return full_lists(block)
    if name == "descending":
        return full_lists(block, descending=True)
    cnt, idx = random_lists(block, seed=5)
    if name == "cnt0":  # one (batch, kv head) lists nothing: its rows give out = 0, lse = +inf
        cnt[1, 0] = 0
    elif name == "last_partial_only":  # one entry, the block the fill level ends in
        for b in range(B_):
            cnt[b, :] = 1
            idx[b, :, 0] = (FILLS[b] - 1) // block
            idx[b, :, 1:] = torch.arange(1, nb, dtype=torch.int32)  # (stale, valid)
    elif name == "per_head":  # the two kv heads of a batch entry read disjoint halves
        for b in range(B_):
            nblk = -(-FILLS[b] // block)
            cnt[b, 0], cnt[b, 1] = (nblk + 1) // 2, nblk // 2
            idx[b, 0, : (nblk + 1) // 2] = torch.arange(0, nblk, 2, dtype=torch.int32)
            idx[b, 1, : nblk // 2] = torch.arange(1, nblk, 2, dtype=torch.int32)
    return cnt, idx


@pytest.mark.parametrize("fp8", [False, True], ids=["16bit", "fp8"])
@pytest.mark.parametrize("form", ["ascending", "descending", "cnt0", "last_partial_only", "per_head"])
def test_sparse_kv_list_forms(form, fp8):
    block = 128 if fp8 else 64
    c = Case(BF, 128, fp8, block, "p64" if fp8 else "dense", "verify", lists=_list_form(form, block), seed=11)
    out, lse = c.check(f"lists-{form}-{'fp8' if fp8 else '16bit'}")
    if form == "cnt0":
        assert torch.all(out[1, :, :4] == 0) and torch.all(lse[1, :4] == float("inf"))  # the heads of kv head 0 of batch 1


def test_sparse_kv_broadcast_lists():
    """One list for every batch entry and kv head: shapes (1, 1) and (1, 1, max_blocks), stride 0 in the C-ABI."""
    cnt, idx = torch.tensor([[3]], dtype=torch.int32), torch.tensor([[[3, 0, 1, 2]]], dtype=torch.int32)
    Case(FP, 64, False, 128, "dense", "decode", lists=(cnt, idx), seed=2).check("broadcast")


@pytest.mark.parametrize("fp8", [False, True], ids=["16bit", "fp8"])
def test_sparse_kv_window_edge_inside_a_listed_block(fp8):
    """Decode under a sliding window (100, 0): batch 1 sees keys 352 .. 452, so listed block 2 of B = 128 (keys 256 .. 383)
    straddles the left edge, block 3 the fill level; batch 0 sees 99 .. 199, block 0 straddles."""
    cnt, idx = full_lists(128)
    Case(BF, 128, fp8, 128, "p64", "decode", lists=(cnt, idx), window=(100, 0), seed=4).check(f"window-{'fp8' if fp8 else '16bit'}")


@pytest.mark.parametrize("fp8", [False, True], ids=["16bit", "fp8"])
def test_sparse_kv_softcap(fp8):
    Case(FP, 64, fp8, 64, "dense", "verify", softcap=15.0, seed=6).check(f"softcap-{'fp8' if fp8 else '16bit'}")


@pytest.mark.parametrize("fp8", [False, True], ids=["16bit", "fp8"])
@pytest.mark.parametrize("num_splits,cnt,splits", [(3, 5, 3), (4, 2, 4), (0, 5, 2)], ids=["3-of-cnt5", "4-of-cnt2", "heuristic"])
def test_sparse_kv_split(num_splits, cnt, splits, fp8):
    """B = 64, 8 list slots.  3 parts of 5 positions: uneven shares (2, 2, 1).  4 parts of 2 positions: two parts without a
    position (LSE -inf in the partials: no weight).  0: the pk heuristic for 8 x 64 keys = 2.  The listed entries of batch 0
    (fill 200: blocks 0 .. 3) include blocks past its fill level, so some parts hold positions but no visible key.  Against the
    oracle, and against the num_splits = 1 run of the same inputs within the same bound."""
    c, idx = random_lists(64, seed=9)
    c[:] = cnt
    for b in range(B_):  # keep the block the fill level ends in among the listed ones
        last = (FILLS[b] - 1) // 64
        for kv in range(HK):
            at = idx[b, kv].tolist().index(last)
            if at >= cnt:
                idx[b, kv, at], idx[b, kv, 0] = idx[b, kv, 0].clone(), idx[b, kv, at].clone()
    case = Case(BF, 128, fp8, 64, "p16" if fp8 else "dense", "verify", lists=(c, idx), seed=9)
    name = f"split-{num_splits}-cnt{cnt}-{'fp8' if fp8 else '16bit'}"
    one, _ = case.check(name + "-unsplit")
    case.check(name, num_splits, splits, also=one)


def test_sparse_kv_split_row_without_a_listed_key():
    """Split with a (batch, kv head) whose count is 0: every part of its rows writes +inf and the merge gives out = 0,
    lse = +inf -- not the -inf of parts that merely hold none of a row's keys."""
    cnt, idx = random_lists(64, seed=1)
    cnt[0, 1] = 0
    case = Case(FP, 64, False, 64, "p64", "decode", lists=(cnt, idx), seed=1)
    out, lse = case.check("split-cnt0", 3, 3)
    assert torch.all(out[0, :, 4:] == 0) and torch.all(lse[0, 4:] == float("inf"))


@pytest.mark.parametrize("num_splits", [1, 2], ids=["unsplit", "splits2"])
@pytest.mark.parametrize("block", [64, 128])
@pytest.mark.parametrize("fp8", [False, True], ids=["16bit", "fp8"])
def test_sparse_kv_bit_equal_to_the_parent_route(fp8, block, num_splits):
    """All blocks listed ascending walks the tiles the range walk visits, in its order, through the same tile step: out and LSE
    are bit-equal to the non-sparse call that runs pk_fwd_kernel (16-bit cache: pack_gqa=True, sq = 3) or kv8_fwd_kernel.
    Split: the sparse call partitions list positions, ceil(fill / B) * B / 64 of them, the parent the ceil(fill / 64) key tiles
    of a row block's range; the two coincide here (fills 200 and 453: 4 and 8 for both B) and would not for a fill level whose
    last block holds at most B - 64 keys (260 at B = 128: 6 positions, 5 tiles) -- there only the unsplit equality holds."""
    case = Case(BF, 128, fp8, block, "dense", "verify", lists=full_lists(block), seed=8)
    for f in FILLS:
        assert -(-f // block) * (block // 64) == -(-f // 64)
    out, lse, plan = case.run(num_splits)
    assert plan == case.plan(num_splits)
    (q, k, v, _, _), kw = case.inputs()
    extra = dict(k_descale=kw["k_descale"], v_descale=kw["v_descale"]) if fp8 else dict(pack_gqa=True)
    out_p, lse_p, *_ = _fa3().flash_attn_with_kvcache(q, k, v, cache_seqlens=kw["cache_seqlens"], cache_batch_idx=kw["cache_batch_idx"],
                                                     causal=True, num_splits=num_splits, return_softmax_lse=True, **extra)
    assert _last_plan() == f"{'kv8' if fp8 else 'pk'}_fwd_kernel D=128 waves=4 block_m=128 splits={num_splits}"
    assert torch.equal(out, out_p.cpu()) and torch.equal(lse, lse_p.cpu())
    case.compare(out, lse, f"bit-equal-{'fp8' if fp8 else '16bit'}-B{block}-s{num_splits}", plan)


@pytest.mark.parametrize("fp8", [False, True], ids=["16bit", "fp8"])
def test_sparse_kv_graph_replay_reads_the_lists_again(fp8):
    """Capture one call (one stream, no branches), replay, overwrite kv_block_cnt / kv_block_idx in place, replay: each replay
    matches the oracle for the lists it found -- the host never read them."""
    case = Case(BF, 128, fp8, 128, "p64", "decode", seed=12)
    args, kw = case.inputs()
    fn = lambda: _fa3().flash_attn_with_kvcache_sparse(*args, num_splits=2, **kw)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()  # (warm-up outside the capture: allocator and lazy initialisation)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, lse = fn()
    plan = _last_plan()
    assert plan == case.plan(2)
    graph.replay()
    torch.cuda.synchronize()
    case.compare(out.cpu(), lse.cpu(), f"graph-first-{'fp8' if fp8 else '16bit'}", plan)
    cnt2, idx2 = random_lists(128, seed=77)
    assert not torch.equal(idx2, case.idx) or not torch.equal(cnt2, case.cnt)
    args[3].copy_(cnt2.to(DEV))
    args[4].copy_(idx2.to(DEV))
    graph.replay()
    torch.cuda.synchronize()
    case.compare(out.cpu(), lse.cpu(), f"graph-second-{'fp8' if fp8 else '16bit'}", plan, ref=case.reference(cnt2, idx2))


def test_sparse_kv_argument_refusals():
    """The binding's refusals by argument, in the style of the neighbouring routes; nothing is launched."""
    case = Case(BF, 64, False, 128, "dense", "decode")
    (q, k, v, cnt, idx), kw = case.inputs()
    call = lambda *a, **over: _fa3().flash_attn_with_kvcache_sparse(*a, **{**kw, **over})
    f8 = lambda t: t.cpu().to(F8).to(DEV)
    with pytest.raises(RuntimeError, match="kv_block_cnt must have dtype int32"):
        call(q, k, v, cnt.long(), idx)
    with pytest.raises(RuntimeError, match="kv_block_idx must have dtype int32"):
        call(q, k, v, cnt, idx.long())
    with pytest.raises(RuntimeError, match="kv_block_idx must be on the same CUDA device as query"):
        call(q, k, v, cnt, idx.cpu())
    with pytest.raises(RuntimeError, match=r"kv_block_cnt must have shape \(batch_size \| 1, num_heads_k \| 1\)"):
        call(q, k, v, cnt.flatten(), idx)
    with pytest.raises(RuntimeError, match=r"kv_block_cnt must have shape \(batch_size \| 1, num_heads_k \| 1\)"):
        call(q, k, v, cnt[:, :1].repeat(1, 3), idx)
    with pytest.raises(RuntimeError, match=r"kv_block_idx must have shape \(batch_size \| 1, num_heads_k \| 1, max_blocks\)"):
        call(q, k, v, cnt, idx[0])
    with pytest.raises(RuntimeError, match="kv_block_idx must have contiguous last dimension"):
        call(q, k, v, cnt, idx.repeat(1, 1, 2)[:, :, ::2])
    with pytest.raises(RuntimeError, match="kv_block_size must be a positive multiple of 64, got 96"):
        call(q, k, v, cnt, idx, kv_block_size=96)
    with pytest.raises(RuntimeError, match="kv_block_size must be a positive multiple of 64, got 0"):
        call(q, k, v, cnt, idx, kv_block_size=0)
    with pytest.raises(RuntimeError, match="k_cache / v_cache must have the dtype of the query or be torch.float8_e4m3fn"):
        call(q.to(FP), k, v, cnt, idx)
    with pytest.raises(RuntimeError, match="fp16 / bf16 queries only"):
        call(f8(q), f8(k), f8(v), cnt, idx)
    with pytest.raises(RuntimeError, match="k_descale and v_descale must be provided with an fp8 KV cache"):
        call(q, f8(k), f8(v), cnt, idx)
    with pytest.raises(RuntimeError, match="k_descale / v_descale belong to an fp8 KV cache"):
        call(q, k, v, cnt, idx, k_descale=torch.ones(B_, HK, device=DEV), v_descale=torch.ones(B_, HK, device=DEV))
    with pytest.raises(RuntimeError, match="head_size <= 128 that is a multiple of 16"):
        call(q[..., :40], k[..., :40], v[..., :40], cnt, idx)
    assert re.match(r"sp_fwd_kernel", case.run()[2])  # and the accepted call still runs
