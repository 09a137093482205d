"""CPU tests of the torch helpers beside tree attention over a KV cache (flash_attention_annotated_amd/hopper_interface.py):
tree_mask_from_parents, tree_visibility / tree_attention_ref (the oracle of tests/test_tree_gpu.py) and kvcache_keep_tree_path_.
Nothing here touches a device."""
import pytest
import torch

from flash_attention_annotated_amd import hopper_interface as fa3
from oracle import attention_ref as oracle

F8 = torch.float8_e4m3fn


def random_parents(batch, T, seed):
    """(batch, T) int32: parents[b, i] in [-1, i), so forests of every shape (several roots, chains, stars)."""
    g = torch.Generator().manual_seed(seed)
    return torch.stack([torch.tensor([int(torch.randint(-1, i, (1,), generator=g)) if i else -1 for i in range(T)], dtype=torch.int32)
                        for _ in range(batch)])


def walk_up(parents):
    """The words by brute force: from every node up its parents, as Python ints (bit 63 folded into the sign)."""
    words = []
    for row in parents.tolist():
        out = []
        for i in range(len(row)):
            w, n = 0, i
            while n >= 0:
                w |= 1 << n
                n = row[n]
            out.append(w - (1 << 64) if w >> 63 else w)
        words.append(out)
    return torch.tensor(words, dtype=torch.int64)


@pytest.mark.parametrize("T", [1, 13, 64])
def test_tree_mask_from_parents_equals_the_walk_up_the_parents(T):
    parents = random_parents(5, T, seed=T)
    words = fa3.tree_mask_from_parents(parents)
    assert words.dtype == torch.int64 and words.shape == (5, T)
    assert torch.equal(words, walk_up(parents))
    assert torch.equal(fa3.tree_mask_from_parents(parents.long()), words)  # any int dtype


@pytest.mark.parametrize("T", [1, 13, 64])
def test_a_chain_gives_bits_0_to_i(T):
    parents = (torch.arange(T, dtype=torch.int32) - 1)[None]
    words = fa3.tree_mask_from_parents(parents)[0].tolist()
    for i, w in enumerate(words):
        assert w % (1 << 64) == (1 << (i + 1)) - 1


def test_tree_mask_from_parents_refuses_65_nodes():
    with pytest.raises(AssertionError, match="T <= 64"):
        fa3.tree_mask_from_parents(torch.full((1, 65), -1, dtype=torch.int32))


def test_tree_visibility_follows_the_definition():
    """sq = 3 at sk = 10 of 12 keys: the prefix [0, 7) for every row, draft key 7 + t by bit t; bits at or above sq and keys at
    or above sk never; more rows than bits: a draft key with t >= 64 is invisible."""
    words = torch.tensor([0b001, 0b110, -1], dtype=torch.int64)  # row 1 names no diagonal, row 2 names everything
    vis = fa3.tree_visibility(words, 10, 12)
    assert vis.shape == (3, 12) and vis[:, :7].all() and not vis[:, 10:].any()
    assert vis[:, 7:10].tolist() == [[True, False, False], [False, True, True], [True, True, True]]
    assert not fa3.tree_visibility(torch.zeros(3, dtype=torch.int64), 3, 12).any()  # no prefix, no bit
    wide = fa3.tree_visibility(torch.full((70,), -1, dtype=torch.int64), 100, 100)
    assert wide[:, :30].all() and wide[:, 30:94].all() and not wide[:, 94:].any()


@pytest.mark.parametrize("softcap", [0.0, 15.0], ids=["plain", "softcap"])
@pytest.mark.parametrize("fill,T", [(200, 13), (64, 64), (7, 7)])
def test_tree_attention_ref_with_a_chain_equals_the_causal_oracle(fill, T, softcap):
    torch.manual_seed(fill)
    b, cap, h, hk, d = 2, 256, 4, 2, 32
    q, k, v = torch.randn(b, T, h, d), torch.randn(b, cap, hk, d), torch.randn(b, cap, hk, d)
    words = fa3.tree_mask_from_parents((torch.arange(T, dtype=torch.int32) - 1).expand(b, T))
    fills = torch.tensor([fill, fill], dtype=torch.int32)
    out, lse = fa3.tree_attention_ref(q, k, v, words, cache_seqlens=fills, softcap=softcap, return_softmax_lse=True)
    ref, _, ref_lse = oracle.attention_ref(q, k[:, :fill], v[:, :fill], causal=True, softcap=softcap, return_lse=True)
    assert out.dtype == torch.float64 and out.shape == q.shape and lse.shape == (b, h, T)
    assert torch.allclose(out.float(), ref, atol=2e-6, rtol=1e-5)
    assert torch.allclose(lse.float(), ref_lse, atol=1e-5, rtol=0)


def test_tree_attention_ref_forms_agree():
    """The same logical problem through a dense cache with cache_batch_idx + cache_leftpad, through pages, with ragged queries and
    over an fp8 cache with descales gives the same numbers; a row with word 0 and no prefix gives out = 0, lse = +inf."""
    torch.manual_seed(1)
    b, cap, h, hk, d, T, page = 2, 64, 4, 2, 16, 5, 16
    fills = torch.tensor([5, 37], dtype=torch.int32)
    q = torch.randn(b, T, h, d)
    k, v = torch.randn(b, cap, hk, d).to(F8), torch.randn(b, cap, hk, d).to(F8)
    kd, vd = torch.tensor([[0.5, 2.0], [4.0, 1.0]]), torch.tensor([[1.0, 0.25], [2.0, 8.0]])
    words = fa3.tree_mask_from_parents(random_parents(b, T, seed=3))
    words[0, 2] = 0
    k_log, v_log = k.float() * kd[:, None, :, None], v.float() * vd[:, None, :, None]
    base, base_lse = fa3.tree_attention_ref(q, k_log, v_log, words, cache_seqlens=fills, return_softmax_lse=True)
    assert torch.all(base[0, 2] == 0) and torch.all(base_lse[0, :, 2] == float("inf")) and torch.isfinite(base_lse[1]).all()
    # fp8 bytes + descales
    out = fa3.tree_attention_ref(q, k, v, words, cache_seqlens=fills, k_descale=kd, v_descale=vd)
    assert torch.allclose(out, base, atol=1e-12)
    # cache_batch_idx + cache_leftpad: entry b lives in slot idx[b], 3 rows further in
    idx, lp = torch.tensor([2, 0], dtype=torch.int32), torch.tensor([3, 3], dtype=torch.int32)
    kk, vv = torch.zeros(3, cap + 3, hk, d), torch.zeros(3, cap + 3, hk, d)
    kk[idx.long(), 3:], vv[idx.long(), 3:] = k_log, v_log
    out = fa3.tree_attention_ref(q, kk, vv, words, cache_seqlens=fills + 3, cache_batch_idx=idx, cache_leftpad=lp)
    assert torch.allclose(out, base, atol=1e-12)
    # pages
    table = torch.randperm(b * cap // page + 2)[: b * cap // page].to(torch.int32).view(b, -1)
    kp, vp = torch.zeros(b * cap // page + 2, page, hk, d), torch.zeros(b * cap // page + 2, page, hk, d)
    kp[table.flatten().long()], vp[table.flatten().long()] = k_log.reshape(-1, page, hk, d), v_log.reshape(-1, page, hk, d)
    out = fa3.tree_attention_ref(q, kp, vp, words, cache_seqlens=fills, page_table=table)
    assert torch.allclose(out, base, atol=1e-12)
    # ragged queries: entry 0 keeps its first 2 nodes (its draft then sits at [3, 5) of the same fill level)
    cu = torch.tensor([0, 2, 2 + T], dtype=torch.int32)
    qr, wr = torch.cat([q[0, :2], q[1]]), torch.cat([words[0, :2], words[1]])
    out, lse = fa3.tree_attention_ref(qr, k_log, v_log, wr, cache_seqlens=fills, cu_seqlens_q=cu, max_seqlen_q=T, return_softmax_lse=True)
    assert out.shape == qr.shape and lse.shape == (h, 2 + T)
    assert torch.allclose(out[2:], base[1], atol=1e-12) and torch.allclose(lse[:, 2:], base_lse[1], atol=1e-12)
    two = fa3.tree_attention_ref(q[:1, :2], k_log[:1], v_log[:1], words[:1, :2], cache_seqlens=fills[:1])
    assert torch.allclose(out[:2], two[0], atol=1e-12)


@pytest.mark.parametrize("dtype", [torch.bfloat16, F8], ids=["16bit", "fp8"])
@pytest.mark.parametrize("form", ["dense", "dense_batch_idx", "paged"])
def test_kvcache_keep_tree_path(form, dtype):
    """Prefixes of 9 and 30 rows, a 13-node draft behind each, paths of 4 and 1 accepted nodes: the kept rows are the originals of
    the named nodes, in order; the prefix (and every other cache entry / page) is untouched; the fill levels are prefix + length."""
    torch.manual_seed(2)
    b, cap, hk, d, T, page = 2, 64, 2, 16, 13, 16
    shift = torch.tensor([9, 30], dtype=torch.int32)
    path = torch.tensor([[0, 2, 5, 12, 0], [3, 7, 1, 0, 0]], dtype=torch.int32)  # (behind path_len: anything)
    path_len = torch.tensor([4, 1], dtype=torch.int32)
    k_log, v_log = torch.randn(b, cap, hk, d).to(dtype), torch.randn(b, cap, hk, d).to(dtype)
    raw = lambda t: t.view(torch.uint8) if t.dtype == F8 else t
    kw = {}
    if form == "paged":
        n = b * cap // page
        table = torch.randperm(n + 2)[:n].to(torch.int32).view(b, -1)
        store = lambda x: _scatter(torch.zeros(n + 2, page, hk, d, dtype=raw(x).dtype), table.flatten().long(), raw(x).reshape(n, page, hk, d))
        logical = lambda c: raw(c)[table.flatten().long()].reshape(b, cap, hk, d)
        kw["page_table"] = table
    else:
        idx = torch.tensor([2, 0]) if form == "dense_batch_idx" else torch.arange(b)
        store = lambda x: _scatter(torch.zeros(3, cap, hk, d, dtype=raw(x).dtype), idx, raw(x))
        logical = lambda c: raw(c)[idx]
        if form == "dense_batch_idx":
            kw["cache_batch_idx"] = idx.to(torch.int32)
    k_cache, v_cache = (store(x).view(dtype) if dtype == F8 else store(x) for x in (k_log, v_log))
    before = [raw(c).clone() for c in (k_cache, v_cache)]
    new = fa3.kvcache_keep_tree_path_(k_cache, v_cache, shift, path, path_len, **kw)
    assert new.dtype == torch.int32 and new.tolist() == [13, 31]
    for cache, orig, was in ((k_cache, k_log, before[0]), (v_cache, v_log, before[1])):
        got = logical(cache)
        for i in range(b):
            s, n = int(shift[i]), int(path_len[i])
            assert torch.equal(got[i, :s], raw(orig)[i, :s])  # the prefix
            assert torch.equal(got[i, s:s + n], raw(orig)[i, s + path[i, :n].long()])  # the accepted nodes, in order
        touched = torch.zeros(was.shape[:2], dtype=torch.bool)  # nothing outside the draft rows of the two entries changed
        for i in range(b):
            for pos in range(int(shift[i]), int(shift[i]) + path.shape[1]):
                if form == "paged":
                    touched[int(table[i, pos // page]), pos % page] = True
                else:
                    touched[int(idx[i]), pos] = True
        assert torch.equal(raw(cache)[~touched], was[~touched])


def _scatter(dst, index, src):
    dst[index] = src
    return dst


def test_kvcache_keep_tree_path_identity_at_the_end_of_the_cache():
    """A chain accepted whole at the very end of the capacity: every move is a row onto itself, also the clamped ones behind the
    path -- the cache is unchanged."""
    k = torch.randn(1, 16, 1, 8)
    v = torch.randn(1, 16, 1, 8)
    k0, v0 = k.clone(), v.clone()
    new = fa3.kvcache_keep_tree_path_(k, v, torch.tensor([12], dtype=torch.int32), torch.tensor([[0, 1, 2, 3, 9, 9]], dtype=torch.int32),
                                      torch.tensor([4], dtype=torch.int32))
    assert new.tolist() == [16] and torch.equal(k, k0) and torch.equal(v, v0)
