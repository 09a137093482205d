"""CPU tests of flash_attention_annotated_amd.layers.rotary against the reference's pure-torch rotary code, frozen by
tools/make_rotary_golden.py into tests/golden/rotary_golden.pt: apply_rotary_emb_torch and the cos / sin / xPos tables of
RotaryEmbedding equal the frozen tensors exactly, and the public signatures are the reference's (written out below)."""
import inspect
import os

import pytest
import torch

from flash_attention_annotated_amd.layers import rotary

GOLDEN = torch.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rotary_golden.pt"))
CASES = GOLDEN["cases"]


def test_golden_covers_the_cases():
    kinds = {(c["kind"], c["interleaved"]) for c in CASES}
    assert kinds == {("plain", False), ("plain", True), ("qkv", False), ("qkv", True)}
    assert len(CASES) >= 20
    plain = [c for c in CASES if c["kind"] == "plain"]
    assert any(2 * c["cos"].shape[1] < c["x"].shape[-1] for c in plain)  # partial rotary_dim
    assert any(isinstance(c["offsets"], int) for c in plain) and any(isinstance(c["offsets"], list) for c in plain)
    assert any(c["kind"] == "qkv" and c["num_heads_q"] is not None for c in CASES)  # the GQA split
    assert all(t.dtype == torch.float32 for c in CASES for t in c.values() if isinstance(t, torch.Tensor))


@pytest.mark.parametrize("case", [c for c in CASES if c["kind"] == "plain"], ids=lambda c: c["name"])
def test_apply_rotary_emb_torch_equals_reference(case):
    x, cos, sin, off = case["x"], case["cos"], case["sin"], case["offsets"]
    s = x.shape[1]
    if off is None:
        cos, sin = cos[:s], sin[:s]
    elif isinstance(off, int):
        cos, sin = cos[off:off + s], sin[off:off + s]
    else:  # one offset per batch entry: tables of shape (b, s, rotary_dim / 2)
        idx = torch.tensor(off)[:, None] + torch.arange(s)[None]
        cos, sin = cos[idx], sin[idx]
    out = rotary.apply_rotary_emb_torch(x, cos, sin, case["interleaved"])
    assert out.shape == case["out"].shape and torch.equal(out, case["out"])


@pytest.mark.parametrize("case", [c for c in CASES if c["kind"] == "qkv"], ids=lambda c: c["name"])
def test_packed_qkv_split_equals_reference(case):
    """q and k rotated (k with tables of its own where given), v passed on: the split apply_rotary_emb_qkv_ makes."""
    qkv, il, hq = case["qkv"], case["interleaved"], case["num_heads_q"]
    cos_k = case["cos"] if case["cos_k"] is None else case["cos_k"]
    sin_k = case["sin"] if case["sin_k"] is None else case["sin_k"]
    if qkv.dim() == 5:
        q, k, v = qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2]
    else:
        _, hk = rotary._qkv_heads(qkv, hq)
        q, k, v = qkv[:, :, :hq], qkv[:, :, hq:hq + hk], qkv[:, :, hq + hk:]
    q, k = rotary.apply_rotary_emb_torch(q, case["cos"], case["sin"], il), rotary.apply_rotary_emb_torch(k, cos_k, sin_k, il)
    out = torch.stack([q, k, v], dim=2) if qkv.dim() == 5 else torch.cat([q, k, v], dim=2)
    assert torch.equal(out, case["out"])


@pytest.mark.parametrize("cache", GOLDEN["caches"], ids=lambda c: f"dim{c['dim']}_sb{c['scale_base']}_{str(c['dtype'])[6:]}")
def test_tables_equal_reference(cache):
    m = rotary.RotaryEmbedding(cache["dim"], base=cache["base"], scale_base=cache["scale_base"])
    assert torch.equal(m.inv_freq, cache["inv_freq"])
    assert (m.scale is None) == (cache["scale"] is None)
    if m.scale is not None:
        assert torch.equal(m.scale, cache["scale"])
    m._update_cos_sin_cache(cache["seqlen"], device=torch.device("cpu"), dtype=cache["dtype"])
    for name in ("cos", "sin", "cos_k", "sin_k"):
        got, want = getattr(m, f"_{name}_cached"), cache[name]
        assert (got is None) == (want is None), name
        if want is not None:
            assert got.dtype == want.dtype and torch.equal(got, want), name
    assert m._seq_len_cached == cache["seqlen"]
    kept = m._cos_cached
    m._update_cos_sin_cache(cache["seqlen"] - 1, device=torch.device("cpu"), dtype=cache["dtype"])  # shorter: the cache stays
    assert m._cos_cached is kept


# the reference's signatures (flash_attn/layers/rotary.py), names and defaults in order
SIGNATURES = {
    "apply_rotary_emb": [("x", None), ("cos", None), ("sin", None), ("interleaved", False), ("inplace", False),
                         ("seqlen_offsets", 0), ("cu_seqlens", None), ("max_seqlen", None)],
    "apply_rotary_emb_torch": [("x", None), ("cos", None), ("sin", None), ("interleaved", False)],
    "apply_rotary_emb_qkv_": [("qkv", None), ("cos", None), ("sin", None), ("cos_k", None), ("sin_k", None), ("interleaved", False),
                              ("seqlen_offsets", 0), ("num_heads_q", None)],
    "apply_rotary_emb_kv_": [("kv", None), ("cos", None), ("sin", None), ("interleaved", False), ("seqlen_offsets", 0)],
}
REQUIRED = {"apply_rotary_emb": 3, "apply_rotary_emb_torch": 3, "apply_rotary_emb_qkv_": 3, "apply_rotary_emb_kv_": 3}


@pytest.mark.parametrize("name", sorted(SIGNATURES))
def test_signatures(name):
    params = inspect.signature(getattr(rotary, name)).parameters
    assert list(params) == [n for n, _ in SIGNATURES[name]]
    for i, (n, default) in enumerate(SIGNATURES[name]):
        if i < REQUIRED[name]:
            assert params[n].default is inspect.Parameter.empty, n
        else:
            assert params[n].default == default and type(params[n].default) is type(default), n


def test_module_signatures_and_exports():
    assert rotary.apply_rotary_emb_func is rotary.apply_rotary_emb
    init = inspect.signature(rotary.RotaryEmbedding.__init__).parameters
    assert [(n, p.default) for n, p in init.items()][1:] == [("dim", inspect.Parameter.empty), ("base", 10000.0), ("interleaved", False),
                                                             ("scale_base", None), ("device", None)]
    fwd = inspect.signature(rotary.RotaryEmbedding.forward).parameters
    assert [(n, p.default) for n, p in fwd.items()][1:] == [("qkv", inspect.Parameter.empty), ("kv", None), ("seqlen_offset", 0),
                                                            ("max_seqlen", None), ("num_heads_q", None)]
    m = rotary.RotaryEmbedding(32)
    assert dict(m.named_buffers()).keys() == {"inv_freq", "scale"} or dict(m.named_buffers()).keys() == {"inv_freq"}
    assert not m.state_dict()  # neither buffer is persistent
    for name in ("ApplyRotaryEmb", "ApplyRotaryEmbQKV_", "ApplyRotaryEmbKV_"):
        assert issubclass(getattr(rotary, name), torch.autograd.Function)


def test_kernel_entry_is_two_custom_ops():
    ns = torch.ops.flash_attn_amd
    assert not ns._rotary_emb.default._schema.is_mutable
    assert ns._rotary_emb_.default._schema.is_mutable
    assert [a.name for a in ns._rotary_emb_.default._schema.arguments if a.alias_info is not None and a.alias_info.is_write] == ["x"]
