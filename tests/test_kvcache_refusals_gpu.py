"""The refusals of the KV-cache host path (csrc/torch_binding.cpp), one table: (route, one broken argument, the exact text).

Six public routes: `flash_attn_2_cuda.fwd_kvcache`; `torch.ops.flash_attn_3.fwd` (what the FA3 `flash_attn_with_kvcache` calls;
the op itself, so that `out` and `seqused_q` can be passed and no Python-side `contiguous()` repairs a broken view) with dense
q over a 16-bit cache, with ragged q (`cu_seqlens_q`, with and without `cu_seqlens_k_new`), over an fp8 cache read only, over
an fp8 cache with `k_new` / `v_new` and rotary; `hopper_interface.kvcache_append_fp8`.  Each case starts from the smallest
valid call of its route (`_bases`) and breaks one thing; every case is refused before any launch.  One valid call per base
pins the output's shape and dtype only: the parity tests own the values.

Shapes: b = 2, seqlen_q 1 and 3, h = 4, h_k = 2, d = 64.  FA2 surface: a (2, 256, 2, 64) cache (its page size must be a
multiple of 256, so the same tensor is two pages).  FA3 surface: 8 pages of 16 rows behind a (2, 4) page table, or a
(2, 64, 2, 64) batched cache.

Checks of the five host functions that no single broken argument reaches from these entry points:
* "paged k/v must have shape (num_blocks, page_block_size, num_heads_k, head_size)" (check_block_table): every route checks
  the cache's dim() first.
* CHECK_SHAPE of q and of a batched kcache on the dense route, "k must have shape ..." of the ragged route's paged kcache:
  the sizes they compare with are read from the same tensor, or (a q of another head dim) the V-headdim rule fires first.
* head_size <= 256 / % 8 / (fp8) <= 128 and % 16: q and both caches would have to change together; the append alone is
  reached with a cache pair of another head dim.
* "If key is supplied, it must have seqlen <= the seqlen of the KV cache": needs a cache shorter than q.
* "k_new / v_new must be fp16 or bf16" and "the fp8 KV cache must have dtype torch.float8_e4m3fn" behind the FA3 op: the
  op's own dtype rules fire first (both are reached through kvcache_append_fp8).
* the learnable-sink refusal of the fp8 route: the FA3 op has no sink argument.
* `out` on the fp8 route with new rows: refused by the read, after the append has been launched -- not a refusal before any
  launch, so not in this table.
* a 1-D rotary_cos and a cache_batch_idx shorter than the batch on the dense 16-bit routes: the table records the texts from
  before the routes shared their checks, when these two calls met torch's own IndexError (size(1) of a 1-D tensor) and a read
  past the index on the device.  The shared checks refuse both; NEWLY_REFUSED below pins that, apart from the table.
"""
import re

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, FP16, FP8, I32, I64, F32 = torch.bfloat16, torch.float16, torch.float8_e4m3fn, torch.int32, torch.int64, torch.float32

FA2_ORDER = ("q", "kcache", "vcache", "k", "v", "seqlens_k", "rotary_cos", "rotary_sin", "cache_batch_idx", "leftpad_k",
             "block_table", "alibi_slopes", "out", "softmax_scale", "is_causal", "window_size_left", "window_size_right",
             "softcap", "is_rotary_interleaved", "num_splits")


def _z(*shape, dtype=BF16):
    if dtype == FP8:
        return torch.zeros(*shape, dtype=torch.uint8, device=DEV).view(FP8)
    return torch.zeros(*shape, dtype=dtype, device=DEV)


def _i(values, dtype=I32):
    return torch.tensor(values, dtype=dtype, device=DEV)


_BASES = {}


def _bases():
    """The smallest valid call of every route, as keyword dicts; built once, never modified (a case works on a copy of the
    dict, and no refused call writes to a tensor)."""
    if _BASES:
        return _BASES
    B = _BASES
    # ---- flash_attn_2_cuda.fwd_kvcache: batched cache, three new rows, rotary
    B["fa2"] = dict(q=_z(2, 3, 4, 64), kcache=_z(2, 256, 2, 64), vcache=_z(2, 256, 2, 64), k=_z(2, 3, 2, 64), v=_z(2, 3, 2, 64),
                    seqlens_k=_i([5, 9]), rotary_cos=_z(256, 16), rotary_sin=_z(256, 16), cache_batch_idx=None, leftpad_k=None,
                    block_table=None, alibi_slopes=None, out=None, softmax_scale=0.125, is_causal=False, window_size_left=-1,
                    window_size_right=-1, softcap=0.0, is_rotary_interleaved=False, num_splits=0)
    B["fa2_paged"] = dict(B["fa2"], block_table=_i([[0], [1]]))
    B["fa2_decode"] = dict(B["fa2"], q=_z(2, 1, 4, 64), k=None, v=None, rotary_cos=None, rotary_sin=None)
    # ---- torch.ops.flash_attn_3.fwd, dense q over a 16-bit cache
    B["fa3"] = dict(q=_z(2, 3, 4, 64), k=_z(8, 16, 2, 64), v=_z(8, 16, 2, 64), k_new=_z(2, 3, 2, 64), v_new=_z(2, 3, 2, 64),
                    seqused_k=_i([5, 9]), page_table=_i([[0, 1, 2, 3], [4, 5, 6, 7]]), rotary_cos=_z(64, 16), rotary_sin=_z(64, 16))
    B["fa3_batched"] = dict(B["fa3"], k=_z(2, 64, 2, 64), v=_z(2, 64, 2, 64), page_table=None)
    B["fa3_decode"] = dict(q=_z(2, 1, 4, 64), k=_z(8, 16, 2, 64), v=_z(8, 16, 2, 64), seqused_k=_i([5, 9]),
                           page_table=_i([[0, 1, 2, 3], [4, 5, 6, 7]]))
    # ---- the same with ragged q (sequences of 1 and 3 rows)
    rag = dict(q=_z(4, 4, 64), cu_seqlens_q=_i([0, 1, 4]), max_seqlen_q=3)
    B["rag"] = dict(B["fa3"], **rag, k_new=_z(4, 2, 64), v_new=_z(4, 2, 64), cu_seqlens_k_new=_i([0, 1, 4]))
    B["rag_dense_new"] = dict(B["fa3"], **rag)
    B["rag_batched"] = dict(B["rag"], k=_z(2, 64, 2, 64), v=_z(2, 64, 2, 64), page_table=None)
    B["rag_read"] = dict(B["fa3_decode"], **rag)
    # ---- over an fp8 cache, read only
    kv8 = dict(k=_z(8, 16, 2, 64, dtype=FP8), v=_z(8, 16, 2, 64, dtype=FP8), k_descale=torch.ones(2, 2, device=DEV),
               v_descale=torch.ones(2, 2, device=DEV))
    B["kv8"] = dict(B["fa3_decode"], **kv8, q=_z(2, 3, 4, 64))
    B["kv8_rag"] = dict(B["rag_read"], **kv8)
    B["kv8_batched"] = dict(B["kv8"], k=_z(2, 64, 2, 64, dtype=FP8), v=_z(2, 64, 2, 64, dtype=FP8), page_table=None)
    B["kv8_nodescale"] = dict(B["kv8"], k_descale=None, v_descale=None)
    # ---- over an fp8 cache with new rows and rotary
    B["kv8a"] = dict(B["fa3"], **kv8)
    B["kv8a_norotary"] = dict(B["kv8a"], rotary_cos=None, rotary_sin=None)
    B["kv8a_rag"] = dict(B["rag"], **kv8)
    B["kv8a_batched"] = dict(B["kv8a"], k=_z(2, 64, 2, 64, dtype=FP8), v=_z(2, 64, 2, 64, dtype=FP8), page_table=None)
    # ---- hopper_interface.kvcache_append_fp8
    B["app"] = dict(k_cache=kv8["k"], v_cache=kv8["v"], k=_z(2, 3, 2, 64), v=_z(2, 3, 2, 64), cache_seqlens=_i([5, 9]),
                    k_descale=kv8["k_descale"], v_descale=kv8["v_descale"], page_table=_i([[0, 1, 2, 3], [4, 5, 6, 7]]),
                    rotary_cos=_z(64, 16), rotary_sin=_z(64, 16))
    B["app_rag"] = dict(B["app"], k=_z(4, 2, 64), v=_z(4, 2, 64), cu_seqlens_k_new=_i([0, 1, 4]), max_seqlen_k_new=3)
    B["app_batched"] = dict(B["app"], k_cache=_z(2, 64, 2, 64, dtype=FP8), v_cache=_z(2, 64, 2, 64, dtype=FP8), page_table=None)
    return B


def _call(base, a):
    if base.startswith("fa2"):
        from flash_attention_annotated_amd import flash_attn_2_cuda
        return flash_attn_2_cuda.fwd_kvcache(*[a[name] for name in FA2_ORDER])
    from flash_attention_annotated_amd import hopper_interface
    if base.startswith("app"):
        a = dict(a)
        head = [a.pop(name) for name in ("k_cache", "v_cache", "k", "v", "cache_seqlens", "k_descale", "v_descale")]
        return hopper_interface.kvcache_append_fp8(*head, **a)
    return torch.ops.flash_attn_3.fwd(**a)


# ---- how a case breaks its argument: mut(name=value or function of the base's value, ...)
def mut(**kw):
    return lambda a: {**a, **{name: (f(a.get(name)) if callable(f) else f) for name, f in kw.items()}}


def cpu(t):
    return t.cpu()


def to(dtype):
    return lambda t: t.to(dtype)


def shape(*s):
    return lambda t: torch.zeros(*s, dtype=torch.uint8 if t.dtype == FP8 else t.dtype, device=t.device).view(t.dtype)


def strided(t):
    """The same shape with a last stride of 2."""
    wide = torch.zeros(*t.shape[:-1], 2 * t.shape[-1], dtype=torch.uint8 if t.dtype == FP8 else t.dtype, device=t.device)
    return wide.view(t.dtype)[..., ::2]


def misaligned(t):
    """The same shape as a [..., 1:] slice: a base one element off, odd row strides."""
    wide = torch.zeros(*t.shape[:-1], t.shape[-1] + 1, dtype=torch.uint8 if t.dtype == FP8 else t.dtype, device=t.device)
    return wide.view(t.dtype)[..., 1:]


def new(values, dtype=I32):
    return lambda _: _i(values, dtype)


def both(k, v, f):
    return mut(**{k: f, v: f})


LAST = "Input tensor must have contiguous last dimension"
PAGED_IDX = "Paged KVcache does not support cache_batch_idx"
PAGED_LEFTPAD = "We don't support Paged KV and leftpad_k running at the same time yet"
HEADS = "Number of heads in key/value must divide number of heads in query"
ENTRIES = "the KV cache must have at least batch_size entries"
ALIGN16 = "the KV cache must be 16-byte aligned with row/head/batch strides that are multiples of 8"
BT_SHAPE = "block_table must have shape (batch_size, max_num_blocks_per_seq)"
NEED_NEW = "If rotary cos/sin are provided, new key / value to be appended to KV cache must also be provided"
RO_HEAD = "rotary_dim must be <= headdim"
RO_16 = "Only rotary dimensions divisible by 16 are currently supported"
RO_SHORT = "cos/sin seqlen must be at least the seqlen of KV cache"
RO_SHAPE = "rotary_cos / rotary_sin must have shape (seqlen_ro, rotary_dim / 2)"
RO_CONTIG = "rotary_cos / rotary_sin must be contiguous"
FP8_4D = "an fp8 k / v must be a KV cache of shape (batch or num_pages, seqlen or page_size, num_heads_k, head_size)"
KV8_SEQUSED = "seqused_k must be int32 of shape (batch_size,)"
KV8_IDX = "cache_batch_idx must be contiguous, (batch_size,)"
KV8_CUQ = "cu_seqlens_q must be a contiguous int32 CUDA tensor"
APP_SEQLENS = "cache_seqlens must be a contiguous int32 CUDA tensor of shape (batch_size,)"
NEW_FP8 = ("This flash attention build does not support fp8 k_new / v_new with an fp8 KV cache: the new rows are fp16 / bf16 "
           "and are quantised by the append.")
OUT_3 = "out must have shape (..., num_heads, head_size_v)"
SEQUSED_NEEDED = "seqused_k must be provided with k_new / leftpad_k"
TOGETHER_RO = "rotary_cos and rotary_sin must be passed together"
RAG_SEQUSED = " must be a contiguous CUDA tensor of shape (batch_size,)"
RO_SEQLENS = "seqlens_rotary must be a contiguous CUDA tensor"


def _dense16(base, paged, batched, decode, cache_k, cache_v, k_new, v_new, fill, idx, table, page_multiple):
    """fwd_kvcache_core, reached from the FA2 entry point and from the FA3 op with dense q: the same rows under each
    surface's argument names."""
    c = [
        (base, "cache k dtype", mut(**{cache_k: to(FP16)}), "query and key must have the same dtype"),
        (base, "cache v dtype", mut(**{cache_v: to(FP16)}), "query and value must have the same dtype"),
        (base, "cache k last stride", mut(**{cache_k: strided}), LAST),
        (base, "cache v last stride", mut(**{cache_v: strided}), LAST),
        (base, "cache k 3-D", mut(**{cache_k: lambda t: t[0]}), "q, kcache must have 4 dimensions"),
        (base, "q 3-D", mut(q=lambda t: t[0]), "q, kcache must have 4 dimensions"),
        (base, "heads", mut(q=shape(2, 3, 3, 64)), HEADS),
        (paged, "paged with cache_batch_idx", mut(**{idx: new([1, 0])}), PAGED_IDX),
        (paged, "page table dtype", mut(**{table: to(I64)}), "block_table must have dtype torch.int32"),
        (paged, "page table on cpu", mut(**{table: cpu}), "block_table must be on CUDA"),
        (paged, "page table last stride", mut(**{table: strided}), "block_table must have contiguous last dimension"),
        (paged, "page table batch", mut(**{table: lambda t: torch.cat([t, t[:1]])}), BT_SHAPE),
        (paged, "page table 1-D", mut(**{table: lambda t: t[0]}), BT_SHAPE),
        (paged, "paged cache v pages", mut(**{cache_v: lambda t: t[:-1]}),
         "vcache must have shape (kcache.size(0), page_block_size, num_heads_k, head_size_v)"),
        (paged, "paged with leftpad_k", mut(leftpad_k=new([0, 0])), PAGED_LEFTPAD),
        (batched, "cache v rows", mut(**{cache_v: lambda t: t[:, :-16]}),
         "vcache must have shape (batch_size_c, seqlen_k, num_heads_k, head_size_v)"),
        (batched, "out dtype", mut(out=lambda _: _z(2, 3, 4, 64, dtype=FP16)), "Output must have the same dtype as inputs"),
        (batched, "out on cpu", mut(out=lambda _: _z(2, 3, 4, 64).cpu()), "out must be on CUDA"),
        (batched, "out last stride", mut(out=lambda _: strided(_z(2, 3, 4, 64))), "Output tensor must have contiguous last dimension"),
        (batched, "out shape", mut(out=lambda _: _z(2, 3, 4, 32)), "out must have shape (batch_size, seqlen_q, num_heads, head_size_v)"),
        (batched, "new k dtype", mut(**{k_new: to(FP16)}), "Key must have the same dtype as query"),
        (batched, "new v dtype", mut(**{v_new: to(FP16)}), "Value must have the same dtype as query"),
        (batched, "new k on cpu", mut(**{k_new: cpu}), "k must be on CUDA"),
        (batched, "new v on cpu", mut(**{v_new: cpu}), "v must be on CUDA"),
        (batched, "new k last stride", mut(**{k_new: strided}), "Key tensor must have contiguous last dimension"),
        (batched, "new v last stride", mut(**{v_new: strided}), "Value tensor must have contiguous last dimension"),
        (batched, "new k heads", mut(**{k_new: shape(2, 3, 1, 64)}), "k must have shape (batch_size, seqlen_knew, num_heads_k, head_size_og)"),
        (batched, "new k 3-D", mut(**{k_new: shape(6, 2, 64)}), "k must have shape (batch_size, seqlen_knew, num_heads_k, head_size_og)"),
        (batched, "new v rows", mut(**{v_new: shape(2, 2, 2, 64)}), "v must have shape (batch_size, seqlen_knew, num_heads_k, head_size_v)"),
        (batched, "fill levels dtype", mut(**{fill: to(I64)}), "seqlens_k must have dtype int32"),
        (batched, "fill levels on cpu", mut(**{fill: cpu}), "seqlens_k must be on CUDA"),
        (batched, "fill levels stride", mut(**{fill: strided}), "seqlens_k must be contiguous"),
        (batched, "fill levels shape", mut(**{fill: new([5, 9, 1])}), "seqlens_k must have shape (batch_size)"),
        (decode, "fill levels shape, no new rows", mut(**{fill: new([5, 9, 1])}), "seqlens_k must have shape (batch_size)"),
        (batched, "leftpad_k dtype", mut(leftpad_k=new([0, 0], I64)), "leftpad_k must have dtype int32"),
        (batched, "leftpad_k on cpu", mut(leftpad_k=lambda _: _i([0, 0]).cpu()), "leftpad_k must be on CUDA"),
        (batched, "leftpad_k stride", mut(leftpad_k=lambda _: _i([0, 0, 0, 0])[::2]), "leftpad_k must be contiguous"),
        (batched, "leftpad_k shape", mut(leftpad_k=new([0, 0, 0])), "leftpad_k must have shape (batch_size)"),
        (batched, "cache_batch_idx on cpu", mut(**{idx: lambda _: _i([1, 0]).cpu()}), "cache_batch_idx must be on CUDA"),
        (batched, "cache_batch_idx stride", mut(**{idx: lambda _: _i([1, 0, 0, 0])[::2]}), "cache_batch_idx must be contiguous"),
        (batched, "cache_batch_idx dtype", mut(**{idx: new([1, 0], I64)}), "cache_batch_idx must have dtype int32"),
        (batched, "cache smaller than the batch", both(cache_k, cache_v, lambda t: t[:1]), ENTRIES),
        (batched, "cache k misaligned", mut(**{cache_k: misaligned}), ALIGN16),
        (batched, "cache v misaligned", mut(**{cache_v: misaligned}), ALIGN16),
        (batched, "rotary without new rows", mut(**{k_new: None, v_new: None}), NEED_NEW),
        (batched, "rotary_cos on cpu", mut(rotary_cos=cpu), "rotary_cos must be on CUDA"),
        (batched, "rotary_dim above the head dim", both("rotary_cos", "rotary_sin", shape(256, 48)), RO_HEAD),
        (batched, "rotary_dim 24", both("rotary_cos", "rotary_sin", shape(256, 12)), RO_16),
        (batched, "cos / sin shorter than the cache", both("rotary_cos", "rotary_sin", lambda t: t[:32]), RO_SHORT),
        (paged, "cos / sin shorter than the pages", both("rotary_cos", "rotary_sin", lambda t: t[:32]), RO_SHORT),
        (batched, "rotary_cos 3-D", mut(rotary_cos=lambda t: t.unsqueeze(-1)), "rotary_cos must have shape (seqlen_ro, rotary_dim / 2)"),
        (batched, "rotary_cos stride", mut(rotary_cos=strided), "rotary_cos must be contiguous"),
        (batched, "rotary_cos dtype", mut(rotary_cos=to(FP16)), "rotary_cos must have the same dtype as query"),
        (batched, "rotary_sin on cpu", mut(rotary_sin=cpu), "rotary_sin must be on CUDA"),
        (batched, "rotary_sin shape", mut(rotary_sin=lambda t: t[:, :8]), "rotary_sin must have shape (seqlen_ro, rotary_dim / 2)"),
        (batched, "rotary_sin stride", mut(rotary_sin=strided), "rotary_sin must be contiguous"),
        (batched, "rotary_sin dtype", mut(rotary_sin=to(FP16)), "rotary_cos must have the same dtype as query"),
    ]
    if page_multiple > 1:
        c.append((paged, "page size", both(cache_k, cache_v, lambda t: t[:, :128]), "Paged KV cache block size must be divisible by 256"))
    return c


CASES = _dense16("fa2", "fa2_paged", "fa2", "fa2_decode", "kcache", "vcache", "k", "v", "seqlens_k", "cache_batch_idx",
                 "block_table", 256) + [
    ("fa2", "q dtype", mut(q=to(F32)), "FlashAttention only support fp16 and bf16 data type"),
    ("fa2", "q on cpu", mut(q=cpu), "q must be on CUDA"),
    ("fa2", "cache k on cpu", mut(kcache=cpu), "kcache must be on CUDA"),
    ("fa2", "cache v on cpu", mut(vcache=cpu), "vcache must be on CUDA"),
    ("fa2", "q last stride", mut(q=strided), LAST),
    ("fa2", "cache v head dim", mut(vcache=shape(2, 256, 2, 32)),
     "vcache must have shape (batch_size_c, seqlen_k, num_heads_k, head_size_og)"),
    ("fa2_paged", "paged cache v head dim", mut(vcache=shape(2, 256, 2, 32)),
     "vcache must have shape (kcache.size(0), page_block_size, num_heads_k, head_size_og)"),
    ("fa2", "q head dim", mut(q=shape(2, 3, 4, 32)),
     "If V headdim is different from Q/K dim, this KV-cache path only supports Q/K <= 64 and V in [256, 512]"),
    ("fa2", "empty batch", mut(q=shape(0, 3, 4, 64)), "batch size must be positive"),
    ("fa2", "k without v", mut(v=None), "If key is supplied, value must also be passed in"),
    ("fa2", "k without seqlens_k", mut(seqlens_k=None), "If key is supplied, seqlens_k must also be passed in"),
    ("fa2", "rotary_cos without rotary_sin", mut(rotary_sin=None), "If rotary cos is provided, rotary sin must also be provided"),
    ("fa2", "alibi_slopes dtype", mut(alibi_slopes=lambda _: _z(4)), "ALiBi slopes must have dtype fp32"),
    ("fa2", "alibi_slopes shape", mut(alibi_slopes=lambda _: _z(3, dtype=F32)),
     "alibi_slopes must have shape (num_heads) or (batch_size, num_heads)"),
] + _dense16("fa3", "fa3", "fa3_batched", "fa3_decode", "k", "v", "k_new", "v_new", "seqused_k", "kv_batch_idx", "page_table", 1) + [
    ("fa3", "q dtype", mut(q=to(F32)), "FlashAttention only supports fp16, bf16, and fp8_e4m3 data type"),
    ("fa3", "q on cpu", mut(q=cpu), "q must be on CUDA"),
    ("fa3", "cache k on cpu", mut(k=cpu), "k must be on CUDA"),
    ("fa3", "cache v on cpu", mut(v=cpu), "v must be on CUDA"),
    ("fa3", "q last stride", mut(q=strided), LAST),
    ("fa3_batched", "empty batch", mut(q=shape(0, 3, 4, 64)), "batch size must be positive"),
    ("fa3", "cu_seqlens_k_new with dense q", mut(cu_seqlens_k_new=new([0, 3, 6])),
     "This flash attention build does not support cu_seqlens_k_new without cu_seqlens_q."),
    ("fa3", "k_new without v_new", mut(v_new=None), "k_new and v_new must be passed together"),
    ("fa3", "rotary_cos without rotary_sin", mut(rotary_sin=None), TOGETHER_RO),
    ("fa3", "k_new without seqused_k", mut(seqused_k=None), SEQUSED_NEEDED),
    ("fa3", "seqused_q with dense q", mut(seqused_q=new([3, 3])),
     "This flash attention build does not support KV-cache arguments together with seqused_q without cu_seqlens_q."),
    ("fa3", "cu_seqlens_k", mut(cu_seqlens_k=new([0, 5, 14])),
     "This flash attention build does not support KV-cache arguments together with cu_seqlens_k."),
    ("fa3", "seqlens_rotary dtype", mut(seqlens_rotary=new([5, 9], I64)), "seqlens_rotary must have dtype torch.int32"),
    ("fa3", "seqlens_rotary on cpu", mut(seqlens_rotary=lambda _: _i([5, 9]).cpu()), RO_SEQLENS),
    ("fa3", "seqlens_rotary stride", mut(seqlens_rotary=lambda _: _i([5, 9, 0, 0])[::2]), RO_SEQLENS),
    ("fa3", "seqlens_rotary shape", mut(seqlens_rotary=new([5, 9, 0])), "seqlens_rotary must have shape (batch_size,)"),
    # ---- ragged q over a 16-bit cache: fwd_kvcache_ragged
    ("rag", "cu_seqlens_q on cpu", mut(cu_seqlens_q=cpu), "cu_seqlens_q must be on CUDA"),
    ("rag", "cu_seqlens_q stride", mut(cu_seqlens_q=strided), "cu_seqlens_q must be contiguous"),
    ("rag", "cu_seqlens_q dtype", mut(cu_seqlens_q=to(I64)), "cu_seqlens_q must have dtype torch.int32"),
    ("rag", "no max_seqlen_q", mut(max_seqlen_q=None), "max_seqlen_q must be provided if cu_seqlens_q is provided"),
    ("rag", "q 4-D", mut(q=lambda t: t.unsqueeze(0)), "q must have shape (total_q, num_heads, head_size)"),
    ("rag_read", "no seqused_k", mut(seqused_k=None), "seqused_k must be provided for a KV-cache call with cu_seqlens_q"),
    ("rag", "k_new without seqused_k", mut(seqused_k=None), SEQUSED_NEEDED),
    ("rag", "paged with kv_batch_idx", mut(kv_batch_idx=new([1, 0])), PAGED_IDX),
    ("rag", "cache k 3-D", mut(k=lambda t: t[0]), "kcache, vcache must have 4 dimensions"),
    ("rag", "cache v 3-D", mut(v=lambda t: t[0]), "kcache, vcache must have 4 dimensions"),
    ("rag", "cache k dtype", mut(k=to(FP16)), "query and key must have the same dtype"),
    ("rag", "cache k last stride", mut(k=strided), LAST),
    ("rag", "empty batch", mut(cu_seqlens_q=new([0])), "batch size must be positive"),
    ("rag", "heads", mut(q=shape(4, 3, 64)), HEADS),
    ("rag", "page table dtype", mut(page_table=to(I64)), "block_table must have dtype torch.int32"),
    ("rag", "page table on cpu", mut(page_table=cpu), "block_table must be on CUDA"),
    ("rag", "page table last stride", mut(page_table=strided), "block_table must have contiguous last dimension"),
    ("rag", "page table batch", mut(page_table=lambda t: torch.cat([t, t[:1]])), BT_SHAPE),
    ("rag", "paged cache v pages", mut(v=lambda t: t[:-1]), "vcache must have shape (kcache.size(0), pr.first, num_heads_k, head_size_v)"),
    ("rag_batched", "cache v rows", mut(v=lambda t: t[:, :-16]), "vcache must have shape (batch_size_c, seqlen_k, num_heads_k, head_size_v)"),
    ("rag", "seqused_k dtype", mut(seqused_k=to(I64)), "seqused_k must have dtype int32"),
    ("rag", "seqused_k on cpu", mut(seqused_k=cpu), "seqused_k" + RAG_SEQUSED),
    ("rag", "seqused_k stride", mut(seqused_k=strided), "seqused_k" + RAG_SEQUSED),
    ("rag", "seqused_k shape", mut(seqused_k=new([5, 9, 1])), "seqused_k" + RAG_SEQUSED),
    ("rag", "seqused_q dtype", mut(seqused_q=new([1, 3], I64)), "seqused_q must have dtype int32"),
    ("rag", "seqused_q shape", mut(seqused_q=new([1, 3, 1])), "seqused_q" + RAG_SEQUSED),
    ("rag", "paged with leftpad_k", mut(leftpad_k=new([0, 0])), PAGED_LEFTPAD),
    ("rag_batched", "leftpad_k dtype", mut(leftpad_k=new([0, 0], I64)), "leftpad_k must have dtype int32"),
    ("rag_batched", "leftpad_k stride", mut(leftpad_k=lambda _: _i([0, 0, 0, 0])[::2]), "leftpad_k must be contiguous"),
    ("rag_batched", "leftpad_k shape", mut(leftpad_k=new([0, 0, 0])), "leftpad_k must have shape (batch_size)"),
    ("rag_batched", "kv_batch_idx on cpu", mut(kv_batch_idx=lambda _: _i([1, 0]).cpu()), "kv_batch_idx must be on CUDA"),
    ("rag_batched", "kv_batch_idx stride", mut(kv_batch_idx=lambda _: _i([1, 0, 0, 0])[::2]), "kv_batch_idx must be contiguous"),
    ("rag_batched", "kv_batch_idx dtype", mut(kv_batch_idx=new([1, 0], I64)), "kv_batch_idx must have dtype int32"),
    ("rag_batched", "kv_batch_idx shape", mut(kv_batch_idx=new([1, 0, 0])), "kv_batch_idx must have shape (batch_size)"),
    ("rag_batched", "cache smaller than the batch", both("k", "v", lambda t: t[:1]), ENTRIES),
    ("rag_batched", "cache k misaligned", mut(k=misaligned), ALIGN16),
    ("rag", "paged cache v misaligned", mut(v=misaligned), ALIGN16),
    ("rag", "k_new dtype", mut(k_new=to(FP16)), "k_new must have the same dtype as query"),
    ("rag", "v_new dtype", mut(v_new=to(FP16)), "v_new must have the same dtype as query"),
    ("rag", "k_new on cpu", mut(k_new=cpu), "k_new must be on CUDA"),
    ("rag", "v_new on cpu", mut(v_new=cpu), "v_new must be on CUDA"),
    ("rag", "k_new last stride", mut(k_new=strided), "k_new tensor must have contiguous last dimension"),
    ("rag", "v_new last stride", mut(v_new=strided), "v_new tensor must have contiguous last dimension"),
    ("rag", "k_new without v_new", mut(v_new=None), "k_new and v_new must be passed together"),
    ("rag", "cu_seqlens_k_new on cpu", mut(cu_seqlens_k_new=cpu), "cu_seqlens_k_new must be on CUDA"),
    ("rag", "cu_seqlens_k_new stride", mut(cu_seqlens_k_new=strided), "cu_seqlens_k_new must be contiguous"),
    ("rag", "cu_seqlens_k_new dtype", mut(cu_seqlens_k_new=to(I64)), "cu_seqlens_k_new must have dtype torch.int32"),
    ("rag", "cu_seqlens_k_new shape", mut(cu_seqlens_k_new=new([0, 1, 2, 4])), "cu_seqlens_k_new must have shape (batch_size + 1)"),
    ("rag", "cu_seqlens_k_new without new rows", mut(k_new=None, v_new=None, rotary_cos=None, rotary_sin=None),
     "cu_seqlens_k_new needs k_new and v_new"),
    ("rag", "ragged k_new 4-D", mut(k_new=lambda t: t.unsqueeze(0)),
     "k_new must have shape (total_k_new, num_heads_k, head_size) with cu_seqlens_k_new"),
    ("rag", "ragged k_new heads", mut(k_new=shape(4, 1, 64)), "k_new must have shape (k_new->size(0), num_heads_k, head_size)"),
    ("rag", "ragged v_new rows", mut(v_new=shape(3, 2, 64)), "v_new must have shape (k_new->size(0), num_heads_k, head_size_v)"),
    ("rag_dense_new", "dense k_new 3-D", mut(k_new=shape(6, 2, 64)),
     "k_new must have shape (batch_size, seqlen_k_new, num_heads_k, head_size) without cu_seqlens_k_new"),
    ("rag_dense_new", "dense k_new batch", mut(k_new=shape(3, 3, 2, 64)), "k_new must have shape (batch_size, k_new->size(1), num_heads_k, head_size)"),
    ("rag_dense_new", "dense v_new rows", mut(v_new=shape(2, 2, 2, 64)), "v_new must have shape (batch_size, k_new->size(1), num_heads_k, head_size_v)"),
    ("rag_dense_new", "rotary without new rows", mut(k_new=None, v_new=None), NEED_NEW),
    ("rag", "rotary_cos on cpu", mut(rotary_cos=cpu), "rotary_cos must be on CUDA"),
    ("rag", "rotary_sin on cpu", mut(rotary_sin=cpu), "rotary_sin must be on CUDA"),
    ("rag", "rotary_cos 1-D", mut(rotary_cos=lambda t: t[:, 0]), RO_SHAPE),
    ("rag", "rotary_sin shape", mut(rotary_sin=lambda t: t[:, :8]), RO_SHAPE),
    ("rag", "rotary_dim above the head dim", both("rotary_cos", "rotary_sin", shape(64, 48)), RO_HEAD),
    ("rag", "rotary_dim 24", both("rotary_cos", "rotary_sin", shape(64, 12)), RO_16),
    ("rag", "cos / sin shorter than the pages", both("rotary_cos", "rotary_sin", lambda t: t[:32]), RO_SHORT),
    ("rag_batched", "cos / sin shorter than the cache", both("rotary_cos", "rotary_sin", lambda t: t[:32]), RO_SHORT),
    ("rag", "rotary_cos stride", mut(rotary_cos=strided), RO_CONTIG),
    ("rag", "rotary_sin stride", mut(rotary_sin=strided), RO_CONTIG),
    ("rag", "rotary_cos dtype", mut(rotary_cos=to(FP16)), "rotary_cos / rotary_sin must have the same dtype as query"),
    ("rag", "rotary_sin dtype", mut(rotary_sin=to(FP16)), "rotary_cos / rotary_sin must have the same dtype as query"),
    ("rag", "rotary_cos without rotary_sin", mut(rotary_sin=None), TOGETHER_RO),
    ("rag", "seqlens_rotary dtype", mut(seqlens_rotary=new([5, 9], I64)), "seqlens_rotary must have dtype torch.int32"),
    ("rag", "seqlens_rotary shape", mut(seqlens_rotary=new([5, 9, 0])), "seqlens_rotary must have shape (batch_size,)"),
    ("rag", "out dtype", mut(out=lambda _: _z(4, 4, 64, dtype=FP16)), "Output must have the same dtype as inputs"),
    ("rag", "out on cpu", mut(out=lambda _: _z(4, 4, 64).cpu()), OUT_3),
    ("rag", "out last stride", mut(out=lambda _: strided(_z(4, 4, 64))), OUT_3),
    ("rag", "out shape", mut(out=lambda _: _z(4, 4, 32)), OUT_3),
    # ---- 16-bit q over an fp8 cache, read only: the refusals of the route and fwd_kv8
    ("kv8_nodescale", "k_new without descales", mut(k_new=lambda _: _z(2, 3, 2, 64), v_new=lambda _: _z(2, 3, 2, 64)),
     "This flash attention build does not support k_new / v_new with an fp8 KV cache: appending to it (quantising the new "
     "rows) is the caller's job."),
    ("kv8_nodescale", "rotary without descales", mut(rotary_cos=lambda _: _z(64, 16), rotary_sin=lambda _: _z(64, 16)),
     "This flash attention build does not support rotary_cos / rotary_sin with an fp8 KV cache."),
    ("kv8", "qv", mut(q_v=lambda _: _z(2, 3, 4, 64)), "This flash attention build does not support qv with an fp8 KV cache."),
    ("kv8", "cache v head dim", mut(v=shape(8, 16, 2, 32)),
     "This flash attention build does not support a V headdim of its own with an fp8 KV cache."),
    ("kv8", "attention_chunk", mut(attention_chunk=4), "This flash attention build does not support attention_chunk with an fp8 KV cache."),
    ("kv8", "cu_seqlens_k", mut(cu_seqlens_k=new([0, 5, 14])), "This flash attention build does not support cu_seqlens_k with an fp8 KV cache."),
    ("kv8", "q on cpu", mut(q=cpu), "q must be on CUDA"),
    ("kv8", "q last stride", mut(q=strided), LAST),
    ("kv8", "cache k on cpu", mut(k=cpu), "k must be on CUDA"),
    ("kv8", "cache v on cpu", mut(v=cpu), "v must be on CUDA"),
    ("kv8", "cache k last stride", mut(k=strided), LAST),
    ("kv8", "cache v last stride", mut(v=strided), LAST),
    ("kv8", "cache k 3-D", mut(k=lambda t: t[0]), FP8_4D),
    ("kv8", "dense q 3-D", mut(q=lambda t: t[0]), "q must have shape (batch_size, seqlen_q, num_heads, head_size)"),
    ("kv8_rag", "ragged q 4-D", mut(q=lambda t: t.unsqueeze(0)), "q must have shape (total_q, num_heads, head_size) with cu_seqlens_q"),
    ("kv8_rag", "cu_seqlens_q dtype", mut(cu_seqlens_q=to(I64)), KV8_CUQ),
    ("kv8_rag", "cu_seqlens_q stride", mut(cu_seqlens_q=strided), KV8_CUQ),
    ("kv8_rag", "cu_seqlens_q on cpu", mut(cu_seqlens_q=cpu), KV8_CUQ),
    ("kv8_rag", "no max_seqlen_q", mut(max_seqlen_q=None), "max_seqlen_q must be provided with cu_seqlens_q"),
    ("kv8_rag", "no seqused_k", mut(seqused_k=None), "seqused_k (the cache fill levels) must be provided with cu_seqlens_q over a KV cache"),
    ("kv8", "seqused_q with dense q", mut(seqused_q=new([3, 3])),
     "This flash attention build does not support KV-cache arguments together with seqused_q without cu_seqlens_q."),
    ("kv8", "empty batch", mut(q=shape(0, 3, 4, 64)), "batch size must be positive"),
    ("kv8", "heads", mut(q=shape(2, 3, 3, 64)), HEADS),
    ("kv8", "paged with kv_batch_idx", mut(kv_batch_idx=new([1, 0])), PAGED_IDX),
    ("kv8", "page table dtype", mut(page_table=to(I64)), "block_table must have dtype torch.int32"),
    ("kv8", "page table on cpu", mut(page_table=cpu), "block_table must be on CUDA"),
    ("kv8", "page table last stride", mut(page_table=strided), "block_table must have contiguous last dimension"),
    ("kv8", "page table batch", mut(page_table=lambda t: torch.cat([t, t[:1]])), BT_SHAPE),
    ("kv8", "cache k head dim", mut(k=shape(8, 16, 2, 32)), "k must have shape (..., 2, 64)"),
    ("kv8", "cache v pages", mut(v=lambda t: t[:-1]), "v must have the shape of k"),
    ("kv8", "seqused_k dtype", mut(seqused_k=to(I64)), KV8_SEQUSED),
    ("kv8", "seqused_k on cpu", mut(seqused_k=cpu), KV8_SEQUSED),
    ("kv8", "seqused_k stride", mut(seqused_k=strided), KV8_SEQUSED),
    ("kv8", "seqused_k shape", mut(seqused_k=new([5, 9, 1])), KV8_SEQUSED),
    ("kv8_rag", "seqused_q shape", mut(seqused_q=new([1, 3, 1])), "seqused_q must be int32 of shape (batch_size,)"),
    ("kv8", "paged with leftpad_k", mut(leftpad_k=new([0, 0])), PAGED_LEFTPAD),
    ("kv8_batched", "leftpad_k dtype", mut(leftpad_k=new([0, 0], I64)), "leftpad_k must have dtype int32"),
    ("kv8_batched", "leftpad_k stride", mut(leftpad_k=lambda _: _i([0, 0, 0, 0])[::2]), "leftpad_k must be contiguous"),
    ("kv8_batched", "leftpad_k shape", mut(leftpad_k=new([0, 0, 0])), "leftpad_k must have shape (batch_size)"),
    ("kv8_batched", "leftpad_k without seqused_k", mut(leftpad_k=new([0, 0]), seqused_k=None), SEQUSED_NEEDED),
    ("kv8_batched", "kv_batch_idx on cpu", mut(kv_batch_idx=lambda _: _i([1, 0]).cpu()), "cache_batch_idx must be on CUDA"),
    ("kv8_batched", "kv_batch_idx stride", mut(kv_batch_idx=lambda _: _i([1, 0, 0, 0])[::2]), KV8_IDX),
    ("kv8_batched", "kv_batch_idx shape", mut(kv_batch_idx=new([1, 0, 0])), KV8_IDX),
    ("kv8_batched", "kv_batch_idx dtype", mut(kv_batch_idx=new([1, 0], I64)), "cache_batch_idx must have dtype int32"),
    ("kv8_batched", "cache smaller than the batch", both("k", "v", lambda t: t[:1]), ENTRIES),
    ("kv8", "k_descale dtype", mut(k_descale=to(BF16)), "k_descale must be fp32 (batch_size, num_heads_k)"),
    ("kv8", "k_descale on cpu", mut(k_descale=cpu), "k_descale must be fp32 (batch_size, num_heads_k)"),
    ("kv8", "v_descale shape", mut(v_descale=shape(2, 4)), "v_descale must be fp32 (batch_size, num_heads_k)"),
    ("kv8", "cache k misaligned", mut(k=misaligned),
     "the fp8 KV cache must be 16-byte aligned with row/head/batch strides that are multiples of 16"),
    ("kv8_batched", "cache v misaligned", mut(v=misaligned),
     "the fp8 KV cache must be 16-byte aligned with row/head/batch strides that are multiples of 16"),
    ("kv8", "out dtype", mut(out=lambda _: _z(2, 3, 4, 64, dtype=FP16)), "Output must have the same dtype as the query"),
    ("kv8", "out on cpu", mut(out=lambda _: _z(2, 3, 4, 64).cpu()), "out must have the shape of q"),
    ("kv8", "out last stride", mut(out=lambda _: strided(_z(2, 3, 4, 64))), "out must have the shape of q"),
    ("kv8", "out shape", mut(out=lambda _: _z(2, 3, 4, 32)), "out must have the shape of q"),
    # ---- 16-bit q over an fp8 cache with new rows and rotary: the step's own refusals, then kvcache_append_kv8's
    ("kv8a", "k_new without v_new, rotary", mut(v_new=None), NEED_NEW),
    ("kv8a_norotary", "k_new without v_new", mut(v_new=None), "k_new and v_new must be passed together"),
    ("kv8a", "rotary_cos without rotary_sin", mut(rotary_sin=None), TOGETHER_RO),
    ("kv8a", "cu_seqlens_k_new with dense q", mut(cu_seqlens_k_new=new([0, 3, 6])),
     "This flash attention build does not support cu_seqlens_k_new without cu_seqlens_q."),
    ("kv8a", "k_new dtype", mut(k_new=to(FP16)), "k_new and v_new must have the same dtype as query"),
    ("kv8a", "v_new fp8", mut(v_new=lambda t: _z(2, 3, 2, 64, dtype=FP8)),
     "k_new and v_new must have the same dtype as query"),
    ("kv8a", "k_new fp8", both("k_new", "v_new", lambda t: _z(2, 3, 2, 64, dtype=FP8)), NEW_FP8),
    ("kv8a", "k_new without seqused_k", mut(seqused_k=None), SEQUSED_NEEDED),
    ("kv8a", "q on cpu", mut(q=cpu), "q must be on CUDA"),
    ("kv8a", "q last stride", mut(q=strided), LAST),
    ("kv8a", "dense q 3-D", mut(q=lambda t: t[0]), "q must have shape (batch_size, seqlen_q, num_heads, head_size)"),
    ("kv8a_rag", "ragged q 4-D", mut(q=lambda t: t.unsqueeze(0)), "q must have shape (total_q, num_heads, head_size) with cu_seqlens_q"),
    ("kv8a_rag", "cu_seqlens_q dtype", mut(cu_seqlens_q=to(I64)), KV8_CUQ),
    ("kv8a_rag", "cu_seqlens_q on cpu", mut(cu_seqlens_q=cpu), KV8_CUQ),
    ("kv8a_rag", "no max_seqlen_q", mut(max_seqlen_q=None), "max_seqlen_q must be provided with cu_seqlens_q"),
    ("kv8a", "seqused_k shape", mut(seqused_k=new([5, 9, 1])), KV8_SEQUSED),
    ("kv8a", "heads", mut(q=shape(2, 3, 3, 64)), HEADS),
    ("kv8a", "cache k 3-D", mut(k=lambda t: t[0]), HEADS),
    ("kv8a", "cache k head dim", mut(k=shape(8, 16, 2, 32)), HEADS),
    ("kv8a", "paged with leftpad_k", mut(leftpad_k=new([0, 0])), PAGED_LEFTPAD),
    ("kv8a_batched", "leftpad_k dtype", mut(leftpad_k=new([0, 0], I64)), "leftpad_k must have dtype int32"),
    ("kv8a_batched", "leftpad_k shape", mut(leftpad_k=new([0, 0, 0])), "leftpad_k must have shape (batch_size)"),
    ("kv8a", "cache k on cpu", mut(k=cpu), "k_cache must be on CUDA"),
    ("kv8a", "cache v on cpu", mut(v=cpu), "v_cache must be on CUDA"),
    ("kv8a", "k_new on cpu", mut(k_new=cpu), "k_new must be on CUDA"),
    ("kv8a", "v_new on cpu", mut(v_new=cpu), "v_new must be on CUDA"),
    ("kv8a", "cache v pages", mut(v=lambda t: t[:-1]), "v must have the shape of k"),
    ("kv8a", "cache k last stride", mut(k=strided), LAST),
    ("kv8a", "k_new last stride", mut(k_new=strided), "k_new tensor must have contiguous last dimension"),
    ("kv8a", "v_new last stride", mut(v_new=strided), "v_new tensor must have contiguous last dimension"),
    ("kv8a", "seqused_k dtype", mut(seqused_k=to(I64)), APP_SEQLENS),
    ("kv8a", "seqused_k on cpu", mut(seqused_k=cpu), APP_SEQLENS),
    ("kv8a", "seqused_k stride", mut(seqused_k=strided), APP_SEQLENS),
    ("kv8a_rag", "cu_seqlens_k_new on cpu", mut(cu_seqlens_k_new=cpu), "cu_seqlens_k_new must be on CUDA"),
    ("kv8a_rag", "cu_seqlens_k_new stride", mut(cu_seqlens_k_new=strided), "cu_seqlens_k_new must be contiguous"),
    ("kv8a_rag", "cu_seqlens_k_new dtype", mut(cu_seqlens_k_new=to(I64)), "cu_seqlens_k_new must have dtype torch.int32"),
    ("kv8a_rag", "cu_seqlens_k_new shape", mut(cu_seqlens_k_new=new([0, 1, 2, 4])), "cu_seqlens_k_new must have shape (batch_size + 1)"),
    ("kv8a_rag", "ragged k_new 4-D", mut(k_new=lambda t: t.unsqueeze(0)),
     "k_new must have shape (total_k_new, num_heads_k, head_size) with cu_seqlens_k_new"),
    ("kv8a_rag", "ragged k_new heads", mut(k_new=shape(4, 1, 64)), "k_new must have shape (k_new.size(0), num_heads_k, head_size)"),
    ("kv8a_rag", "ragged v_new rows", mut(v_new=shape(3, 2, 64)), "v_new must have shape (k_new.size(0), num_heads_k, head_size)"),
    ("kv8a", "dense k_new 3-D", mut(k_new=shape(6, 2, 64)),
     "k_new must have shape (batch_size, seqlen_k_new, num_heads_k, head_size) without cu_seqlens_k_new"),
    ("kv8a", "dense k_new batch", mut(k_new=shape(3, 3, 2, 64)), "k_new must have shape (batch_size, k_new.size(1), num_heads_k, head_size)"),
    ("kv8a", "dense v_new rows", mut(v_new=shape(2, 2, 2, 64)), "v_new must have shape (batch_size, k_new.size(1), num_heads_k, head_size)"),
    ("kv8a", "paged with kv_batch_idx", mut(kv_batch_idx=new([1, 0])), PAGED_IDX),
    ("kv8a", "page table dtype", mut(page_table=to(I64)), "block_table must have dtype torch.int32"),
    ("kv8a", "page table batch", mut(page_table=lambda t: torch.cat([t, t[:1]])), BT_SHAPE),
    ("kv8a_batched", "kv_batch_idx on cpu", mut(kv_batch_idx=lambda _: _i([1, 0]).cpu()), "cache_batch_idx must be on CUDA"),
    ("kv8a_batched", "kv_batch_idx shape", mut(kv_batch_idx=new([1, 0, 0])), KV8_IDX),
    ("kv8a_batched", "kv_batch_idx dtype", mut(kv_batch_idx=new([1, 0], I64)), "cache_batch_idx must have dtype int32"),
    ("kv8a_batched", "cache smaller than the batch", both("k", "v", lambda t: t[:1]), ENTRIES),
    ("kv8a", "k_descale dtype", mut(k_descale=to(BF16)), "k_descale must be fp32 (batch_size, num_heads_k)"),
    ("kv8a", "v_descale shape", mut(v_descale=shape(2, 4)), "v_descale must be fp32 (batch_size, num_heads_k)"),
    ("kv8a", "cache k misaligned", mut(k=misaligned),
     "the fp8 KV cache must be 8-byte aligned with row/head/batch strides that are multiples of 8 to be appended to"),
    ("kv8a", "rotary_cos on cpu", mut(rotary_cos=cpu), "rotary_cos must be on CUDA"),
    ("kv8a", "rotary_cos 1-D", mut(rotary_cos=lambda t: t[:, 0]), RO_SHAPE),
    ("kv8a", "rotary_sin shape", mut(rotary_sin=lambda t: t[:, :8]), RO_SHAPE),
    ("kv8a", "rotary_dim above the head dim", both("rotary_cos", "rotary_sin", shape(64, 48)), RO_HEAD),
    ("kv8a", "rotary_dim 24", both("rotary_cos", "rotary_sin", shape(64, 12)), RO_16),
    ("kv8a", "cos / sin shorter than the pages", both("rotary_cos", "rotary_sin", lambda t: t[:32]), RO_SHORT),
    ("kv8a_batched", "cos / sin shorter than the cache", both("rotary_cos", "rotary_sin", lambda t: t[:32]), RO_SHORT),
    ("kv8a", "rotary_sin stride", mut(rotary_sin=strided), RO_CONTIG),
    ("kv8a", "rotary_cos dtype", mut(rotary_cos=to(FP16)), "rotary_cos / rotary_sin must have the same dtype as k_new"),
    ("kv8a", "seqlens_rotary on cpu", mut(seqlens_rotary=lambda _: _i([5, 9]).cpu()), RO_SEQLENS),
    ("kv8a", "seqlens_rotary dtype", mut(seqlens_rotary=new([5, 9], I64)), "seqlens_rotary must have dtype torch.int32"),
    ("kv8a", "seqlens_rotary shape", mut(seqlens_rotary=new([5, 9, 0])), "seqlens_rotary must have shape (batch_size,)"),
    # ---- hopper_interface.kvcache_append_fp8: kvcache_append_kv8 on its own
    ("app", "cache dtype", mut(k_cache=lambda t: _z(8, 16, 2, 64)), "the fp8 KV cache must have dtype torch.float8_e4m3fn"),
    ("app", "k fp8", mut(k=lambda t: _z(2, 3, 2, 64, dtype=FP8)), NEW_FP8),
    ("app", "k / v fp32", both("k", "v", to(F32)), "k_new / v_new must be fp16 or bf16"),
    ("app", "v dtype", mut(v=to(FP16)), "k_new and v_new must have the same dtype"),
    ("app", "k_cache on cpu", mut(k_cache=cpu), "k_cache must be on CUDA"),
    ("app", "v_cache on cpu", mut(v_cache=cpu), "v_cache must be on CUDA"),
    ("app", "k on cpu", mut(k=cpu), "k_new must be on CUDA"),
    ("app", "v on cpu", mut(v=cpu), "v_new must be on CUDA"),
    ("app", "k_cache 3-D", mut(k_cache=lambda t: t[0]), FP8_4D),
    ("app", "v_cache pages", mut(v_cache=lambda t: t[:-1]), "v must have the shape of k"),
    ("app", "k_cache last stride", mut(k_cache=strided), LAST),
    ("app", "v_cache last stride", mut(v_cache=strided), LAST),
    ("app", "k last stride", mut(k=strided), "k_new tensor must have contiguous last dimension"),
    ("app", "v last stride", mut(v=strided), "v_new tensor must have contiguous last dimension"),
    ("app", "cache head dim", both("k_cache", "v_cache", shape(8, 16, 2, 144)),
     "This flash attention build supports an fp8 KV cache for head_size <= 128 that is a multiple of 16, got 144"),
    ("app", "cache_seqlens dtype", mut(cache_seqlens=to(I64)), APP_SEQLENS),
    ("app", "cache_seqlens on cpu", mut(cache_seqlens=cpu), APP_SEQLENS),
    ("app", "cache_seqlens stride", mut(cache_seqlens=strided), APP_SEQLENS),
    ("app", "cache_seqlens 2-D", mut(cache_seqlens=lambda t: t.unsqueeze(0)), APP_SEQLENS),
    ("app", "cache_seqlens empty", mut(cache_seqlens=lambda t: t[:0]), APP_SEQLENS),
    ("app_rag", "cu_seqlens_k_new on cpu", mut(cu_seqlens_k_new=cpu), "cu_seqlens_k_new must be on CUDA"),
    ("app_rag", "cu_seqlens_k_new stride", mut(cu_seqlens_k_new=strided), "cu_seqlens_k_new must be contiguous"),
    ("app_rag", "cu_seqlens_k_new dtype", mut(cu_seqlens_k_new=to(I64)), "cu_seqlens_k_new must have dtype torch.int32"),
    ("app_rag", "cu_seqlens_k_new shape", mut(cu_seqlens_k_new=new([0, 1, 2, 4])), "cu_seqlens_k_new must have shape (batch_size + 1)"),
    ("app_rag", "ragged k 4-D", mut(k=lambda t: t.unsqueeze(0)),
     "k_new must have shape (total_k_new, num_heads_k, head_size) with cu_seqlens_k_new"),
    ("app_rag", "ragged k heads", mut(k=shape(4, 1, 64)), "k_new must have shape (k_new.size(0), num_heads_k, head_size)"),
    ("app_rag", "ragged v rows", mut(v=shape(3, 2, 64)), "v_new must have shape (k_new.size(0), num_heads_k, head_size)"),
    ("app_rag", "max_seqlen_k_new", mut(max_seqlen_k_new=-1), "max_seqlen_k_new must be non-negative"),
    ("app", "dense k 3-D", mut(k=shape(6, 2, 64)),
     "k_new must have shape (batch_size, seqlen_k_new, num_heads_k, head_size) without cu_seqlens_k_new"),
    ("app", "dense k batch", mut(k=shape(3, 3, 2, 64)), "k_new must have shape (batch_size, k_new.size(1), num_heads_k, head_size)"),
    ("app", "dense v rows", mut(v=shape(2, 2, 2, 64)), "v_new must have shape (batch_size, k_new.size(1), num_heads_k, head_size)"),
    ("app", "paged with cache_batch_idx", mut(cache_batch_idx=new([1, 0])), PAGED_IDX),
    ("app", "page table dtype", mut(page_table=to(I64)), "block_table must have dtype torch.int32"),
    ("app", "page table on cpu", mut(page_table=cpu), "block_table must be on CUDA"),
    ("app", "page table last stride", mut(page_table=strided), "block_table must have contiguous last dimension"),
    ("app", "page table batch", mut(page_table=lambda t: torch.cat([t, t[:1]])), BT_SHAPE),
    ("app_batched", "cache_batch_idx on cpu", mut(cache_batch_idx=lambda _: _i([1, 0]).cpu()), "cache_batch_idx must be on CUDA"),
    ("app_batched", "cache_batch_idx stride", mut(cache_batch_idx=lambda _: _i([1, 0, 0, 0])[::2]), KV8_IDX),
    ("app_batched", "cache_batch_idx shape", mut(cache_batch_idx=new([1, 0, 0])), KV8_IDX),
    ("app_batched", "cache_batch_idx dtype", mut(cache_batch_idx=new([1, 0], I64)), "cache_batch_idx must have dtype int32"),
    ("app_batched", "cache smaller than the batch", both("k_cache", "v_cache", lambda t: t[:1]), ENTRIES),
    ("app", "k_descale dtype", mut(k_descale=to(BF16)), "k_descale must be fp32 (batch_size, num_heads_k)"),
    ("app", "k_descale on cpu", mut(k_descale=cpu), "k_descale must be fp32 (batch_size, num_heads_k)"),
    ("app", "v_descale shape", mut(v_descale=shape(2, 4)), "v_descale must be fp32 (batch_size, num_heads_k)"),
    ("app", "k_cache misaligned", mut(k_cache=misaligned),
     "the fp8 KV cache must be 8-byte aligned with row/head/batch strides that are multiples of 8 to be appended to"),
    ("app_batched", "v_cache misaligned", mut(v_cache=misaligned),
     "the fp8 KV cache must be 8-byte aligned with row/head/batch strides that are multiples of 8 to be appended to"),
    ("app", "rotary_cos without rotary_sin", mut(rotary_sin=None), TOGETHER_RO),
    ("app", "rotary_cos on cpu", mut(rotary_cos=cpu), "rotary_cos must be on CUDA"),
    ("app", "rotary_sin on cpu", mut(rotary_sin=cpu), "rotary_sin must be on CUDA"),
    ("app", "rotary_cos 1-D", mut(rotary_cos=lambda t: t[:, 0]), RO_SHAPE),
    ("app", "rotary_sin shape", mut(rotary_sin=lambda t: t[:, :8]), RO_SHAPE),
    ("app", "rotary_dim above the head dim", both("rotary_cos", "rotary_sin", shape(64, 48)), RO_HEAD),
    ("app", "rotary_dim 24", both("rotary_cos", "rotary_sin", shape(64, 12)), RO_16),
    ("app", "cos / sin shorter than the pages", both("rotary_cos", "rotary_sin", lambda t: t[:32]), RO_SHORT),
    ("app_batched", "cos / sin shorter than the cache", both("rotary_cos", "rotary_sin", lambda t: t[:32]), RO_SHORT),
    ("app", "rotary_cos stride", mut(rotary_cos=strided), RO_CONTIG),
    ("app", "rotary_sin stride", mut(rotary_sin=strided), RO_CONTIG),
    ("app", "rotary_cos dtype", mut(rotary_cos=to(FP16)), "rotary_cos / rotary_sin must have the same dtype as k_new"),
    ("app", "rotary_sin dtype", mut(rotary_sin=to(FP16)), "rotary_cos / rotary_sin must have the same dtype as k_new"),
    ("app", "rotary_seqlens on cpu", mut(rotary_seqlens=lambda _: _i([5, 9]).cpu()), RO_SEQLENS),
    ("app", "rotary_seqlens stride", mut(rotary_seqlens=lambda _: _i([5, 9, 0, 0])[::2]), RO_SEQLENS),
    ("app", "rotary_seqlens dtype", mut(rotary_seqlens=new([5, 9], I64)), "seqlens_rotary must have dtype torch.int32"),
    ("app", "rotary_seqlens shape", mut(rotary_seqlens=new([5, 9, 0])), "seqlens_rotary must have shape (batch_size,)"),
]


@pytest.mark.parametrize("base,what,breaks,text", CASES, ids=[f"{c[0]}-{c[1]}".replace(" ", "_") for c in CASES])
def test_refused_with_the_exact_text(base, what, breaks, text):
    args = breaks(dict(_bases()[base]))
    with pytest.raises(RuntimeError, match=r"\A" + re.escape(text) + r"(?:\n|\Z)"):
        _call(base, args)


NEWLY_REFUSED = [  # calls the dense 16-bit routes did not refuse by a text of their own before the checks were shared
    ("fa2", "rotary_cos 1-D", mut(rotary_cos=lambda t: t[:, 0]), "rotary_cos must have shape (seqlen_ro, rotary_dim / 2)"),
    ("fa3_batched", "rotary_cos 1-D", mut(rotary_cos=lambda t: t[:, 0]), "rotary_cos must have shape (seqlen_ro, rotary_dim / 2)"),
    ("fa2", "cache_batch_idx shorter than the batch", mut(cache_batch_idx=new([1])), "cache_batch_idx must have shape (batch_size)"),
    ("fa3_batched", "kv_batch_idx shorter than the batch", mut(kv_batch_idx=new([1])), "cache_batch_idx must have shape (batch_size)"),
]


@pytest.mark.parametrize("base,what,breaks,text", NEWLY_REFUSED, ids=[f"{c[0]}-{c[1]}".replace(" ", "_") for c in NEWLY_REFUSED])
def test_newly_refused_with_a_text(base, what, breaks, text):
    with pytest.raises(RuntimeError, match=r"\A" + re.escape(text) + r"(?:\n|\Z)"):
        _call(base, breaks(dict(_bases()[base])))


def test_longer_batch_idx_is_still_served_on_the_dense_route():
    """(the dense 16-bit route never checked the length of the index: the first batch_size entries are read)"""
    args = dict(_bases()["fa2_decode"], cache_batch_idx=_i([1, 0, 1]), kcache=_bases()["fa2"]["kcache"].clone())
    out = _call("fa2_decode", args)[0]
    torch.cuda.synchronize()
    assert tuple(out.shape) == (2, 1, 4, 64) and out.dtype == BF16


def test_case_ids_are_unique():
    ids = [(c[0], c[1]) for c in CASES]
    assert len(set(ids)) == len(ids)


VALID = {  # base -> (index of the output in the result, its shape, its dtype)
    "fa2": (0, (2, 3, 4, 64), BF16), "fa2_paged": (0, (2, 3, 4, 64), BF16), "fa2_decode": (0, (2, 1, 4, 64), BF16),
    "fa3": (0, (2, 3, 4, 64), BF16), "fa3_batched": (0, (2, 3, 4, 64), BF16), "fa3_decode": (0, (2, 1, 4, 64), BF16),
    "rag": (0, (4, 4, 64), BF16), "rag_dense_new": (0, (4, 4, 64), BF16), "rag_batched": (0, (4, 4, 64), BF16),
    "rag_read": (0, (4, 4, 64), BF16),
    "kv8": (0, (2, 3, 4, 64), BF16), "kv8_rag": (0, (4, 4, 64), BF16), "kv8_batched": (0, (2, 3, 4, 64), BF16),
    "kv8_nodescale": (0, (2, 3, 4, 64), BF16),
    "kv8a": (0, (2, 3, 4, 64), BF16), "kv8a_norotary": (0, (2, 3, 4, 64), BF16), "kv8a_rag": (0, (4, 4, 64), BF16),
    "kv8a_batched": (0, (2, 3, 4, 64), BF16),
    "app": (None, (2,), I32), "app_rag": (None, (2,), I32), "app_batched": (None, (2,), I32),
}


@pytest.mark.parametrize("base", sorted(VALID))
def test_base_call_is_valid(base):
    """Every base the table breaks is itself served (on copies of its caches: the append writes)."""
    assert set(VALID) == set(_bases())
    args = {k: (v.clone() if torch.is_tensor(v) and v.dim() == 4 and k in ("k", "v", "kcache", "vcache", "k_cache", "v_cache") else v)
            for k, v in _bases()[base].items()}
    index, shape_, dtype = VALID[base]
    r = _call(base, args)
    out = r if index is None else r[index]
    torch.cuda.synchronize()
    assert tuple(out.shape) == shape_ and out.dtype == dtype
